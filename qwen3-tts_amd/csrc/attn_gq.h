// attn_gq.h -- decode attention for every head shape the engine accepts: head_dim 64 | 128, a GQA group of 1..8 query heads per kv
// head (run-time value: 3, 5, 6 and 7 included), 1 or 2 new tokens.  Included by attention.hip, which owns the __global__ wrappers
// (and their LDS arrays) and the launcher; the five older decode kernels there keep head_dim 128 with a group <= 2.
//
// The contract is AttnDecodeParams': fused q / k RMSNorm, rotate-half RoPE at position S0 + t - n_pad, K / V append through the
// cache type, left-pad and causal masks, output rows t * B + b in the caller's layout.  One workgroup (4 waves) per (sequence, kv
// head[, split]); the NQ = group * n_new <= 16 queries of a kv head are the COLUMNS of the problem (column c = token c / group, head
// c % group), columns >= NQ are zero.  Three stages:
//   1. the NQ + 2 n_new new vectors, one wave each in turn: norm + RoPE, K / V rounded through the cache type and appended (split 0
//      only), all of them to LDS as fp32; the scores of the new keys against every column as fp32 q . k.
//   2. the CACHED keys [0, S0) with an online softmax (running max / sum per column, accumulators rescaled), state in registers:
//      nothing in LDS grows with the sequence length.
//        attn_gq16 (bf16 cache, transposed V pages): both products on v_mfma_f32_16x16x32_bf16, attn_tk16's formulation -- S = K q^T
//          with the columns as the B operand, O^T = V^T P with the V pages [HD][16 keys] as the A operand; a wave takes the 32-key
//          blocks w, w + 4, ... of its split.
//        attn_gqv (fp32 cache, or bf16 cache with row-major V): fp32 on the VALU.  16 lanes per key (HD / 16 dims each, DPP row
//          reduction), lane group g takes keys g, g + 16, ... of its split.
//   3. the partial states (4 waves | 16 lane groups) and the new keys are combined in a FIXED order -- the result does not depend
//      on wave scheduling -- and leave as output rows, or with split-KV as (numerator | max | denominator) for attn_gq_merge.
// split-KV partials: part[(b * nkv + kvh) * nsplit + split][NQ][HD + 2].
// (The host-emulation build of the test suite stamps attention.hip, not this header: after an edit of this file alone, remove
// tests/hostemu/libqtts_hostemu.so.sha once.)
#pragma once
#include "common.h"
#include "kernels.h"
#include "attn_helpers.h"

namespace qtts {

// ---- stage 1: norm + RoPE + append of the new vectors; xs[NQ + 2 n_new][HD] = q columns | new keys | new values (fp32; keys and
// values as a later step reads them back from the cache).  A lane owns dims `lane` and `lane + HD / 2` (the rotate-half pair).
template <typename KVT, int HD, bool CT, bool VT>
__device__ __forceinline__ void gq_stage1(const AttnDecodeParams& p, int b, int kvh, int GQ, int NQ, int S0, int npad, bool append, float* xs) {
    constexpr int HH = HD / 2;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nvec = NQ + 2 * p.n_new, pps = p.kv.pages_per_seq;
    const bool act = lane < HH;
    for (int vi = wave; vi < nvec; vi += 4) {
        int t, col;
        const float* w = nullptr;
        if (vi < NQ) { t = vi / GQ; col = (kvh * GQ + vi % GQ) * HD; w = p.qw; }
        else if (vi < NQ + p.n_new) { t = vi - NQ; col = (p.nh + kvh) * HD; w = p.kw; }
        else { t = vi - NQ - p.n_new; col = (p.nh + p.nkv + kvh) * HD; }
        const float* src = p.qkv + ((size_t)t * p.B + b) * p.ld + col;
        float x0 = act ? src[lane] : 0.f, x1 = act ? src[lane + HH] : 0.f;
        if (w) {
            const float ss = wave_sum64_dpp(x0 * x0 + x1 * x1);
            const float rs = rsqrtf(ss / (float)HD + p.eps);
            x0 = (act ? w[lane] : 0.f) * (x0 * rs);
            x1 = (act ? w[lane + HH] : 0.f) * (x1 * rs);
            const float ang = (float)(S0 + t - npad) * (act ? p.inv_freq[lane] : 0.f);
            const float c = cosf(ang), sn = sinf(ang);
            const float o0 = x0 * c - x1 * sn, o1 = x1 * c + x0 * sn;
            x0 = o0; x1 = o1;
        }
        if (vi >= NQ) {                                      // K or V of a new token: round through the cache type, append
            const int s = S0 + t;
            const bool isk = vi < NQ + p.n_new;
            const KVT h0 = kv_cast<KVT>(x0), h1 = kv_cast<KVT>(x1);
            if (append && act && (s >> 4) < pps) {           // (a step at capacity writes nothing; the host refuses it first)
                const int page = CT ? b * pps + (s >> 4) : p.kv.page_table[b * pps + (s >> 4)];
                const size_t pb = (((size_t)p.layer * p.kv.n_pages + page) * p.kv.nkv + kvh) * (size_t)(16 * HD);
                KVT* cdst = reinterpret_cast<KVT*>(isk ? p.kv.k : p.kv.v);
                if (isk || !VT) { const size_t o = pb + (size_t)(s & 15) * HD; cdst[o + lane] = h0; cdst[o + lane + HH] = h1; }
                else { const size_t o = pb + (s & 15); cdst[o + (size_t)lane * 16] = h0; cdst[o + (size_t)(lane + HH) * 16] = h1; }   // V page [HD][16]
            }
            x0 = kv_load(&h0); x1 = kv_load(&h1);
        }
        if (act) { xs[vi * HD + lane] = x0; xs[vi * HD + lane + HH] = x1; }
    }
}

// scores of the new keys (after the barrier behind stage 1): snew[c * 2 + t2] = q_c . k_t2 / sqrt(HD), -inf where the causal or the
// pad mask hides key S0 + t2 from column c.  One 16-lane group per (column, key) pair.
template <int HD>
__device__ __forceinline__ void gq_new_scores(const AttnDecodeParams& p, const float* xs, int GQ, int NQ, int S0, int npad, float* snew) {
    constexpr int DPL = HD / 16;
    const int g = threadIdx.x >> 4, li = threadIdx.x & 15;
    for (int pr = g; pr < NQ * p.n_new; pr += 16) {
        const int c = pr / p.n_new, t2 = pr % p.n_new;
        const float* q = xs + c * HD + li * DPL;
        const float* k = xs + (NQ + t2) * HD + li * DPL;
        float a = 0.f;
#pragma unroll
        for (int e = 0; e < DPL; ++e) a += q[e] * k[e];
        a = row16_sum(a) * rsqrtf((float)HD);
        if (li == 0) snew[c * 2 + t2] = (t2 <= c / GQ && S0 + t2 >= npad) ? a : -INFINITY;
    }
}

// stage 3 for ONE output element (column c, dim dd): `np` partial states in their fixed order -- numerators redc[i * rstride + dd],
// maxima gmc[i * mstride], denominators glc[i * mstride] -- then, in the split that owns them, the new keys.
template <typename KVT, int HD>
__device__ __forceinline__ void gq_finish(const AttnDecodeParams& p, int b, int kvh, int GQ, int NQ, int c, int dd, int np, const float* redc, int rstride,
                                          const float* gmc, const float* glc, int mstride, bool has_new, const float* snew, const float* xs, int nsplit,
                                          int split) {
    float mm = -INFINITY;
    if (has_new)
        for (int t2 = 0; t2 < p.n_new; ++t2) mm = fmaxf(mm, snew[c * 2 + t2]);
    for (int i = 0; i < np; ++i) mm = fmaxf(mm, gmc[i * mstride]);
    float num = 0.f, den = 0.f;
    for (int i = 0; i < np; ++i) {
        const float ms = gmc[i * mstride];
        const float f = ms > -INFINITY ? att_exp<KVT>(ms - mm) : 0.f;
        num += redc[i * rstride + dd] * f;
        den += glc[i * mstride] * f;
    }
    if (has_new)
        for (int t2 = 0; t2 < p.n_new; ++t2) {
            const float s = snew[c * 2 + t2];
            if (s > -INFINITY) {
                const float f = att_exp<KVT>(s - mm);
                num += xs[(NQ + p.n_new + t2) * HD + dd] * f;
                den += f;
            }
        }
    if (nsplit > 1) {                                        // partial result of this split: numerator | max | denominator
        float* pp = p.part + (((size_t)blockIdx.x * nsplit + split) * NQ + c) * (HD + 2);
        pp[dd] = num;
        if (dd == 0) { pp[HD] = mm; pp[HD + 1] = den; }
        return;
    }
    const int t = c / GQ, gq = c % GQ;
    const size_t o = ((size_t)t * p.B + b) * p.ldo + (size_t)(kvh * GQ + gq) * HD + dd;
    const float r = num / den;
    if (p.out_bf16) reinterpret_cast<bf16_t*>(p.out)[o] = f32_to_bf16(r);
    else p.out[o] = r;
}

// the 32-key blocks [b0, bend) of CACHED keys this workgroup reads: split y of gridDim.y takes ceil(blocks(max_len) / nsplit) blocks,
// the last split whatever lies beyond (a length past the span is still read completely)
__device__ __forceinline__ void gq_block_range(const AttnDecodeParams& p, int S0, int& b0, int& bend) {
    const int nsplit = gridDim.y, split = blockIdx.y, total = (S0 + 31) >> 5;
    if (nsplit == 1) { b0 = 0; bend = total; return; }
    const int bps = (((p.max_len + 31) >> 5) + nsplit - 1) / nsplit;
    b0 = split * bps;
    bend = split == nsplit - 1 ? total : min(b0 + bps, total);
}

// =================================================================================== attn_gq16: bf16 cache, transposed V, matrix pipe
// The layout of the fragments is attn_tk16's (attention.hip), with HD / 32 k-steps and HD / 16 dim blocks: the rows of the two S
// tiles of a 32-key block are permuted keys (tile A row 4q + r = key 8q + r, tile B row 4q + r = key 8q + 4 + r), so that lane
// (column lj, lq) ends up with the scores of keys 8 lq .. 8 lq + 7 -- the fragment the PV product wants from it as its B operand.
// LDS (from the wrapper): xs[NC + 4][HD] | red[4][NC][HD] | gm[4][NC] | gl[4][NC] | snew[2 NC].
template <int HD, int NC, bool CT>
__device__ __forceinline__ void attn_gq16_body(const AttnDecodeParams& p, float* xs, float* red, float* gm, float* gl, float* snew) {
    constexpr int NB = 2, KT = HD / 32, DB = HD / 16;        // NB: 32-key blocks per wave requested at kernel entry
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    const int b = blockIdx.x / p.nkv, kvh = blockIdx.x % p.nkv;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lj = lane & 15, lq = lane >> 4;
    const int GQ = p.nh / p.nkv, NQ = GQ * p.n_new;
    const bf16_t* kc = reinterpret_cast<const bf16_t*>(p.kv.k);
    const bf16_t* vc = reinterpret_cast<const bf16_t*>(p.kv.v);
    const int pps = p.kv.pages_per_seq;
    // element offset of (page pg of this sequence, this kv head): the same for the K pool ([16][HD]) and the V pool ([HD][16]).
    // Speculative READS stay inside the sequence's pages (what they fetch beyond the live length is dropped at use).
    auto page_base = [&](int pg) -> size_t {
        pg = pg < pps ? pg : pps - 1;
        const int page = CT ? b * pps + pg : p.kv.page_table[b * pps + pg];
        return (((size_t)p.layer * p.kv.n_pages + page) * p.kv.nkv + kvh) * (size_t)(16 * HD);
    };
    auto load_block = [&](u32x4 (&kA)[KT], u32x4 (&kB)[KT], u32x4 (&vT)[DB], int blk) {
        const size_t pk = page_base(2 * blk + (lj >> 3));                  // rows 0-7: first page, rows 8-15: second page
        const int kin = ((lj >> 2) & 1) * 8 + (lj & 3);                    // key inside the page for tile A (tile B: + 4)
        const u32x4* ka = reinterpret_cast<const u32x4*>(kc + pk + (size_t)kin * HD + lq * 8);
        const u32x4* kb = reinterpret_cast<const u32x4*>(kc + pk + (size_t)(kin + 4) * HD + lq * 8);
#pragma unroll
        for (int t = 0; t < KT; ++t) { kA[t] = ka[t * 4]; kB[t] = kb[t * 4]; }
        const size_t pv = page_base(2 * blk + (lq >> 1));
        const u32x4* vb = reinterpret_cast<const u32x4*>(vc + pv + (size_t)lj * 16 + (lq & 1) * 8);
#pragma unroll
        for (int d = 0; d < DB; ++d) vT[d] = vb[d * 32];
    };

    const int nsplit = gridDim.y, split = blockIdx.y;
    const int S0 = attn_len(p, b);    // KV length before this step = position of the first new key
    const int npad = p.n_pad ? p.n_pad[b] : 0;
    const int done = p.done_flag ? *p.done_flag : 0;
    if (done) return;
    int b0s, bend;
    gq_block_range(p, S0, b0s, bend);
    u32x4 kA[NB][KT], kB[NB][KT], vT[NB][DB];
#pragma unroll
    for (int n = 0; n < NB; ++n) load_block(kA[n], kB[n], vT[n], b0s + wave + 4 * n);

    gq_stage1<bf16_t, HD, CT, true>(p, b, kvh, GQ, NQ, S0, npad, split == 0, xs);
    __syncthreads();
    gq_new_scores<HD>(p, xs, GQ, NQ, S0, npad, snew);
    // B operand of S = K q^T: lane (column lj, lq) <- q[lj][32 t + 8 lq .. + 8] as bf16; columns >= NQ are zero
    u32x4 qB[KT];
#pragma unroll
    for (int t = 0; t < KT; ++t) {
        const float* q = xs + (lj < NQ ? lj : 0) * HD + 32 * t + 8 * lq;
        const float4 a = *reinterpret_cast<const float4*>(q);
        const float4 c = *reinterpret_cast<const float4*>(q + 4);
        u32x4 v;
        v[0] = pack_bf16(a.x, a.y); v[1] = pack_bf16(a.z, a.w); v[2] = pack_bf16(c.x, c.y); v[3] = pack_bf16(c.z, c.w);
        qB[t] = lj < NQ ? v : (u32x4){0u, 0u, 0u, 0u};
    }

    const float scale = rsqrtf((float)HD);
    float m = -INFINITY, l = 0.f;                // of column lj; l: this lane's keys only until the end
    f32x4 acc[DB];
#pragma unroll
    for (int d = 0; d < DB; ++d) acc[d] = (f32x4){0.f, 0.f, 0.f, 0.f};
    auto process = [&](const u32x4 (&ka)[KT], const u32x4 (&kb)[KT], const u32x4 (&vt)[DB], int blk) {
        f32x4 sA = {0.f, 0.f, 0.f, 0.f}, sB = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < KT; ++t) {
            bf16x8 a, bq, c;
            *reinterpret_cast<u32x4*>(&a) = ka[t]; *reinterpret_cast<u32x4*>(&c) = kb[t]; *reinterpret_cast<u32x4*>(&bq) = qB[t];
            sA = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bq, sA, 0, 0, 0);
            sB = __builtin_amdgcn_mfma_f32_16x16x32_bf16(c, bq, sB, 0, 0, 0);
        }
        const int key0 = 32 * blk + 8 * lq;      // this lane: keys key0 + e (tile A: e = 0..3, tile B: e = 4..7) of column lj
        float sc[8];
        float mc = -INFINITY;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int key = key0 + e;
            const bool valid = key < S0 && key >= npad;      // left-pad slots were never written; slots >= S0 hold nothing yet
            const float v = (e < 4 ? sA[e] : sB[e - 4]) * scale;
            sc[e] = valid ? v : -INFINITY;
            mc = fmaxf(mc, sc[e]);
        }
        mc = fmaxf(mc, __shfl_xor(mc, 16));
        mc = fmaxf(mc, __shfl_xor(mc, 32));
        const float mn = fmaxf(m, mc);
        const float f = m > -INFINITY ? att_exp<bf16_t>(m - mn) : 0.f;
        float pr[8], ps = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) { pr[e] = sc[e] > -INFINITY ? att_exp<bf16_t>(sc[e] - mn) : 0.f; ps += pr[e]; }
        l = l * f + ps;
        m = mn;
        u32x4 pb;
        pb[0] = pack_bf16(pr[0], pr[1]); pb[1] = pack_bf16(pr[2], pr[3]); pb[2] = pack_bf16(pr[4], pr[5]); pb[3] = pack_bf16(pr[6], pr[7]);
        // V fragments of never-written / not-yet-written keys may hold anything (NaN x 0 = NaN): mask them to zero
        u32x4 vm;
#pragma unroll
        for (int e2 = 0; e2 < 4; ++e2) {
            const int k0 = key0 + 2 * e2;
            vm[e2] = ((k0 < S0 && k0 >= npad) ? 0x0000ffffu : 0u) | ((k0 + 1 < S0 && k0 + 1 >= npad) ? 0xffff0000u : 0u);
        }
        bf16x8 pB;
        *reinterpret_cast<u32x4*>(&pB) = pb;
#pragma unroll
        for (int d = 0; d < DB; ++d) {
            bf16x8 va;
            *reinterpret_cast<u32x4*>(&va) = vt[d] & vm;
            acc[d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va, pB, acc[d] * f, 0, 0, 0);
        }
    };
#pragma unroll
    for (int n = 0; n < NB; ++n)
        if (b0s + wave + 4 * n < bend) process(kA[n], kB[n], vT[n], b0s + wave + 4 * n);
    for (int blk = b0s + wave + 4 * NB; blk < bend; blk += 4 * NB) {        // beyond the register window: NB blocks per latency round
#pragma unroll
        for (int n = 0; n < NB; ++n)
            if (blk + 4 * n < bend) load_block(kA[n], kB[n], vT[n], blk + 4 * n);
#pragma unroll
        for (int n = 0; n < NB; ++n)
            if (blk + 4 * n < bend) process(kA[n], kB[n], vT[n], blk + 4 * n);
    }
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
    // acc[d][r] of lane (column lj, lq) = dim 16 d + 4 lq + r
    if (lj < NQ) {
#pragma unroll
        for (int d = 0; d < DB; ++d) *reinterpret_cast<f32x4*>(&red[(wave * NC + lj) * HD + 16 * d + 4 * lq]) = acc[d];
        if (lq == 0) { gm[wave * NC + lj] = m; gl[wave * NC + lj] = l; }
    }
    __syncthreads();
    for (int i = tid; i < NQ * HD; i += 256) {
        const int c = i / HD, dd = i % HD;
        gq_finish<bf16_t, HD>(p, b, kvh, GQ, NQ, c, dd, 4, red + c * HD, NC * HD, gm + c, gl + c, NC, split == 0, snew, xs, nsplit, split);
    }
}

// =================================================================================== attn_gqv: fp32 | bf16 row-major cache, VALU
// LDS (from the wrapper): xs[NC + 4][HD] | red[16][HD] | gm[16] | gl[16] | snew[2 NC].
template <typename KVT, int HD, int NC, bool CT>
__device__ __forceinline__ void attn_gqv_body(const AttnDecodeParams& p, float* xs, float* red, float* gm, float* gl, float* snew) {
    constexpr int DPL = HD / 16;                             // dims per lane of a 16-lane key group
    const int b = blockIdx.x / p.nkv, kvh = blockIdx.x % p.nkv;
    const int tid = threadIdx.x, g = tid >> 4, li = tid & 15;
    const int GQ = p.nh / p.nkv, NQ = GQ * p.n_new;
    const KVT* kc = reinterpret_cast<const KVT*>(p.kv.k);
    const KVT* vc = reinterpret_cast<const KVT*>(p.kv.v);
    const int pps = p.kv.pages_per_seq;
    const int nsplit = gridDim.y, split = blockIdx.y;
    const int S0 = attn_len(p, b);
    const int npad = p.n_pad ? p.n_pad[b] : 0;
    const int done = p.done_flag ? *p.done_flag : 0;
    if (done) return;
    int b0s, bend;
    gq_block_range(p, S0, b0s, bend);
    const int k1 = min(32 * bend, S0);

    gq_stage1<KVT, HD, CT, false>(p, b, kvh, GQ, NQ, S0, npad, split == 0, xs);
    __syncthreads();
    gq_new_scores<HD>(p, xs, GQ, NQ, S0, npad, snew);
    // the columns' q fragments live in registers while they fit beside the accumulators (NC x DPL <= 64); at 16 columns of head_dim 128
    // they are re-read from LDS per key instead (two 16-B reads per column: the accumulators alone are 128 registers)
    constexpr bool QREG = NC * DPL <= 64;
    float q[QREG ? NC : 1][DPL], acc[NC][DPL], m[NC], l[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        m[c] = -INFINITY; l[c] = 0.f;
#pragma unroll
        for (int e = 0; e < DPL; ++e) {
            if constexpr (QREG) q[c][e] = c < NQ ? xs[c * HD + li * DPL + e] : 0.f;
            acc[c][e] = 0.f;
        }
    }
    const float scale = rsqrtf((float)HD);
    for (int s = max(32 * b0s, npad & ~15) + g; s < k1; s += 16) {     // (pages wholly inside the left pad are skipped; same key -> group map)
        if (s < npad) continue;                              // never-written slot
        const int page = CT ? b * pps + (s >> 4) : p.kv.page_table[b * pps + (s >> 4)];
        const size_t o = ((((size_t)p.layer * p.kv.n_pages + page) * p.kv.nkv + kvh) * 16 + (s & 15)) * HD + li * DPL;
        float kx[DPL], vx[DPL];
#pragma unroll
        for (int e = 0; e < DPL; ++e) { kx[e] = kv_load(kc + o + e); vx[e] = kv_load(vc + o + e); }
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            if (c < NQ) {
                float a = 0.f;
#pragma unroll
                for (int e = 0; e < DPL; ++e) a += (QREG ? q[c][e] : xs[c * HD + li * DPL + e]) * kx[e];
                a = row16_sum(a) * scale;
                const float mn = fmaxf(m[c], a);
                const float f = m[c] > -INFINITY ? att_exp<KVT>(m[c] - mn) : 0.f;
                const float pr = att_exp<KVT>(a - mn);
                l[c] = l[c] * f + pr;
#pragma unroll
                for (int e = 0; e < DPL; ++e) acc[c][e] = acc[c][e] * f + pr * vx[e];
                m[c] = mn;
            }
        }
    }
    // the 16 key groups combine through LDS in group order, one column at a time
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        if (c < NQ) {
#pragma unroll
            for (int e = 0; e < DPL; ++e) red[g * HD + li * DPL + e] = acc[c][e];
            if (li == 0) { gm[g] = m[c]; gl[g] = l[c]; }
            __syncthreads();
            if (tid < HD) gq_finish<KVT, HD>(p, b, kvh, GQ, NQ, c, tid, 16, red, HD, gm, gl, 1, split == 0, snew, xs, nsplit, split);
            __syncthreads();
        }
    }
}

// merge of the split-KV partial results (fixed order): out = sum_s num_s e^(m_s - m) / sum_s den_s e^(m_s - m)
template <int HD>
__device__ __forceinline__ void attn_gq_merge_body(const AttnDecodeParams& p) {
    if (p.done_flag && *p.done_flag) return;
    const int b = blockIdx.x / p.nkv, kvh = blockIdx.x % p.nkv;
    const int GQ = p.nh / p.nkv, NQ = GQ * p.n_new;
    const size_t stride = (size_t)NQ * (HD + 2);
    for (int i = threadIdx.x; i < NQ * HD; i += 256) {
        const int c = i / HD, dd = i % HD;
        const float* base = p.part + ((size_t)blockIdx.x * p.nsplit * NQ + c) * (HD + 2);
        float mm = -INFINITY;
        for (int s = 0; s < p.nsplit; ++s) mm = fmaxf(mm, base[s * stride + HD]);
        float num = 0.f, den = 0.f;
        for (int s = 0; s < p.nsplit; ++s) {
            const float ms = base[s * stride + HD];
            const float f = ms > -INFINITY ? expf(ms - mm) : 0.f;
            num += base[s * stride + dd] * f;
            den += base[s * stride + HD + 1] * f;
        }
        const int t = c / GQ, gq = c % GQ;
        const size_t o = ((size_t)t * p.B + b) * p.ldo + (size_t)(kvh * GQ + gq) * HD + dd;
        const float r = num / den;
        if (p.out_bf16) reinterpret_cast<bf16_t*>(p.out)[o] = f32_to_bf16(r);
        else p.out[o] = r;
    }
}

}  // namespace qtts

// stream_kernels.hip -- the small kernels the state-carrying codec decode adds: everything else in
// that path reuses the validated kernels of the non-streaming decoder.  Thread-independent code (no LDS, no cross-lane
// ops): tests/hostemu also executes THESE SOURCES on the CPU through a sequential block/thread interpreter.
#include "common.h"
#include "kernels.h"

namespace qtts {

// ---------------------------------------------------------------------------------- streaming codec decode helpers
// Every layer of the decoder is causal, so a packet of new frames only needs, per stateful layer, the last
// (k-1)*dilation input rows of the previous packet (oracle/codec_stream_ref.py).  `stage_rows` builds
// [carried rows | new rows] so that the UNCHANGED conv / attention kernels run on it; `save_tail` refreshes the carry.
// `stage_rows` itself is the form without a carry (h == 0 in the stream: plain compaction); the carried forms are below.
__global__ __launch_bounds__(256) void stage_rows_kernel(const float* src, int src_T, int skip, int n, const float* state,
                                                         int h, float* dst, int C4) {
    const int r = blockIdx.x, b = blockIdx.y;
    const float4* from = r < h ? reinterpret_cast<const float4*>(state) + ((size_t)b * h + r) * C4
                               : reinterpret_cast<const float4*>(src) + ((size_t)b * src_T + skip + (r - h)) * C4;
    float4* to = reinterpret_cast<float4*>(dst) + ((size_t)b * (h + n) + r) * C4;
    for (int c = threadIdx.x; c < C4; c += 256) to[c] = from[c];
}
void launch_stage_rows(const float* src, int src_T, int skip, int n, const float* state, int h, float* dst, int B, int C,
                       hipStream_t st) {
    QTTS_REQUIRE(C % 4 == 0 && n >= 1 && h >= 0 && skip >= 0 && skip + n <= src_T, QTTS_ERR_ARG, "stage_rows: bad shape");
    QTTS_REQUIRE(h == 0 || state, QTTS_ERR_ARG, "stage_rows: state missing");
    hipLaunchKernelGGL(stage_rows_kernel, dim3(h + n, B), dim3(256), 0, st, src, src_T, skip, n, state, h, dst, C / 4);
    QTTS_CHECK_HIP(hipGetLastError());
}

// ---------------------------------------------------------------------------------- per-slot carries
// A stream owns B slots, each with its own carries and its own position; a push decodes a packet for any M of them.  The staged and
// activation buffers stay dense [M][h + n][C]; only the carry is addressed through the device slot map: row m of the push reads and
// refreshes state[slot[m]].  (The lockstep push is the identity map.)
__global__ __launch_bounds__(256) void stage_rows_slots_kernel(const float* src, int src_T, int skip, int n, const float* state,
                                                               const int* slot, int h, float* dst, int C4) {
    const int r = blockIdx.x, m = blockIdx.y;
    const float4* from = r < h ? reinterpret_cast<const float4*>(state) + ((size_t)slot[m] * h + r) * C4
                               : reinterpret_cast<const float4*>(src) + ((size_t)m * src_T + skip + (r - h)) * C4;
    float4* to = reinterpret_cast<float4*>(dst) + ((size_t)m * (h + n) + r) * C4;
    for (int c = threadIdx.x; c < C4; c += 256) to[c] = from[c];
}
void launch_stage_rows_slots(const float* src, int src_T, int skip, int n, const float* state, const int* slot, int h, float* dst,
                             int M, int C, hipStream_t st) {
    QTTS_REQUIRE(C % 4 == 0 && n >= 1 && h >= 1 && skip >= 0 && skip + n <= src_T && M >= 1, QTTS_ERR_ARG, "stage_rows_slots: bad shape");
    QTTS_REQUIRE(state && slot, QTTS_ERR_ARG, "stage_rows_slots: state or slot map missing");
    hipLaunchKernelGGL(stage_rows_slots_kernel, dim3(h + n, M), dim3(256), 0, st, src, src_T, skip, n, state, slot, h, dst, C / 4);
    QTTS_CHECK_HIP(hipGetLastError());
}

__global__ __launch_bounds__(256) void save_tail_slots_kernel(const float* buf, int Tp, float* state, const int* slot, int h, int C4) {
    const int j = blockIdx.x, m = blockIdx.y;
    const float4* from = reinterpret_cast<const float4*>(buf) + ((size_t)m * Tp + (Tp - h + j)) * C4;
    float4* to = reinterpret_cast<float4*>(state) + ((size_t)slot[m] * h + j) * C4;
    for (int c = threadIdx.x; c < C4; c += 256) to[c] = from[c];
}
void launch_save_tail_slots(const float* buf, int Tp, float* state, const int* slot, int h, int M, int C, hipStream_t st) {
    QTTS_REQUIRE(C % 4 == 0 && h >= 1 && Tp >= h && M >= 1 && state && slot, QTTS_ERR_ARG, "save_tail_slots: bad shape");
    hipLaunchKernelGGL(save_tail_slots_kernel, dim3(h, M), dim3(256), 0, st, buf, Tp, state, slot, h, C / 4);
    QTTS_CHECK_HIP(hipGetLastError());
}

// ---------------------------------------------------------------------------------- priming a slot
// stream_prime_rows starts sequences of DIFFERENT lengths in one set of launches: sequence m is right-aligned in its block, so its first
// lead[m] frames (lead[m] * rate rows at a stage that runs at `rate` rows per frame) are padding.  Every stateful layer must see them as
// the causal zero padding of a sequence that starts behind them, and the stateless layers in between write bias terms into them; the
// staging step is where every stateful layer's input passes, so it writes the zeros: dst[m] = [h zeros (the carry of a sequence that
// starts) | lead zeros | src rows].  The carry -- the last h rows of dst[m] -- is stored by the block that wrote the row: stage_rows_slots
// + save_tail_slots in one launch, and nothing reads the carry, so no block depends on another.
__global__ __launch_bounds__(256) void stage_prime_slots_kernel(const float* src, int src_T, int skip, int n, const int* lead, int rate,
                                                                float* state, const int* slot, int h, float* dst, int C4) {
    const int r = blockIdx.x, m = blockIdx.y;
    const bool pad = r < h + lead[m] * rate;
    const float4* from = reinterpret_cast<const float4*>(src) + ((size_t)m * src_T + skip + (pad ? 0 : r - h)) * C4;
    float4* to = reinterpret_cast<float4*>(dst) + ((size_t)m * (h + n) + r) * C4;
    float4* keep = r >= n ? reinterpret_cast<float4*>(state) + ((size_t)slot[m] * h + (r - n)) * C4 : nullptr;
    for (int c = threadIdx.x; c < C4; c += 256) {
        const float4 v = pad ? make_float4(0.f, 0.f, 0.f, 0.f) : from[c];
        to[c] = v;
        if (keep) keep[c] = v;
    }
}
void launch_stage_prime_slots(const float* src, int src_T, int skip, int n, const int* lead, int rate, float* state, const int* slot,
                              int h, float* dst, int M, int C, hipStream_t st) {
    QTTS_REQUIRE(C % 4 == 0 && n >= 1 && h >= 1 && skip >= 0 && skip + n <= src_T && M >= 1 && rate >= 1, QTTS_ERR_ARG,
                 "stage_prime_slots: bad shape");
    QTTS_REQUIRE(src && dst && state && slot && lead, QTTS_ERR_ARG, "stage_prime_slots: null argument");
    hipLaunchKernelGGL(stage_prime_slots_kernel, dim3(h + n, M), dim3(256), 0, st, src, src_T, skip, n, lead, rate, state, slot, h, dst, C / 4);
    QTTS_CHECK_HIP(hipGetLastError());
}

// rvq_gather (elementwise.hip) for the right-aligned blocks of a prime: codes (M, Q, T) contiguous, the first lead[m] columns of
// sequence m are padding whose VALUES are not the caller's to define -- they are not read (no error flag, no table row), and their
// output rows are zeros.  The real columns are summed in rvq_gather's order.
__global__ __launch_bounds__(256) void rvq_gather_lead_kernel(const int64_t* codes, int Q, int T, const int* lead, const float* tables,
                                                              int bins, int vq, float* out, int* err) {
    const int row = blockIdx.x;          // m * T + t
    const int m = row / T, t = row % T;
    const bool pad = t < lead[m];
    const int64_t* cp = codes + ((size_t)m * Q) * T + t;
    if (!pad && threadIdx.x < Q && cp[(size_t)threadIdx.x * T] >= bins) *err = 1;
    for (int j = threadIdx.x; j < 2 * vq; j += 256) {
        float acc = 0.f;
        if (!pad && j < vq) {
            int64_t c = cp[0]; if (c < 0 || c >= bins) c = 0;
            acc = tables[((size_t)c) * vq + j];
        } else if (!pad) {
            for (int q = 1; q < Q; ++q) {
                int64_t c = cp[(size_t)q * T]; if (c < 0 || c >= bins) c = 0;
                const float e = tables[((size_t)q * bins + c) * vq + (j - vq)];
                acc = (q == 1) ? e : acc + e;
            }
        }
        out[(size_t)row * 2 * vq + j] = acc;
    }
}
void launch_rvq_gather_lead(const int64_t* codes, int M, int Q, int T, const int* lead, const float* tables, int bins, int vq, float* out,
                            int* err, hipStream_t st) {
    QTTS_REQUIRE(Q >= 1 && Q <= 256 && M >= 1 && T >= 1 && codes && lead && err, QTTS_ERR_ARG, "rvq_gather_lead: bad shape");
    hipLaunchKernelGGL(rvq_gather_lead_kernel, dim3(M * T), dim3(256), 0, st, codes, Q, T, lead, tables, bins, vq, out, err);
    QTTS_CHECK_HIP(hipGetLastError());
}

// rotate-half RoPE at positions pos0[row / T] + (row % T): T new frames per sequence, sequence m of the push starts at frame pos0[m]
// of its own stream
__global__ __launch_bounds__(256) void rope_offset_rows_kernel(float* qkv, int ld, int T, const int* pos0, int nheads, int hd,
                                                               const float* inv_freq, int64_t total) {
    const int half = hd / 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int d = (int)(i % half);
        const int h = (int)((i / half) % nheads);
        const int64_t row = i / ((int64_t)half * nheads);
        const float ang = (float)(pos0[row / T] + (int)(row % T)) * inv_freq[d];
        const float c = cosf(ang), s = sinf(ang);
        float* p = qkv + row * ld + h * hd;
        const float x0 = p[d], x1 = p[d + half];
        p[d] = x0 * c - x1 * s;
        p[d + half] = x1 * c + x0 * s;
    }
}
void launch_rope_offset_rows(float* qkv, int ld, int rows, int T, const int* pos0, int n_heads_total, int hd, const float* inv_freq,
                             hipStream_t st) {
    QTTS_REQUIRE(T >= 1 && rows % T == 0 && pos0, QTTS_ERR_ARG, "rope_offset_rows: bad shape");
    const int64_t total = (int64_t)rows * n_heads_total * (hd / 2);
    const int grid = (int)std::min<int64_t>((total + 255) / 256, 65535);
    hipLaunchKernelGGL(rope_offset_rows_kernel, dim3(grid), dim3(256), 0, st, qkv, ld, T, pos0, n_heads_total, hd, inv_freq, total);
    QTTS_CHECK_HIP(hipGetLastError());
}

// zero every carry of the listed slots (zeros == the causal left padding of a sequence that starts): one launch, stream-ordered
// with the pushes around it.  blockIdx.y = carry, blockIdx.z = listed slot.
__global__ __launch_bounds__(256) void stream_reset_slots_kernel(StreamCarryTable t, const int* slot) {
    const int k = blockIdx.y;
    const int n4 = t.elems4[k];
    float4* to = reinterpret_cast<float4*>(t.state[k]) + (size_t)slot[blockIdx.z] * n4;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256) to[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}
void launch_stream_reset_slots(const StreamCarryTable& t, const int* slot, int n_slots, hipStream_t st) {
    QTTS_REQUIRE(t.n >= 1 && t.n <= StreamCarryTable::MAX && n_slots >= 1 && slot, QTTS_ERR_ARG, "stream_reset_slots: bad shape");
    hipLaunchKernelGGL(stream_reset_slots_kernel, dim3(16, t.n, n_slots), dim3(256), 0, st, t, slot);
    QTTS_CHECK_HIP(hipGetLastError());
}

}  // namespace qtts

"""The general decode attention (csrc/attn_gq.h: head_dim 64 | 128, GQA groups of 1..8) on the CPU: its real source on the SIMT
emulator against float64 numpy, and the talker engine's C++ on it against fixtures the REFERENCE produced at three head shapes
(tools/gen_golden_gq.py -> tests/golden/talker_tiny_gq*.npz).  Not marked `gpu`: runs anywhere."""
import ctypes as C
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

import synth
import talker_ref
from qwen3_tts_amd import _lib
from qwen3_tts_amd.config import TalkerConfig
from test_hostemu import emu, _bf16_round, _ptr, _talker_emu, _talker_generate  # noqa: F401  (`emu` is a fixture)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import gen_golden_gq  # noqa: E402  (the fixtures' configs and prompt; its reference imports are inside generate())

MARGIN_EXEMPT = 1e-3
FIXTURES = sorted(gen_golden_gq.SHAPES)


def _compare_greedy(codes, tokens, g_codes, g_tokens, margin):
    """The rule of tests/test_gpu_parity.py: bit-exact; a cb-0 mismatch is exempt only behind a reference margin below MARGIN_EXEMPT,
    and the comparison stops there.  Compares the frames both sides have; returns how many."""
    n = min(codes.shape[1], g_codes.shape[1])
    for f in range(n + 1):
        if f < tokens.shape[1] and not np.array_equal(tokens[:, f], g_tokens[:, f]):
            bad = np.nonzero(tokens[:, f] != g_tokens[:, f])[0]
            assert (margin[bad, f] < MARGIN_EXEMPT).all(), f"token mismatch at step {f}, rows {bad.tolist()}, margins {margin[bad, f]}"
            return f
        if f < n:
            assert np.array_equal(codes[:, f], g_codes[:, f]), f"sub-codebook mismatch in frame {f}"
    return n


# ============================================================================================ the kernels, directly
# (S0, n_pad per row | None = the code predictor's call: static length, no pad array, permuted page table)
_LENGTHS = [(0, None, False), (1, [0, 1], False),                                   # pass 0; a row whose only valid key is the new one
            (15, [0, 3], False), (16, None, True), (17, [0, 16], True),             # page edge
            (31, [0, 5], False), (32, [0, 32], False), (33, [2, 0], True),          # 32-key block edge
            (255, [0, 100], False), (256, [70, 0], True), (257, [0, 257], False)]   # register window; a pad that masks whole leading blocks
_SPLIT = [(300, [0, 40], True), (701, [9, 650], False)]                             # 3 splits (the talker's call: one new token)


def _attn_case(emu, g, mode, nh, nkv, n_new, S0, npads, permute, nsplit):
    HD, eps, B = 128, 1e-6, 2
    bf16, vt = mode != "f32", mode == "vt"
    GQ = nh // nkv
    inv_freq = (1.0 / (10000.0 ** (np.arange(64) / 64.0))).astype(np.float32)
    qw = (1 + 0.1 * g.standard_normal(HD)).astype(np.float32)
    kw = (1 + 0.1 * g.standard_normal(HD)).astype(np.float32)
    rnd = (lambda a: _bf16_round(a)[0]) if bf16 else (lambda a: a)

    def normrope(x, w, pos):
        x = x.astype(np.float64)
        x = w * (x / np.sqrt((x ** 2).mean() + eps))
        ang = np.float32(pos) * inv_freq                     # fp32 angle like the kernel, then exact cos / sin
        c, s = np.cos(ang.astype(np.float64)), np.sin(ang.astype(np.float64))
        return np.concatenate([x[:64] * c - x[64:] * s, x[64:] * c + x[:64] * s])

    pps = (S0 + n_new + 15) // 16 + 1
    n_pages = B * pps
    table = g.permutation(n_pages).astype(np.int32).reshape(B, pps) if permute else np.arange(n_pages, dtype=np.int32).reshape(B, pps)
    ld = (nh + 2 * nkv) * HD
    qkv = g.standard_normal((n_new * B, ld)).astype(np.float32)
    K = rnd((g.standard_normal((B, nkv, S0, HD)) * 0.7).astype(np.float32))
    V = rnd(g.standard_normal((B, nkv, S0, HD)).astype(np.float32))
    kp = np.full((n_pages, nkv, 16, HD), np.nan, np.float32)          # never-written slots hold NaN: none may reach the result
    vp_ = np.full((n_pages, nkv, HD, 16) if vt else (n_pages, nkv, 16, HD), np.nan, np.float32)
    cp_call = npads is None
    npad = np.zeros(B, np.int32) if cp_call else np.asarray(npads, np.int32)
    for b in range(B):
        for s in range(npad[b], S0):
            kp[table[b, s // 16], :, s % 16] = K[b, :, s]
            if vt:
                vp_[table[b, s // 16], :, :, s % 16] = V[b, :, s]
            else:
                vp_[table[b, s // 16], :, s % 16] = V[b, :, s]
    if bf16:
        kpool, vpool = _bf16_round(np.nan_to_num(kp, nan=0.0))[1].copy(), _bf16_round(np.nan_to_num(vp_, nan=0.0))[1].copy()
        kpool[np.isnan(kp)] = 0x7FC0; vpool[np.isnan(vp_)] = 0x7FC0
    else:
        kpool, vpool = kp.copy(), vp_.copy()
    tag = (mode, nh, nkv, n_new, S0, nsplit)

    def launch(order):
        kk, vv = kpool.copy(), vpool.copy()
        out = np.full((n_new * B, nh * HD + 4), 5.0, np.float32)
        emu.hostemu_set_fiber_order(order)
        try:
            rc = emu.hostemu_attn_decode(_ptr(qkv), ld, B, n_new, nh, nkv, _ptr(qw), _ptr(kw), eps, _ptr(inv_freq),
                                         None if cp_call else _ptr(npad), S0, _ptr(kk), _ptr(vv), _ptr(table) if permute else None,
                                         pps, 1 if bf16 else 0, _ptr(out), nh * HD + 4, 32 if (cp_call and S0 + n_new <= 32) else S0 + n_new + 3)
        finally:
            emu.hostemu_set_fiber_order(0)
        assert rc == 0, (tag, (emu.qtts_last_error() or b"").decode())
        gotk = np.zeros((B, nkv, n_new, HD), np.float32); gotv = np.zeros((B, nkv, n_new, HD), np.float32)
        for b in range(B):
            for t in range(n_new):
                s = S0 + t
                k_, v_ = kk[table[b, s // 16], :, s % 16], (vv[table[b, s // 16], :, :, s % 16] if vt else vv[table[b, s // 16], :, s % 16])
                if bf16:
                    k_, v_ = [(x.astype(np.uint32) << 16).view(np.float32) for x in (k_, v_)]
                gotk[b, :, t], gotv[b, :, t] = k_, v_
        return out, gotk, gotv

    runs = [launch(order) for order in (0, 1, 2)]
    # ---- the appended rows: V is the input rounded once (exact); K is norm + RoPE in fp32, rounded once -- within fp32 error of the
    # float64 value, or, behind the bf16 rounding, within one bf16 step of it (2^-8 relative)
    newk = np.zeros((B, nkv, n_new, HD)); newv = np.zeros((B, nkv, n_new, HD))
    for b in range(B):
        for h in range(nkv):
            for t in range(n_new):
                row = qkv[t * B + b]
                newk[b, h, t] = normrope(row[(nh + h) * HD:(nh + h + 1) * HD], kw, S0 + t - npad[b])
                newv[b, h, t] = rnd(row[(nh + nkv + h) * HD:(nh + nkv + h + 1) * HD])
    for _, gotk, gotv in runs:
        assert np.array_equal(gotv, newv.astype(np.float32)), tag
        assert np.all(np.abs(gotk - newk) <= (2.0 ** -8 if bf16 else 1e-6) * np.abs(newk) + 1e-5), tag
        assert np.array_equal(gotk, runs[0][1]), tag
    if bf16:        # the attention below is checked on the cache's contents: the key as the kernel rounded it (a float64 value next to a
        newk = runs[0][1].astype(np.float64)       # bf16 rounding boundary may round the other way than its fp32 image -- 0.4 % of one element)
    # ---- float64 reference
    ref = np.zeros((n_new * B, nh * HD))
    for b in range(B):
        for h in range(nkv):
            keys = np.concatenate([K[b, h].astype(np.float64), newk[b, h]], 0)
            vals = np.concatenate([V[b, h].astype(np.float64), newv[b, h]], 0)
            sidx = np.arange(S0 + n_new)
            for t in range(n_new):
                for gq in range(GQ):
                    hq = h * GQ + gq
                    q = normrope(qkv[t * B + b][hq * HD:(hq + 1) * HD], qw, S0 + t - npad[b])
                    sc = keys @ q / np.sqrt(HD)
                    sc[(sidx < npad[b]) | (sidx > S0 + t)] = -np.inf
                    pr = np.exp(sc - sc.max()); pr /= pr.sum()
                    ref[t * B + b, hq * HD:(hq + 1) * HD] = pr @ np.where(np.isfinite(sc)[:, None], vals, 0.0)
    outs = [r[0] for r in runs]
    for order, out in enumerate(outs):
        d = out[:, :nh * HD] - ref
        assert np.isfinite(out).all(), tag
        if vt:      # q, K, P, V enter the matrix pipe as bf16: 2 % of the largest output, 0.4 % RMS
            assert float(np.abs(d).max()) <= 2e-2 * max(1.0, float(np.abs(ref).max())), (tag, order, float(np.abs(d).max()))
            assert float(np.sqrt((d ** 2).mean())) <= 4e-3 * float(np.sqrt((ref ** 2).mean())) + 1e-4, (tag, order)
        else:       # fp32 arithmetic on the cache's values
            assert float(np.abs(d).max()) <= 3e-5 * max(1.0, float(np.abs(ref).max())), (tag, order, float(np.abs(d).max()))
        assert np.all(out[:, nh * HD:] == 5.0), tag
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2]), tag


@pytest.mark.parametrize("nh,nkv", [(8, 1), (8, 2), (5, 1), (6, 2)])
@pytest.mark.parametrize("mode", ["f32", "bf16", "vt"])
def test_attn_gq_kernels_real_source(emu, qopt, mode, nh, nkv):
    """attn_gq.h's kernels from their real source, through the existing `hostemu_attn_decode` entry (head_dim 128; groups 8, 4, 5, 3)
    against float64 numpy: q / k RMSNorm + RoPE at S0 + t - n_pad, K / V append through the cache type, left-pad and causal masks, one
    and two new tokens, cache lengths at every edge of the code (empty, one key, page, 32-key block, register window), pads that mask
    whole leading blocks or everything but the new key, permuted page tables, NaN in never-written slots, and split-KV (3 splits) with
    the merge.  fp32 cache and bf16 row-major cache: attn_gqv (VALU, fp32 arithmetic) at 3e-5 x max(1, |ref|max); bf16 cache with
    transposed V pages: attn_gq16 (both products on the matrix pipe) at 2 % of the largest output and 0.4 % RMS + 1e-4.  Three wave
    scheduling orders, bit-identical."""
    g = np.random.default_rng(1000 + 10 * nh + nkv + {"f32": 0, "bf16": 100, "vt": 200}[mode])
    if mode == "vt":
        qopt(emu, "QTTS_DEBUG_ATTN_VT", "1")
    for n_new in (1, 2):
        for S0, npads, permute in _LENGTHS:
            _attn_case(emu, g, mode, nh, nkv, n_new, S0, npads, permute, 1)
    qopt(emu, "QTTS_DEBUG_ATTN_NSPLIT", "3")
    for S0, npads, permute in _SPLIT:
        _attn_case(emu, g, mode, nh, nkv, 1, S0, npads, permute, 3)


# ============================================================================================ the engine on the emulator
def _stats(emu, h):
    emu.qtts_talker_get_stats.argtypes = [C.c_void_p, C.POINTER(_lib.TalkerStatsC)]
    st = _lib.TalkerStatsC()
    assert emu.qtts_talker_get_stats(h, C.byref(st)) == 0
    return st


def _fixture(golden_dir, name):
    g = np.load(os.path.join(golden_dir, f"talker_tiny_{name}.npz"))
    t = gen_golden_gq.cfg(name)
    wn = synth.talker_weights(t, with_text=False)
    return g, t, wn, {k: torch.from_numpy(v) for k, v in wn.items()}


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_reproduces_the_reference_at_other_head_shapes(golden_dir, name):
    """Oracle pin: `talker_ref.talker_generate` reproduces the reference's greedy codes of the three committed fixtures (5 ragged rows
    x 39 frames x 16 codebooks), and the fixtures carry the inputs and weights this tree builds."""
    g, t, wn, w = _fixture(golden_dir, name)
    assert abs(synth.weights_checksum(synth.talker_weights(t)) - float(g["weights_checksum"])) < 1e-3 * max(1.0, abs(float(g["weights_checksum"])))
    emb, mask, tr, pad = gen_golden_gq.prompt(t)
    assert np.array_equal(emb.numpy(), g["embeds"]) and np.array_equal(mask.numpy(), g["mask"])
    assert g["codes"].shape == (5, 39, 16) and g["tokens"].shape == (5, 40) and float(g["margin"].min()) > MARGIN_EXEMPT
    sp = talker_ref.SamplingParams(do_sample=False, subtalker_dosample=False)
    with torch.no_grad():
        r = talker_ref.talker_generate(w, t, emb, mask, tr, pad, max_new_tokens=40, min_new_tokens=40, sp=sp)
    assert np.array_equal(r["tokens"].numpy(), g["tokens"]) and np.array_equal(r["codes"].numpy(), g["codes"])


@pytest.mark.parametrize("use_graph", [0, 1])
@pytest.mark.parametrize("name", FIXTURES)
def test_talker_engine_other_head_shapes_fp32_vs_reference(emu, golden_dir, name, use_graph):
    """The talker engine's C++ at group 8 / head_dim 128, group 4 and 8 / head_dim 64, group 5 and 3 / head_dim 128 (talker / code
    predictor), fp32, eager and through the captured frame graph: the first 8 frames of the REFERENCE's greedy run, bit for bit (a cb-0
    mismatch exempt only behind a margin below 1e-3: none in these fixtures); the general attention family ran in every layer."""
    g, t, _, w = _fixture(golden_dir, name)
    h = _talker_emu(emu, t, w, max_batch=5, max_seq=64, use_graph=use_graph)
    try:
        args = [g[k] for k in ("embeds", "mask", "trailing", "tts_pad")]
        codes, tokens, _ = _talker_generate(emu, h, t, *args, max_new=9, min_new=9)
        assert codes.shape[1] == 8
        assert _compare_greedy(codes, tokens, g["codes"], g["tokens"], g["margin"]) == 8
        st = _stats(emu, h)
        assert st.attn_gq_per_step == t.num_hidden_layers + (t.num_code_groups - 1) * t.cp_num_hidden_layers, st.attn_gq_per_step
    finally:
        emu.qtts_talker_destroy(h)


@pytest.mark.parametrize("name", FIXTURES)
def test_talker_engine_other_head_shapes_bf16_graph_equals_eager(emu, golden_dir, name):
    """bf16 engines (matrix-pipe attention on transposed V pages for the talker, the VALU kernel on the code predictor's row-major
    cache): the captured frame graph and the eager launches give the same codes, bit for bit."""
    g, t, _, w = _fixture(golden_dir, name)
    args = [g[k] for k in ("embeds", "mask", "trailing", "tts_pad")]
    res = []
    for use_graph in (0, 1):
        h = _talker_emu(emu, t, w, max_batch=5, max_seq=64, dtype=_lib.QTTS_BF16, use_graph=use_graph)
        try:
            res.append(_talker_generate(emu, h, t, *args, max_new=5, min_new=5))
            assert _stats(emu, h).attn_gq_per_step > 0
        finally:
            emu.qtts_talker_destroy(h)
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2])


def test_default_head_shape_through_the_general_family_vs_reference_golden(emu, golden_dir, qopt):
    """QTTS_ATTN_GQ=1 routes EVERY decode-attention launch of the default tiny config (4 / 2 / 128) through attn_gq.h: the fp32 greedy
    codes are still those of tests/golden/talker_tiny.npz, which the reference signed.  With the option off the family is not used."""
    g = np.load(os.path.join(golden_dir, "talker_tiny.npz"))
    t = synth.talker_tiny()
    w = {k: torch.from_numpy(v) for k, v in synth.talker_weights(t, with_text=False).items()}
    args = [g[k] for k in ("embeds", "mask", "trailing", "tts_pad")]
    per_step = t.num_hidden_layers + (t.num_code_groups - 1) * t.cp_num_hidden_layers
    for flag, want in (("1", per_step), (None, 0)):
        qopt(emu, "QTTS_ATTN_GQ", flag)
        h = _talker_emu(emu, t, w, max_batch=4, max_seq=64, use_graph=1)
        try:
            codes, tokens, hidden = _talker_generate(emu, h, t, *args, max_new=14)
            assert np.array_equal(tokens, g["tokens"]) and np.array_equal(codes, g["codes"])
            assert np.abs(hidden - g["hidden"]).max() <= 2e-3
            assert _stats(emu, h).attn_gq_per_step == want
        finally:
            emu.qtts_talker_destroy(h)


# ============================================================================================ host logic
def test_config_without_kv_heads_and_head_dim_loads_and_generates(emu):
    """A talker dict without `num_key_value_heads` and `head_dim` takes the reference's defaults (2 kv heads, hidden // heads) -- and an
    engine at tiny dims with that shape (4 / 2 / 64) creates and generates what the oracle generates."""
    tiny = synth.talker_tiny()
    d = synth.cfg_dict(tiny)
    del d["num_key_value_heads"], d["head_dim"]
    c = TalkerConfig.from_any(d)
    assert c.num_key_value_heads == 2 and c.head_dim == tiny.hidden_size // tiny.num_attention_heads == 64
    t = dataclasses.replace(tiny, num_key_value_heads=c.num_key_value_heads, head_dim=c.head_dim)
    w = {k: torch.from_numpy(v) for k, v in synth.talker_weights(t, with_text=False).items()}
    emb, mask, tr, pad = synth.rand_prompt(np.random.default_rng(5), t, [4, 7], 2, scale=0.5)
    sp = talker_ref.SamplingParams(do_sample=False, subtalker_dosample=False)
    with torch.no_grad():
        r = talker_ref.talker_generate(w, t, emb, mask, tr, pad, max_new_tokens=4, sp=sp)
    h = _talker_emu(emu, t, w, max_batch=2, max_seq=32)
    try:
        codes, tokens, _ = _talker_generate(emu, h, t, emb.numpy(), mask.numpy(), tr.numpy(), pad.numpy(), max_new=4)
        assert np.array_equal(tokens, r["tokens"].numpy()) and np.array_equal(codes, r["codes"].numpy())
    finally:
        emu.qtts_talker_destroy(h)


@pytest.mark.parametrize("change", [dict(num_attention_heads=16, num_key_value_heads=1), dict(head_dim=96),
                                    dict(cp_num_attention_heads=16, cp_num_key_value_heads=1), dict(cp_head_dim=96),
                                    dict(num_attention_heads=5, num_key_value_heads=2)])
def test_unsupported_head_shapes_are_refused_with_the_limits_named(emu, change):
    """A group of 16, a head_dim of 96 (talker or code predictor) and heads that are no multiple of the kv heads are refused at finalize,
    with a message that names the supported set."""
    t = dataclasses.replace(synth.talker_tiny(), **change)
    w = {k: torch.from_numpy(v) for k, v in synth.talker_weights(t, with_text=False).items()}
    with pytest.raises(AssertionError, match=r"head_dim 64 or 128.*1\.\.8"):
        emu.qtts_talker_destroy(_talker_emu(emu, t, w, max_batch=2, max_seq=32))

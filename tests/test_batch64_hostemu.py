"""Talker batches of 33..64 rows on the CPU: the 65..128-row decode GEMM (csrc/skinny.hip: skinny_wide_kernel, and the fp32 kernel's
8-tile form) from its real source on the SIMT emulator, and the talker engine's C++ on it against fixtures the REFERENCE produced at
64 and 40 rows (tools/gen_golden_b64.py -> tests/golden/talker_tiny_b64.npz, talker_tiny_b40.npz).  Not marked `gpu`: runs anywhere."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import synth
from qwen3_tts_amd import _lib
from test_hostemu import emu, _bf16_round, _ptr, _talker_emu, _talker_generate  # noqa: F401  (`emu` is a fixture)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import gen_golden_b64  # noqa: E402  (the fixtures' prompt; its reference imports are inside generate())

MARGIN_EXEMPT = 1e-3
ACT_NONE, ACT_SWIGLU = 0, 2
QTTS_ERR_LIMIT = -6


def compare_greedy(codes, tokens, g_codes, g_tokens, margin):
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


def fixture(golden_dir, name):
    g = np.load(os.path.join(golden_dir, f"talker_tiny_{name}.npz"))
    t = synth.talker_tiny()
    wn = synth.talker_weights(t, with_text=False)
    assert abs(synth.weights_checksum(synth.talker_weights(t)) - float(g["weights_checksum"])) < 1e-3 * max(1.0, abs(float(g["weights_checksum"])))
    assert float(g["margin"].min()) >= MARGIN_EXEMPT          # no step at which the comparison rule could stop early
    args = [x.numpy() for x in gen_golden_b64.prompt(name)]
    return g, t, {k: torch.from_numpy(v) for k, v in wn.items()}, args


def split_prompt(t, seed, half):
    """2 x `half` ragged rows, both halves with the same left padding: the last row of each half is the longest prompt."""
    lens = ([3 + (5 * i) % 11 for i in range(half - 1)] + [15]) * 2
    return [x.numpy() for x in synth.rand_prompt(np.random.default_rng(seed), t, lens, 2, scale=0.5)]


def _stats(emu, h):
    emu.qtts_talker_get_stats.argtypes = [C.c_void_p, C.POINTER(_lib.TalkerStatsC)]
    st = _lib.TalkerStatsC()
    assert emu.qtts_talker_get_stats(h, C.byref(st)) == 0
    return st


PER_STEP = ("cp_fused_per_step", "cp_mlp_per_step", "cp_layer_per_step", "ks_split_per_step", "attn_gq_per_step")


# ============================================================================================ the kernel, directly
# (K, N, fs, norm, act, bias, residual, shadow)
_TINY = [(128, 64, 16, 1, ACT_NONE, 0, 0, 0),        # tiny engine's q|k|v: 4 k-tiles, 4 waves, tail-guarded
         (128, 64, 16, 1, ACT_SWIGLU, 0, 0, 0),      # ... its gate|up
         (256, 32, 8, 0, ACT_NONE, 1, 1, 1),         # ... its down / projection: 8 k-tiles, 4 waves, two k-tiles per chunk
         (256, 48, 16, 0, ACT_NONE, 0, 1, 1),
         (160, 32, 4, 1, ACT_NONE, 0, 1, 0)]         # 5 k-tiles over 4 waves: waves with one and with two tiles
_REAL = [(1024, 64, 16, 1, ACT_NONE, 0, 0, 0),       # cp q|k|v: norm, EXACT, four chunks of 1
         (2048, 32, 4, 0, ACT_NONE, 0, 1, 1),        # cp o-projection: residual + shadow, 4-feature strips, EXACT chunks of 2
         (2048, 32, 16, 0, ACT_NONE, 1, 1, 1),       # ... in 16-feature strips (chunks of 1)
         (1024, 64, 16, 1, ACT_SWIGLU, 0, 0, 0),     # cp gate|up: strip pairs
         (3072, 32, 8, 0, ACT_NONE, 0, 1, 1)]        # cp down: residual + shadow, six chunks of 2
_ROWS = [65, 80, 96, 127, 128]


def _reference(x, W, gw, bias, res, K, norm, act, bf16):
    M, N = x.shape[0], W.shape[0]
    Wf = W * gw if norm else W
    xv = x[:, :K]
    if bf16:
        Wf, xv = _bf16_round(Wf)[0], _bf16_round(xv)[0]
    acc = xv.astype(np.float64) @ Wf.astype(np.float64).T
    if norm:
        acc *= 1 / np.sqrt((xv.astype(np.float64) ** 2).mean(1, keepdims=True) + 1e-6)
    if bias is not None:
        acc += bias
    if act == ACT_SWIGLU:
        a = acc.reshape(M, N // 32, 2, 16)
        acc = ((a[:, :, 0] / (1 + np.exp(-a[:, :, 0]))) * a[:, :, 1]).reshape(M, N // 2)
    return acc + res if res is not None else acc


def _launch(emu, bf16, x, W, gw, bias, res, K, norm, act, fs, shadow, rows=slice(None)):
    """One launch_skinny call on rows `rows` of the problem; returns (out, out16) with 4 guard columns."""
    xs = np.ascontiguousarray(x[rows])
    rs = np.ascontiguousarray(res[rows]) if res is not None else None
    M, N = xs.shape[0], W.shape[0]
    No = N // 2 if act == ACT_SWIGLU else N
    out = np.full((M, No + 4), 7.0, np.float32)
    out16 = np.full((M, No + 4), 0x4242, np.uint16)
    if bf16:
        rc = emu.hostemu_skinny_bf16x(_ptr(xs), xs.shape[1], M, _ptr(W), N, K, _ptr(gw) if norm else None, norm, 1e-6,
                                      _ptr(bias) if bias is not None else None, _ptr(rs) if rs is not None else None, No, act, _ptr(out), No + 4, fs,
                                      out16.ctypes.data_as(C.c_void_p) if shadow else None)
    else:
        rc = emu.hostemu_skinny(_ptr(xs), xs.shape[1], M, _ptr(W), N, K, _ptr(gw) if norm else None, norm, 1e-6,
                                _ptr(bias) if bias is not None else None, _ptr(rs) if rs is not None else None, No, act, _ptr(out), No + 4, 0)
    assert rc == 0, ((M, N, K, fs, bf16), (emu.qtts_last_error() or b"").decode())
    return out, out16


@pytest.mark.parametrize("bf16", [1, 0])
@pytest.mark.parametrize("shapes", ["tiny", "real"])
def test_skinny_65_to_128_rows_real_source(emu, qopt, bf16, shapes):
    """The decode GEMM at M = 65, 80, 96, 127, 128 rows -- bf16: skinny_wide_kernel on the bf16 copy of x (8 m-tiles, RMSNorm statistic on
    the matrix pipe, SwiGLU strip pairs, bias, residual, bf16 shadow output), fp32: the generic kernel's 8-tile form -- against float64
    numpy with skinny2_kernel's bounds (2e-3 x max(1, |ref|max), shadow within 8e-3 of the fp32 output; fp32 mode: 2e-5), at the tiny
    engine's pass-0 shapes (tail-guarded instantiations) and the released code predictor's K (the branch-free EXACT instantiations).
    Every row is bit-identical to the same row computed in two launches of <= 64 rows on the existing kernels, to the library's own
    fallback (QTTS_SKINNY_WIDE=0), and under three wave scheduling orders; nothing is written outside the rows and columns."""
    g = np.random.default_rng(640 + 2 * bf16 + (shapes == "real"))
    cases = _TINY if shapes == "tiny" else _REAL
    if not bf16:                                            # (the fp32 kernel: 16-feature strips only, no bf16 shadow)
        cases = list(dict.fromkeys((K, N, 16, norm, act, hb, hr, 0) for (K, N, fs, norm, act, hb, hr, sh) in cases))
    for (K, N, fs, norm, act, hb, hr, sh) in cases:
        for M in _ROWS:
            x = (g.standard_normal((M, K + 8)) * 0.7).astype(np.float32)
            W = (g.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
            gw = (1 + 0.1 * g.standard_normal(K)).astype(np.float32) if norm else None
            bias = g.standard_normal(N).astype(np.float32) if hb else None
            No = N // 2 if act == ACT_SWIGLU else N
            res = g.standard_normal((M, No)).astype(np.float32) if hr else None
            ref = _reference(x, W, gw, bias, res, K, norm, act, bf16)
            tag = (bf16, M, N, K, fs, norm, act)
            args = (emu, bf16, x, W, gw, bias, res, K, norm, act, fs, sh)
            runs = []
            for order in (0, 1, 2):
                emu.hostemu_set_fiber_order(order)
                try:
                    runs.append(_launch(*args))
                finally:
                    emu.hostemu_set_fiber_order(0)
            out, out16 = runs[0]
            err = float(np.abs(out[:, :No] - ref).max())
            assert err <= (2e-3 if bf16 else 2e-5) * max(1.0, float(np.abs(ref).max())), (tag, err)
            assert np.all(out[:, No:] == 7.0), (tag, "wrote outside its columns")
            if sh:
                got = (out16[:, :No].astype(np.uint32) << 16).view(np.float32)
                assert np.abs(got - out[:, :No]).max() <= 8e-3 * max(1.0, float(np.abs(out).max())), (tag, "bf16 shadow differs from the fp32 output")
                assert np.all(out16[:, No:] == 0x4242), tag
            for o, o16 in runs[1:]:
                assert np.array_equal(o, out) and np.array_equal(o16, out16), (tag, "depends on the wave scheduling order")
            # the same rows on the existing <= 64-row kernels (both parts above 8 rows: the batch <= 8 kernels deal k-tile PAIRS to the
            # waves -- skinny.hip: skinny8_kernel, skinny8_f32_kernel -- which is another summation order by design)
            cut = 64 if M - 64 > 8 else 48
            lo, lo16 = _launch(*args, rows=slice(0, cut))
            hi, hi16 = _launch(*args, rows=slice(cut, M))
            assert np.array_equal(out, np.concatenate([lo, hi])), (tag, "differs from two launches of <= 64 rows")
            assert np.array_equal(out16, np.concatenate([lo16, hi16])), tag
            # ... and the library's own fallback
            qopt(emu, "QTTS_SKINNY_WIDE", "0")
            try:
                off, off16 = _launch(*args)
            finally:
                qopt(emu, "QTTS_SKINNY_WIDE", None)
            assert np.array_equal(out, off) and np.array_equal(out16, off16), (tag, "QTTS_SKINNY_WIDE=0 differs")


def test_skinny_refuses_more_than_128_rows(emu):
    x = np.zeros((129, 64), np.float32)
    W = np.zeros((16, 64), np.float32)
    out = np.zeros((129, 16), np.float32)
    rc = emu.hostemu_skinny(_ptr(x), 64, 129, _ptr(W), 16, 64, None, 0, 1e-6, None, None, 16, ACT_NONE, _ptr(out), 16, 1)
    assert rc == QTTS_ERR_LIMIT


# ============================================================================================ the engine on the emulator
@pytest.mark.parametrize("use_graph", [0, 1])
@pytest.mark.parametrize("name", ["b64", "b40"])
def test_talker_engine_fp32_64_and_40_rows_vs_reference(emu, golden_dir, name, use_graph):
    """The talker engine's C++ at 64 and 40 ragged rows (pass 0 of the code predictor: 128 / 80 rows), fp32, eager and through the
    captured frame graph: all 9 frames of the REFERENCE's greedy run, bit for bit (no cb-0 margin of these fixtures is below 1e-3, so
    the comparison rule cannot stop early -- and all 9 frames must have been compared)."""
    g, t, w, args = fixture(golden_dir, name)
    B = g["codes"].shape[0]
    h = _talker_emu(emu, t, w, max_batch=B, max_seq=64, use_graph=use_graph)
    try:
        codes, tokens, _ = _talker_generate(emu, h, t, *args, max_new=10, min_new=10)
        assert codes.shape == (B, 9, 16) and g["codes"].shape == (B, 9, 16)
        assert compare_greedy(codes, tokens, g["codes"], g["tokens"], g["margin"]) == 9
        if use_graph:
            assert _stats(emu, h).graph_nodes > 0
    finally:
        emu.qtts_talker_destroy(h)


@pytest.mark.parametrize("B", [40, 64])
def test_talker_engine_bf16_one_call_equals_two_half_calls(emu, qopt, B):
    """bf16, greedy, 6 tokens: B = 40 (64) rows in one call give exactly the codes of two calls of 20 (32) rows with the same left
    padding -- a row's sums do not depend on how many rows travel with it, through the 8-tile kernel, the 4- and 2-tile kernels.
    (ks-split regroups fp32 sums at 17..32 rows where it has an instantiation: off.)"""
    t = synth.talker_tiny()
    w = {k: torch.from_numpy(v) for k, v in synth.talker_weights(t, with_text=False).items()}
    e, m, tr, pad = split_prompt(t, 70 + B, B // 2)
    qopt(emu, "QTTS_SKINNY_KS", "0")
    h = _talker_emu(emu, t, w, max_batch=B, max_seq=64, dtype=_lib.QTTS_BF16)
    emu.hostemu_set_real_gemm(1)
    try:
        whole, wtok, _ = _talker_generate(emu, h, t, e, m, tr, pad, max_new=6, min_new=6)
        assert whole.shape == (B, 5, 16)
        for half in (slice(0, B // 2), slice(B // 2, B)):
            part, ptok, _ = _talker_generate(emu, h, t, e[half], m[half], tr[half], pad, max_new=6, min_new=6)
            assert np.array_equal(part, whole[half]) and np.array_equal(ptok, wtok[half])
    finally:
        from test_hostemu import FULL
        emu.hostemu_set_real_gemm(1 if FULL else 0)
        emu.qtts_talker_destroy(h)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_skinny_wide_option_changes_nodes_not_results(emu, golden_dir, qopt, dtype):
    """QTTS_SKINNY_WIDE on against off (pass 0's GEMMs as two launches of <= 64 rows): codes and hidden states bit-identical in bf16
    and fp32; the captured frame graph is smaller with the option on."""
    g, t, w, args = fixture(golden_dir, "b40")
    res = {}
    for flag in ("1", "0"):
        qopt(emu, "QTTS_SKINNY_WIDE", flag)
        h = _talker_emu(emu, t, w, max_batch=40, max_seq=64, dtype=_lib.QTTS_BF16 if dtype == "bf16" else None, use_graph=1)
        try:
            codes, tokens, hidden = _talker_generate(emu, h, t, *args, max_new=4, min_new=4)
            res[flag] = (codes, tokens, hidden, int(_stats(emu, h).graph_nodes))
        finally:
            emu.qtts_talker_destroy(h)
    on, off = res["1"], res["0"]
    assert on[0].shape == (40, 3, 16)
    assert np.array_equal(on[0], off[0]) and np.array_equal(on[1], off[1]) and np.array_equal(on[2], off[2])
    assert 0 < on[3] < off[3], (on[3], off[3])


@pytest.mark.parametrize("rows", [20, 8])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_engine_for_64_rows_called_with_fewer_makes_the_small_engines_launches(emu, dtype, rows):
    """An engine created with max_batch = 64 and called with 20 (8) rows returns the codes of an engine created with max_batch = 20 (8)
    and reports the same per-step statistics and graph size: the frame step's launches follow the live batch of the call."""
    t = synth.talker_tiny()
    w = {k: torch.from_numpy(v) for k, v in synth.talker_weights(t, with_text=False).items()}
    args = [x.numpy() for x in synth.rand_prompt(np.random.default_rng(81), t, [3 + (7 * i) % 13 for i in range(rows)], 2, scale=0.5)]
    res = []
    for mb in (64, rows):
        h = _talker_emu(emu, t, w, max_batch=mb, max_seq=64, dtype=_lib.QTTS_BF16 if dtype == "bf16" else None, use_graph=1)
        try:
            codes, tokens, hidden = _talker_generate(emu, h, t, *args, max_new=4, min_new=4)
            st = _stats(emu, h)
            res.append((codes, tokens, hidden, {k: getattr(st, k) for k in PER_STEP + ("graph_nodes",)}))
        finally:
            emu.qtts_talker_destroy(h)
    big, small = res
    assert np.array_equal(big[0], small[0]) and np.array_equal(big[1], small[1]) and np.array_equal(big[2], small[2])
    assert big[3] == small[3], (big[3], small[3])


def test_max_batch_limits_are_refused_with_the_range_named(emu):
    """max_batch 65 and 0 are refused at finalize with QTTS_ERR_LIMIT and a message that names 1..64; a 65-row call on a 64-row engine is
    refused too (QTTS_ERR_LIMIT from the engine; the Python wrapper's ValueError: tests/test_batch64_gpu.py)."""
    t = synth.talker_tiny()
    w = {k: torch.from_numpy(v) for k, v in synth.talker_weights(t, with_text=False).items()}
    for mb in (65, 0):
        with pytest.raises(AssertionError, match=r"max_batch must be 1\.\.64"):
            emu.qtts_talker_destroy(_talker_emu(emu, t, w, max_batch=mb, max_seq=32))
    h = _talker_emu(emu, t, w, max_batch=64, max_seq=32)
    try:
        emb, mask, tr, pad = [x.numpy() for x in synth.rand_prompt(np.random.default_rng(3), t, [4] * 65, 2, scale=0.5)]
        npad = (C.c_int32 * 65)(*([0] * 65))
        rc = emu.qtts_talker_prefill(h, _ptr(emb), 65, 4, npad, _ptr(tr), 2, _ptr(pad), None)
        assert rc == QTTS_ERR_LIMIT, rc
    finally:
        emu.qtts_talker_destroy(h)


def test_debug_cp_logits_is_packed_with_the_live_batch(emu, golden_dir):
    """qtts_talker_debug_cp_logits packs pass j at j x B x V with the LIVE batch: read with that B (as TalkerEngine.debug_cp_logits now
    allocates) on an engine created for more rows, every pass's argmax is the sub-codebook the engine itself chose in its last frame."""
    g, t, w, args = fixture(golden_dir, "b40")
    B, G, V = 12, t.num_code_groups, t.cp_vocab_size
    args = [args[0][:B], args[1][:B], args[2][:B], args[3]]
    h = _talker_emu(emu, t, w, max_batch=40, max_seq=64)
    try:
        codes, _, _ = _talker_generate(emu, h, t, *args, max_new=3, min_new=3)
        emu.qtts_talker_debug_cp_logits.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        out = np.full((G - 1, B, V), np.nan, np.float32)
        assert emu.qtts_talker_debug_cp_logits(h, _ptr(out), None) == 0
        assert np.isfinite(out).all()
        assert np.array_equal(out.argmax(-1).T, codes[:, -1, 1:])
    finally:
        emu.qtts_talker_destroy(h)

"""Opt-in FP8 (e4m3) weights for the talker's decode GEMMs, on the CPU: the library's quantizer against tests/fp8_ref.py, the fp8 forms
of skinny2_kernel / skinny8_kernel from their real source on the SIMT emulator (bitwise the bf16 kernels on d), and the engine identity
-- an engine with weight_format fp8 on W is, bit for bit, the bf16 engine on fp8.effective_state_dict(W).  Not marked `gpu`."""
import ctypes as C
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

import fp8_cases
import fp8_ref
import synth
from qwen3_tts_amd import _lib
from test_hostemu import emu, _ok, _ptr, _talker_generate  # noqa: F401  (`emu` is a fixture)

QTTS_ERR_ARG, QTTS_ERR_STATE = -1, -3


@pytest.fixture(scope="module")
def lib(emu):
    vp, i32 = C.c_void_p, C.c_int32
    emu.qtts_talker_set_weight_format.argtypes = [vp, i32]
    emu.qtts_talker_weight_format.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    emu.qtts_talker_debug_logits.argtypes = [vp, vp, vp]
    for f in ("qtts_talker_set_weight_format", "qtts_talker_weight_format", "qtts_talker_debug_logits"):
        getattr(emu, f).restype = C.c_int
    return fp8_cases.prototypes(emu)


def test_abi_is_additive():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qtts.h")).read()
    assert "#define QTTS_ABI_VERSION 15" in src and "#define QTTS_ERR_ARG (-1)" in src and "#define QTTS_ERR_STATE (-3)" in src
    for f in ("qtts_talker_set_weight_format", "qtts_talker_weight_format", "qtts_fp8_quantize_rows", "qtts_fp8_effective_rows", "qtts_debug_decode_gemm",
              "qtts_debug_last_decode_gemm_kernel"):
        assert f in src and f in _lib.SYMBOLS + _lib.SYMBOLS_FP8


# ============================================================================================ the quantizer
def _quantizer_inputs():
    g = np.random.default_rng(11)
    W = (g.standard_normal((40, 96)) * 0.02).astype(np.float32)
    W[3] = 0.0                                                           # an all-zero row
    W[5, 17] = np.float32(448.0 * 2.0 ** -9)                             # a row whose maximum is exactly 448 * 2^e
    allc = np.ldexp(fp8_ref.TABLE[fp8_ref.FINITE], -4).astype(np.float32)[None, :]    # a row that holds every finite code
    gw = (1 + 0.1 * g.standard_normal(96)).astype(np.float32)
    return W, gw, allc


def test_library_quantizer_equals_the_reference_code_for_code(lib):
    W, gw, allc = _quantizer_inputs()
    for w_, g_ in ((W, None), (W, gw), (allc, None)):
        codes, exps = fp8_cases.lib_quantize(lib, w_, g_)
        rc, re_ = fp8_ref.quantize_rows(w_, g_)
        assert np.array_equal(exps, re_), (exps, re_)
        assert np.array_equal(codes, rc), np.argwhere(codes != rc)[:5]
    codes, exps = fp8_cases.lib_quantize(lib, W)
    assert exps[3] == 0 and not codes[3].any()
    assert exps[5] == -9 and codes[5, 17] == 0x7e
    codes, exps = fp8_cases.lib_quantize(lib, allc)
    assert exps[0] == -4 and np.array_equal(codes[0], fp8_ref.FINITE)


def test_library_effective_rows_is_d_over_g_with_a_zero_in_g(lib):
    W, gw, _ = _quantizer_inputs()
    gw = gw.copy()
    gw[9] = 0.0
    eff = fp8_cases.lib_effective(lib, W, gw)
    assert np.array_equal(eff.view(np.uint32), fp8_ref.effective_rows(W, gw).view(np.uint32))
    assert np.array_equal(eff[:, 9], W[:, 9])
    assert np.array_equal(fp8_cases.lib_effective(lib, W), fp8_ref.dequantize(*fp8_ref.quantize_rows(W)))


# ============================================================================================ the kernels
@pytest.mark.parametrize("case", fp8_cases.SKINNY2, ids=lambda c: "x".join(map(str, c[:4])))
def test_skinny2_fp8_is_bitwise_the_bf16_kernel_on_d(lib, case):
    fp8_cases.check_case(lib, case, seed=sum(case))


@pytest.mark.parametrize("case", fp8_cases.SKINNY8, ids=lambda c: "x".join(map(str, c[:4])) + f"a{c[5]}")
def test_skinny8_fp8_is_bitwise_the_bf16_kernel_on_d(lib, case):
    fp8_cases.check_case(lib, case, seed=sum(case))


@pytest.mark.parametrize("case", [fp8_cases.SKINNY2[2], fp8_cases.SKINNY8[5]], ids=["skinny2", "skinny8"])
def test_fp8_kernels_do_not_depend_on_the_wave_scheduling_order(lib, case):
    runs = []
    for order in (0, 1, 2):
        lib.hostemu_set_fiber_order(order)
        try:
            runs.append(fp8_cases.check_case(lib, case, seed=3))
        finally:
            lib.hostemu_set_fiber_order(0)
    for o, s in runs[1:]:
        assert np.array_equal(o.view(np.uint32), runs[0][0].view(np.uint32)) and np.array_equal(s, runs[0][1])


def test_every_finite_code_through_each_conversion_path(lib):
    fp8_cases.all_codes_skinny2(lib)
    fp8_cases.all_codes_skinny8(lib, 16)
    fp8_cases.all_codes_skinny8(lib, 8)


def test_fp8_launch_refuses_what_it_is_not_built_for(lib):
    x = np.zeros((4, 64), np.float32)
    W = np.zeros((16, 64), np.float32)
    out = np.zeros((4, 20), np.float32)
    rc = lib.qtts_debug_decode_gemm(_ptr(x), _ptr(W), None, None, None, 4, 16, 64, 16, 0, 0, 7, 20, _ptr(out), None)
    assert rc == QTTS_ERR_ARG and b"format" in lib.qtts_last_error()


# ============================================================================================ the engine
def _mid():
    """Every talker GEMM on skinny8_kernel (K = 1024), ACT_SWIGLU8 included."""
    return dataclasses.replace(synth.talker_tiny(), hidden_size=1024, intermediate_size=1024, num_attention_heads=8, num_key_value_heads=4)


def _weights(t):
    return {k: torch.from_numpy(v) for k, v in synth.talker_weights(t, with_text=False).items()}


@pytest.fixture(scope="module")
def shim(emu):
    """The product's Python layer on the emulation library (fp8.effective_state_dict goes through _lib.load_library())."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostemu"))
    import pyshim
    pyshim.install()
    yield
    pyshim.uninstall()


_EFF = {}


def _effective(shim, name, t, w):
    if name not in _EFF:
        from qwen3_tts_amd import fp8
        _EFF[name] = fp8.effective_state_dict(synth.cfg_dict(t), w)
    return _EFF[name]


def _engine(lib, t, w, max_batch, fmt=None, dtype=_lib.QTTS_BF16, use_graph=0, max_seq=48, expect=0):
    """create -> [set_weight_format(fmt)] -> bind -> finalize; `expect`: the setter's return code (a refusal destroys the handle)."""
    from test_hostemu import _talker_emu
    vp = C.c_void_p
    from qwen3_tts_amd.config import TalkerConfig
    c = TalkerConfig.from_any(synth.cfg_dict(t))
    tc = _lib.TalkerConfigC()
    for f in ("vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "num_key_value_heads",
              "head_dim", "num_code_groups", "text_hidden_size", "codec_eos_token_id", "cp_vocab_size", "cp_hidden_size",
              "cp_intermediate_size", "cp_num_hidden_layers", "cp_num_attention_heads", "cp_num_key_value_heads", "cp_head_dim"):
        setattr(tc, f, int(getattr(c, f)))
    tc.rms_norm_eps, tc.rope_theta = float(c.rms_norm_eps), float(c.rope_theta)
    tc.cp_rms_norm_eps, tc.cp_rope_theta = float(c.cp_rms_norm_eps), float(c.cp_rope_theta)
    tc.weight_dtype, tc.max_batch, tc.max_seq, tc.use_graph = dtype, max_batch, max_seq, use_graph
    if fmt is None and expect == 0:
        return _talker_emu(lib, t, w, max_batch, max_seq, dtype, use_graph)          # (an engine that never called the setter)
    h = vp()
    _ok(lib, lib.qtts_talker_create(C.byref(tc), C.byref(h)))
    rc = lib.qtts_talker_set_weight_format(h, fmt)
    if rc != expect or rc != 0:
        msg = (lib.qtts_last_error() or b"").decode()
        lib.qtts_talker_destroy(h)
        assert rc == expect, (rc, msg)
        return msg
    for name, x in w.items():
        _lib.bind_tensor(lib.qtts_talker_bind, h, name, x)
    _ok(lib, lib.qtts_talker_finalize(h))
    return h


def _run(lib, h, t, prompt, frames):
    codes, tokens, hidden = _talker_generate(lib, h, t, *prompt, max_new=frames + 1, min_new=frames + 1)
    B = prompt[0].shape[0]
    logits = np.full((B, t.vocab_size), np.nan, np.float32)
    _ok(lib, lib.qtts_talker_debug_logits(h, _ptr(logits), None))
    assert codes.shape[1] == frames and np.isfinite(logits).all()
    return codes, tokens, hidden, logits


def _packed_bytes(lib, h):
    fmt, n = C.c_int32(-1), C.c_int64(-1)
    _ok(lib, lib.qtts_talker_weight_format(h, C.byref(fmt), C.byref(n)))
    return int(fmt.value), int(n.value)


def _fp8_ops(t, max_batch):
    """(N, K) of every fp8 operator of the talker stack."""
    H, I = t.hidden_size, t.intermediate_size
    qd, kvd = t.num_attention_heads * t.head_dim, t.num_key_value_heads * t.head_dim
    ops = [(qd + 2 * kvd, H), (H, qd), (2 * I, H), (H, I)]
    if (max_batch <= 8 or max_batch > 32) and H in (1024, 2048, 3072, 6144):
        ops.append((2 * I, H))                                                       # the ACT_SWIGLU8 copy of gate|up
    return ops * t.num_hidden_layers


@pytest.mark.parametrize("name,rows,frames,use_graph", [("tiny", 2, 8, 0), ("tiny", 2, 8, 1), ("mid", 2, 3, 0), ("mid", 2, 3, 1), ("tiny", 20, 3, 0)])
def test_fp8_engine_is_the_bf16_engine_of_the_effective_checkpoint(lib, shim, name, rows, frames, use_graph):
    """Greedy, ragged prompt: codes, tokens, hidden rows and the logits after the last step are identical.  20 rows: two m-tiles of
    skinny2_fp8_kernel, no split-K."""
    t = synth.talker_tiny() if name == "tiny" else _mid()
    w = _weights(t)
    lens = [7, 4] if rows == 2 else [3 + (5 * i) % 9 for i in range(rows)]
    prompt = [x.numpy() for x in synth.rand_prompt(np.random.default_rng(21 + rows), t, lens, 2, scale=0.5 if name == "tiny" else 0.05)]
    mb = 4 if rows == 2 else rows
    res = []
    for sd, fmt in ((w, 1), (_effective(shim, name, t, w), 0)):
        h = _engine(lib, t, sd, mb, fmt=fmt, use_graph=use_graph)
        try:
            res.append(_run(lib, h, t, prompt, frames) + (_packed_bytes(lib, h),))
        finally:
            lib.qtts_talker_destroy(h)
    a, b = res
    for i, what in enumerate(("codes", "tokens", "hidden", "logits")):
        assert np.array_equal(a[i], b[i]), (what, name, rows)
    assert a[4][0] == 1 and b[4][0] == 0
    assert a[4][1] == b[4][1] - sum(N * K - 4 * N for N, K in _fp8_ops(t, mb)), (a[4], b[4])


def test_format_0_set_explicitly_is_the_engine_that_never_called_the_setter(lib):
    t = synth.talker_tiny()
    w = _weights(t)
    prompt = [x.numpy() for x in synth.rand_prompt(np.random.default_rng(22), t, [7, 4], 2, scale=0.5)]
    res = []
    for fmt in (0, None):
        h = _engine(lib, t, w, 4, fmt=fmt, use_graph=1)
        try:
            res.append(_run(lib, h, t, prompt, 4) + (_packed_bytes(lib, h),))
        finally:
            lib.qtts_talker_destroy(h)
    for i in range(5):
        assert np.array_equal(res[0][i], res[1][i]), i


def test_setter_refusals(lib):
    t = synth.talker_tiny()
    w = _weights(t)
    msg = _engine(lib, t, w, 4, fmt=1, dtype=_lib.QTTS_F32, expect=QTTS_ERR_ARG)
    assert "bf16 engine" in msg
    msg = _engine(lib, t, w, 4, fmt=3, expect=QTTS_ERR_ARG)
    assert "unknown format" in msg
    h = _engine(lib, t, w, 4, fmt=None)
    try:
        assert lib.qtts_talker_set_weight_format(h, 1) == QTTS_ERR_STATE
        assert b"after finalize" in lib.qtts_last_error()
    finally:
        lib.qtts_talker_destroy(h)


def test_python_surface(shim):
    """TalkerEngine(weight_format=): plain ValueErrors before anything is created; fp8.quantize_rows / effective_weight over the library."""
    from qwen3_tts_amd import TalkerEngine, fp8
    t = synth.talker_tiny()
    w = _weights(t)
    with pytest.raises(ValueError, match="None or 'fp8'"):
        TalkerEngine(synth.cfg_dict(t), w, weight_format="int4")
    with pytest.raises(ValueError, match="bf16 engine"):
        TalkerEngine(synth.cfg_dict(t), w, weight_dtype=torch.float32, weight_format="fp8")
    eng = TalkerEngine(synth.cfg_dict(t), w, max_batch=4, max_seq=32, weight_format="fp8")
    ref = TalkerEngine(synth.cfg_dict(t), w, max_batch=4, max_seq=32)
    assert eng.packed_weight_bytes == ref.packed_weight_bytes - sum(N * K - 4 * N for N, K in _fp8_ops(t, 4))
    W = w["model.layers.0.self_attn.q_proj.weight"]
    g = w["model.layers.0.input_layernorm.weight"]
    codes, exps = fp8.quantize_rows(W, g)
    rc, re_ = fp8_ref.quantize_rows(W.numpy(), g.numpy())
    assert np.array_equal(codes.numpy(), rc) and np.array_equal(exps.numpy(), re_)
    sd = fp8.effective_state_dict(synth.cfg_dict(t), w)
    assert set(sd) == set(w)
    changed = {k for k in w if not torch.equal(sd[k].float(), w[k].float())}
    assert changed == {f"model.layers.{l}.{m}.weight" for l in range(t.num_hidden_layers)
                       for m in ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")}
    assert np.array_equal(sd["model.layers.0.self_attn.q_proj.weight"].numpy(), fp8_ref.effective_rows(W.numpy(), g.numpy()))
    pref = fp8.effective_state_dict(synth.cfg_dict(t), {"talker." + k: v for k, v in w.items()})
    assert all(torch.equal(pref["talker." + k], sd[k]) for k in sd)

"""FP8 weights at batch 17..32 on the CPU: skinny2_ks_fp8_kernel (the fp8 form of the split-K decode GEMM) from its real source on the
SIMT emulator -- bitwise the bf16 split-K kernel on d in its four instantiations, under three wave scheduling orders -- and the engine
identity where the o- and down-projections split: an fp8 engine on W is, bit for bit, the bf16 engine on fp8.effective_state_dict(W),
with QTTS_SKINNY_KS_FP8=0 as the control.  Not marked `gpu`."""
import ctypes as C
import os

import numpy as np
import pytest

import fp8_ks_cases as ks
import synth
from qwen3_tts_amd import _lib
from test_hostemu import emu, _ok  # noqa: F401  (`emu` is a fixture)
from test_fp8_weights_hostemu import shim, _effective, _engine, _run, _weights  # noqa: F401  (`shim` is a fixture)


@pytest.fixture(scope="module")
def lib(emu):
    vp, i32 = C.c_void_p, C.c_int32
    emu.qtts_talker_set_weight_format.argtypes = [vp, i32]
    emu.qtts_talker_weight_format.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    emu.qtts_talker_debug_logits.argtypes = [vp, vp, vp]
    emu.qtts_talker_get_stats.argtypes = [vp, C.POINTER(_lib.TalkerStatsC)]
    for f in ("qtts_talker_set_weight_format", "qtts_talker_weight_format", "qtts_talker_debug_logits", "qtts_talker_get_stats"):
        getattr(emu, f).restype = C.c_int
    return ks.prototypes(emu)


def test_the_hook_is_declared_and_the_abi_version_stays():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qtts.h")).read()
    assert "#define QTTS_ABI_VERSION 15" in src
    assert "qtts_debug_decode_gemm_ks(" in src and "qtts_debug_decode_gemm_ks" in _lib.SYMBOLS


# ============================================================================================ the kernel
@pytest.mark.parametrize("case", ks.CASES, ids=ks.IDS)
def test_fp8_split_k_is_bitwise_the_bf16_split_k_kernel_on_d(lib, case):
    ks.check_case(lib, case)


@pytest.mark.parametrize("case", ks.CASES, ids=ks.IDS)
def test_fp8_split_k_does_not_depend_on_the_wave_scheduling_order(lib, case):
    runs = []
    for order in (0, 1, 2):
        lib.hostemu_set_fiber_order(order)
        try:
            runs.append(ks.check_bitwise(lib, case, serial=11 + order))
        finally:
            lib.hostemu_set_fiber_order(0)
    for o, s in runs[1:]:
        assert np.array_equal(o.view(np.uint32), runs[0][0].view(np.uint32)) and np.array_equal(s, runs[0][1])


@pytest.mark.parametrize("shape", ks.ALL_CODES, ids=lambda s: "x".join(map(str, s)))
def test_every_finite_code_through_the_split_path(lib, shape):
    ks.all_codes(lib, *shape)


def test_shapes_outside_the_split_keep_the_unsplit_fp8_kernel(lib):
    ks.not_split(lib)


# ============================================================================================ the engine
def _stats(lib, h):
    st = _lib.TalkerStatsC()
    _ok(lib, lib.qtts_talker_get_stats(h, C.byref(st)))
    return st


def test_fp8_engine_is_the_bf16_engine_of_the_effective_checkpoint_where_k_splits(lib, shim):
    """18 rows, ragged prompt, 3 greedy frames, captured graph, K floor 2048: the o- and down-projections of both talker layers split in
    either engine (`ks_split_per_step`), and codes, tokens, hidden rows and the last logits are identical.  QTTS_SKINNY_KS_FP8=0: the fp8
    engine's talker operators keep skinny2_fp8_kernel -- the counter drops by 2 per layer, the hidden rows are another fp32 grouping of the
    same products.  A second generation on the same handle repeats the first bit for bit."""
    t = ks.engine_config()
    w = _weights(t)
    weff = _effective(shim, "ks", t, w)
    prompt = [x.numpy() for x in synth.rand_prompt(np.random.default_rng(21 + ks.ENGINE_ROWS), t, ks.ENGINE_LENS, 2, scale=0.05)]
    L = t.num_hidden_layers
    res = {}
    for name, sd, fmt, fp8_split in (("fp8", w, 1, None), ("bf16", weff, 0, None), ("fp8_unsplit", w, 1, "0")):
        with ks.options(lib, QTTS_SKINNY_KS_MINK=ks.MINK, QTTS_SKINNY_KS_FP8=fp8_split):
            h = _engine(lib, t, sd, ks.ENGINE_ROWS, fmt=fmt, use_graph=1)
            try:
                res[name] = _run(lib, h, t, prompt, ks.ENGINE_FRAMES) + (_stats(lib, h).ks_split_per_step,)
                assert _stats(lib, h).cp_fused_giveups == 0
                if name == "fp8":
                    again = _run(lib, h, t, prompt, ks.ENGINE_FRAMES)
                    for i, what in enumerate(("codes", "tokens", "hidden", "logits")):
                        assert np.array_equal(again[i], res[name][i]), ("second generation", what)
            finally:
                lib.qtts_talker_destroy(h)
    a, b, u = res["fp8"], res["bf16"], res["fp8_unsplit"]
    print("ks_split_per_step: fp8", a[4], "bf16 on W_eff", b[4], "fp8 with QTTS_SKINNY_KS_FP8=0", u[4])
    assert a[4] == b[4] and a[4] >= 2 * L, (a[4], b[4])
    for i, what in enumerate(("codes", "tokens", "hidden", "logits")):
        assert np.array_equal(a[i], b[i]), (what, "fp8 engine differs from the bf16 engine on the effective checkpoint")
    assert u[4] == a[4] - 2 * L, (u[4], a[4])
    assert not np.array_equal(a[2], u[2]), "QTTS_SKINNY_KS_FP8=0 did not select another kernel"
    dh = float(np.abs(a[2] - u[2]).max())
    print(f"|hidden split - unsplit|max {dh:.3e} (bound {3e-2 * max(1.0, float(np.abs(u[2]).max())):.3e})")
    assert dh <= 3e-2 * max(1.0, float(np.abs(u[2]).max())), dh

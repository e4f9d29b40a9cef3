"""Kernel cases of the fp8 split-K decode GEMM (skinny.hip: skinny2_ks_fp8_kernel, batch 17..32), shared by the emulator tests
(tests/test_fp8_ks_hostemu.py) and the hardware tests (tests/test_fp8_ks_gpu.py): both drive `qtts_debug_decode_gemm_ks` (include/qtts.h)
of the library they are given, with the K floor of the split lowered to 2048 through the option table.

The pin: an fp8 split launch is BITWISE the bf16 split launch on d = code * 2^e -- fp32 rows and bf16 shadow -- within the decode-GEMM
family's bound of float64 NumPy on d (2e-3 * max(1, |ref|max)), and within fp32 regrouping (2e-5 * max(1, |ref|max), not zero) of the
unsplit fp8 launch."""
import ctypes as C

import numpy as np

import fp8_cases
import fp8_ref
from qwen3_tts_amd import _lib
from fp8_cases import FMT_BF16, FMT_FP8, KERNEL_2, KERNEL_FP8, _p

KERNEL_KS = 4                                     # qtts_debug_last_decode_gemm_kernel: the split-K family
MINK = "2048"

# (M, N, K, fs, bias, res, shadow): the smallest shapes skinny.hip's ksplit_choice maps to each of the four instantiations (4 parts need
# N >= 2048, 8 parts take N = 32)
CASES = [(32, 2048, 6144, 8, 0, 1, 1),            # <4, 8, 8, 6, 4>: the talker's down-projection at 1.7B
         (19, 32, 3072, 8, 1, 1, 1),              # <4, 8, 4, 3, 8>: ragged second m-tile, bias
         (17, 2048, 2048, 16, 0, 1, 0),           # <2, 16, 8, 2, 4>: tile pairs, one row in m-tile 1
         (25, 32, 2048, 8, 0, 0, 1)]              # <4, 8, 8, 1, 8>: no residual
IDS = ["x".join(map(str, c[:4])) for c in CASES]


def prototypes(lib):
    vp, i32 = C.c_void_p, C.c_int32
    fp8_cases.prototypes(lib)
    lib.qtts_debug_decode_gemm_ks.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, i32, i32]
    lib.qtts_debug_decode_gemm_ks.restype = C.c_int
    return lib


def options(lib, **kw):
    """A/B switches of `lib` through its option table for a `with` block (None: the default)."""
    return _lib.options(lib, **kw)


def gemm_ks(lib, x, W, bias, res, fs, fmt, shadow, launches=1, serial=5):
    """`launches` launches on one workspace; returns (out, out16, family) with 4 guard columns and a guard row M (7.0 / 0x4242 where the
    kernel must not write)."""
    M, K = x.shape
    N = W.shape[0]
    ldo = N + 4
    out = np.full((M + 1, ldo), 7.0, np.float32)
    out16 = np.full((M + 1, ldo), 0x4242, np.uint16)
    rs = None
    if res is not None:
        rs = np.zeros((M, ldo), np.float32)
        rs[:, :N] = res
    x, W = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(W, np.float32)
    rc = lib.qtts_debug_decode_gemm_ks(_p(x), _p(W), None, _p(bias), _p(rs), M, N, K, fs, fmt, ldo, _p(out), _p(out16) if shadow else None,
                                       launches, serial)
    assert rc == 0, ((M, N, K, fs, fmt, launches, serial), (lib.qtts_last_error() or b"").decode())
    kind = C.c_int32(-1)
    assert lib.qtts_debug_last_decode_gemm_kernel(C.byref(kind)) == 0
    return out, out16, kind.value


_CASE = {}


def case_data(case):
    """(x, W, bias, res, d, ref) of a case: built once, shared by the tests, never modified."""
    if case not in _CASE:
        M, N, K, fs, hb, hr, sh = case
        x, W, _, bias, res = fp8_cases.make_case((M, N, K, fs, 0, fp8_cases.ACT_NONE, hb, hr, sh), seed=sum(case))
        d = fp8_ref.dequantize(*fp8_ref.quantize_rows(W))
        ref = fp8_cases.reference(x, d, bias, res, 0, fp8_cases.ACT_NONE)
        for a in (x, W, bias, res, d, ref):
            if a is not None:
                a.setflags(write=False)
        _CASE[case] = (x, W, bias, res, d, ref)
    return _CASE[case]


def _same(a, b):
    return np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])


def check_bitwise(lib, case, serial=5):
    """fp8 split launch == bf16 split launch on d, bitwise (fp32 rows, shadow, guards); the families say both split.  Returns the fp8 pair."""
    M, N, K, fs, hb, hr, sh = case
    x, W, bias, res, d, ref = case_data(case)
    with options(lib, QTTS_SKINNY_KS_MINK=MINK):
        o8 = gemm_ks(lib, x, W, bias, res, fs, FMT_FP8, sh, 1, serial)
        ob = gemm_ks(lib, x, d, bias, res, fs, FMT_BF16, sh, 1, serial)
    assert o8[2] == KERNEL_KS | KERNEL_FP8 and ob[2] == KERNEL_KS, (case, "ran on kernel families", o8[2], ob[2])
    assert np.array_equal(o8[0].view(np.uint32), ob[0].view(np.uint32)), (case, "fp8 split launch differs from the bf16 split launch on d",
                                                                            float(np.abs(o8[0] - ob[0]).max()))
    assert np.array_equal(o8[1], ob[1]), (case, "bf16 shadow differs")
    return o8[:2]


def check_case(lib, case):
    """Everything the split fp8 launch of a case must satisfy (module docstring), plus: two launches on one workspace and another serial
    give the same bits; rows >= M and columns >= N untouched."""
    M, N, K, fs, hb, hr, sh = case
    x, W, bias, res, d, ref = case_data(case)
    o8 = check_bitwise(lib, case)
    out, s16 = o8
    bound = max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(out[:M, :N] - ref).max())
    print(f"{case}: |fp8 split - float64 on d|max {err:.3e} (bound {2e-3 * bound:.3e})")
    assert err <= 2e-3 * bound, (case, err)
    assert np.all(out[:M, N:] == 7.0) and np.all(out[M] == 7.0), (case, "wrote outside its rows / columns")
    if sh:
        got = (s16[:M, :N].astype(np.uint32) << 16).view(np.float32)
        assert np.abs(got - out[:M, :N]).max() <= 8e-3 * max(1.0, float(np.abs(out[:M, :N]).max())), (case, "bf16 shadow differs from the fp32 output")
        assert np.all(s16[:M, N:] == 0x4242) and np.all(s16[M] == 0x4242), case
    else:
        assert np.all(s16 == 0x4242), case
    with options(lib, QTTS_SKINNY_KS_MINK=MINK):
        two = gemm_ks(lib, x, W, bias, res, fs, FMT_FP8, sh, 2, 5)
        again = gemm_ks(lib, x, W, bias, res, fs, FMT_FP8, sh, 1, 77)
    assert two[2] == again[2] == KERNEL_KS | KERNEL_FP8
    assert _same(two, o8), (case, "the second launch on the workspace differs from the first")
    assert _same(again, o8), (case, "another serial gives other bits")
    with options(lib, QTTS_SKINNY_KS_MINK=MINK, QTTS_SKINNY_KS="0"):
        un = gemm_ks(lib, x, W, bias, res, fs, FMT_FP8, sh, 1, 5)
    assert un[2] == KERNEL_2 | KERNEL_FP8, (case, "QTTS_SKINNY_KS=0 ran on kernel family", un[2])
    diff = float(np.abs(out[:M, :N] - un[0][:M, :N]).max())
    print(f"{case}: |split - unsplit|max {diff:.3e} (bound {2e-5 * bound:.3e})")
    assert 0.0 < diff <= 2e-5 * bound, (case, "split and unsplit sums differ by more than fp32 regrouping (or the split did not run)", diff)


# every finite code through the split path: (N, K, fs) and the k the 32 one-hot rows select -- every K part (4 parts of 512 / 8 parts of
# 256), several waves (tile % 8), every k-slice, and for fs = 16 both halves of a tile pair (even and odd tiles)
ALL_CODES = [(32, 2048, 8), (2048, 2048, 16)]


def all_codes(lib, N, K, fs):
    """x = 32 one-hot rows, so out[m][n] must be d[n][k_m] exactly.  k = 1 carries +-448, which fixes every row's exponent; the codes at
    the 32 selected k walk the 254 finite codes over every 8 consecutive rows (the construction of fp8_cases.all_codes_skinny8)."""
    M = 32
    ks = np.array([64 * m + 32 * (m % 2) + 8 * (m % 4) + (5 * m) % 8 for m in range(M)])      # tile 2 m + (m & 1), k-slice m % 4
    assert len(set(ks.tolist())) == M and 1 not in ks
    tiles = ks // 32
    parts = 4 if N >= 2048 else 8
    assert set((tiles // (K // 32 // parts)).tolist()) == set(range(parts)) and len(set((tiles % 8).tolist())) >= 2
    assert set((tiles % 2).tolist()) == {0, 1} and set(((ks % 32) // 8).tolist()) == {0, 1, 2, 3}
    codes = np.zeros((N, K), np.uint8)
    exps = (np.arange(N, dtype=np.int32) % 32) - 20
    flat = np.concatenate([fp8_ref.FINITE, fp8_ref.FINITE[:2]])              # 256 = 8 rows x 32 positions
    for n in range(N):
        codes[n, 1] = 0x7e if n % 2 else 0xfe
        codes[n, ks] = flat[(n % 8) * 32:(n % 8 + 1) * 32]
    assert set(codes[:8][:, ks].ravel().tolist()) == set(fp8_ref.FINITE.tolist())
    d = fp8_ref.dequantize(codes, exps)
    x = np.zeros((M, K), np.float32)
    x[np.arange(M), ks] = 1.0
    with options(lib, QTTS_SKINNY_KS_MINK=MINK):
        out, _, kind = gemm_ks(lib, x, d, None, None, fs, FMT_FP8, 0)
        outb, _, kindb = gemm_ks(lib, x, d, None, None, fs, FMT_BF16, 0)
    assert kind == KERNEL_KS | KERNEL_FP8 and kindb == KERNEL_KS, (kind, kindb)
    assert np.array_equal(out[:M, :N], d[:, ks].T), ((N, K, fs), "a code converts to another number")        # (by value: 0 + 1 x -0 is +0)
    assert np.array_equal(out.view(np.uint32), outb.view(np.uint32)), (N, K, fs)


def not_split(lib):
    """M = 16 and M = 33 at the down-projection's shape keep skinny2_fp8_kernel; so does a K below the default floor with the option unset."""
    g = np.random.default_rng(5)
    for (M, N, K, fs, opts) in [(16, 2048, 6144, 8, dict(QTTS_SKINNY_KS_MINK=MINK)), (33, 2048, 6144, 8, dict(QTTS_SKINNY_KS_MINK=MINK)),
                                (25, 32, 2048, 8, {})]:
        x = (g.standard_normal((M, K)) * 0.7).astype(np.float32)
        W = (g.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
        with options(lib, **opts):
            out, _, kind = gemm_ks(lib, x, W, None, None, fs, FMT_FP8, 0)
            ob, _, kindb = gemm_ks(lib, x, fp8_ref.dequantize(*fp8_ref.quantize_rows(W)), None, None, fs, FMT_BF16, 0)
        assert kind == KERNEL_2 | KERNEL_FP8 and kindb == KERNEL_2, ((M, N, K, fs), kind, kindb)
        assert np.array_equal(out.view(np.uint32), ob.view(np.uint32)) and np.all(out[M] == 7.0), (M, N, K, fs)


# ------------------------------------------------------------------------------------------------ the engine-level configuration
def engine_config():
    """hidden 1024, intermediate 3072, 16 query / 8 kv heads of 128: the o-projection (1024 x 2048) and the down-projection (1024 x 3072)
    are the two 8-part split shapes of the 1024-wide stacks (8-feature strips)."""
    import dataclasses

    import synth
    return dataclasses.replace(synth.talker_tiny(), hidden_size=1024, intermediate_size=3072, num_attention_heads=16, num_key_value_heads=8,
                               head_dim=128, num_hidden_layers=2)


ENGINE_ROWS, ENGINE_FRAMES = 18, 3
ENGINE_LENS = [3 + (5 * i) % 9 for i in range(ENGINE_ROWS)]

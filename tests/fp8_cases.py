"""Kernel cases of the fp8 decode GEMMs, shared by the emulator tests (tests/test_fp8_weights_hostemu.py) and the hardware tests
(tests/test_fp8_weights_gpu.py): both drive `qtts_debug_decode_gemm` (include/qtts.h) of the library they are given.

The pin: an fp8 launch is BITWISE the bf16 launch of the same call on d = code * 2^e (g omitted, the norm flag kept), and within the
decode-GEMM family's bound of float64 NumPy on d (2e-3 * max(1, |ref|max); the bf16 shadow within 8e-3 of the fp32 output)."""
import ctypes as C

import numpy as np

import fp8_ref

ACT_NONE, ACT_SWIGLU, ACT_SWIGLU8 = 0, 2, 5
FMT_BF16, FMT_FP8 = 0, 1

# (M, N, K, fs, norm, act, bias, res, shadow)
SKINNY2 = [(3, 48, 160, 16, 1, ACT_NONE, 1, 0, 0),        # odd number of k-tiles: guarded tail, a padded tile pair
           (8, 64, 128, 16, 1, ACT_SWIGLU, 0, 0, 0),
           (24, 32, 256, 8, 0, ACT_NONE, 1, 1, 1),        # two m-tiles
           (40, 32, 2048, 8, 1, ACT_NONE, 0, 1, 0),       # four m-tiles, EXACT
           (20, 32, 256, 4, 0, ACT_NONE, 0, 1, 0)]        # ragged second m-tile
SKINNY8 = [(5, 32, 2048, 8, 1, ACT_NONE, 1, 1, 1),
           (8, 32, 3072, 8, 0, ACT_NONE, 0, 1, 0),        # rotated weights
           (1, 64, 3072, 16, 1, ACT_SWIGLU, 0, 1, 0),
           (8, 48, 2048, 16, 0, ACT_NONE, 1, 0, 1),
           (8, 64, 2048, 16, 1, ACT_SWIGLU8, 0, 0, 0),
           (3, 48, 1024, 16, 1, ACT_SWIGLU8, 0, 1, 0),
           (8, 32, 6144, 8, 0, ACT_NONE, 1, 1, 0)]


def prototypes(lib):
    vp, i32 = C.c_void_p, C.c_int32
    lib.qtts_last_error.restype = C.c_char_p
    lib.qtts_debug_decode_gemm.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp]
    lib.qtts_fp8_quantize_rows.argtypes = [vp, vp, i32, i32, vp, vp]
    lib.qtts_fp8_effective_rows.argtypes = [vp, vp, i32, i32, vp]
    lib.qtts_debug_last_decode_gemm_kernel.argtypes = [C.POINTER(C.c_int32)]
    for f in ("qtts_debug_decode_gemm", "qtts_fp8_quantize_rows", "qtts_fp8_effective_rows", "qtts_debug_last_decode_gemm_kernel"):
        getattr(lib, f).restype = C.c_int
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def lib_quantize(lib, W, g=None):
    W = np.ascontiguousarray(W, np.float32)
    N, K = W.shape
    codes, exps = np.zeros((N, K), np.uint8), np.zeros(N, np.int32)
    rc = lib.qtts_fp8_quantize_rows(_p(W), _p(g), N, K, _p(codes), _p(exps))
    assert rc == 0, (lib.qtts_last_error() or b"").decode()
    return codes, exps


def lib_effective(lib, W, g=None):
    W = np.ascontiguousarray(W, np.float32)
    out = np.zeros_like(W)
    rc = lib.qtts_fp8_effective_rows(_p(W), _p(g), W.shape[0], W.shape[1], _p(out))
    assert rc == 0, (lib.qtts_last_error() or b"").decode()
    return out


KERNEL_2, KERNEL_8, KERNEL_FP8 = 2, 8, 16          # qtts_debug_last_decode_gemm_kernel


def gemm(lib, x, W, g, bias, res, fs, norm, act, fmt, shadow, kernel=None):
    """One launch; returns (out, out16) with 4 guard columns (7.0 / 0x4242 where the kernel must not write).  `kernel`: the family the
    launch must have run on (KERNEL_2 | KERNEL_8; the fp8 flag follows `fmt`)."""
    M, K = x.shape
    N = W.shape[0]
    No = N // 2 if act in (ACT_SWIGLU, ACT_SWIGLU8) else N
    ldo = No + 4
    out = np.full((M, ldo), 7.0, np.float32)
    out16 = np.full((M, ldo), 0x4242, np.uint16)
    rs = None
    if res is not None:
        rs = np.zeros((M, ldo), np.float32)
        rs[:, :No] = res
    x, W = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(W, np.float32)
    rc = lib.qtts_debug_decode_gemm(_p(x), _p(W), _p(g), _p(bias), _p(rs), M, N, K, fs, norm, act, fmt, ldo, _p(out), _p(out16) if shadow else None)
    assert rc == 0, ((M, N, K, fs, norm, act, fmt), (lib.qtts_last_error() or b"").decode())
    if kernel is not None:
        kind = C.c_int32(-1)
        assert lib.qtts_debug_last_decode_gemm_kernel(C.byref(kind)) == 0
        assert kind.value == kernel | (KERNEL_FP8 if fmt == FMT_FP8 else 0), ((M, N, K, fs, act, fmt), "ran on kernel family", kind.value)
    return out, out16


def _bf16(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32)).view(np.float32).reshape(x.shape)


def reference(x, d, bias, res, norm, act):
    """float64 NumPy on d (x rounded to bf16 as the call does)."""
    M, N = x.shape[0], d.shape[0]
    xv = _bf16(x).astype(np.float64)
    acc = xv @ d.astype(np.float64).T
    if norm:
        acc *= 1 / np.sqrt((xv ** 2).mean(1, keepdims=True) + 1e-6)
    if bias is not None:
        acc += bias
    if act in (ACT_SWIGLU, ACT_SWIGLU8):
        h = 16 if act == ACT_SWIGLU else 8
        a = acc.reshape(M, N // (2 * h), 2, h)
        acc = ((a[:, :, 0] / (1 + np.exp(-a[:, :, 0]))) * a[:, :, 1]).reshape(M, N // 2)
    return acc + res if res is not None else acc


def make_case(case, seed):
    M, N, K, fs, norm, act, hb, hr, sh = case
    g = np.random.default_rng(seed)
    x = (g.standard_normal((M, K)) * 0.7).astype(np.float32)
    W = (g.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    W[N // 2] *= 300.0                                         # rows with very different exponents
    W[1] *= 1e-3
    gw = (1 + 0.1 * g.standard_normal(K)).astype(np.float32) if norm else None
    bias = g.standard_normal(N).astype(np.float32) if hb else None
    No = N // 2 if act in (ACT_SWIGLU, ACT_SWIGLU8) else N
    res = g.standard_normal((M, No)).astype(np.float32) if hr else None
    return x, W, gw, bias, res


def check_case(lib, case, seed=0):
    """fp8 launch == bf16 launch on d, bitwise; both within the family's bound of float64 on d; guards untouched.  Returns the fp8 pair."""
    M, N, K, fs, norm, act, hb, hr, sh = case
    x, W, gw, bias, res = make_case(case, seed)
    d = fp8_ref.dequantize(*fp8_ref.quantize_rows(W, gw))
    kernel = KERNEL_8 if case in SKINNY8 else KERNEL_2          # (which list a case is in says which kernel it is meant for)
    o8, s8 = gemm(lib, x, W, gw, bias, res, fs, norm, act, FMT_FP8, sh, kernel)
    ob, sb = gemm(lib, x, d, None, bias, res, fs, norm, act, FMT_BF16, sh, kernel)
    assert np.array_equal(o8.view(np.uint32), ob.view(np.uint32)), (case, "fp8 launch differs from the bf16 launch on d",
                                                                      float(np.abs(o8 - ob).max()))
    assert np.array_equal(s8, sb), (case, "bf16 shadow differs")
    No = o8.shape[1] - 4
    ref = reference(x, d, bias, res, norm, act)
    err = float(np.abs(o8[:, :No] - ref).max())
    assert err <= 2e-3 * max(1.0, float(np.abs(ref).max())), (case, err)
    assert np.all(o8[:, No:] == 7.0), (case, "wrote outside its columns")
    if sh:
        got = (s8[:, :No].astype(np.uint32) << 16).view(np.float32)
        assert np.abs(got - o8[:, :No]).max() <= 8e-3 * max(1.0, float(np.abs(o8[:, :No]).max())), (case, "bf16 shadow differs from the fp32 output")
        assert np.all(s8[:, No:] == 0x4242), case
    else:
        assert np.all(s8 == 0x4242), case
    return o8, s8


def all_codes_skinny2(lib):
    """(64, 16, 64): x = one-hot rows of 1.0, so out[m][n] must be d[n][m] exactly.  Every row starts with +-448 (its exponent is then
    the one chosen, -8 .. 7) and the other 63 entries walk the 254 finite codes."""
    N, K = 16, 64
    codes = np.zeros((N, K), np.uint8)
    exps = np.arange(N, dtype=np.int32) - 8
    for n in range(N):
        codes[n, 0] = 0x7e if n % 2 == 0 else 0xfe
        codes[n, 1:] = fp8_ref.FINITE[(n * 63 + np.arange(63)) % 254]
    assert set(codes.ravel().tolist()) == set(fp8_ref.FINITE.tolist())
    d = fp8_ref.dequantize(codes, exps)
    x = np.eye(64, dtype=np.float32)
    for fs in (16, 8, 4):
        out, _ = gemm(lib, x, d, None, None, None, fs, 0, ACT_NONE, FMT_FP8, 0, KERNEL_2)
        assert np.array_equal(out[:, :N], d.T), (fs, "a code converts to another number")        # (by value: 0 + 1 x -0 is +0 in either kernel)
        outb, _ = gemm(lib, x, d, None, None, None, fs, 0, ACT_NONE, FMT_BF16, 0)
        assert np.array_equal(out.view(np.uint32), outb.view(np.uint32)), fs


def all_codes_skinny8(lib, fs):
    """(8, 32, 1024): the 254 finite codes at the eight k the one-hot rows select (different waves, tiles, k-slices, even and odd tiles of
    a pair); k = 1 carries +-448, which fixes every row's exponent (-20 .. 11)."""
    M, N, K = 8, 32, 1024
    ks = [0, 37, 70, 333, 520, 777, 1000, 1023]
    codes = np.zeros((N, K), np.uint8)
    exps = np.arange(N, dtype=np.int32) - 20
    flat = np.concatenate([fp8_ref.FINITE, fp8_ref.FINITE[:2]])
    for n in range(N):
        codes[n, 1] = 0x7e if n % 2 else 0xfe
        codes[n, ks] = flat[n * 8:(n + 1) * 8]
    d = fp8_ref.dequantize(codes, exps)
    x = np.zeros((M, K), np.float32)
    x[np.arange(M), ks] = 1.0
    out, _ = gemm(lib, x, d, None, None, None, fs, 0, ACT_NONE, FMT_FP8, 0, KERNEL_8)
    assert np.array_equal(out[:, :N], d[:, ks].T), (fs, "a code converts to another number")        # (by value, as above)
    outb, _ = gemm(lib, x, d, None, None, None, fs, 0, ACT_NONE, FMT_BF16, 0)
    assert np.array_equal(out.view(np.uint32), outb.view(np.uint32)), fs

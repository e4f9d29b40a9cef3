"""NumPy / torch restatement of the fp8 row quantizer (include/qtts.h: qtts_fp8_quantize_rows) -- the tests' reference, no library.

  w'[n][k] = fl32(W[n][k] * g[k]);  e[n] = the smallest integer with 448 * 2^e >= max_k |w'[n][k]| (0 for an all-zero row, clamped to
  [-100, 100]);  code = RNE_e4m3fn(w' * 2^-e)  -- the rounding is torch's CPU cast to float8_e4m3fn;  d = code * 2^e;
  W_eff = fl32(d / g), W where g == 0.
"""
import math

import numpy as np
import torch


def e4m3_table():
    """Closed form of OCP e4m3fn: value of every code as float64; the two NaN codes (0x7f, 0xff) are nan."""
    t = np.empty(256, np.float64)
    for c in range(256):
        s, E, m = c >> 7, (c >> 3) & 15, c & 7
        v = m * 2.0 ** -9 if E == 0 else (1 + m / 8.0) * 2.0 ** (E - 7)
        t[c] = math.nan if (E == 15 and m == 7) else (-v if s else v)
    return t


TABLE = e4m3_table()
FINITE = np.array([c for c in range(256) if c & 0x7f != 0x7f], np.uint8)      # the 254 finite codes


def row_exponent(amax: float) -> int:
    """Exact: amax = f * 2^ex with f in [0.5, 1), 448 = 0.875 * 2^9."""
    if not amax > 0:
        return 0
    f, ex = math.frexp(float(amax))
    return max(-100, min(100, ex - 9 if f <= 0.875 else ex - 8))


def scaled_rows(W, g=None):
    W = np.ascontiguousarray(W, np.float32)
    wp = W * np.asarray(g, np.float32)[None, :] if g is not None else W          # the fp32 product pack_skinny_weight forms
    exps = np.array([row_exponent(float(np.abs(r).max())) for r in wp], np.int32)
    return wp, exps


def quantize_rows(W, g=None):
    """(codes uint8 (N, K), exps int32 (N))."""
    wp, exps = scaled_rows(W, g)
    v = np.ldexp(wp, -exps[:, None]).astype(np.float32)                          # exact (a power of two)
    codes = torch.from_numpy(v).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    return codes, exps


def dequantize(codes, exps):
    """d[n][k] = code * 2^e as float32 (exact: every d is a bf16 number)."""
    d = np.ldexp(TABLE[codes], np.asarray(exps, np.int64)[:, None])
    assert np.array_equal(d.astype(np.float32).astype(np.float64), d)
    return d.astype(np.float32)


def effective_rows(W, g=None):
    W = np.ascontiguousarray(W, np.float32)
    d = dequantize(*quantize_rows(W, g))
    if g is None:
        return d
    g = np.asarray(g, np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = (d / g[None, :]).astype(np.float32)
    return np.where(g[None, :] == 0, W, e)

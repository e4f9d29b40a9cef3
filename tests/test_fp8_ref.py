"""The tests' own fp8 quantizer (tests/fp8_ref.py) against the closed-form table of OCP e4m3fn: all 254 finite codes, ties to even,
subnormals, the exact row exponent, idempotence on d.  CPU, no library."""
import numpy as np

import fp8_ref


def test_table_is_e4m3fn():
    t = fp8_ref.TABLE
    assert len(fp8_ref.FINITE) == 254 and np.isnan(t[0x7f]) and np.isnan(t[0xff])
    assert t[0x7e] == 448.0 and t[0xfe] == -448.0 and t[0x08] == 2.0 ** -6 and t[0x01] == 2.0 ** -9 and t[0x38] == 1.0
    pos = t[:0x7f]
    assert np.all(np.diff(pos) > 0) and np.array_equal(t[0x80:0xff], -pos)


def test_every_finite_code_is_a_fixed_point():
    """A row that holds every finite code has max 448 -> exponent 0 and quantizes to itself; scaled by 2^e it gives the same codes and e."""
    row = fp8_ref.TABLE[fp8_ref.FINITE].astype(np.float32)[None, :]
    for e in (0, -12, 5, -100, 100):
        codes, exps = fp8_ref.quantize_rows(np.ldexp(row, e))
        assert exps[0] == e and np.array_equal(codes[0], fp8_ref.FINITE)
        d = fp8_ref.dequantize(codes, exps)
        c2, e2 = fp8_ref.quantize_rows(d)                    # idempotence on d
        assert np.array_equal(c2, codes) and np.array_equal(e2, exps)


def test_ties_go_to_the_even_code_and_subnormals_round_on_the_2_pow_minus_9_grid():
    t = fp8_ref.TABLE
    lo = np.arange(0, 0x7e)
    mid = ((t[lo] + t[lo + 1]) / 2).astype(np.float32)       # exact midpoints of neighbours (one more bit: exact in fp32)
    row = np.concatenate([mid, [448.0]]).astype(np.float32)[None, :]
    codes, exps = fp8_ref.quantize_rows(row)
    assert exps[0] == 0
    want = np.where(lo % 2 == 0, lo, lo + 1)
    assert np.array_equal(codes[0, :-1], want)
    neg, _ = fp8_ref.quantize_rows(-row)
    assert np.array_equal(neg[0, :-1], want | 0x80)
    # just off a midpoint: the nearer neighbour
    up = np.nextafter(mid, np.float32(np.inf)).astype(np.float32)
    codes, _ = fp8_ref.quantize_rows(np.concatenate([up, [448.0]]).astype(np.float32)[None, :])
    assert np.array_equal(codes[0, :-1], lo + 1)
    sub = np.array([[0.0, 2.0 ** -11, 2.0 ** -10, 1.5 * 2.0 ** -9, 2.5 * 2.0 ** -9, 7.5 * 2.0 ** -9, 448.0]], np.float32)
    codes, _ = fp8_ref.quantize_rows(sub)
    assert codes[0].tolist() == [0, 0, 0, 2, 2, 8, 0x7e]      # ties at 0.5, 1.5, 2.5, 7.5 grid steps -> even


def test_row_exponent_is_the_exact_comparison():
    assert fp8_ref.row_exponent(0.0) == 0
    for e in (-100, -13, 0, 1, 31, 100):
        top = float(np.ldexp(np.float32(448.0), e))
        assert fp8_ref.row_exponent(top) == e
        assert fp8_ref.row_exponent(float(np.nextafter(np.float32(top), np.float32(np.inf)))) == min(100, e + 1)
        assert fp8_ref.row_exponent(float(np.nextafter(np.float32(top), np.float32(0)))) == e
        assert fp8_ref.row_exponent(float(np.ldexp(np.float32(224.0), e))) == max(-100, e - 1)
    assert fp8_ref.row_exponent(1e-38) == -100 and fp8_ref.row_exponent(3e38) == 100


def test_effective_rows_keeps_w_where_g_is_zero_and_requantizes_to_d():
    g = np.random.default_rng(5)
    W = (g.standard_normal((6, 64)) * 0.02).astype(np.float32)
    gw = (1 + 0.1 * g.standard_normal(64)).astype(np.float32)
    gw[7] = 0.0
    codes, exps = fp8_ref.quantize_rows(W, gw)
    assert not np.any((codes & 0x7f) == 0x7f) and np.all((codes & 0x7f).max(1) >= 0x76)      # no NaN code; the row maximum lies in (224, 448]
    eff = fp8_ref.effective_rows(W, gw)
    assert np.array_equal(eff[:, 7], W[:, 7]) and np.all(codes[:, 7] & 0x7f == 0)
    d = fp8_ref.dequantize(codes, exps)
    # what a bf16 engine bound with W_eff packs: bf16(fl32(W_eff * g)) == d
    p = (eff * gw[None, :]).astype(np.float32)
    u = p.view(np.uint32).astype(np.uint64)
    b = (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)
    assert np.array_equal(b, d)

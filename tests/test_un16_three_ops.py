"""plh_un16_3 (devmath.hiph): a 16-bit unorm code as fp32 in two instructions behind the conversion,

    fmaf(x, r, x * r_lo),   r = fp32(1 / 65535),  r_lo = fp32(1 / 65535 - r),

against plh_un16's three, fmaf(fmaf(-q, 65535, x), r, q) with q = x * r: the same fp32 bits for every
one of the 65536 codes (and both are the correctly rounded quotient x / 65535).

fp32 arithmetic is spelled out: a product of two fp32 numbers is exact in float64 here (at most 24 +
24 bits), and an fma's sum is formed in float64 with its rounding error recovered (TwoSum) and
folded into the last bit (round to odd), so that the one rounding to fp32 is the fma's own."""
import numpy as np

R = np.float32(1.0 / 65535.0)
R_LO = np.float32(1.0 / 65535.0 - np.float64(R))


def fma32(a, b, c):
    """fp32 fma(a, b, c) of fp32 arrays whose products a * b are exact in float64"""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)     # s + err = p + c exactly
    bits = s.view(np.int64).copy()
    # round to odd: where the sum is inexact, the float64 towards zero with its last bit set
    away = (err != 0) & ((err > 0) != (s > 0))
    bits[away] -= 1
    bits[err != 0] |= 1
    return bits.view(np.float64).astype(np.float32)


def mul32(a, b):
    return (a.astype(np.float64) * b.astype(np.float64)).astype(np.float32)


def test_constants():
    assert float(R) == 2.0 ** -16 * (1 + 2.0 ** -16)        # 0x1.0001p-16
    assert float(R_LO) == 2.0 ** -48 * (1 + 2.0 ** -16)     # 0x1.0001p-48


def test_fma_emulation():
    one = np.array([1.0], np.float32)
    half_ulp = np.array([2.0 ** -12], np.float32)       # squared: half an fp32 ulp of 1
    assert fma32(half_ulp, half_ulp, one)[0] == np.float32(1.0)     # the tie goes to even
    above = np.array([2.0 ** -12 + 2.0 ** -30], np.float32)
    assert fma32(above, half_ulp, one)[0] == np.float32(1.0 + 2.0 ** -23)
    # (2^-30 * 2^-30 is below float64's last bit of the sum: kept as a sticky bit, it moves nothing here)
    tiny = np.array([2.0 ** -30], np.float32)
    assert fma32(tiny, tiny, np.array([1.0 + 2.0 ** -23], np.float32))[0] == np.float32(1.0 + 2.0 ** -23)
    assert fma32(-tiny, tiny, one)[0] == np.float32(1.0)


def test_all_codes():
    x = np.arange(65536, dtype=np.uint32).astype(np.float32)
    q = mul32(x, np.full_like(x, R))
    three = fma32(fma32(-q, np.full_like(x, 65535.0), x), np.full_like(x, R), q)
    two = fma32(x, np.full_like(x, R), mul32(x, np.full_like(x, R_LO)))
    assert np.array_equal(two.view(np.uint32), three.view(np.uint32)), np.nonzero(two != three)
    quotient = (np.arange(65536) / 65535.0).astype(np.float32)
    assert np.array_equal(two.view(np.uint32), quotient.view(np.uint32))

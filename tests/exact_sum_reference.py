"""The number format of the exact adjoint sums (course5_amd/csrc/exact_sum.hpp, include/course5_hip.h: "exact adjoint
sums") restated in Python integers and fractions.Fraction: nothing here rounds but where the format says so.

For an image of res_x x res_y pixels (the whole image) and per cell for each of the two sums:
    h = ceil(log2(res_x res_y)) + 1,  m = 62 - h
    e   the largest ilogb(|x|) over the non-zero finite contributions x (NONE: no contribution; NOT_FINITE: one is not finite)
    for |x| < 2^(e+1):  y = x 2^(m-e-1),  k1 = rint(y),  k0 = rint((y - k1) 2^m)          (ties to even)
    s1 = sum k1,  s0 = sum k0
    value = (s1 2^m + s0) 2^(e+1-2m) rounded once to fp64 (ties to even, subnormals included); NONE: +0.0; NOT_FINITE: NaN
Each contribution is off by at most 2^(e-2m)."""
import math
from fractions import Fraction

NONE = -2**31          # INT32_MIN
NOT_FINITE = 2**31 - 1  # INT32_MAX


def word_bits(res_x: int, res_y: int) -> int:
    """m of an image of res_x x res_y pixels."""
    n = int(res_x) * int(res_y)
    assert n >= 1
    h = (n - 1).bit_length() + 1  # ceil(log2 n) + 1
    return 62 - h


def exponent_of(x: float) -> int:
    """ilogb(|x|) of a non-zero finite x; NONE for a zero, NOT_FINITE for an infinity or a NaN."""
    if math.isnan(x) or math.isinf(x):
        return NOT_FINITE
    if x == 0.0:
        return NONE
    f = abs(Fraction(x))
    e = f.numerator.bit_length() - f.denominator.bit_length()
    return e if Fraction(2) ** e <= f else e - 1


def exponent_over(xs) -> int:
    """e of a cell with the contributions xs."""
    return max((exponent_of(float(x)) for x in xs), default=NONE)


def quantise(x: float, e: int, m: int):
    """(k1, k0) of a finite x with |x| < 2^(e+1)."""
    f = Fraction(x)
    if f == 0:
        return 0, 0
    assert e != NONE and abs(f) < Fraction(2) ** (e + 1), (x, e)
    y = f * Fraction(2) ** (m - e - 1)
    k1 = round(y)  # (Fraction.__round__: to the nearest integer, ties to even)
    k0 = round((y - k1) * 2**m)
    return k1, k0


def words(xs, e: int, m: int):
    """(s1, s0) of the contributions xs against the exponent e."""
    if e == NOT_FINITE:
        return 0, 0
    s1 = s0 = 0
    for x in xs:
        k1, k0 = quantise(float(x), e, m)
        s1 += k1
        s0 += k0
    return s1, s0


def exact_value(e: int, s1: int, s0: int, m: int) -> Fraction:
    """The value of the words before the final rounding (e neither NONE nor NOT_FINITE)."""
    return Fraction(s1 * 2**m + s0) * Fraction(2) ** (e + 1 - 2 * m)


def finish(e: int, s1: int, s0: int, m: int) -> float:
    """The words' value rounded once to fp64."""
    if e == NOT_FINITE:
        return math.nan
    if e == NONE:
        return 0.0
    v = exact_value(e, s1, s0, m)
    if v == 0:
        return 0.0
    try:
        return v.numerator / v.denominator  # (int / int: correctly rounded, ties to even, subnormals included)
    except OverflowError:
        return math.inf if v > 0 else -math.inf

// The number format of the exact adjoint sums ("adjoint_exact", c5_render_adjoint_exact_*; include/course5_hip.h states
// it for callers, tests/exact_sum_reference.py restates it in Python integers).  Float adds do not commute, integer adds
// do: every contribution is rounded ONCE onto a fixed-point grid of its cell, and everything after that is int64.
//
// For an image of res_x x res_y pixels (the WHOLE image of c5_set_image, not a rank's rows):
//     h = ceil(log2(res_x res_y)) + 1     headroom: a cell is crossed at most once per ray, res_x res_y contributions at most
//     m = 62 - h                          bits per word
// Per cell and sum (grad_alpha, grad_q):
//     e (int32)   the largest ilogb(|x|) over the non-zero finite contributions x; kNone (INT32_MIN): no contribution;
//                 kNotFinite (INT32_MAX): some contribution was not finite, the sum is NaN
//     for |x| < 2^(e+1):   y = x 2^(m-e-1);   k1 = rint(y);   k0 = rint((y - k1) 2^m)      (ties to even, nothing else rounds)
//     s1 = sum k1, s0 = sum k0 (int64: |s1| <= 2^61, |s0| <= 2^60)
//     value = (s1 2^m + s0) 2^(e+1-2m), rounded once to fp64 (ties to even, subnormals included)
// Each contribution is off by at most 2^(e-2m): 2^(e-76) at 2400 x 1800 (h = 24, m = 38), so that the sum of up to 2^23
// of them stays within 2^(e-53) of the exact sum of the fp64 contributions.
//
// quantise() scales by powers of two only where the result stays normal and leaves early where it would not: every
// operation in it is exact, so the host and the device give the same words.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define C5_EXACT_HD __host__ __device__ inline
#else
#define C5_EXACT_HD inline
#endif

namespace c5 {
namespace exact {

constexpr int32_t kNone = INT32_MIN;       // no contribution
constexpr int32_t kNotFinite = INT32_MAX;  // a contribution was not finite
constexpr int kMinWordBits = 22;           // images beyond 2^39 pixels are refused

C5_EXACT_HD int leading_zeros(uint64_t v) { return v ? __builtin_clzll(v) : 64; }

// h of an image of n_px pixels (n_px >= 1)
C5_EXACT_HD int headroom_bits(int64_t n_px) {
    const uint64_t n = n_px > 1 ? static_cast<uint64_t>(n_px) : 1u;
    return (64 - leading_zeros(n - 1)) + 1;  // ceil(log2 n) + 1
}
// m; below kMinWordBits: no format for such an image
C5_EXACT_HD int word_bits(int64_t n_px) { return 62 - headroom_bits(n_px); }

C5_EXACT_HD uint64_t bits_of(double x) {
    union {
        double d;
        uint64_t u;
    } c;
    c.d = x;
    return c.u;
}
C5_EXACT_HD double double_of(uint64_t u) {
    union {
        double d;
        uint64_t u;
    } c;
    c.u = u;
    return c.d;
}

// ilogb(|x|) of a non-zero finite x (subnormals included); kNone for a zero, kNotFinite for an infinity or a NaN
C5_EXACT_HD int32_t exponent_of(double x) {
    if ((bits_of(x) & 0x7ff0000000000000ull) == 0x7ff0000000000000ull) return kNotFinite;
    if (x == 0.0) return kNone;
    int ex;
    (void)frexp(x, &ex);  // x = f 2^ex, 1/2 <= |f| < 1
    return ex - 1;
}

// (k1, k0) of x against the cell's exponent e with m bits per word.  False - nothing may be added then - where x does
// not fit (|x| >= 2^(e+1), or x is not finite): the exponent given is too small.  A zero gives (0, 0).
// Every floating-point operation here is exact: the scalings are by powers of two of values that stay normal (what
// would underflow is below half a unit of the second word and leaves before it is scaled), y - rint(y) is exact for any
// y, and both rint see |.| <= 2^61.  rint rounds ties to even (the host's default rounding mode; v_rndne_f64).
C5_EXACT_HD bool quantise(double x, int32_t e, int m, int64_t& k1, int64_t& k0) {
    k1 = k0 = 0;
    const int32_t ex = exponent_of(x);
    if (ex == kNone) return true;
    if (ex == kNotFinite || ex > e) return false;  // (e == kNone: every ex is beyond it)
    const int64_t scale = static_cast<int64_t>(m) - e - 1;  // y = x 2^scale, 2^(ex+scale) <= |y| < 2^m
    if (ex + scale < -m - 1) return true;                   // |y| < 2^-m-1: |y 2^m| < 1/2, both words are 0
    const double y = ldexp(x, static_cast<int>(scale));
    const double whole = rint(y);
    k1 = static_cast<int64_t>(whole);
    k0 = static_cast<int64_t>(rint(ldexp(y - whole, m)));
    return true;
}

// (s1 2^m + s0) 2^(e+1-2m) rounded once to fp64, ties to even; +0.0 for kNone (and for words that cancel), NaN for kNotFinite
C5_EXACT_HD double finish(int32_t e, int64_t s1, int64_t s0, int m) {
    if (e == kNotFinite) return double_of(0x7ff8000000000000ull);
    if (e == kNone) return 0.0;
    const __int128 w = static_cast<__int128>(s1) * (static_cast<__int128>(1) << m) + s0;
    if (w == 0) return 0.0;
    const uint64_t sign = w < 0 ? uint64_t{1} << 63 : 0u;
    const unsigned __int128 mag = w < 0 ? -static_cast<unsigned __int128>(w) : static_cast<unsigned __int128>(w);
    const uint64_t hi = static_cast<uint64_t>(mag >> 64), lo = static_cast<uint64_t>(mag);
    const int len = hi ? 128 - leading_zeros(hi) : 64 - leading_zeros(lo);  // mag < 2^len
    const int64_t p = static_cast<int64_t>(e) + 1 - 2 * m;                  // value = mag 2^p
    // q = mag / 2^shift: 53 bits of a normal result, or the multiple of 2^-1074 of a subnormal one
    int64_t shift = len - 53;
    if (shift < -1074 - p) shift = -1074 - p;
    if (p + shift + 1074 >= 2047) return double_of(sign | 0x7ff0000000000000ull);
    uint64_t q;
    if (shift <= 0) {
        q = lo << -shift;  // (mag < 2^53 here, and the result has at most 53 bits)
    } else if (shift > len + 1) {
        q = 0;
    } else {
        const int t = static_cast<int>(shift);
        const unsigned __int128 one = 1;
        const unsigned __int128 quot = mag >> t, rem = mag & ((one << t) - 1), half = one << (t - 1);
        q = static_cast<uint64_t>(quot) + ((rem > half) || (rem == half && (static_cast<uint64_t>(quot) & 1u)));
    }
    // (q <= 2^53: a carry out of the 53 bits, like a subnormal reaching 2^52, moves the exponent field by one)
    const uint64_t bits = (static_cast<uint64_t>(p + shift + 1074) << 52) + q;
    if ((bits >> 52) >= 2047) return double_of(sign | 0x7ff0000000000000ull);
    return double_of(sign | bits);
}

}  // namespace exact
}  // namespace c5

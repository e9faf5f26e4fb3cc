"""The exact adjoint sums without a GPU: the host side of the format (c5_exact_sums_finish, and exact_sum.hpp's quantise
through the test-only export c5_exact_quantise) against its restatement in Python integers and fractions
(tests/exact_sum_reference.py), the wrappers' argument checks and calls, and sharding.combine_exact."""
import ctypes
import math
import struct
from fractions import Fraction

import numpy as np
import pytest

from course5_amd import capi, sharding
from tests import exact_sum_reference as er
from tests.fake_library import RecordingLibrary, bare_context

IMAGES = [(1, 1), (2, 1), (3, 1), (29, 21), (160, 120), (2400, 1800), (8192, 8192)]  # 1 pixel ... 2^26


def _bits(x):
    return struct.unpack("<q", struct.pack("<d", float(x)))[0]


def _quantise(xs, e, rx, ry):
    lib = capi.load_library()
    xs = np.ascontiguousarray(xs, dtype=np.float64)
    words = np.zeros((len(xs), 2), np.int64)
    rc = lib.c5_exact_quantise(capi._dp(xs), len(xs), e, rx, ry, words.ctypes.data_as(capi._lp_t))
    return rc, words


def test_the_format_of_the_header_the_restatement_and_the_benchmark_frame():
    assert [er.word_bits(*im) for im in IMAGES] == [61, 60, 59, 51, 46, 38, 35]
    # 2400 x 1800: h = 24, m = 38; n <= 2^23 contributions, each off by at most 2^(e-2m): within 2^(e-53) in all
    m = er.word_bits(2400, 1800)
    assert 62 - m == 24 and 2400 * 1800 <= 2**23
    assert Fraction(2) ** 23 * Fraction(2) ** (-2 * m) <= Fraction(2) ** -53
    for x, e in ((1.0, 0), (-1.5, 0), (0.75, -1), (5e-324, -1074), (2.0**-1022, -1022), (1.7976931348623157e308, 1023),
                 (0.0, er.NONE), (-0.0, er.NONE), (math.inf, er.NOT_FINITE), (math.nan, er.NOT_FINITE)):
        assert er.exponent_of(x) == e


def test_finish_equals_the_restatement_bit_for_bit():
    rng = np.random.default_rng(20)
    cases = []  # (res_x, res_y, e, s1, s0)
    for rx, ry in IMAGES:
        m = er.word_bits(rx, ry)
        h = 62 - m
        top1, top0 = 2**61, 2**60
        for _ in range(400):
            kind = rng.integers(8)
            e = int(rng.integers(-1100, 1030))
            s1 = int(rng.integers(-top1, top1, endpoint=True))
            s0 = int(rng.integers(-top0, top0, endpoint=True))
            if kind == 0:    # a few bits only
                s1, s0 = int(rng.integers(-4, 5)), int(rng.integers(-4, 5))
            elif kind == 1:  # an exact tie of the final rounding: 53 bits, then a one, then zeros
                total = (int(rng.integers(2**52, 2**53)) * 2 + 1) << int(rng.integers(0, 2 * m + h - 56))
                total *= int(rng.choice([-1, 1]))
                s1, s0 = total >> m, total & (2**m - 1)  # (floor and remainder: s1 2^m + s0 == total)
            elif kind == 2:  # subnormal results, ties among them
                e = int(rng.integers(-1200, -1000))
            elif kind == 3:  # results that overflow, or nearly
                e = int(rng.integers(1015, 1100))
            elif kind == 4:  # the words cancel
                s1, s0 = int(rng.integers(-2**20, 2**20)), 0
                s0 = -s1 * 2**m if abs(s1 * 2**m) <= top0 else 0
            cases.append((rx, ry, e, s1, s0))
        cases += [(rx, ry, er.NONE, 5, 7), (rx, ry, er.NOT_FINITE, 0, 0), (rx, ry, er.NOT_FINITE, -9, 3), (rx, ry, 0, 0, 0),
                  (rx, ry, -1074 + 2 * m - 1, 0, 1), (rx, ry, -1074 + 2 * m - 2, 0, 1), (rx, ry, -1074 + 2 * m - 2, 0, 3),
                  (rx, ry, -1074 + 2 * m - 2, 0, -1), (rx, ry, 1023, top1, 0), (rx, ry, 1023, -top1, -top0),
                  (rx, ry, 1023 - h + 1, top1 - 1, 2**m - 1), (rx, ry, 5000, 1, 0), (rx, ry, -5000, top1, top0), (rx, ry, -5000, -top1, 0)]
    seen = {"negative": 0, "subnormal": 0, "inf": 0, "nan": 0, "zero": 0, "tie": 0}
    for rx, ry in IMAGES:
        mine = [c for c in cases if c[:2] == (rx, ry)]
        m = er.word_bits(rx, ry)
        exp = np.array([c[2] for c in mine], np.int32)
        sums = np.array([[c[3], c[4]] for c in mine], np.int64)
        got = capi.exact_sums_finish(exp, sums, rx, ry)
        for (_, _, e, s1, s0), g in zip(mine, got):
            want = er.finish(e, s1, s0, m)
            if math.isnan(want):
                assert math.isnan(g) and e == er.NOT_FINITE
                seen["nan"] += 1
                continue
            assert _bits(g) == _bits(want), (rx, ry, e, s1, s0, g, want)
            seen["negative"] += want < 0
            seen["subnormal"] += 0 < abs(want) < 2.0**-1022
            seen["inf"] += math.isinf(want)
            seen["zero"] += want == 0
            if e not in (er.NONE, er.NOT_FINITE) and want != 0 and not math.isinf(want):
                seen["tie"] += abs(er.exact_value(e, s1, s0, m) - Fraction(want)) * 2 == Fraction(math.ulp(want))
    assert len(cases) > 2500 and seen.pop("nan") == 2 * len(IMAGES) and all(v >= 20 for v in seen.values()), seen
    assert _bits(capi.exact_sums_finish(np.array([er.NONE], np.int32), np.array([[1, 1]], np.int64), 4, 4)[0]) == 0  # +0.0


def test_finish_checks_its_arguments_before_the_library():
    e, s = np.zeros(3, np.int32), np.zeros((3, 2), np.int64)
    assert capi.exact_sums_finish(e, s, 29, 21).tolist() == [0.0, 0.0, 0.0]
    for bad_e, bad_s in ((e.astype(np.int64), s), (e, s.astype(np.int32)), (e, s[:2]), (e, np.zeros((3, 3), np.int64)[:, :2]),
                         (np.zeros(6, np.int32)[::2], s), (e.reshape(3, 1), s), (e, s.reshape(6))):
        with pytest.raises(ValueError):
            capi.exact_sums_finish(bad_e, bad_s, 29, 21)
    with pytest.raises(ValueError):
        capi.exact_sums_finish(e, s, 0, 21)
    with pytest.raises(capi.C5Error) as err:  # (no format for 2^40 pixels: the library says so)
        capi.exact_sums_finish(e, s, 2**20, 2**20)
    assert err.value.code == capi.C5_ERR_INVALID


@pytest.mark.parametrize("image", [(29, 21), (2400, 1800), (1, 1), (8192, 8192)])
def test_quantise_sums_in_any_order_and_stays_within_its_bound(image):
    rx, ry = image
    m = er.word_bits(rx, ry)
    rng = np.random.default_rng(rx)
    for e in (0, 7, -30, 1023, -1022, -1060):
        n = 200
        below = math.ldexp(2.0 - 2.0**-52, e) if e > -1022 else math.ldexp(1.0, e + 1) - 5e-324  # 2^(e+1) minus one ulp
        largest = math.ldexp(1.75, e)
        xs = np.ldexp(rng.uniform(-1.0, 1.0, n) * 2.0, e)
        xs[:40] *= np.exp2(-rng.integers(1, 120, 40).astype(np.float64))  # down to far below the grid
        xs[40:44] = [below, -below, largest, math.ldexp(1.0, e)]
        tiny = math.ldexp(1.0, e - 80)  # 2^-80 below the largest: lost in fp64, kept in the second word where m > 40
        xs[44:52] = [tiny, -tiny, 3 * tiny, tiny * (1 + 2.0**-52), math.ldexp(1.0, e - m), math.ldexp(1.5, e - 2 * m),
                     math.ldexp(0.5, e - 2 * m), -math.ldexp(1.0, e - 1 - m)]
        xs[52:56] = [0.0, -0.0, 5e-324, -5e-324]
        assert er.exponent_over(xs) == e
        rc, words = _quantise(xs, e, rx, ry)
        assert rc == capi.C5_OK
        for x, (k1, k0) in zip(xs, words):  # every pair is the restatement's
            assert (int(k1), int(k0)) == er.quantise(float(x), e, m), (x, e, m)
            assert abs(Fraction(float(x)) - er.exact_value(e, int(k1), int(k0), m)) <= Fraction(2) ** (e - 2 * m)
        if rx * ry < n:  # (a cell has at most one contribution per pixel: each value is a sum of its own)
            for x, w in zip(xs, words):
                one = capi.exact_sums_finish(np.array([e], np.int32), w.reshape(1, 2).copy(), rx, ry)[0]
                assert _bits(one) == _bits(er.finish(e, int(w[0]), int(w[1]), m))
                assert one == x or abs(x) < math.ldexp(1.0, e + 53 - 2 * m)  # (a value whose last bit is on the grid survives)
            continue
        sums = words.sum(axis=0)
        for _ in range(5):  # the words summed in several orders: identical
            order = rng.permutation(n)
            acc = np.zeros(2, np.int64)
            for i in order:
                acc += words[i]
            assert np.array_equal(acc, sums)
        assert (int(sums[0]), int(sums[1])) == er.words(xs, e, m)
        got = capi.exact_sums_finish(np.array([e], np.int32), sums.reshape(1, 2), rx, ry)[0]
        assert _bits(got) == _bits(er.finish(e, int(sums[0]), int(sums[1]), m))
        exact = sum(Fraction(float(x)) for x in xs)
        assert abs(er.exact_value(e, int(sums[0]), int(sums[1]), m) - exact) <= n * Fraction(2) ** (e - 2 * m)
        if e > -1000 and not math.isinf(got):  # (the finished fp64 adds its one rounding: half an ulp of the result, or of the smallest normal)
            half_ulp = Fraction(math.ulp(got)) / 2
            assert abs(Fraction(got) - exact) <= n * Fraction(2) ** (e - 2 * m) + half_ulp


def test_quantise_refuses_what_does_not_fit():
    for xs, e in (([2.0], 0), ([-2.0], 0), ([1.0, math.inf], 5), ([math.nan], 5), ([1e-300], er.NONE), ([1.0], -1)):
        rc, words = _quantise(xs, e, 29, 21)
        assert rc == capi.C5_ERR_INVALID
        assert "beyond the exponent" in capi.load_library().c5_last_error(None).decode()
    rc, words = _quantise([0.0, -0.0], er.NONE, 29, 21)  # (a zero is no contribution: it fits anywhere)
    assert rc == capi.C5_OK and not words.any()
    rc, words = _quantise([math.nextafter(2.0, 0.0)], 0, 29, 21)  # (rounds up to the very top of the first word, 2^m)
    assert rc == capi.C5_OK and words[0].tolist() == [2**51, -2**49] == list(er.quantise(math.nextafter(2.0, 0.0), 0, 51))


# ---- wrappers ------------------------------------------------------------------------------------------------------
G = np.zeros((5, 6, 2), np.float32)
E = np.zeros(7, np.int32)
P1, P2, P3, P4, P5 = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
EXPS, WORDS = ("int32", (7,)), ("int64", (7, 2))

CASES = [
    ("render_adjoint_exact_bounds", (G,),
     [("c5_render_adjoint_exact_bounds", (None, "ptr", "ptr", "ptr"))], (EXPS, EXPS)),
    ("render_adjoint_exact_bounds", (G.astype(np.float64),),
     [("c5_render_adjoint_exact_bounds", (None, "ptr", "ptr", "ptr"))], (EXPS, EXPS)),
    ("render_adjoint_exact_sums", (G, E, E),
     [("c5_render_adjoint_exact_sums", (None, "ptr", "ptr", "ptr", "ptr", "ptr"))], (WORDS, WORDS)),
    ("render_adjoint_exact_bounds_device", (P1, P2, P3),
     [("c5_render_adjoint_exact_bounds_device", (None, P1, P2, P3))], None),
    ("render_adjoint_exact_sums_device", (P1, P2, P3, P4, P5),
     [("c5_render_adjoint_exact_sums_device", (None, P1, P2, P3, P4, P5))], None),
]


@pytest.mark.parametrize("method, args, calls, returned", CASES, ids=[f"{c[0]}-{i}" for i, c in enumerate(CASES)])
def test_the_exact_wrappers_send_what_the_header_declares(method, args, calls, returned):
    ctx = bare_context()
    ctx.lib = RecordingLibrary()
    out = getattr(ctx, method)(*args)
    assert ctx.lib.calls == calls
    if returned is None:
        assert out is None
    else:
        assert tuple((str(a.dtype), a.shape) for a in out) == returned


def test_the_exact_wrappers_check_their_arguments_before_the_library():
    ctx = bare_context()  # (over NoLibrary: entering the library fails the test)
    for bad in (np.zeros((5, 6)), np.zeros((4, 6, 2)), np.zeros((2, 5, 6, 2))):
        with pytest.raises(ValueError):
            ctx.render_adjoint_exact_bounds(bad)
        with pytest.raises(ValueError):
            ctx.render_adjoint_exact_sums(bad, E, E)
    for bad in (np.zeros(7, np.int64), np.zeros(6, np.int32), np.zeros((7, 1), np.int32), np.zeros(14, np.int32)[::2], np.zeros(7)):
        with pytest.raises(ValueError):
            ctx.render_adjoint_exact_sums(G, bad, E)
        with pytest.raises(ValueError):
            ctx.render_adjoint_exact_sums(G, E, bad)


def test_the_library_and_the_binding_name_the_new_symbols():
    lib = ctypes.CDLL(capi.LIB_PATH)
    for name in ("c5_render_adjoint_exact_bounds", "c5_render_adjoint_exact_bounds_device", "c5_render_adjoint_exact_sums",
                 "c5_render_adjoint_exact_sums_device", "c5_exact_sums_finish", "c5_exact_quantise"):
        assert hasattr(lib, name) and name in capi.EXPORTS
    assert lib.c5_abi_version() == 2  # (symbols were added, nothing changed)


# ---- sharding.combine_exact -----------------------------------------------------------------------------------------
def test_combine_exact_takes_the_max_of_exponents_and_the_integer_sum_of_words():
    n = 6
    ea = [np.array([er.NONE, 3, -5, er.NONE, er.NOT_FINITE, 0], np.int32), np.array([er.NONE, 2, -4, 7, 1, 0], np.int32),
          np.array([-1000, 3, -9, er.NONE, 1, er.NONE], np.int32)]
    eq = [e[::-1].copy() for e in ea]
    rng = np.random.default_rng(2)
    sa = [rng.integers(-2**59, 2**59, (n, 2)) for _ in ea]
    sq = [rng.integers(-2**59, 2**59, (n, 2)) for _ in ea]
    out = sharding.combine_exact(list(zip(ea, eq, sa, sq)))
    assert out[0].tolist() == [-1000, 3, -4, 7, er.NOT_FINITE, 0] and out[0].dtype == np.int32
    assert out[1].tolist() == np.maximum(np.maximum(eq[0], eq[1]), eq[2]).tolist()
    want = [[sum(int(s[i, j]) for s in sa) for j in range(2)] for i in range(n)]
    assert out[2].tolist() == want and out[2].dtype == np.int64
    assert np.array_equal(out[3], sq[0] + sq[1] + sq[2])
    assert sa[0] is not out[2] and np.array_equal(sharding.combine_exact([(ea[0], eq[0], sa[0], sq[0])])[2], sa[0])
    # the order of the parts does not matter; exponents alone combine too
    back = sharding.combine_exact(list(zip(ea, eq, sa, sq))[::-1])
    assert all(np.array_equal(a, b) for a, b in zip(out, back))
    only = sharding.combine_exact([(a, b, None, None) for a, b in zip(ea, eq)])
    assert np.array_equal(only[0], out[0]) and only[2] is None and only[3] is None
    for bad in ([], [(ea[0], eq[0], sa[0])], [(ea[0].astype(np.int64), eq[0], sa[0], sq[0])], [(ea[0], eq[0], sa[0].astype(np.float64), sq[0])],
                [(ea[0], eq[0], sa[0], sq[0]), (ea[1][:3], eq[1], sa[1], sq[1])]):
        with pytest.raises(ValueError):
            sharding.combine_exact(bad)

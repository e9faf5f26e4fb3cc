"""What the priors' fuzz sweep (tests/test_gpu_prior_fuzz.py) stands on, pinned without a GPU.

The conditioned scale of tests/shape_prior_reference.py: the float64 restatement against 80-digit mpmath on the
unstructured scenes 7000 - 7011 (tests/unstructured_scenes.py: graded cells, slivers, a point in hundreds of cells) at
x = displaced(X), and on kuhn_box(2, jitter 0.2) under the six strain regimes (shape_prior_reference.STRAINS) - at sampled
points, at most 48 per scene with at most 64 incident cells each.  The worst ratio gives K_CONDITIONED by the project's rule (4
x worst, rounded up to a power of two), and the stored constant must be that.  The negative control keeps the reason on
record: under the OLD scale the restatement itself is hundreds of times past K on these scenes.

The value's tree (prior_reference.tree_sum) against hand-made cases, and the pseudo-Huber penalty's three functions
against 80 digits over |d| / delta from 1e-300 to 1e300: the closed-form tail past 2^256 and the d d overflow branch."""
import math

import numpy as np
import pytest

from course5_amd import meshgen as mg
from tests import prior_reference as pr
from tests import shape_prior_reference as sr
from tests import unstructured_scenes as us

EPS, K, K_CONDITIONED = sr.EPS, sr.K, sr.K_CONDITIONED
ENERGIES = (sr.DIRICHLET, sr.NEO_HOOKEAN)
NAMES = {sr.DIRICHLET: "dirichlet", sr.NEO_HOOKEAN: "neo_hookean"}
KAPPA, LAM = 1.5, 0.75


def _measure(X, cells, x_of, seed, old_scale=False):
    """{(quantity, energy): worst ratio of the restatement against 80 digits at the sampled points}."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    vert = sr.welded_cells(X, cells)
    n_pts = len(X)
    B, V0, n_deg = sr.rest(X, vert)
    x = x_of(X, vert)
    assert n_deg == 0 and sr.quality(B, V0, vert, x)[1] == 0
    v = sr.directions(n_pts, seed)
    points = sr.sampled_points(vert, n_pts, seed)
    want = sr.MpSamples(B, V0, vert, x, v, KAPPA, LAM, points)
    out = {}
    for energy in ENERGIES:
        args = (B, V0, vert, n_pts, x, energy, KAPPA, LAM)
        if old_scale:
            got = want.ratios(energy, gradient=sr.gradient(*args, with_scale=True),
                              product=sr.product(B, V0, vert, n_pts, x, v, energy, KAPPA, LAM, with_scale=True))
        else:
            terms, scales = sr.value_terms(B, V0, vert, x, energy, KAPPA)
            got = want.ratios(energy, gradient=sr.conditioned(*args, "gradient"), product=sr.conditioned(*args, "product", v=v),
                              diagonal=sr.conditioned(*args, "diagonal"), value_terms=(LAM * terms, LAM * scales),
                              quality=sr.conditioned_quality(B, V0, vert, x)[::2] if energy == sr.DIRICHLET else None)
        out.update({(name, energy): r for name, r in got.items()})
    return out


def _displaced(X, vert):
    return sr.displaced(X, vert)


@pytest.fixture(scope="module")
def measured():
    """{(scene, quantity, energy): ratio} under the conditioned scale."""
    out = {}
    for seed in sr.FUZZ_SEEDS:
        X, cells = us.scene(seed)[:2]
        out.update({(f"{seed}", *k): r for k, r in _measure(X, cells, _displaced, seed).items()})
    X, cells = mg.kuhn_box(2, jitter=0.2)
    for i, regime in enumerate(sr.STRAINS):
        got = _measure(X, cells, lambda X_, vert, regime=regime: sr.strained(X_, vert, regime), 100 + i)
        out.update({(regime, *k): r for k, r in got.items()})
    return out


def test_the_conditioned_scale_gives_K_CONDITIONED(measured):
    scenes = [str(s) for s in sr.FUZZ_SEEDS] + list(sr.STRAINS)
    quantities = sorted({k[1:] for k in measured}, key=str)
    print("\nrestatement against 80 digits, in units of 2^-52 x the conditioned scale")
    print(f"{'scene':12s}" + "".join(f"{q[0][:5] + ' ' + NAMES[q[1]][:3]:>11s}" for q in quantities))
    for s in scenes:
        info = us.describe(int(s)) if s.isdigit() else None
        print(f"{s:12s}" + "".join(f"{measured.get((s, *q), float('nan')):11.3f}" for q in quantities)
              + (f"   {info['base']}, {info['cells']} cells" if info else ""))
    worst_key = max(measured, key=measured.get)
    worst = measured[worst_key]
    want = 2.0 ** math.ceil(math.log2(4.0 * worst))
    print(f"worst ratio {worst:.3f} at {worst_key}: K_CONDITIONED = 4 x that, rounded up to a power of two = {want:g}; "
          f"tests/shape_prior_reference.py holds {K_CONDITIONED}")
    assert set(scenes) == {k[0] for k in measured}
    assert 4.0 * worst <= K_CONDITIONED
    assert K_CONDITIONED == max(want, 1.0)


def test_the_sweep_s_seeds_hold_every_class():
    infos = [us.describe(s) for s in sr.FUZZ_SEEDS]
    assert all(sum(i["base"] == b for i in infos) == 4 for b in us.BASES)
    assert sum(i["cells"] > us.LARGE for i in infos) == 3 and all(i["cells"] <= 9000 for i in infos)
    assert max(i["point_valence"] for i in infos) > 256  # (an incidence list longer than a block is wide)


def test_under_the_old_scale_the_restatement_misses_K_on_graded_grids():
    """The negative control: K x 2^-52 x (the terms of P and P B^T) is no bound where |Ds| |B| >> |F|."""
    X, cells = us.scene(7004)[:2]
    got = _measure(X, cells, _displaced, 7004, old_scale=True)
    for k, r in sorted(got.items(), key=str):
        print(f"7004 {k[0]:9s} {NAMES[k[1]]:12s} {r:10.1f} x 2^-52 of the old scale (K = {K})")
    assert all(got[("gradient", energy)] > K for energy in ENERGIES)


# ---- the value's tree -------------------------------------------------------------------------------------------------------------
def test_the_tree_s_order_of_additions():
    # one value that only the right pairing keeps: 2^53 + 1 + (-2^53) is 0 or 1 by the order
    big = 2.0 ** 53
    v = np.zeros(64)
    v[0], v[32], v[16] = big, 1.0, -big  # off 32: v0 = big + 1 = big; off 16: v0 = big - big = 0
    assert pr.tree_sum(v) == 0.0
    v = np.zeros(64)
    v[0], v[16], v[32], v[48] = big, -big, 1.0, 0.0  # off 32: v0 = big + 1 -> big, v16 = -big; off 16: 0
    assert pr.tree_sum(v) == 0.0
    v = np.zeros(64)
    v[0], v[32], v[1] = big, -big, 1.0  # off 32: v0 = 0; off 1: 0 + 1
    assert pr.tree_sum(v) == 1.0
    # the block's wavefronts in order from 0: ((0 + w0) + w1) + w2 ...
    v = np.zeros(256)
    v[0], v[64], v[128] = big, 1.0, -big
    assert pr.tree_sum(v) == 0.0
    v[0], v[64], v[128] = big, -big, 1.0
    assert pr.tree_sum(v) == 1.0
    # the second stage: lane j takes partials j, j + 256, ... from 0 - at 65 537 cells lane 0 takes two
    v = np.zeros(65537)
    v[0], v[65536], v[256] = big, 1.0, -big  # partials 0, 256 in lane 0: big + 1 = big; partial 1 in lane 1: -big
    assert pr.tree_sum(v) == 0.0
    v[0], v[65536], v[256] = big, -big, 1.0
    assert pr.tree_sum(v) == 1.0
    rng = np.random.default_rng(3)
    for n in (1, 63, 64, 65, 255, 256, 257, 65536, 65537, 73002):
        v = rng.normal(size=n) * 10.0 ** rng.integers(-3, 4, n)
        assert abs(pr.tree_sum(v) - math.fsum(v)) <= pr.tree_depth(n) * EPS * math.fsum(np.abs(v)), n
    assert [pr.tree_depth(n) for n in (1, 256, 65536, 65537, 73002)] == [21, 21, 21, 22, 22]
    assert sr.tree_sum is pr.tree_sum


def test_value_tree_is_value_within_the_tree_s_depth():
    X, cells = mg.kuhn_box(4, jitter=0.1)
    adj = pr.adjacency(X, cells)
    w = pr.weights(X, cells, adj, pr.TPFA)[0].astype(np.float64)
    x = np.random.default_rng(5).normal(size=len(cells))
    for penalty in (pr.QUADRATIC, pr.PSEUDO_HUBER):
        terms = pr.value_terms(w, adj, x, penalty, 0.5)
        assert (terms >= 0).all()
        exact, tree = pr.value(w, adj, x, 0.7, penalty, 0.5), pr.value_tree(w, adj, x, 0.7, penalty, 0.5)
        assert exact > 0 and abs(tree - exact) <= (pr.tree_depth(len(cells)) + 1) * EPS * exact
    vert = sr.welded_cells(X, cells)
    B, V0, _n = sr.rest(X, vert)
    xs = sr.displaced(X, vert)
    for energy in ENERGIES:
        exact, scale = sr.value(B, V0, vert, xs, energy, KAPPA, LAM, with_scale=True)
        assert abs(sr.value_tree(B, V0, vert, xs, energy, KAPPA, LAM) - exact) <= (pr.tree_depth(len(cells)) + 1) * EPS * scale
    turned = xs.copy()
    turned[vert[7][3]] = xs[vert[7][:3]].mean(axis=0) * 2.0 - xs[vert[7][3]]
    assert sr.quality(B, V0, vert, turned)[1] >= 1 and sr.value_tree(B, V0, vert, turned, sr.NEO_HOOKEAN, KAPPA, LAM) == math.inf
    assert np.isfinite(sr.value_tree(B, V0, vert, turned, sr.DIRICHLET, KAPPA, LAM))


# ---- the pseudo-Huber penalty over the format's range ------------------------------------------------------------------------------
def test_the_pseudo_huber_penalty_over_the_whole_range():
    cases = pr.huber_sweep()
    assert len(cases) > 1200
    tail = below = over = 0
    for delta, d in cases:
        want = pr.huber_at_80_digits(d, delta)
        got = (pr.psi(pr.PSEUDO_HUBER, np.float64(d), delta), pr.slope(pr.PSEUDO_HUBER, np.float64(d), delta),
               pr.curvature(pr.PSEUDO_HUBER, np.float64(d), delta))
        for name, g, w in zip(("psi", "slope", "curvature"), got, want):
            assert pr.huber_within_the_bar(float(g), w), (name, delta, d, float(g), float(w) if abs(w) < 1e308 else "beyond")
        with np.errstate(over="ignore"):
            u = abs(np.float64(d) / np.float64(delta))
            tail += u >= pr.TAIL
            below += u < pr.TAIL
            over += (u < pr.TAIL) and not np.float64(d) * np.float64(d) < np.inf
    assert tail > 100 and below > 100 and over > 10  # (every branch is met)
    # what the forms without the branches return there: the slope 0 and the value NaN - the negative control
    with np.errstate(all="ignore"):
        d, delta = np.float64(1e200), np.float64(1.0)
        u = d / delta
        assert d / np.sqrt(1.0 + u * u) == 0.0 and np.isnan((d * d) / (1.0 + np.sqrt(1.0 + u * u)))
    assert pr.slope(pr.PSEUDO_HUBER, d, 1.0) == 1.0 and pr.slope(pr.PSEUDO_HUBER, -d, 1.0) == -1.0
    assert pr.psi(pr.PSEUDO_HUBER, d, 1.0) == 1e200
    # a quotient d / delta that is itself inf
    assert pr.slope(pr.PSEUDO_HUBER, np.float64(-1e200), 1e-150) == -1e-150 and pr.psi(pr.PSEUDO_HUBER, np.float64(1e200), 1e-150) == 1e50
    assert pr.curvature(pr.PSEUDO_HUBER, np.float64(1e200), 1e-150) == 0.0
    # NaN in, NaN out: the branch does not turn it into a number
    assert all(np.isnan(f(pr.PSEUDO_HUBER, np.float64("nan"), 1.0)) for f in (pr.psi, pr.slope, pr.curvature))
    # arrays as before
    d = np.array([-3.5, 0.0, 1e-9, 2.0, 1e200])
    assert pr.slope(pr.PSEUDO_HUBER, d, 1.0).shape == (5,) and pr.slope(pr.PSEUDO_HUBER, d, 1.0)[4] == 1.0

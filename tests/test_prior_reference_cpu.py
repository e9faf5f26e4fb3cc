"""The numpy restatement of the smoothness prior (tests/prior_reference.py), pinned without a GPU: its adjacency against
c5_face_adjacency, its operators against a dense assembly, its penalties against 80-digit mpmath, the conditioning of the
GPU tests' grids, and the new entries of the ABI, the binding and the build."""
import ctypes as C

import numpy as np
import pytest

from course5_amd import build, capi, fit
from tests import prior_reference as pr

BAR = 8 * pr.EPS  # psi, psi', psi'' against mpmath, relative (the header's forms take at most 6 roundings each)


@pytest.fixture(scope="module")
def grids():
    return pr.grids()


def test_adjacency_is_c5_face_adjacency_s_over_welded_points(grids):
    for name, (xyz, cells) in grids.items():
        want, _nb = capi.face_adjacency(pr.welded_cells(xyz, cells).astype(np.int32), len(xyz))
        got = pr.adjacency(xyz, cells)
        assert np.array_equal(got, want), name
        # symmetric: the partner names the cell back, across exactly one face
        for c, f in zip(*np.nonzero(got >= 0)):
            assert (got[got[c, f]] == c).sum() == 1, (name, c, f)
    assert (pr.adjacency(*grids["one_tet"]) == -1).all()
    assert pr.n_interior_faces(pr.adjacency(*grids["cube8"])) > 0
    # neighbours through welding only: without it every face of the soup is a boundary face
    xyz, cells = grids["soup"]
    raw, _ = capi.face_adjacency(cells, len(xyz))
    assert (raw == -1).all() and pr.n_interior_faces(pr.adjacency(xyz, cells)) > 0
    with pytest.raises(ValueError, match="more than two"):
        pr.adjacency(*pr.three_on_a_face())


def test_the_interface_of_the_refined_grid_is_uncoupled():
    from course5_amd import meshgen as mg
    xyz, cells, n_coarse = mg.refined_interface(n=2)
    adj = pr.adjacency(xyz, cells)
    coarse = np.arange(len(cells)) < n_coarse
    for c, f in zip(*np.nonzero(adj >= 0)):
        assert coarse[c] == coarse[adj[c, f]], "a face couples the two sides of the non-conforming interface"
    assert pr.n_interior_faces(adj) > 0


def test_the_cross_products_of_the_gpu_grids_are_well_conditioned(grids):
    """The TPFA bar of tests/test_gpu_prior.py is 2^-52 (8 + 8 factor): below 100 it says something."""
    for name, (xyz, cells) in grids.items():
        adj = pr.adjacency(xyz, cells)
        w, factor = pr.weights(xyz, cells, adj, pr.TPFA)
        assert factor.max() < 100.0, (name, factor.max())
        assert ((w > 0) == (adj >= 0)).all() and np.isfinite(w.astype(np.float64)).all(), name
        # the weight belongs to the unordered pair
        for c, f in zip(*np.nonzero(adj >= 0)):
            n = adj[c, f]
            assert abs(w[c, f] - w[n, np.flatnonzero(adj[n] == c)[0]]) <= 4 * 2.0 ** -63 * w[c, f], (name, c, f)


def test_degenerate_faces_weigh_nothing():
    xyz = np.array([[0.0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0], [0, -1, 0]])  # the shared face (0, 1, 2) has no area
    cells = np.array([[0, 1, 2, 3], [0, 1, 2, 4]], dtype=np.int32)
    adj = pr.adjacency(xyz, cells)
    assert pr.n_interior_faces(adj) == 1
    w, _ = pr.weights(xyz, cells, adj, pr.TPFA)
    assert (w == 0).all()
    assert pr.weights(xyz, cells, adj, pr.UNIT)[0].sum() == 2


@pytest.mark.parametrize("grid", ["cube8", "kuhn2"])
@pytest.mark.parametrize("penalty", [pr.QUADRATIC, pr.PSEUDO_HUBER])
def test_operators_against_a_dense_assembly(grid, penalty):
    from course5_amd import meshgen as mg
    xyz, cells = mg.cube8() if grid == "cube8" else mg.kuhn_box(2)
    adj = pr.adjacency(xyz, cells)
    n = len(cells)
    rng = np.random.default_rng(3)
    x, p = rng.normal(size=n) * 10.0 ** rng.integers(-2, 3, n), rng.normal(size=n)
    lam, delta = 0.7, 0.5
    for weighting in (pr.UNIT, pr.TPFA):
        w = pr.weights(xyz, cells, adj, weighting)[0].astype(np.float64)
        L = pr.dense_laplacian(w, adj)
        if penalty == pr.QUADRATIC:
            want_g, want_v, Lx = lam * L @ x, 0.5 * lam * x @ L @ x, L
        else:
            d = x[:, None] - x[np.where(adj >= 0, adj, 0)]
            Lx = pr.dense_laplacian(w, adj, coefficient=(1.0 + (d / delta) ** 2) ** -1.5)
            want_g, want_v = np.zeros(n), 0.0
            for c in range(n):
                for f in range(4):
                    if adj[c, f] >= 0:
                        want_g[c] += lam * w[c, f] * d[c, f] / np.sqrt(1.0 + (d[c, f] / delta) ** 2)
                        want_v += 0.5 * lam * w[c, f] * delta ** 2 * np.expm1(0.5 * np.log1p((d[c, f] / delta) ** 2))
        tol = 1e-12
        got_g = pr.gradient(w, adj, x, lam, penalty, delta)
        assert np.abs(got_g - want_g).max() <= tol * np.abs(want_g).max()
        assert abs(pr.value(w, adj, x, lam, penalty, delta) - want_v) <= tol * want_v
        got_p = pr.product(w, adj, x, p, lam, penalty, delta)
        assert np.abs(got_p - lam * Lx @ p).max() <= tol * np.abs(lam * Lx @ p).max()
        got_d = pr.diagonal(w, adj, x, lam, penalty, delta)
        assert np.abs(got_d - lam * np.diag(Lx)).max() <= tol * np.abs(np.diag(Lx)).max() * lam
        # the header's identities
        if penalty == pr.QUADRATIC:
            assert np.array_equal(pr.gradient(w, adj, x, lam), pr.product(w, adj, None, x, lam))
            assert (pr.gradient(w, adj, np.full(n, 3.25), lam) == 0).all()
        # with_scale bounds the sum
        g, s = pr.gradient(w, adj, x, lam, penalty, delta, with_scale=True)
        assert (np.abs(g) <= s * (1 + 1e-15)).all()


def test_penalties_against_mpmath_and_the_ruled_out_form_fails():
    """psi, psi', psi'' at d / delta from 1e-12 to 1e12, every value within 8 x 2^-52 relative of 80 digits; the form
    delta^2 (sqrt(1 + t) - 1) is outside that at 1e-9 (it returns 0): the negative control."""
    import mpmath as mp  # (what tests/derivative_reference_mp.py uses)
    mp.mp.dps = 80
    rng = np.random.default_rng(17)
    worst = {"psi": 0.0, "slope": 0.0, "curvature": 0.0}
    for delta in (1.0, 0.37, 1e-3, 4.2e5):
        for k in range(-12, 13):
            for mant in (1.0, float(rng.uniform(1.0, 9.9)), -float(rng.uniform(1.0, 9.9))):
                d = np.float64(mant * 10.0 ** k * delta)
                md, mdelta = mp.mpf(float(d)), mp.mpf(delta)
                t = (md / mdelta) ** 2
                want = {"psi": mdelta ** 2 * (mp.sqrt(1 + t) - 1), "slope": md / mp.sqrt(1 + t), "curvature": (1 + t) ** mp.mpf(-1.5)}
                got = {"psi": pr.psi(pr.PSEUDO_HUBER, d, delta), "slope": pr.slope(pr.PSEUDO_HUBER, d, delta),
                       "curvature": pr.curvature(pr.PSEUDO_HUBER, d, delta)}
                for name in want:
                    err = float(abs(mp.mpf(float(got[name])) - want[name]) / abs(want[name]))
                    worst[name] = max(worst[name], err)
                    assert err <= BAR, (name, delta, float(d), err / pr.EPS)
    print({k: f"{v / pr.EPS:.2f} eps" for k, v in worst.items()})
    # the quadratic penalty is what a large delta tends to, and what the header says of it
    d = np.array([-3.5, 0.0, 1e-9, 2.0])
    assert np.array_equal(pr.psi(pr.PSEUDO_HUBER, d, 1e300), pr.psi(pr.QUADRATIC, d, 1.0))
    assert np.array_equal(pr.slope(pr.PSEUDO_HUBER, d, 1e300), d) and (pr.curvature(pr.PSEUDO_HUBER, d, 1e300) == 1).all()
    # negative control
    d, delta = np.float64(1e-9), 1.0
    want = mp.sqrt(1 + mp.mpf(float(d)) ** 2) - 1
    assert abs(mp.mpf(float(pr.psi_naive(d, delta))) - want) / want > BAR
    assert abs(mp.mpf(float(pr.psi(pr.PSEUDO_HUBER, d, delta))) - want) / want <= BAR


def test_abi_binding_and_build_carry_the_prior():
    lib = capi.load_library()
    vp, dp, lp, pp = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(capi.Prior)
    want = {"c5_prior_weights": [vp, C.c_int, dp, lp, lp], "c5_prior_weights_device": [vp, C.c_int, vp, lp, lp],
            "c5_prior_gradient": [vp, pp] + [dp] * 5, "c5_prior_gradient_device": [vp, pp] + [vp] * 5,
            "c5_prior_product": [vp, pp] + [dp] * 6, "c5_prior_product_device": [vp, pp] + [vp] * 6,
            "c5_prior_diagonal": [vp, pp] + [dp] * 4, "c5_prior_diagonal_device": [vp, pp] + [vp] * 4}
    for name, args in want.items():
        assert hasattr(lib, name) and name in capi.EXPORTS
        assert capi.SIGNATURES[name] == args and getattr(lib, name).argtypes == args
    assert lib.c5_abi_version() == 2
    assert C.sizeof(capi.Prior) == 40  # two int32, four doubles
    assert (capi.C5_PRIOR_QUADRATIC, capi.C5_PRIOR_PSEUDO_HUBER, capi.C5_PRIOR_UNIT, capi.C5_PRIOR_TPFA) == (0, 1, 0, 1)
    flags = dict(build.LIB_SOURCES)
    assert flags["prior_kernels.hip"] == ["-ffp-contract=off"] and "prior.hip" in flags
    assert "prior_kernels.hip" not in build.DEVICE_SOURCES and "prior_kernels.hpp" not in build.DEVICE_SOURCES
    # null context: refused before anything else, without a GPU
    assert lib.c5_prior_weights(None, 0, None, None, None) == capi.C5_ERR_INVALID
    assert lib.c5_prior_gradient(None, C.byref(capi.Prior()), None, None, None, None, None) == capi.C5_ERR_INVALID


def test_smoothness_prior_checks_its_arguments():
    for bad in (dict(penalty="huber"), dict(weighting="area"), dict(lambda_q=-1.0), dict(lambda_alpha=float("nan")),
                dict(penalty="pseudo_huber", lambda_q=1.0), dict(penalty="pseudo_huber", lambda_q=1.0, delta_q=0.0)):
        with pytest.raises(ValueError):
            fit.SmoothnessPrior(None, **bad)
    p = fit.SmoothnessPrior(None, lambda_q=2.0, penalty="pseudo_huber", delta_q=0.25).prior
    assert (p.penalty, p.weighting, p.lambda_alpha, p.lambda_q, p.delta_q) == (1, 1, 0.0, 2.0, 0.25)

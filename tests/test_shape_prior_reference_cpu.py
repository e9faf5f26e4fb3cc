"""The numpy restatement of the shape prior (tests/shape_prior_reference.py), pinned without a GPU: its rest data and
operators against 80-digit mpmath (which gives K, the constant of every bar), its gradient against the derivative of the
value, its product against the derivative of the gradient, the diagonal against the product, symmetry, the invariances, the
rest state, and the new entries of the ABI, the binding and the build."""
import ctypes as C
import inspect
import math

import numpy as np
import pytest

from course5_amd import build, capi, fit
from course5_amd import meshgen as mg
from tests import shape_prior_reference as sr

EPS, K = sr.EPS, sr.K
ENERGIES = (sr.DIRICHLET, sr.NEO_HOOKEAN)
KAPPA, LAM = 1.5, 0.75


class _Grid:
    def __init__(self, name, xyz, cells):
        self.name, self.X = name, np.ascontiguousarray(xyz, dtype=np.float64)
        self.vert = sr.welded_cells(xyz, cells)
        self.n_pts = len(self.X)
        self.B, self.V0, self.n_deg = sr.rest(self.X, self.vert)
        self.x = sr.displaced(self.X, self.vert, 0.08)
        rng = np.random.default_rng(7)
        self.v, self.u = rng.normal(size=(self.n_pts, 3)), rng.normal(size=(self.n_pts, 3))

    def args(self, energy):
        return self.B, self.V0, self.vert, self.n_pts, self.x, energy, KAPPA, LAM


@pytest.fixture(scope="module")
def grids():
    out = {"one_tet": sr.one_tet(), "cube8": mg.cube8(), "kuhn2": mg.kuhn_box(2, jitter=0.2)}
    return {k: _Grid(k, *g) for k, g in out.items()}


def _f(t):
    return float(t)


def _ratio(got, want_mp, scale):
    """max |got - want| / (2^-52 scale) over the entries whose scale is not 0 (where it is 0, got must be 0)."""
    mp = sr._mp()
    worst = 0.0
    got, scale = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(scale, dtype=np.float64).reshape(-1)
    for g, w, s in zip(got, want_mp, scale):
        if s == 0:
            assert g == 0 and abs(w) < mp.mpf(10) ** -60
            continue
        worst = max(worst, _f(abs(mp.mpf(float(g)) - w) / (mp.mpf(EPS) * mp.mpf(float(s)))))
    return worst


def _flat(rows):
    return [t for row in rows for t in row]


@pytest.fixture(scope="module")
def measured(grids):
    """{(quantity, grid, energy): worst ratio of the float64 restatement against 80 digits}."""
    mp = sr._mp()
    out = {}
    for name, g in grids.items():
        B, V0, _n, scale = sr.rest(g.X, g.vert, with_scale=True)
        want = []
        for c in range(len(V0)):
            Bc, _v = sr.mp_B(g.X[g.vert[c]])
            want += [Bc[r, k] for r in range(3) for k in range(3)]
        out[("B", name, None)] = _ratio(B, want, scale)
        for energy in ENERGIES:
            got, sc = sr.gradient(*g.args(energy), with_scale=True)
            out[("gradient", name, energy)] = _ratio(got, _flat(sr.mp_operator(*g.args(energy))), sc)
            got, sc = sr.product(g.B, g.V0, g.vert, g.n_pts, g.x, g.v, energy, KAPPA, LAM, with_scale=True)
            out[("product", name, energy)] = _ratio(got, _flat(sr.mp_operator(*g.args(energy), v=g.v)), sc)
            got, sc = sr.value(g.B, g.V0, g.vert, g.x, energy, KAPPA, LAM, with_scale=True)
            want = sr.mp_value(g.B, g.V0, g.vert, sr._mp_points(g.x), energy, KAPPA, LAM)
            out[("value", name, energy)] = _ratio([got], [want], [sc])
    assert mp.mp.dps == 80
    return out


def test_the_restatement_s_error_against_mpmath_gives_K(measured):
    for key, r in sorted(measured.items(), key=str):
        print(f"{key[0]:9s} {key[1]:8s} {'-' if key[2] is None else ('dirichlet', 'neo_hookean')[key[2]]:12s} {r:.3f} x 2^-52 of the terms' sum")
    worst = max(measured.values())
    want = 2.0 ** math.ceil(math.log2(4.0 * worst))
    print(f"worst ratio {worst:.3f}: K = 4 x that, rounded up to a power of two = {want:g}; tests/shape_prior_reference.py holds K = {K}")
    assert 4.0 * worst <= K
    assert K == max(want, 1.0)


@pytest.mark.parametrize("energy", ENERGIES)
def test_the_gradient_is_the_derivative_of_the_value(grids, energy):
    """d R / d x_(p, r) by a central difference in 80 digits (step 1e-25: truncation 1e-50 of the third derivative)."""
    mp = sr._mp()
    h = mp.mpf(10) ** -25
    for name, g in grids.items():
        got, sc = sr.gradient(*g.args(energy), with_scale=True)
        coords = [(p, r) for p in range(g.n_pts) for r in range(3)][::(4 if name == "kuhn2" else 1)]
        for p, r in coords:
            cells = np.flatnonzero((g.vert == p).any(axis=1))
            xs = sr._mp_points(g.x)

            def at(t):
                xs[p][r] = mp.mpf(float(g.x[p, r])) + t
                return sr.mp_value(g.B, g.V0, g.vert, xs, energy, KAPPA, LAM, cells=cells)

            want = (at(h) - at(-h)) / (2 * h)
            assert abs(mp.mpf(float(got[p, r])) - want) <= K * EPS * sc[p, r] + mp.mpf(10) ** -40, (name, p, r)


@pytest.mark.parametrize("energy", ENERGIES)
def test_the_product_is_the_derivative_of_the_gradient(grids, energy):
    mp = sr._mp()
    h = mp.mpf(10) ** -25
    for name, g in grids.items():
        got, sc = sr.product(g.B, g.V0, g.vert, g.n_pts, g.x, g.v, energy, KAPPA, LAM, with_scale=True)
        xs, vs = sr._mp_points(g.x), sr._mp_points(g.v)

        def grad_at(t):
            moved = [[a + t * b for a, b in zip(p, q)] for p, q in zip(xs, vs)]
            return _flat(sr.mp_operator(g.B, g.V0, g.vert, g.n_pts, moved, energy, KAPPA, LAM))

        want = [(a - b) / (2 * h) for a, b in zip(grad_at(h), grad_at(-h))]
        for i, (w, s) in enumerate(zip(want, sc.reshape(-1))):
            assert abs(mp.mpf(float(got.reshape(-1)[i])) - w) <= K * EPS * s + mp.mpf(10) ** -40, (name, i)


@pytest.mark.parametrize("energy", ENERGIES)
def test_the_diagonal_is_the_product_on_unit_vectors(grids, energy):
    for name, g in grids.items():
        diag = sr.diagonal(*g.args(energy))
        H = sr.dense_hessian(*g.args(energy))
        assert np.array_equal(diag.reshape(-1), np.diag(H)), name
        assert (diag[np.unique(g.vert)] > 0).all() if energy == sr.DIRICHLET else np.isfinite(diag).all()


@pytest.mark.parametrize("energy", ENERGIES)
def test_a_dense_assembly_is_symmetric(grids, energy):
    for name, g in grids.items():
        H = sr.dense_hessian(*g.args(energy))
        S = np.zeros_like(H)
        for j in range(3 * g.n_pts):
            e = np.zeros(3 * g.n_pts)
            e[j] = 1.0
            S[:, j] = sr.product(g.B, g.V0, g.vert, g.n_pts, g.x, e.reshape(-1, 3), energy, KAPPA, LAM, with_scale=True)[1].reshape(-1)
        assert (np.abs(H - H.T) <= K * EPS * (S + S.T)).all(), name
        assert np.abs(H).max() > 0
        # <u, H v> = <v, H u>
        hv = sr.product(g.B, g.V0, g.vert, g.n_pts, g.x, g.v, energy, KAPPA, LAM, with_scale=True)
        hu = sr.product(g.B, g.V0, g.vert, g.n_pts, g.x, g.u, energy, KAPPA, LAM, with_scale=True)
        terms = (np.abs(g.u) * hv[1]).sum() + (np.abs(g.v) * hu[1]).sum()
        assert abs((g.u * hv[0]).sum() - (g.v * hu[0]).sum()) <= (K + 3 * g.n_pts) * EPS * terms, name


def _rotation():
    a, b = 0.7, -0.4
    Rz = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]])
    return Rz @ Rx


def test_invariances(grids):
    """Neo-Hookean: value and gradient norm under a rotation of x; both energies under a translation.  The moved
    coordinates are rounded (and the rotation matrix orthogonal only to 2^-52), so the bar is the terms' sum times K 2^-52
    plus the derivative times the coordinates' rounding: 8 x 2^-52 |x| |grad| and |Hess| likewise through the scales."""
    R = _rotation()
    for name, g in grids.items():
        for energy in ENERGIES:
            v0, s0 = sr.value(g.B, g.V0, g.vert, g.x, energy, KAPPA, LAM, with_scale=True)
            g0, gs = sr.gradient(*g.args(energy), with_scale=True)
            moves = [g.x + np.array([0.25, -1.5, 0.75])] + ([g.x @ R.T] if energy == sr.NEO_HOOKEAN else [])
            for moved in moves:
                slack = 8 * EPS * np.abs(moved).max() * np.abs(g0).sum()
                v1 = sr.value(g.B, g.V0, g.vert, moved, energy, KAPPA, LAM)
                assert abs(v1 - v0) <= K * EPS * s0 + slack, (name, energy)
                g1 = sr.gradient(g.B, g.V0, g.vert, g.n_pts, moved, energy, KAPPA, LAM)
                hs = sr.product(g.B, g.V0, g.vert, g.n_pts, g.x, np.ones_like(g.x), energy, KAPPA, LAM, with_scale=True)[1]
                bar = K * EPS * np.linalg.norm(gs) + 8 * EPS * np.abs(moved).max() * np.linalg.norm(hs)
                assert abs(np.linalg.norm(g1) - np.linalg.norm(g0)) <= bar, (name, energy)
    # the Dirichlet energy is NOT invariant under rotation: the control
    g = grids["cube8"]
    assert abs(sr.value(g.B, g.V0, g.vert, g.x @ R.T, sr.DIRICHLET, KAPPA, LAM) - sr.value(g.B, g.V0, g.vert, g.x, sr.DIRICHLET, KAPPA, LAM)) > 1e-3


def test_at_rest_the_value_and_the_gradient_vanish(grids):
    for name, g in grids.items():
        for energy in ENERGIES:
            v, s = sr.value(g.B, g.V0, g.vert, g.X, energy, KAPPA, LAM, with_scale=True)
            assert abs(v) <= K * EPS * s, (name, energy, v)
            got, sc = sr.gradient(g.B, g.V0, g.vert, g.n_pts, g.X, energy, KAPPA, LAM, with_scale=True)
            assert (np.abs(got) <= K * EPS * sc).all(), (name, energy)
            assert sr.quality(g.B, g.V0, g.vert, g.X)[1] == 0
        # and away from it they do not
        assert sr.value(g.B, g.V0, g.vert, g.x, sr.NEO_HOOKEAN, KAPPA, LAM) > 0
        assert sr.quality(g.B, g.V0, g.vert, g.x)[1] == 0


def test_inverted_and_degenerate_cells():
    X, cells = sr.with_a_flat_cell()
    vert = sr.welded_cells(X, cells)
    B, V0, n_deg = sr.rest(X, vert)
    assert n_deg == 1 and V0[-1] == 0 and (B[-1] == 0).all() and (V0[:-1] > 0).all()
    x = sr.displaced(X, vert)
    ratio, n_inv = sr.quality(B, V0, vert, x)
    assert n_inv == 0 and ratio[-1] == 0 and (ratio[:-1] > 0.5).all()
    # the flat cell's points get nothing
    g = sr.gradient(B, V0, vert, len(X), x, sr.NEO_HOOKEAN, KAPPA, LAM)
    assert (g[-4:] == 0).all() and np.abs(g[:-4]).max() > 0
    # one vertex through its opposite face
    X, cells = sr.one_tet()
    vert = sr.welded_cells(X, cells)
    B, V0, _n = sr.rest(X, vert)
    x = X.copy()
    centre = X[:3].mean(axis=0)
    x[3] = centre - 0.5 * (X[3] - centre)
    ratio, n_inv = sr.quality(B, V0, vert, x)
    assert n_inv == 1 and ratio[0] == pytest.approx(-0.5)
    assert sr.value(B, V0, vert, x, sr.NEO_HOOKEAN, KAPPA, LAM) == math.inf
    assert (sr.gradient(B, V0, vert, 4, x, sr.NEO_HOOKEAN, KAPPA, LAM) == 0).all()
    assert np.isfinite(sr.value(B, V0, vert, x, sr.DIRICHLET, KAPPA, LAM))
    assert np.abs(sr.gradient(B, V0, vert, 4, x, sr.DIRICHLET, KAPPA, LAM)).max() > 0


def test_the_gpu_grids_are_displaced_without_inverting(grids):
    for name, (X, cells) in sr.grids().items():
        vert = sr.welded_cells(X, cells)
        B, V0, n_deg = sr.rest(X, vert)
        x = sr.displaced(X, vert)
        ratio, n_inv = sr.quality(B, V0, vert, x)
        live = V0 > 0
        print(f"{name}: {len(V0)} cells, {n_deg} degenerate, J in [{ratio[live].min():.3f}, {ratio[live].max():.3f}]")
        assert n_inv == 0 and n_deg == (1 if name == "flat" else 0), name
        assert np.abs(x - X).max() > 0 and 0.5 < ratio[live].min() and ratio[live].max() < 2.0, name
    from tests import unstructured_scenes as us
    assert us.describe(sr.STAR_SEED)["point_valence"] >= 200


def test_abi_binding_and_build_carry_the_shape_prior():
    lib = capi.load_library()
    vp, dp, lp, ip, sp = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(capi.ShapePrior)
    want = {"c5_shape_prior_rest": [vp, dp, C.c_int64, lp], "c5_shape_prior_rest_device": [vp, vp, C.c_int64, lp],
            "c5_shape_prior_rest_data": [vp, dp, dp, ip], "c5_shape_prior_rest_data_device": [vp, vp, vp, vp],
            "c5_shape_prior_gradient": [vp, sp, dp, dp, lp, dp], "c5_shape_prior_gradient_device": [vp, sp, vp, vp, vp, vp],
            "c5_shape_prior_product": [vp, sp, dp, dp, dp], "c5_shape_prior_product_device": [vp, sp, vp, vp, vp],
            "c5_shape_prior_diagonal": [vp, sp, dp, dp], "c5_shape_prior_diagonal_device": [vp, sp, vp, vp],
            "c5_shape_prior_quality": [vp, dp, dp, lp], "c5_shape_prior_quality_device": [vp, vp, vp, vp]}
    for name, args in want.items():
        assert hasattr(lib, name) and name in capi.EXPORTS
        assert capi.SIGNATURES[name] == args and getattr(lib, name).argtypes == args
    assert C.sizeof(capi.ShapePrior) == 24  # two int32, two doubles
    assert (capi.C5_SHAPE_DIRICHLET, capi.C5_SHAPE_NEO_HOOKEAN) == (0, 1)
    # the header declares them with these parameter lists
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "course5_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    kinds = {"const double*": dp, "double*": dp, "const void*": vp, "void*": vp, "int64_t*": lp, "int32_t*": ip, "int64_t": C.c_int64,
             "c5_context*": vp, "const c5_shape_prior*": sp}
    for name, args in want.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, name
        declared = [kinds[" ".join(p.split()[:-1])] for p in m.group(1).split(",")]
        assert declared == args, name
    flags = dict(build.LIB_SOURCES)
    assert flags["shape_prior_kernels.hip"] == ["-ffp-contract=off"] and "shape_prior.hip" in flags
    assert "shape_prior_kernels.hip" not in build.DEVICE_SOURCES and "shape_prior_kernels.hpp" not in build.DEVICE_SOURCES
    # null context: refused before anything else, without a GPU
    P = capi.ShapePrior(capi.C5_SHAPE_DIRICHLET, 1.0)
    assert lib.c5_shape_prior_rest(None, None, 0, None) == capi.C5_ERR_INVALID
    assert lib.c5_shape_prior_gradient(None, C.byref(P), None, None, None, None) == capi.C5_ERR_INVALID
    assert lib.c5_shape_prior_quality_device(None, None, None, None) == capi.C5_ERR_INVALID


def test_nothing_that_exists_changed():
    assert build.kernel_source_hash() == "63c90aeb24365e47"
    assert capi.load_library().c5_abi_version() == 2
    assert list(inspect.signature(fit.shape_step).parameters) == ["ctx", "alpha", "q", "residual", "weight", "damping", "iters", "free"]
    assert list(inspect.signature(fit.shape_gradient).parameters) == ["ctx", "alpha", "q", "residual", "weight"]


def test_shape_prior_checks_its_arguments():
    for bad in (dict(lam=-1.0), dict(lam=float("nan")), dict(lam=1.0, energy="hooke"), dict(lam=1.0, kappa=-0.5), dict(lam=1.0, kappa=float("inf"))):
        with pytest.raises(ValueError):
            fit.ShapePrior(None, **bad)
    p = fit.ShapePrior(None, 2.0, energy="dirichlet", kappa=0.25).prior
    assert (p.energy, p.reserved, p.lambda_, p.kappa) == (0, 0, 2.0, 0.25)
    assert fit.ShapePrior(None, 1.0).prior.energy == capi.C5_SHAPE_NEO_HOOKEAN

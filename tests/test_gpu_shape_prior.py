"""The shape prior on the GPU (c5_shape_prior_*, capi.Context.shape_prior_*) against the numpy restatement
(tests/shape_prior_reference.py) fed the library's own rest data: the Dirichlet operators bit for bit, the Neo-Hookean ones
and the value within K x 2^-52 x (the terms' absolute sum) - K from tests/test_shape_prior_reference_cpu.py - symmetry, the
rest state's life, welding, degenerate and inverted cells, and the contract's edges.

The grids are shape_prior_reference.grids(): one tetrahedron, cube8, kuhn_box(4) (384 cells: the second 256-thread block is
partial), kuhn_box(9) with the caller's ids permuted (4 374 cells: the device keeps them in Morton order), a soup of per-cell
point copies (welding), a refined interface (non-conforming-style connectivity), an unstructured star (a point in 368
cells: a long incidence list) and cube8 with one flat rest cell.  x is the rest shape plus a smooth displacement of 7 % of
the local cell size; the CPU test confirms that the restatement finds no inverted cell there.  One context per grid for the
whole module; no image and no view is ever set."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from course5_amd import capi
from course5_amd import meshgen as mg
from tests import prior_reference as pr
from tests import shape_prior_reference as sr

pytestmark = pytest.mark.gpu
EPS, K = sr.EPS, sr.K
GRIDS = ("one_tet", "cube8", "kuhn4", "kuhn9", "soup", "interface", "star", "flat")
ENERGIES = (sr.DIRICHLET, sr.NEO_HOOKEAN)
KAPPA, LAM = 1.5, 0.75


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _prior(energy, lam=LAM, kappa=KAPPA):
    return capi.ShapePrior(energy, lam, kappa)


def _context(xyz, cells, cell_order=1):
    ctx = capi.Context(0)
    ctx.set_option("cell_order", cell_order)
    ctx.upload_grid(xyz, cells, np.ones(len(cells)), np.ones(len(cells)))  # (the scalars play no part)
    return ctx


class _Case:
    def __init__(self, name, X, cells):
        self.name, self.X, self.cells, self.n_pts, self.n = name, X, cells, len(X), len(cells)
        self.ctx = _context(X, cells)
        self.n_deg = self.ctx.shape_prior_rest(X)
        self.B, self.V0, vert = self.ctx.shape_prior_rest_data()
        self.vert = vert.astype(np.int64)
        self.x = sr.displaced(X, self.vert)
        rng = np.random.default_rng(31)
        self.v, self.u = rng.normal(size=(self.n_pts, 3)), rng.normal(size=(self.n_pts, 3))

    def ref(self, what, energy, x="x", v=None, lam=LAM, with_scale=False):
        x = self.x if isinstance(x, str) else x
        args = (self.B, self.V0, self.vert, self.n_pts, x)
        if what == "product":
            return sr.product(*args, self.v if v is None else v, energy, KAPPA, lam, with_scale=with_scale)
        return getattr(sr, what)(*args, energy, KAPPA, lam, with_scale=with_scale)


@pytest.fixture(scope="module")
def cases():
    out = {name: _Case(name, *g) for name, g in sr.grids().items()}
    assert out["kuhn4"].n == 384 and out["kuhn9"].n == 4374 and set(out) == set(GRIDS)
    yield out
    for c in out.values():
        c.ctx.close()


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def _device_ops(ctx, P, x, v):
    """(value, n_inverted, gradient, product, diagonal) from the _device forms."""
    n = ctx.n_pts
    xs, vs = (None if x is None else _dev(x)), _dev(v)
    value = torch.full((1,), 7.0, dtype=torch.float64, device="cuda")
    n_inv = torch.full((1,), 7, dtype=torch.int64, device="cuda")
    g, h, d = (torch.full((n, 3), 7.0, dtype=torch.float64, device="cuda") for _ in range(3))
    torch.cuda.synchronize()
    if xs is not None:
        ctx.shape_prior_gradient_device(P, xs, value, n_inv, g)
    ctx.shape_prior_product_device(P, xs, vs, h)
    ctx.shape_prior_diagonal_device(P, xs, d)
    ctx.synchronize()
    return float(value.cpu()[0]), int(n_inv.cpu()[0]), g.cpu().numpy(), h.cpu().numpy(), d.cpu().numpy()


def _host_ops(ctx, P, x, v):
    value, n_inv, g = ctx.shape_prior_gradient(P, x)
    return value, n_inv, g, ctx.shape_prior_product(P, x, v), ctx.shape_prior_diagonal(P, x)


# ---- rest data -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
def test_rest_data(cases, grid):
    c = cases[grid]
    welded = sr.welded_cells(c.X, c.cells)
    assert np.array_equal(np.sort(c.vert, axis=1), np.sort(welded, axis=1))  # the representatives, in the arithmetic's order
    B, V0, n_deg, scale = sr.rest(c.X, c.vert, with_scale=True)
    assert c.n_deg == n_deg == (1 if grid == "flat" else 0)
    _C, _det, _aC, adet = sr._cofactors(sr._edges(c.X, c.vert))
    err_b, err_v = np.abs(c.B - B), np.abs(c.V0 - V0)
    live = V0 > 0
    worst_b = (err_b / (EPS * np.where(scale > 0, scale, 1.0))).max()
    print(f"{grid}: B worst {worst_b:.2f}, V0 worst {(err_v[live] / (EPS * adet[live] / 6)).max():.2f} x 2^-52 of the terms' sum")
    assert (err_b <= K * EPS * scale).all() and (err_v <= K * EPS * adet / 6.0).all()
    assert ((c.V0 > 0) == live).all() and (c.B[~live] == 0).all()
    # the device form, and every output may be left out
    b, v, t = (torch.zeros(s, dtype=d, device="cuda") for s, d in (((c.n, 3, 3), torch.float64), ((c.n,), torch.float64), ((c.n, 4), torch.int32)))
    c.ctx.shape_prior_rest_data_device(b, v, t)
    c.ctx.shape_prior_rest_data_device(None, None, None)
    c.ctx.synchronize()
    assert _same(b.cpu().numpy(), c.B) and _same(v.cpu().numpy(), c.V0) and np.array_equal(t.cpu().numpy(), c.vert)
    assert c.ctx.lib.c5_shape_prior_rest_data(c.ctx.handle, None, None, None) == capi.C5_OK


# ---- the Dirichlet operators: bit for bit --------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
def test_dirichlet_operators_are_the_restatement_s_bits(cases, grid):
    c, ctx = cases[grid], cases[grid].ctx
    P = _prior(sr.DIRICHLET)
    want = (c.ref("gradient", sr.DIRICHLET), c.ref("product", sr.DIRICHLET), c.ref("diagonal", sr.DIRICHLET))
    host, device = _host_ops(ctx, P, c.x, c.v), _device_ops(ctx, P, c.x, c.v)
    for name, w, h, d in zip(("gradient", "product", "diagonal"), want, host[2:], device[2:]):
        assert _same(h, w), (name, "host")
        assert _same(d, w), (name, "device")
    assert host[1] == device[1] == 0 and _bits(host[0]) == _bits(device[0])
    # the point is ignored by product and diagonal: NULL, and anything else
    far = c.x * 3.0 + 1.0
    for x in (None, far):
        assert _same(ctx.shape_prior_product(P, x, c.v), want[1]) and _same(ctx.shape_prior_diagonal(P, x), want[2])
    assert _same(_device_ops(ctx, P, None, c.v)[3], want[1])
    # the diagonal is the product on unit vectors (a few of them)
    for p, r in ((0, 0), (c.n_pts // 2, 1), (c.n_pts - 1, 2)):
        e = np.zeros((c.n_pts, 3))
        e[p, r] = 1.0
        assert ctx.shape_prior_product(P, None, e)[p, r] == host[4][p, r]
    # lambda multiplies last
    assert _same(ctx.shape_prior_gradient(_prior(sr.DIRICHLET, lam=3.5), c.x)[2], c.ref("gradient", sr.DIRICHLET, lam=3.5))


# ---- the Neo-Hookean operators and the value ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
def test_neo_hookean_operators_against_the_restatement(cases, grid):
    c, ctx = cases[grid], cases[grid].ctx
    P = _prior(sr.NEO_HOOKEAN)
    host, device, again = _host_ops(ctx, P, c.x, c.v), _device_ops(ctx, P, c.x, c.v), _host_ops(ctx, P, c.x, c.v)
    for name, h, d, a in zip(("gradient", "product", "diagonal"), host[2:], device[2:], again[2:]):
        want, scale = c.ref(name, sr.NEO_HOOKEAN, with_scale=True)
        err = np.abs(h - want)
        print(f"{grid} {name}: worst error {(err / np.where(scale > 0, scale, 1.0)).max() / EPS:.2f} x 2^-52 of the terms' sum")
        assert (err <= K * EPS * scale).all(), name
        assert _same(d, h) and _same(a, h), name
        assert np.isfinite(h).all()
    assert host[1] == device[1] == 0
    p, r = c.n_pts // 2, 1
    e = np.zeros((c.n_pts, 3))
    e[p, r] = 1.0
    assert ctx.shape_prior_product(P, c.x, e)[p, r] == host[4][p, r]


@pytest.mark.parametrize("energy", ENERGIES)
@pytest.mark.parametrize("grid", GRIDS)
def test_value(cases, grid, energy):
    c, ctx = cases[grid], cases[grid].ctx
    P = _prior(energy)
    value = ctx.shape_prior_gradient(P, c.x)[0]
    want, scale = sr.value(c.B, c.V0, c.vert, c.x, energy, KAPPA, LAM, with_scale=True)
    print(f"{grid}: value {value:.17g}, error {abs(value - want) / (EPS * scale):.3f} x 2^-52 of the terms' sum")
    assert want > 0 and abs(value - want) <= K * EPS * scale
    assert _bits(ctx.shape_prior_gradient(P, c.x)[0]) == _bits(value) == _bits(_device_ops(ctx, P, c.x, c.v)[0])
    # at rest: the restatement's value and gradient there within the bar (that those vanish is the CPU test's business: on
    # the star's slivers F - I at rest is the rounding of B, which the cells' conditioning magnifies)
    v0, _n, g0 = ctx.shape_prior_gradient(P, c.X)
    want0, scale0 = sr.value(c.B, c.V0, c.vert, c.X, energy, KAPPA, LAM, with_scale=True)
    want_g0, gs = c.ref("gradient", energy, x=c.X, with_scale=True)
    assert abs(v0 - want0) <= K * EPS * scale0 and (np.abs(g0 - want_g0) <= K * EPS * gs).all()
    if grid != "star":
        assert abs(v0) <= K * EPS * scale0 and (np.abs(g0) <= K * EPS * gs).all()
    # value and n_inverted may be NULL
    g = np.zeros((c.n_pts, 3))
    assert ctx.lib.c5_shape_prior_gradient(ctx.handle, C.byref(P), capi._dp(c.x), None, None, capi._dp(g)) == capi.C5_OK
    assert _same(g, ctx.shape_prior_gradient(P, c.x)[2])


@pytest.mark.parametrize("energy", ENERGIES)
def test_the_hessian_is_symmetric(cases, energy):
    for name in ("cube8", "kuhn4", "kuhn9", "star"):
        c, ctx = cases[name], cases[name].ctx
        P = _prior(energy)
        hv, hu = ctx.shape_prior_product(P, c.x, c.v), ctx.shape_prior_product(P, c.x, c.u)
        sv = c.ref("product", energy, with_scale=True)[1]
        su = c.ref("product", energy, v=c.u, with_scale=True)[1]
        terms = math.fsum((np.abs(c.u) * sv).reshape(-1)) + math.fsum((np.abs(c.v) * su).reshape(-1))
        diff = abs(math.fsum((c.u * hv).reshape(-1)) - math.fsum((c.v * hu).reshape(-1)))
        print(f"{name}: <u, Hv> - <v, Hu> = {diff / (EPS * terms):.3f} x 2^-52 of the terms' sum")
        assert diff <= K * EPS * terms, name


# ---- cell order, contexts ----------------------------------------------------------------------------------------------------------
def test_nothing_depends_on_the_cell_order_or_the_context(cases):
    for name in ("kuhn4", "kuhn9", "soup", "star"):
        c = cases[name]
        with _context(c.X, c.cells, cell_order=0) as plain, _context(c.X, c.cells) as fresh:
            for ctx in (plain, fresh):
                assert ctx.shape_prior_rest(c.X) == c.n_deg
                B, V0, vert = ctx.shape_prior_rest_data()
                assert _same(B, c.B) and _same(V0, c.V0) and np.array_equal(vert, c.vert), name
            for energy in ENERGIES:
                P = _prior(energy)
                want = _host_ops(c.ctx, P, c.x, c.v)
                for a, b in zip(_host_ops(plain, P, c.x, c.v)[2:], want[2:]):  # (the vectors; the value is summed in the device's order)
                    assert _same(a, b), (name, energy, "cell_order 0")
                for a, b in zip(_device_ops(plain, P, c.x, c.v)[2:], want[2:]):
                    assert _same(a, b), (name, energy, "cell_order 0, device")
                got = _host_ops(fresh, P, c.x, c.v)
                assert _bits(got[0]) == _bits(want[0]) and all(_same(a, b) for a, b in zip(got[2:], want[2:])), (name, energy, "fresh")
                assert _same(plain.shape_prior_quality(c.x)[0], c.ctx.shape_prior_quality(c.x)[0])


# ---- the rest state -------------------------------------------------------------------------------------------------------------------
def test_the_rest_state_outlives_update_points_and_not_upload_grid(cases):
    c = cases["kuhn4"]
    P = _prior(sr.NEO_HOOKEAN)
    moved = sr.displaced(c.X, c.vert, 0.09, phase=1.0)
    with _context(c.X, c.cells) as ctx, _context(c.X, c.cells) as other:
        x = np.zeros((c.n_pts, 3))
        # before a rest shape is set: every call but _rest
        for call in (lambda: ctx.shape_prior_rest_data(), lambda: ctx.shape_prior_gradient(P, c.x), lambda: ctx.shape_prior_product(P, c.x, c.v),
                     lambda: ctx.shape_prior_diagonal(P, c.x), lambda: ctx.shape_prior_quality(c.x)):
            with pytest.raises(capi.C5Error) as e:
                call()
            assert e.value.code == capi.C5_ERR_STATE and "rest" in e.value.message
        assert ctx.shape_prior_rest(c.X) == 0
        before = ctx.shape_prior_rest_data()
        g = ctx.shape_prior_gradient(P, c.x)
        ctx.update_points(moved)
        after = ctx.shape_prior_rest_data()
        assert all(np.array_equal(a, b) for a, b in zip(before, after))
        assert _same(ctx.shape_prior_gradient(P, c.x)[2], g[2])
        # rest = NULL: the points the context holds now, i.e. the moved ones
        assert ctx.shape_prior_rest(None) == 0
        assert other.shape_prior_rest(moved) == 0
        a, b = ctx.shape_prior_rest_data(), other.shape_prior_rest_data()
        assert _same(a[0], b[0]) and _same(a[1], b[1]) and not _same(a[0], before[0])
        assert other.shape_prior_rest_device(_dev(moved)) == 0 and _same(other.shape_prior_rest_data()[0], a[0])
        assert abs(ctx.shape_prior_gradient(P, moved)[0]) <= K * EPS * sr.value(a[0], a[1], c.vert, moved, sr.NEO_HOOKEAN, KAPPA, LAM, with_scale=True)[1]
        # a new upload drops the rest shape
        ctx.upload_grid(c.X, c.cells, np.ones(c.n), np.ones(c.n))
        with pytest.raises(capi.C5Error) as e:
            ctx.shape_prior_gradient(P, x)
        assert e.value.code == capi.C5_ERR_STATE


def test_welded_points_get_zero_and_their_representative_the_group_s_sum():
    X, cells = mg.kuhn_box(2, jitter=0.1)
    sX, scells = mg.per_cell_point_copies(X, cells)
    rep, _merged = capi.weld_points(sX)
    with _context(X, cells) as indexed, _context(sX, scells) as soup:
        assert indexed.shape_prior_rest(X) == 0 and soup.shape_prior_rest(sX) == 0
        vert = indexed.shape_prior_rest_data()[2].astype(np.int64)
        x = sr.displaced(X, vert)
        sx = x[cells.reshape(-1)]
        garbage = sx.copy()
        garbage[rep != np.arange(len(rep))] = 1e6  # a welded point's own coordinates are ignored
        assert np.array_equal(sX, X[cells.reshape(-1)]) and np.array_equal(scells.reshape(-1), np.arange(len(sX)))
        first = np.full(len(X), len(sX))
        np.minimum.at(first, cells.reshape(-1), np.arange(len(sX)))  # point p of the indexed grid -> its first copy, the representative
        assert np.array_equal(rep[first], first)
        for energy in ENERGIES:
            P = _prior(energy)
            want = _host_ops(indexed, P, x, np.ones_like(x))
            for sxx in (sx, garbage):
                got = _host_ops(soup, P, sxx, np.ones_like(sx))
                assert _bits(got[0]) == _bits(want[0])
                for a, b in zip(got[2:], want[2:]):
                    assert (a[rep != np.arange(len(rep))] == 0).all() and _same(a[first], b), energy


def test_a_degenerate_rest_cell_is_counted_and_contributes_nothing(cases):
    flat, cube = cases["flat"], cases["cube8"]
    assert flat.n_deg == 1 and flat.V0[-1] == 0 and (flat.B[-1] == 0).all()
    ratio, n_inv = flat.ctx.shape_prior_quality(flat.x)
    assert n_inv == 0 and ratio[-1] == 0
    for energy in ENERGIES:
        P = _prior(energy)
        got, want = _host_ops(flat.ctx, P, flat.x, flat.v), _host_ops(cube.ctx, P, flat.x[:cube.n_pts], flat.v[:cube.n_pts])
        assert _bits(got[0]) == _bits(want[0]) and got[1] == 0
        for a, b in zip(got[2:], want[2:]):
            assert (a[-4:] == 0).all() and _same(a[:-4], b)


# ---- inverted cells ---------------------------------------------------------------------------------------------------------------------
def test_a_vertex_pushed_through_its_opposite_face(cases):
    c, ctx = cases["one_tet"], cases["one_tet"].ctx
    x = c.X.copy()
    k = int(c.vert[0][3])
    centre = c.X[c.vert[0][:3]].mean(axis=0)
    x[k] = centre - 0.5 * (c.X[k] - centre)
    ratio, n_inv = ctx.shape_prior_quality(x)
    want, want_inv = sr.quality(c.B, c.V0, c.vert, x)
    F = sr._times_b(sr._edges(x, c.vert), c.B)
    adet = sr._cofactors(F)[3]
    assert n_inv == want_inv == 1 and ratio[0] < 0 and abs(ratio[0] - want[0]) <= K * EPS * adet[0]
    assert ratio[0] == pytest.approx(-0.5, rel=1e-12)
    for energy in ENERGIES:
        P = _prior(energy)
        for value, n, g, h, d in (_host_ops(ctx, P, x, c.v), _device_ops(ctx, P, x, c.v)):
            assert n == 1
            assert np.isfinite(g).all() and np.isfinite(h).all() and np.isfinite(d).all()
            if energy == sr.NEO_HOOKEAN:
                assert value == math.inf and (g == 0).all() and (h == 0).all() and (d == 0).all()
            else:
                assert np.isfinite(value) and _same(g, c.ref("gradient", energy, x=x))
    # among many cells: the count and the ratios are the restatement's, the vectors stay finite, the other cells contribute
    c, ctx = cases["kuhn9"], cases["kuhn9"].ctx
    x = c.x.copy()
    cell = 1234
    k = int(c.vert[cell][3])
    centre = c.x[c.vert[cell][:3]].mean(axis=0)
    x[k] = centre - 0.5 * (c.x[k] - centre)
    ratio, n_inv = ctx.shape_prior_quality(x)
    want, want_inv = sr.quality(c.B, c.V0, c.vert, x)
    assert n_inv == want_inv >= 1 and ratio[cell] < 0 and np.array_equal(ratio <= 0, want <= 0)
    adet = sr._cofactors(sr._times_b(sr._edges(x, c.vert), c.B))[3]
    assert (np.abs(ratio - want) <= K * EPS * adet).all()
    P = _prior(sr.NEO_HOOKEAN)
    value, n, g = ctx.shape_prior_gradient(P, x)
    want_g, scale = c.ref("gradient", sr.NEO_HOOKEAN, x=x, with_scale=True)
    assert value == math.inf and n == want_inv and np.isfinite(g).all() and (np.abs(g - want_g) <= K * EPS * scale).all()
    n_dev = torch.zeros(1, dtype=torch.int64, device="cuda")
    ctx.shape_prior_quality_device(_dev(x), None, n_dev)
    ctx.synchronize()
    assert int(n_dev.cpu()[0]) == want_inv
    assert ctx.shape_prior_gradient(_prior(sr.DIRICHLET), x)[1] == want_inv


# ---- the contract's edges ------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused_and_leave_everything_alone(cases):
    c, ctx = cases["cube8"], cases["cube8"].ctx
    lib, h, dp = ctx.lib, ctx.handle, capi._dp
    nan, inf = float("nan"), float("inf")
    bad = [capi.ShapePrior(2, 1.0, 1.0), capi.ShapePrior(-1, 1.0, 1.0), capi.ShapePrior(sr.DIRICHLET, -1.0, 1.0), capi.ShapePrior(sr.DIRICHLET, nan, 1.0),
           capi.ShapePrior(sr.NEO_HOOKEAN, inf, 1.0), capi.ShapePrior(sr.NEO_HOOKEAN, 1.0, -0.5), capi.ShapePrior(sr.NEO_HOOKEAN, 1.0, nan),
           capi.ShapePrior(sr.NEO_HOOKEAN, 1.0, inf), capi.ShapePrior(sr.DIRICHLET, 1.0, 1.0, reserved=1)]
    x, v = np.ascontiguousarray(c.x), np.ascontiguousarray(c.v)
    for P in bad:
        value, n_inv, out = np.full(1, 7.0), C.c_int64(7), np.full((c.n_pts, 3), 7.0)
        calls = (lambda: lib.c5_shape_prior_gradient(h, C.byref(P), dp(x), dp(value), C.byref(n_inv), dp(out)),
                 lambda: lib.c5_shape_prior_product(h, C.byref(P), dp(x), dp(v), dp(out)),
                 lambda: lib.c5_shape_prior_diagonal(h, C.byref(P), dp(x), dp(out)))
        for call in calls:
            assert call() == capi.C5_ERR_INVALID and lib.c5_last_error(h)
        assert value[0] == 7 and n_inv.value == 7 and (out == 7).all()
    # NULL arrays
    out = np.full((c.n_pts, 3), 7.0)
    for P in (_prior(sr.DIRICHLET), _prior(sr.NEO_HOOKEAN)):
        assert lib.c5_shape_prior_gradient(h, C.byref(P), None, None, None, dp(out)) == capi.C5_ERR_INVALID
        assert lib.c5_shape_prior_gradient(h, C.byref(P), dp(x), None, None, None) == capi.C5_ERR_INVALID
        assert lib.c5_shape_prior_product(h, C.byref(P), dp(x), None, dp(out)) == capi.C5_ERR_INVALID
        assert lib.c5_shape_prior_product(h, C.byref(P), dp(x), dp(v), None) == capi.C5_ERR_INVALID
        assert lib.c5_shape_prior_diagonal(h, C.byref(P), dp(x), None) == capi.C5_ERR_INVALID
    P = _prior(sr.NEO_HOOKEAN)  # (its Hessian needs the point)
    assert lib.c5_shape_prior_product(h, C.byref(P), None, dp(v), dp(out)) == capi.C5_ERR_INVALID
    assert lib.c5_shape_prior_diagonal(h, C.byref(P), None, dp(out)) == capi.C5_ERR_INVALID
    assert lib.c5_shape_prior_gradient(h, None, dp(x), None, None, dp(out)) == capi.C5_ERR_INVALID
    assert lib.c5_shape_prior_quality(h, None, None, None) == capi.C5_ERR_INVALID
    assert lib.c5_shape_prior_quality_device(h, None, None, None) == capi.C5_ERR_INVALID
    assert lib.c5_shape_prior_gradient_device(h, C.byref(P), None, None, None, None) == capi.C5_ERR_INVALID
    assert (out == 7).all()
    # a wrong n_pts, a non-finite rest coordinate: refused, and the rest shape set before stays
    before = ctx.shape_prior_rest_data()
    poisoned = c.X.copy()
    poisoned[3, 1] = nan
    assert lib.c5_shape_prior_rest(h, dp(c.X), c.n_pts + 1, None) == capi.C5_ERR_INVALID
    assert lib.c5_shape_prior_rest(h, None, c.n_pts - 1, None) == capi.C5_ERR_INVALID
    assert lib.c5_shape_prior_rest(h, dp(poisoned), c.n_pts, None) == capi.C5_ERR_INVALID
    for bad_x in (poisoned, np.where(np.isnan(poisoned), inf, poisoned)):
        with pytest.raises(capi.C5Error) as e:
            ctx.shape_prior_rest_device(_dev(bad_x))
        assert e.value.code == capi.C5_ERR_INVALID
    assert lib.c5_shape_prior_rest_device(h, _dev(c.X).data_ptr(), c.n_pts + 1, None) == capi.C5_ERR_INVALID
    assert all(np.array_equal(a, b) for a, b in zip(before, ctx.shape_prior_rest_data()))
    assert ctx.shape_prior_quality(c.x)[1] == 0


def test_a_call_before_any_upload_and_a_grid_without_adjacency():
    P = _prior(sr.DIRICHLET)
    with capi.Context(0) as ctx:  # nothing uploaded: the c5_prior_* calls' answer
        for call in (lambda: ctx.shape_prior_rest(None), lambda: ctx.shape_prior_rest_data(), lambda: ctx.shape_prior_gradient(P, np.zeros((0, 3))),
                     lambda: ctx.shape_prior_quality(np.zeros((0, 3)))):
            with pytest.raises(capi.C5Error) as e:
                call()
            assert e.value.code == capi.C5_ERR_STATE
    # three cells on one face: uploaded as non-conforming, no adjacency - and none is needed
    X, cells = pr.three_on_a_face()
    with _context(X, cells) as ctx:
        assert ctx.shape_prior_rest(X) == 0
        B, V0, vert = ctx.shape_prior_rest_data()
        x = sr.displaced(X, vert.astype(np.int64))
        for energy in ENERGIES:
            value, n_inv, g = ctx.shape_prior_gradient(_prior(energy), x)
            want, scale = sr.gradient(B, V0, vert.astype(np.int64), len(X), x, energy, KAPPA, LAM, with_scale=True)
            assert n_inv == 0 and value > 0 and (np.abs(g - want) <= K * EPS * scale).all()
            assert energy != sr.DIRICHLET or _same(g, want)


def test_outstanding_async_frames_are_refused(cases):
    c = cases["cube8"]
    P = _prior(sr.DIRICHLET)
    with _context(c.X, c.cells) as ctx:
        ctx.set_image(16, 12, mg.REFERENCE_BOUNDS)
        ctx.set_view(mg.view_rotations(0.1, 0.07))
        assert ctx.shape_prior_rest(c.X) == 0
        frame = ctx.host_image()
        ctx.render_host_async(frame)
        for call in (lambda: ctx.shape_prior_rest(c.X), lambda: ctx.shape_prior_rest_data(), lambda: ctx.shape_prior_gradient(P, c.x),
                     lambda: ctx.shape_prior_product(P, None, c.v), lambda: ctx.shape_prior_diagonal(P), lambda: ctx.shape_prior_quality(c.x),
                     lambda: ctx.shape_prior_quality_device(_dev(c.x), None, None)):
            with pytest.raises(capi.C5Error) as e:
                call()
            assert e.value.code == capi.C5_ERR_STATE and "outstanding" in e.value.message
        assert ctx.render_host_wait() in (capi.C5_OK, capi.C5_RETRY)
        assert ctx.shape_prior_gradient(P, c.x)[1] == 0
        ctx.free_host_image(frame)

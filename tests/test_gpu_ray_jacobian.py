"""Ray Jacobian on the GPU (c5_ray_jacobian_fill*; capi.Context.ray_jacobian, autograd.ray_jacobian, fit.ExplicitJacobian):
d tau / d alpha, d I / d alpha and d I / d Q per segment as CSR arrays over the ray matrix's structure.

  structure        col and dz are c5_ray_matrix_fill's bit for bit (walk and "algorithm" 1, host and _device forms);
  one definition   a row of dI_dalpha / dI_dq is, bit for bit, what c5_render_adjoint returns for the one-hot upstream image
                   (0, 1) at that pixel, and a row of dz what it returns for (1, 0): one lane, one term, fma(1, t, 0) - the
                   kernels share adjoint_walk_body / adjoint_resolve_body with the adjoint's, and this is what holds that;
  per element      every stored value against the numpy restatement on tests/ray_jacobian_checks.py's bar (its docstring
                   derives the chord sensitivity of a single element; checked here on the CPU by moving the chords);
  in sums          J^T g, the column sums of squares, J v and fit.ExplicitJacobian's product against the library's renders,
                   every bar taken from the two sides' own roundings;
  bit identities, contract edges, and fit.gn_step through the explicit Jacobian.

THE SUMMATION BARS.  u = 2^-53.  A sum of n doubles in any order is within (n - 1) u sum |t_i| of the exact one (first
order); each t_i here is a product or an fma of two products, formed with at most 2 roundings on either side.  Two sides
summing the same n terms therefore differ by at most (2 (n - 1) + 4) u sum |t_i| <= (n + 1) 2^-52 sum |t_i|: "the number
of terms x 2^-53 x sum |terms|" with both sides' terms counted, n_terms = 2 n + 2.  The library's fp32 outputs (the
tangent; J v inside the product) add 2^-23 |ref| + 2^-103 (tests/derivative_fuzz.py).

Scenes are small: a Kuhn box of 4 x 4 x 4 cubes (384 cells) and a ball of 5 (non-convex: rays re-enter it) under a view about
three axes, 13 x 21 pixels - off the 8 x 8 tile both ways.  Every reference is computed once per module and shared."""
import ctypes as C
import functools
import os
import types

import numpy as np
import pytest

from course5_amd import capi
from course5_amd import meshgen as mg
from course5_amd import sharding
from tests import adjoint_reference as ar, derivative_fuzz as fz, ray_jacobian_checks as rjc, ray_matrix_checks as rmc

pytestmark = pytest.mark.gpu
B = mg.REFERENCE_BOUNDS
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VIEW = mg.view_rotations(0.1, 0.07, 0.05)
RX, RY = 13, 21
BOX_BOUNDS = (1.7, 0.3, 0.7, -0.7)
BALL_BOUNDS = (1.6, 0.4, 0.55, -0.55)
LIMIT = 1.5
U52 = 2.0 ** -52
EPS = float(np.finfo(np.float64).eps)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b):
    return all(x.shape == y.shape and np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _ctx(s, options=(), limit=True):
    ctx = capi.Context(0)
    for k, v in options:
        ctx.set_option(k, v)
    ctx.upload_grid(s.xyz, s.cells, s.alpha, s.q)
    ctx.set_image(s.rx, s.ry, s.bounds)
    ctx.set_view(s.rots)
    if limit:
        ctx.set_alpha_limit(s.limit)
    return ctx


def _scalars(cells, xyz, rots, rx, ry, bounds, seed):
    """alpha below the limit, at it, above it, 0 and below DBL_EPSILON, on cells the image sees; Q in [0, 1) with zeros."""
    n = len(cells)
    rng = np.random.default_rng(seed)
    alpha = rng.uniform(0.0, 1.4, n)
    q = rng.uniform(0.0, 1.0, n)
    seen = np.unique(ar.segment_lists(xyz, cells, rots, rx, ry, bounds)[1])
    pick = rng.permutation(seen)
    alpha[pick[0:6]] = LIMIT
    alpha[pick[6:14]] = rng.uniform(1.6, 3.0, 8)
    alpha[pick[14:18]] = 0.0
    alpha[pick[18:20]] = 0.25 * EPS
    alpha[pick[20]] = np.nextafter(LIMIT, np.inf)
    q[pick[21:25]] = 0.0
    return alpha, q


@functools.lru_cache(maxsize=None)
def _scene(kind):
    s = types.SimpleNamespace(kind=kind, rots=VIEW, rx=RX, ry=RY, limit=LIMIT, options=(), solid=None)
    if kind in ("box", "box_soup"):
        s.xyz, s.cells = mg.kuhn_box(4, jitter=0.1)
        s.bounds = BOX_BOUNDS
        s.alpha, s.q = _scalars(s.cells, s.xyz, VIEW, RX, RY, BOX_BOUNDS, 7)
        if kind == "box_soup":
            s.xyz, s.cells = mg.per_cell_point_copies(s.xyz, s.cells)
            s.options = (("algorithm", 1),)
    elif kind == "ball":
        s.xyz, s.cells = mg.ball(5)
        s.bounds = BALL_BOUNDS
        s.alpha, s.q = _scalars(s.cells, s.xyz, VIEW, RX, RY, BALL_BOUNDS, 8)
        c = np.array([1.0, 0.2, 0.0])
        e = 0.12
        s.solid = np.array([[c + (e, 0, 0), c + (-e, e, 0), c + (-e, -e, e), c + (0, 0, -e)]]).reshape(1, 12)
    elif ":" in kind:  # a golden fixture and one of its views, the scalars and the default limit of the fixture
        name, view = kind.split(":")
        g = np.load(os.path.join(GOLDEN, name + ".npz"))
        s.xyz, s.cells, s.alpha, s.q, s.rots = g["xyz"], g["cells"], g["alpha"], g["q"], g[f"rots{view}"]
        s.rx, s.ry = (int(v) for v in g["res"])
        s.bounds, s.limit = tuple(g["bounds"]), 2.5
    else:
        assert kind == "morton"
        s.xyz, s.cells = mg.kuhn_box(9, jitter=0.1)  # 4 374 cells: kept in Morton order on the device ("cell_order" 1)
        s.alpha, s.q = mg.scalars(len(s.cells))
        s.rots, s.rx, s.ry, s.bounds, s.limit, s.options = mg.view_rotations(0.1, 0.07), 61, 43, B, 2.5, (("cell_order", 1),)
    assert kind not in ("box", "box_soup") or len(s.cells) == 384
    return s


@functools.lru_cache(maxsize=None)
def _reference(kind):
    """(adjoint_reference.ray_matrices' dict, element_terms without a solid, dz_err) of the scene."""
    s = _scene(kind)
    m = ar.ray_matrices(s.xyz, s.cells, s.alpha, s.q, s.rots, s.rx, s.ry, s.bounds, s.limit)
    return m, rjc.element_terms(m), fz.dz_err(s)


@functools.lru_cache(maxsize=None)
def _jacobian(kind, options=None):
    """The GPU's arrays of the scene: (row_ptr, col, dz, dI_dalpha, dI_dq), read-only."""
    s = _scene(kind)
    with _ctx(s, s.options if options is None else options) as ctx:
        j = ctx.ray_jacobian()
    for a in j:
        a.setflags(write=False)
    return j


def _pixels_of(row_ptr):
    return rmc.rows_of(row_ptr)


# ---- the scenes hold what they are said to hold (CPU, before the GPU is asked) ------------------------------------------

def test_the_reference_lists_show_every_case():
    for kind in ("box", "ball"):
        s = _scene(kind)
        _m, t, _e = _reference(kind)
        a_raw = s.alpha[t["cell"]]
        x = t["x"][t["active"]]
        assert (a_raw < LIMIT).any() and (a_raw == LIMIT).any() and (a_raw > LIMIT).any() and (a_raw == 0).any()
        assert ((a_raw > 0) & (a_raw < EPS)).any() and t["clamped"].any() and (~t["active"]).any()
        # both branches of segment_terms: a dz below and above 1/8, well populated
        assert (x < 0.125).sum() > 20 and (x >= 0.125).sum() > 20, (kind, (x < 0.125).sum(), (x >= 0.125).sum())
        per_px = np.bincount(t["pixel"], minlength=RX * RY).reshape(RY, RX)
        assert (per_px[16:, 8:] > 0).any(), "no covered pixel in the last partial tile"
        assert (per_px > 0).sum() > 40
    assert _reentering_pixels("ball").size > 0


def _reentering_pixels(kind):
    """Pixels whose ray leaves the grid and enters it again: a gap between two consecutive segments."""
    s = _scene(kind)
    pix, _cell, zh, dz = ar.segment_lists(s.xyz, s.cells, s.rots, s.rx, s.ry, s.bounds)  # by pixel, ascending z_hi
    same = pix[1:] == pix[:-1]
    gap = (zh[1:] - dz[1:]) - zh[:-1]
    return np.unique(pix[1:][same & (gap > 1e-6)])


def test_the_sensitivity_of_a_single_element_bounds_what_moved_chords_do():
    """ray_jacobian_checks' derivation, on the CPU: every chord moved by e F_j with e = 1e-4 min(dz / F) - large against
    rounding (1e-16 of scale), small enough that the second order, (e F / dz)^2 <= 1e-8 of the element against the first
    order's e F / dz, stays below 1e-3 of the bar - moves no element by more than e sens (1 + 1e-3) + 2^-40 scale."""
    rng = np.random.default_rng(3)
    for kind in ("box", "ball"):
        s = _scene(kind)
        m, t, _e = _reference(kind)
        valid = m["valid"]
        e = 1e-4 * float((m["D"][valid] / m["F"][valid]).min())
        worst = 0.0
        for sign in (1.0, -1.0, rng.choice([-1.0, 1.0], size=m["D"].shape)):
            D2 = np.where(valid, m["D"] + sign * e * m["F"], 0.0)
            t2 = rjc.element_terms(ar.matrices_of(m["C"], D2, m["F"], s.alpha, s.q, s.limit, m["shape"]))
            for name, scale, sens in (("da", "scale_a", "sens_a"), ("dq", "scale_q", "sens_q")):
                moved = np.abs(t2[name] - t[name])
                bar = e * t[sens] * (1.0 + 1e-3) + 2.0 ** -40 * t[scale]
                assert (moved <= bar).all(), (kind, name, float((moved / np.maximum(bar, 1e-300)).max()))
                worst = max(worst, float((moved / np.maximum(e * t[sens], 1e-300))[t[sens] > 0].max()))
        print(f"{kind}: chords moved by {e:.3g} F: worst |change| / (e sens) {worst:.3g}")
        assert worst > 0.5  # (the bound is not idle: some element uses more than half of it)


# ---- 1. structure ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["box", "box_soup", "ball"])
def test_structure_is_the_ray_matrix_s_in_both_forms(kind):
    import torch
    s = _scene(kind)
    row_ptr, col, dz, da, dq = _jacobian(kind)
    with _ctx(s, s.options) as ctx:
        if s.solid is not None:
            ctx.set_solid(0, s.solid)
            ctx.set_solid_view(0, s.rots)
        rp, mcol, mdz = ctx.ray_matrix()
        j = ctx.ray_jacobian()
        assert np.array_equal(j[0], rp) and np.array_equal(j[1], mcol) and np.array_equal(_bits(j[2]), _bits(mdz))
        if s.solid is None:
            assert _same(j, (row_ptr, col, dz, da, dq))
        else:
            assert rp[-1] < row_ptr[-1]  # (solid-marked pixels: empty rows)
        nnz = int(rp[-1])
        assert nnz > 300 and j[1].dtype == np.int32 and all(a.dtype == np.float64 and a.shape == (nnz,) for a in j[2:])
        # the _device form, with room to spare: the same arrays, nothing behind them
        d_rp = torch.tensor(rp, device="cuda")
        d_col = torch.full((nnz + 32,), -7, dtype=torch.int32, device="cuda")
        d = [torch.full((nnz + 32,), -7.0, dtype=torch.float64, device="cuda") for _ in range(3)]
        torch.cuda.synchronize()
        ctx.ray_jacobian_fill_device(d_rp, d_col, d[0], d[1], d[2])
        assert ctx.synchronize() == capi.C5_OK
        got = (d_col.cpu().numpy(),) + tuple(t.cpu().numpy() for t in d)
        assert _same([g[:nnz] for g in got], j[1:]) and all((g[nnz:] == -7).all() for g in got)


# ---- 2. the same terms as the adjoint, bit for bit -------------------------------------------------------------------

def _chosen_pixels(kind, row_ptr, solid_px):
    """A handful of covered pixels: every re-entering one (up to 3), one next to a solid-marked pixel, one in the last
    partial tile, and a few spread over the rest."""
    s = _scene(kind)
    covered = np.flatnonzero(np.diff(row_ptr) > 0)
    chosen = {}
    for p in np.intersect1d(_reentering_pixels(kind), covered)[:3]:
        chosen[int(p)] = "re-entering"
    if solid_px is not None:
        grid = solid_px.reshape(s.ry, s.rx)
        near = np.zeros_like(grid)
        near[1:] |= grid[:-1]
        near[:-1] |= grid[1:]
        near[:, 1:] |= grid[:, :-1]
        near[:, :-1] |= grid[:, 1:]
        beside = np.intersect1d(np.flatnonzero((near & ~grid).reshape(-1)), covered)
        assert beside.size, "no covered pixel beside the solid"
        chosen[int(beside[len(beside) // 2])] = "next to a solid"
    rows, cols = covered // s.rx, covered % s.rx
    last = covered[(rows >= 8 * (s.ry // 8)) & (cols >= 8 * (s.rx // 8))]
    assert last.size, "no covered pixel in the last partial tile"
    chosen[int(last[0])] = "last partial tile"
    for p in covered[:: max(1, len(covered) // 5)]:
        chosen.setdefault(int(p), "spread")
    return chosen


@pytest.mark.parametrize("kind", ["ball", "box_soup"])
def test_rows_are_the_adjoint_of_one_hot_images_bit_for_bit(kind):
    """ball: the walk (adjoint_walk<2>), with a solid and re-entering rays; box_soup: "algorithm" 1 (adjoint_resolve)."""
    s = _scene(kind)
    n = len(s.cells)
    with _ctx(s, s.options) as ctx:
        solid_px = None
        if s.solid is not None:
            ctx.set_solid(0, s.solid)
            ctx.set_solid_view(0, s.rots)
            solid_px = np.isnan(ctx.render()[..., 0]).reshape(-1)
            assert solid_px.any()
        row_ptr, col, dz, da, dq = ctx.ray_jacobian()
        if solid_px is not None:
            assert (np.diff(row_ptr)[solid_px] == 0).all()
        chosen = _chosen_pixels(kind, row_ptr, solid_px)
        assert kind != "ball" or {"re-entering", "next to a solid", "last partial tile"} <= set(chosen.values())
        assert (da == 0).any() and (da != 0).any() and (dq == 0).any()
        for p, why in chosen.items():
            sl = slice(row_ptr[p], row_ptr[p + 1])
            want_a, want_q, want_tau = np.zeros(n), np.zeros(n), np.zeros(n)
            want_a[col[sl]] = da[sl] + 0.0  # (an element of -0 reads +0 in a sum that starts at +0)
            want_q[col[sl]] = dq[sl] + 0.0
            want_tau[col[sl]] = dz[sl]
            g = np.zeros((s.ry, s.rx, 2), np.float32)
            g.reshape(-1, 2)[p, 1] = 1.0
            ga, gq = ctx.render_adjoint(g)
            assert np.array_equal(_bits(ga), _bits(want_a)) and np.array_equal(_bits(gq), _bits(want_q)), (p, why)
            g = np.zeros((s.ry, s.rx, 2), np.float32)
            g.reshape(-1, 2)[p, 0] = 1.0
            ga, gq = ctx.render_adjoint(g)
            assert np.array_equal(_bits(ga), _bits(want_tau)) and not gq.any(), (p, why)
        print(f"{kind}: {len(chosen)} one-hot pixels bit-equal: {sorted(set(chosen.values()))}")


# ---- 3. per element against the restatement --------------------------------------------------------------------------

def _held_to_the_restatement(s, jac, skip, what):
    m = ar.ray_matrices(s.xyz, s.cells, s.alpha, s.q, s.rots, s.rx, s.ry, s.bounds, s.limit)
    ref = rjc.element_terms(m, skip)
    worst = rjc.worst_ratios(jac, ref, fz.dz_err(s), s.rx * s.ry, len(s.cells))
    print(f"{what}: nnz {len(jac[1])}, worst error / bar: " + ", ".join(f"{name} {r:.3g} ({where})" for name, (r, where)
                                                                         in zip(("dz", "dI_dalpha", "dI_dq"), worst)))
    for name, (r, where) in zip(("dz", "dI_dalpha", "dI_dq"), worst):
        assert r <= 1.0, f"{what}: {name} at {where}: error / bar {r:.3g}"


@pytest.mark.parametrize("kind", ["g2_kuhn4_120x90:0", "g2_kuhn4_120x90:1", "g2_kuhn4_120x90:2", "ball12_150x112:1",
                                  "g8_hanging_nodes_120x90:3", "g1_cube8_60x45:0", "morton", "box", "box_soup", "ball"])
def test_every_element_against_the_restatement(kind):
    _held_to_the_restatement(_scene(kind), _jacobian(kind), None, kind)


@pytest.mark.parametrize("seed", range(3000, 3010))
def test_every_element_on_the_fuzz_scenes(seed, oracle_port):
    """The first ten seeds of tests/test_gpu_derivative_fuzz.py, the whole image of each: alpha by class, soups on
    "algorithm" 1, solids, every alpha limit, threshold and underflow scenes."""
    s = fz.derivative_scene(seed)
    why = fz.qualify(s, oracle_port)
    if why is not None:
        print(f"seed {seed} is not used, as in the derivative sweep: {why}")
        return
    s.rx, s.ry = s.res
    s.bounds = B
    with _ctx(s, (("algorithm", 1),) if s.soup else ()) as ctx:
        skip = None
        if s.solid:
            ctx.set_solid(0, fz._solid_of(s))
            skip = np.isnan(ctx.render()[..., 0])
        jac = ctx.ray_jacobian()
    _held_to_the_restatement(s, jac, skip, f"seed {seed} ({s.mode}{', soup' if s.soup else ''}{', solid' if s.solid else ''})")


# ---- 4. against the renders, in sums ---------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _box_frame():
    """The box scene's Jacobian with what the sums need: pixel of every element, counts, a random upstream image, weights
    and a direction."""
    s = _scene("box")
    row_ptr, col, dz, da, dq = _jacobian("box")
    rng = np.random.default_rng(17)
    f = types.SimpleNamespace(s=s, n=len(s.cells), n_px=s.rx * s.ry, pix=_pixels_of(row_ptr), col=col, dz=dz, da=da, dq=dq)
    f.count_c = np.bincount(col, minlength=f.n)
    f.count_p = np.diff(row_ptr)
    f.g = rng.normal(size=(s.ry, s.rx, 2)).astype(np.float32)
    f.g[4:9, 3:7] = 0.0
    f.w = rng.uniform(0.0, 2.0, (s.ry, s.rx, 2)).astype(np.float32)
    f.w[10:12] = 0.0
    f.va, f.vq = rng.normal(size=f.n), rng.normal(size=f.n)
    return f


def _to_cells(f, t):
    return np.bincount(f.col, weights=t, minlength=f.n)


def _to_pixels(f, t):
    return np.bincount(f.pix, weights=t, minlength=f.n_px)


def _report(what, got, want, bar):
    r = np.abs(got - want) / np.maximum(bar, 1e-300)
    r = np.where(np.abs(got - want) == 0, 0.0, r)
    print(f"{what}: worst error / bar {r.max():.3g}; largest |difference| {np.abs(got - want).max():.3g}, largest |value| {np.abs(want).max():.3g}")
    assert np.isfinite(got).all() and np.abs(want).max() > 0 and (np.abs(got - want) <= bar).all(), what


def test_transpose_and_squares_against_the_adjoint_and_the_diagonal():
    f = _box_frame()
    g = f.g.astype(np.float64).reshape(-1, 2)
    w = f.w.astype(np.float64).reshape(-1, 2)
    with _ctx(f.s) as ctx:
        ga, gq = ctx.render_adjoint(f.g)
        diag_a, diag_q = ctx.render_gn_diagonal(f.w)
    gt, gi, wt, wi = g[f.pix, 0], g[f.pix, 1], w[f.pix, 0], w[f.pix, 1]
    # (module docstring: n_terms = 2 n + 2 over both sides, n = 2 per element where two products make one term)
    _report("J^T g, alpha", _to_cells(f, gt * f.dz + gi * f.da), ga, (2 * f.count_c + 1) * U52 * _to_cells(f, np.abs(gt) * f.dz + np.abs(gi * f.da)))
    _report("J^T g, q", _to_cells(f, gi * f.dq), gq, (f.count_c + 1) * U52 * _to_cells(f, np.abs(gi) * f.dq))
    _report("sum w value^2, alpha", _to_cells(f, wt * f.dz ** 2 + wi * f.da ** 2), diag_a,
            (2 * f.count_c + 1) * U52 * 2 * _to_cells(f, wt * f.dz ** 2 + wi * f.da ** 2))  # (a square: one more rounding per term)
    _report("sum w value^2, q", _to_cells(f, wi * f.dq ** 2), diag_q, (f.count_c + 1) * U52 * 2 * _to_cells(f, wi * f.dq ** 2))


def test_j_v_against_the_tangent():
    f = _box_frame()
    with _ctx(f.s) as ctx:
        t = ctx.render_tangent(f.va, f.vq).astype(np.float64).reshape(-1, 2)
    tau = _to_pixels(f, f.dz * f.va[f.col])
    I = _to_pixels(f, f.da * f.va[f.col] + f.dq * f.vq[f.col])
    _report("J v, tau", t[:, 0], tau, 2.0 ** -23 * np.abs(tau) + 2.0 ** -103 + (f.count_p + 1) * U52 * _to_pixels(f, np.abs(f.dz * f.va[f.col])))
    _report("J v, I", t[:, 1], I, 2.0 ** -23 * np.abs(I) + 2.0 ** -103
            + (2 * f.count_p + 1) * U52 * _to_pixels(f, np.abs(f.da * f.va[f.col]) + np.abs(f.dq * f.vq[f.col])))


def _product_bars(f, va, vq, w):
    """Per cell, what separates fit.ExplicitJacobian's product (fp64 throughout) from the library's (J v rounded to fp32 and
    multiplied by the weight in fp32: 2 x 2^-24, carried through |J|^T): 2^-23 |J|^T W |J v|, plus the summation terms of
    the inner and the outer sums (module docstring).  From the exported arrays alone."""
    za, zq = (np.zeros(f.n) if v is None else v for v in (va, vq))
    tau, I = _to_pixels(f, f.dz * za[f.col]), _to_pixels(f, f.da * za[f.col] + f.dq * zq[f.col])
    e_tau = (f.count_p + 1) * U52 * _to_pixels(f, np.abs(f.dz * za[f.col]))
    e_I = (2 * f.count_p + 1) * U52 * _to_pixels(f, np.abs(f.da * za[f.col]) + np.abs(f.dq * zq[f.col]))
    w_tau, w_I = w[:, 0], w[:, 1]
    g_tau, g_I = w_tau * (2.0 ** -23 * np.abs(tau) + e_tau), w_I * (2.0 ** -23 * np.abs(I) + e_I)
    bar_a = _to_cells(f, g_tau[f.pix] * f.dz + g_I[f.pix] * np.abs(f.da))
    bar_q = _to_cells(f, g_I[f.pix] * f.dq)
    out_a = (2 * f.count_c + 1) * U52 * _to_cells(f, (w_tau * np.abs(tau))[f.pix] * f.dz + (w_I * np.abs(I))[f.pix] * np.abs(f.da))
    out_q = (f.count_c + 1) * U52 * _to_cells(f, (w_I * np.abs(I))[f.pix] * f.dq)
    return bar_a + out_a, bar_q + out_q


def test_explicit_product_against_the_library_s():
    import torch
    from course5_amd import autograd, fit
    f = _box_frame()
    s = f.s
    dev = torch.device("cuda", 0)
    alpha, q = torch.tensor(s.alpha, device=dev), torch.tensor(s.q, device=dev)
    va, vq, w = torch.tensor(f.va, device=dev), torch.tensor(f.vq, device=dev), torch.tensor(f.w, device=dev)
    with _ctx(s) as ctx:
        ops = fit.ExplicitJacobian(ctx).gn_operators(alpha, q, w)
        assert isinstance(ops, fit.JacobianOperators)
        mine = [t.cpu().numpy() for t in ops.product(va, vq)]
        theirs = [t.cpu().numpy() for t in autograd.gn_product(ctx, alpha, q, va, vq, w)]
        A, Ja, Jq = autograd.ray_jacobian(ctx, alpha, q)
    bar_a, bar_q = _product_bars(f, f.va, f.vq, f.w.astype(np.float64).reshape(-1, 2))
    _report("H v, alpha", mine[0], theirs[0], bar_a)
    _report("H v, q", mine[1], theirs[1], bar_q)
    # autograd.ray_jacobian: three CSR tensors over one index storage, the arrays of the host form
    assert all(t.layout == torch.sparse_csr and t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == (f.n_px, f.n) for t in (A, Ja, Jq))
    assert A.crow_indices().dtype == torch.int32 and A.col_indices().dtype == torch.int32
    assert A.crow_indices().data_ptr() == Ja.crow_indices().data_ptr() == Jq.crow_indices().data_ptr()
    assert A.col_indices().data_ptr() == Ja.col_indices().data_ptr() == Jq.col_indices().data_ptr()
    assert _same([A.col_indices().cpu().numpy()] + [t.values().cpu().numpy() for t in (A, Ja, Jq)], _jacobian("box")[1:])


# ---- 5. bit identities -----------------------------------------------------------------------------------------------

def test_calls_repeat_and_options_change_nothing():
    s = _scene("box")
    whole = _jacobian("box")
    with _ctx(s) as ctx:
        assert _same(ctx.ray_jacobian(), whole) and _same(ctx.ray_jacobian(), whole)
    for options in ((("lds_stage", 0),), (("integration", 1),), (("depth_split", 2),), (("adjoint_exact", 1),), (("exact_sums", 1),)):
        assert _same(_jacobian("box", options), whole), options


def test_row_ranges_and_row_tiles_are_rows_of_the_whole_frame():
    s = _scene("box")
    rp, col, dz, da, dq = _jacobian("box")
    seen = 0

    def held(part, rows):
        px = (np.asarray(rows)[:, None] * s.rx + np.arange(s.rx)).reshape(-1)
        prp, pcol, pdz, pda, pdq = part
        return (rmc.bit_equal_rows((prp, pcol, pdz, pda), (rp, col, dz, da), px) and rmc.bit_equal_rows((prp, pcol, pdz, pdq), (rp, col, dz, dq), px))

    with _ctx(s) as ctx:
        for begin, count in ((0, 13), (13, 8)):  # (cut off the 8-row tile)
            ctx.set_row_range(begin, count)
            part = ctx.ray_jacobian()
            assert part[0][-1] > 0 and held(part, np.arange(begin, begin + count)), (begin, count)
            seen += part[0][-1]
    assert seen == rp[-1]
    seen = 0
    for rank in range(2):
        with _ctx(s) as ctx:
            ctx.set_row_tiles(4, rank, 2)
            part = ctx.ray_jacobian()
        assert held(part, sharding.local_rows(s.ry, 4, rank, 2)), rank
        seen += part[0][-1]
    assert seen == rp[-1]


# ---- 6. contract edges -----------------------------------------------------------------------------------------------

def test_capacity_is_a_guard_in_both_forms():
    import torch
    s = _scene("box")
    row_ptr, col, dz, da, dq = _jacobian("box")
    nnz = int(row_ptr[-1])
    lp, ip, dp = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double)
    with _ctx(s) as ctx:
        rp = np.ascontiguousarray(row_ptr)
        hc, h = np.full(nnz, -7, np.int32), [np.full(nnz, -7.0) for _ in range(3)]
        assert ctx.lib.c5_ray_jacobian_fill(ctx.handle, rp.ctypes.data_as(lp), nnz - 1, hc.ctypes.data_as(ip),
                                            *(a.ctypes.data_as(dp) for a in h)) == capi.C5_ERR_INVALID
        assert str(nnz) in ctx.lib.c5_last_error(ctx.handle).decode()
        assert (hc == -7).all() and all((a == -7.0).all() for a in h)
        cap = nnz - 1
        d_rp = torch.tensor(rp, device="cuda")
        d_col = torch.full((nnz + 64,), -7, dtype=torch.int32, device="cuda")
        d = [torch.full((nnz + 64,), -7.0, dtype=torch.float64, device="cuda") for _ in range(3)]
        torch.cuda.synchronize()
        ctx.ray_jacobian_fill_device(d_rp, d_col.data_ptr(), *(t.data_ptr() for t in d), capacity=cap)
        with pytest.raises(capi.C5Error) as e:
            ctx.synchronize()
        assert e.value.code == capi.C5_ERR_STATE and "ray jacobian fill" in e.value.message
        got = [d_col.cpu().numpy()] + [t.cpu().numpy() for t in d]
        assert all((g[cap:] == -7).all() for g in got)  # nothing at or past capacity
        assert _same([g[:cap] for g in got], [a[:cap] for a in (col, dz, da, dq)])
        assert ctx.synchronize() == capi.C5_OK  # (reported once)


def test_a_changed_view_is_reported_and_changed_scalars_change_only_the_values():
    s = _scene("box")
    first = _jacobian("box")
    with _ctx(s) as ctx:
        row_ptr = ctx.ray_matrix_rows()
        # col and dz NULL: the same values
        values = ctx.ray_jacobian_fill(row_ptr, with_structure=False)
        assert _same(values, first[3:])
        # other scalars and another limit: other values on the same structure
        ctx.update_scalars(0.5 * s.alpha + 0.1, s.q[::-1].copy())
        ctx.set_alpha_limit(0.7)
        second = ctx.ray_jacobian_fill(row_ptr)
        assert _same(second[:2], first[1:3])
        assert not np.array_equal(second[2], first[3]) and not np.array_equal(second[3], first[4])
        assert (second[2] == 0).sum() != (first[3] == 0).sum()  # (another set of clamped cells)
        ctx.update_scalars(s.alpha, s.q)
        ctx.set_alpha_limit(s.limit)
        assert _same((row_ptr,) + ctx.ray_jacobian_fill(row_ptr), first)
        # a view changed between the rows call and the fill
        ctx.set_view(mg.view_rotations(0.4, -0.3, 0.2))
        with pytest.raises(capi.C5Error) as e:
            ctx.ray_jacobian_fill(row_ptr)
        assert e.value.code == capi.C5_ERR_STATE and "the frame changed" in e.value.message
        now = ctx.ray_jacobian()
        assert not np.array_equal(now[0], first[0])


def test_bad_arguments_and_outstanding_async_frames_are_refused():
    s = _scene("box")
    first = _jacobian("box")
    nnz = int(first[0][-1])
    lp, ip, dp, vp = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_void_p
    rp = np.ascontiguousarray(first[0])
    col, a, b, c = np.zeros(nnz, np.int32), np.zeros(nnz), np.zeros(nnz), np.zeros(nnz)
    with _ctx(s) as ctx:
        lib, h = ctx.lib, ctx.handle
        p_rp, p_col, pa, pb, pc = rp.ctypes.data_as(lp), col.ctypes.data_as(ip), a.ctypes.data_as(dp), b.ctypes.data_as(dp), c.ctypes.data_as(dp)
        assert lib.c5_ray_jacobian_fill(None, p_rp, nnz, p_col, pa, pb, pc) == capi.C5_ERR_INVALID
        assert lib.c5_ray_jacobian_fill(h, None, nnz, p_col, pa, pb, pc) == capi.C5_ERR_INVALID
        assert lib.c5_ray_jacobian_fill(h, p_rp, nnz, p_col, pa, None, None) == capi.C5_ERR_INVALID  # both value arrays missing
        assert lib.c5_ray_jacobian_fill(h, p_rp, -1, p_col, pa, pb, pc) == capi.C5_ERR_INVALID
        some = rp.ctypes.data  # (a non-null stand-in: the checks come before anything is read or written)
        assert lib.c5_ray_jacobian_fill_device(h, None, nnz, vp(some), vp(some), vp(some), vp(some)) == capi.C5_ERR_INVALID
        assert lib.c5_ray_jacobian_fill_device(h, vp(some), nnz, vp(some), vp(some), None, None) == capi.C5_ERR_INVALID
        assert lib.c5_ray_jacobian_fill_device(h, vp(some), -1, vp(some), vp(some), vp(some), vp(some)) == capi.C5_ERR_INVALID
        # one value array alone is enough
        assert lib.c5_ray_jacobian_fill(h, p_rp, nnz, None, None, None, pc) == capi.C5_OK and np.array_equal(_bits(c), _bits(first[4]))
        assert lib.c5_ray_jacobian_fill(h, p_rp, nnz, None, None, pb, None) == capi.C5_OK and np.array_equal(_bits(b), _bits(first[3]))
        buf = ctx.host_image()
        ctx.render_host_async(buf)
        with pytest.raises(capi.C5Error) as e:
            ctx.ray_jacobian_fill(rp)
        assert e.value.code == capi.C5_ERR_STATE
        assert lib.c5_ray_jacobian_fill_device(h, vp(some), nnz, vp(some), vp(some), vp(some), vp(some)) == capi.C5_ERR_STATE
        assert ctx.render_host_wait() == capi.C5_OK
        ctx.free_host_image(buf)
        assert _same(ctx.ray_jacobian(), first)


def test_a_scene_of_solids_only_has_empty_rows():
    sx, sc = mg.kuhn_box(2, lo=(0.9, -0.15, 0.3), size=0.3)
    with capi.Context(0) as ctx:
        ctx.set_solid(0, sx[sc].reshape(-1, 12), 0.5)
        ctx.set_image(RX, RY, BOX_BOUNDS)
        ctx.set_view(VIEW)
        ctx.set_solid_view(0, VIEW)
        assert (ctx.render()[..., 0] == 0.5).any()
        row_ptr, col, dz, da, dq = ctx.ray_jacobian()
        stale = np.zeros(RX * RY + 1, np.int64)
        stale[-1] = 3
        with pytest.raises(capi.C5Error) as e:
            ctx.ray_jacobian_fill(stale)
        assert e.value.code == capi.C5_ERR_STATE
    assert row_ptr.shape == (RX * RY + 1,) and not row_ptr.any() and len(col) == len(dz) == len(da) == len(dq) == 0


def test_a_pool_that_has_to_grow_says_retry_and_then_gives_the_right_arrays():
    import torch
    kind = "ball12_150x112:1"
    s = _scene(kind)
    want = _jacobian(kind)
    nnz = int(want[0][-1])
    with _ctx(s) as ctx:
        row_ptr = ctx.ray_matrix_rows()
        assert row_ptr[-1] == nnz
        # the pool of 16 does overflow on this frame: the raw _device call's wait says C5_RETRY (and the pool has grown by then)
        ctx.set_option("entry_pool", 16)
        d_rp = torch.tensor(row_ptr, device="cuda")
        d = [torch.zeros(nnz, dtype=torch.float64, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        ctx.ray_jacobian_fill_device(d_rp, None, None, d[0], d[1])
        assert ctx.synchronize() == capi.C5_RETRY
        ctx.ray_jacobian_fill_device(d_rp, None, None, d[0], d[1])
        assert ctx.synchronize() == capi.C5_OK
        assert _same([t.cpu().numpy() for t in d], want[3:])
        ctx.set_option("entry_pool", 16)
        assert _same((row_ptr,) + ctx.ray_jacobian_fill(row_ptr), want)  # (the host form retries by itself)


def test_renders_around_the_calls_are_untouched():
    s = _scene("ball")
    with _ctx(s) as a, _ctx(s) as b:
        for _ in range(3):  # (three frames: the view cache is in use by the third)
            ia, ib = a.render(), b.render()
        before = a.stats()
        j = a.ray_jacobian()
        assert a.stats() == before
        for _ in range(3):
            ja, jb = a.render(), b.render()
            assert np.array_equal(ja.view(np.uint32), ia.view(np.uint32)) and np.array_equal(jb.view(np.uint32), ib.view(np.uint32))
        assert a.stats()["segments"] == b.stats()["segments"] == j[0][-1]
    assert _same(j, _jacobian("ball"))


# ---- 7. fit.gn_step with the explicit Jacobian -----------------------------------------------------------------------

# |model_explicit - model_library| / |model_library| after three CG iterations of the toy below, as measured (the two
# paths differ by the fp32 rounding of J v inside the library's product, which CG amplifies); the assertion allows twice that
MEASURED_FINAL_MODEL_FACTOR = 4.93e-10  # (profiles/ray_jacobian.md)


def test_gn_step_through_the_explicit_jacobian():
    """A fit of Q on the 384-cell box, three CG iterations, by the library's operators and by the explicit Jacobian's.  The
    first iterate is x_1 = t p with p = -g / d and t = (p . g) / (p . H p) (no damping): g and d of the two paths differ by
    their summation (dg, dd: the bars of the sums above), H p by the product's bar e_H.  To first order
        |dp_i| <= (dg_i + |p_i| dd_i) / d_i,   d(p.g) <= sum |dp_i| |g_i| + |p_i| dg_i,
        d(p.Hp) <= sum |p_i| e_H,i + 2 |dp_i| |(H p)_i|,   dt / t <= d(p.g) / |p.g| + d(p.Hp) / (p.Hp),
        |dx_i| <= |x_i| dt / t + t |dp_i|,   d model / |model| <= dt / t + d(p.g) / |p.g|      (model_1 = t (p.g) / 2),
    every inner product's own summation (n_cells terms) added."""
    import torch
    from course5_amd import autograd, fit
    f = _box_frame()
    s = f.s
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(23)
    q_true = s.q * (1.0 + 0.3 * rng.normal(size=f.n))
    alpha, q0 = torch.tensor(s.alpha, device=dev), torch.tensor(s.q, device=dev)
    with _ctx(s) as ctx:
        ctx.update_scalars(s.alpha, q_true)
        target = ctx.render()
        ctx.update_scalars(s.alpha, s.q)
        residual = torch.tensor(ctx.render() - target, device=dev)
        (_, x_lib), m_lib = fit.gn_step(ctx, alpha, q0, residual, fit=("q",), iters=3)
        (_, x_exp), m_exp = fit.gn_step(fit.ExplicitJacobian(ctx), alpha, q0, residual, fit=("q",), iters=3)
        (_, x1_lib), m1_lib = fit.gn_step(ctx, alpha, q0, residual, fit=("q",), iters=1)
        (_, x1_exp), m1_exp = fit.gn_step(fit.ExplicitJacobian(ctx), alpha, q0, residual, fit=("q",), iters=1)
    assert len(m_lib) == len(m_exp) == 3 and len(m1_lib) == len(m1_exp) == 1
    # the first iteration, on the propagated bars (from the exported arrays)
    r = residual.cpu().numpy().astype(np.float64).reshape(-1, 2)
    gi = r[f.pix, 1]
    g = _to_cells(f, gi * f.dq)
    d = _to_cells(f, f.dq ** 2)
    dg = (f.count_c + 1) * U52 * _to_cells(f, np.abs(gi) * f.dq)
    dd = (f.count_c + 1) * U52 * 2 * d
    live = d > 0
    p = np.where(live, -g / np.where(live, d, 1.0), 0.0)
    dp = np.where(live, (dg + np.abs(p) * dd) / np.where(live, d, 1.0), 0.0)
    hp = _to_cells(f, _to_pixels(f, f.dq * p[f.col])[f.pix] * f.dq)
    _ea, e_h = _product_bars(f, None, p, np.ones((f.n_px, 2)))
    pg, php = p @ g, p @ hp
    d_pg = (dp * np.abs(g) + np.abs(p) * dg).sum() + f.n * U52 * np.abs(p * g).sum()
    d_php = (np.abs(p) * e_h + 2 * dp * np.abs(hp)).sum() + f.n * U52 * np.abs(p * hp).sum()
    rel_t = d_pg / abs(pg) + d_php / php
    t = -pg / php
    x1 = t * p
    dx = np.abs(x1) * rel_t + t * dp
    got_lib, got_exp = x1_lib.cpu().numpy(), x1_exp.cpu().numpy()
    rel_m = rel_t + d_pg / abs(pg)
    print(f"first iteration: model {m1_lib[0]:.9g} (library) {m1_exp[0]:.9g} (explicit); relative difference "
          f"{abs(m1_lib[0] - m1_exp[0]) / abs(m1_lib[0]):.3g}, bar {rel_m:.3g}; step: worst difference / bar "
          f"{(np.abs(got_lib - got_exp) / np.maximum(dx, 1e-300)).max():.3g}")
    assert m1_lib[0] < 0 and abs(m1_lib[0] - m1_exp[0]) <= rel_m * abs(m1_lib[0])
    assert (np.abs(got_lib - got_exp) <= dx).all() and np.abs(got_lib).max() > 0
    # later iterations: monotone, and the end within the measured factor
    for models in (m_lib, m_exp):
        assert all(b < a for a, b in zip(models, models[1:])) and models[0] < 0, models
    factor = abs(m_exp[-1] - m_lib[-1]) / abs(m_lib[-1])
    print(f"after 3 iterations: model {m_lib[-1]:.9g} (library) {m_exp[-1]:.9g} (explicit): relative difference {factor:.3g}; "
          f"largest |step difference| {float((x_lib - x_exp).abs().max()):.3g} of {float(x_lib.abs().max()):.3g}")
    assert factor <= 2 * MEASURED_FINAL_MODEL_FACTOR

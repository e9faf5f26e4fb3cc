"""Vertex Gauss-Newton product on the GPU (c5_render_vertex_gn_product*): H v = J^T W J v for per-point fields in one call,
against the composition it is defined by - render_vertex_adjoint_batch(np.float32(w) * render_vertex_tangent(v)) - and
against the numpy restatement of the vertex adjoint on the library's own g = w * jv_out.  Every test opens its own contexts.

Bars.  jv_out against render_vertex_tangent: bit for bit.  h against the composition: with "vertex_exact" 0, 1e-9 x max |h|
per field (DESIGN 4.7's bar for the same statement about the scalar product: the two differ in the order of fp64 additions
alone); with "vertex_exact" 1, bit for bit.  Against the restatement: tests/test_gpu_vertex_adjoint.py's two bars for an
upstream image (1e-6 x max per component column; 1e-9 scale_raw + dz_err sens_raw + 2^-970 per component).  Structure:
<u, H v> against sum w jv_u jv_v (fp64) within 2^-22 sum |w jv_v| |jv_u|, the library's duality bar with g = w jv_v.

Measured on an MI355X: composition with "vertex_exact" 0 at most 1.2e-15 of a field's largest component; restatement 9.4e-15 of
a column's maximum and 3.8e-5 of the element bar; the bilinear form at most 0.06 of its bar."""
import ctypes as C
import functools

import numpy as np
import pytest

from course5_amd import capi
from course5_amd import meshgen as mg
from tests import adjoint_reference as ar, motion_reference as mr, vertex_adjoint_reference as vr
from tests.test_gpu_motion import B, ROTS, SMALL_BOUNDS, SMALL_ROTS, _ctx, _scene
from tests.test_gpu_vertex_adjoint_batch import _assert_close, _dz_err, _interpenetrating_boxes

pytestmark = pytest.mark.gpu
KS = (1, 3, 8, 11)


def _bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _weight(ry, rx, seed):
    """Random weights in [0, 2) with a patch and a tenth of the values exactly 0."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.0, 2.0, (ry, rx, 2)).astype(np.float32)
    w[ry // 4:ry // 2, rx // 3:2 * rx // 3] = 0.0
    w[rng.uniform(size=w.shape) < 0.1] = 0.0
    return w


def _fields(k, n_pts, seed):
    return np.random.default_rng(seed).normal(size=(k, n_pts, 3))


def _composition(ctx, fields, w):
    """The two renders and the fp32 multiply the product stands for: (h [K, n_pts, 3], jv [K, rows, res_x, 2])."""
    jv = ctx.render_vertex_tangent(fields)
    g = jv if w is None else np.float32(w) * jv
    assert g.dtype == np.float32
    return ctx.render_vertex_adjoint_batch(g), jv


def _assert_composition(h, want, what):
    assert h.shape == want.shape and np.isfinite(h).all()
    for j, (a, b) in enumerate(zip(h, want)):
        top, err = np.abs(b).max(), np.abs(a - b).max()
        print(f"{what} field {j}: max |h - composition| {err:.3g} of max {top:.3g} ({err / top if top else 0.0:.3g})")
        assert top > 0 and err <= 1e-9 * top, f"{what} field {j}: {err:.3g} vs max {top:.3g}"


def _scenes(kind):
    """(xyz, cells, rots, rx, ry, bounds, options, solid): the scenes every composition test runs on."""
    if kind in ("kuhn3_off_tile", "ball", "hanging_nodes"):
        return _scene(kind) + ((), None)
    if kind == "morton":  # 4 374 cells: kept in Morton order on the device under "cell_order" 1
        xyz, cells = mg.kuhn_box(9, jitter=0.1)
        assert len(cells) >= 4096
        return xyz, cells, ROTS, 33, 26, B, (("cell_order", 1),), None
    if kind == "solid":
        xyz, cells = mg.kuhn_box(5, jitter=0.1)
        sx, sc = mg.kuhn_box(2, lo=(0.9, -0.15, 0.3), size=0.3)
        return xyz, cells, ROTS, 40, 30, B, (), sx[sc].reshape(-1, 12)
    if kind == "soup":  # per-cell copies of the points, on bin_sort_resolve's lists
        xyz, cells = mg.per_cell_point_copies(*mg.kuhn_box(3, jitter=0.2))
        return xyz, cells, SMALL_ROTS, 50, 37, SMALL_BOUNDS, (("algorithm", 1),), None
    assert kind == "boxes"  # the first walk finds the overlap: C5_RETRY, settled inside the call
    xyz, cells = _interpenetrating_boxes()
    return xyz, cells, ROTS, 80, 60, B, (), None


ALL_SCENES = ("kuhn3_off_tile", "ball", "hanging_nodes", "morton", "solid", "soup", "boxes")


def _open(kind, seed, options=()):
    xyz, cells, rots, rx, ry, bounds, opts, solid = _scenes(kind)
    alpha, q = mr.scalars(len(cells), seed)
    given = dict(opts)
    given.update(dict(options))
    ctx = _ctx(xyz, cells, alpha, q, rots, rx, ry, bounds, tuple(given.items()))
    if solid is not None:
        ctx.set_solid(0, solid)
    return ctx, xyz, rx, ry


def _welded_garbage(xyz, fields, seed):
    """(fields with garbage in the rows of welded non-representatives - never read -, the mask of those rows)."""
    rep, merged = capi.weld_points(xyz)
    others = rep != np.arange(len(rep))
    assert others.sum() == merged
    moved = fields[:, rep]  # (a weld group moves as one)
    garbage = moved.copy()
    if merged:
        garbage[:, others] = 1e6 * np.random.default_rng(seed).normal(size=(len(fields), int(merged), 3))
    return garbage, others


# ---- jv_out ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("width", [4, 8])
def test_jv_out_is_the_tangent_render_bit_for_bit(width):
    ctx, xyz, rx, ry = _open("kuhn3_off_tile", 3, (("batch_width", width),))
    fields, w = _fields(max(KS), len(xyz), 91), _weight(ry, rx, 92)
    with ctx:
        want = ctx.render_vertex_tangent(fields)
        assert np.abs(want).max() > 0
        for k in KS:
            for weight in (w, None):
                h, jv = ctx.render_vertex_gn_product(fields[:k], weight, want_jv=True)
                assert jv.shape == (k, ry, rx, 2) and np.array_equal(_bits32(jv), _bits32(want[:k])), (k, weight is None)
                assert h.shape == (k, len(xyz), 3)
        h, jv = ctx.render_vertex_gn_product(fields[0], w, want_jv=True)  # one field without the batch axis
        assert h.shape == (len(xyz), 3) and np.array_equal(_bits32(jv), _bits32(want[0]))


# ---- the composition, "vertex_exact" 0 --------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ALL_SCENES)
def test_composition_with_atomic_sums(kind):
    ctx, xyz, rx, ry = _open(kind, 4)
    fields, others = _welded_garbage(xyz, _fields(max(KS), len(xyz), 93), 94)
    w = _weight(ry, rx, 95)
    with ctx:
        for merge in (1, 0):  # ("vertex_merge" is the one field's: the batch always merges)
            ctx.set_option("vertex_merge", merge)
            for k in KS if merge else (1, 3):
                want, jv = _composition(ctx, fields[:k], w)
                h, jv_out = ctx.render_vertex_gn_product(fields[:k], w, want_jv=True)
                assert np.array_equal(_bits32(jv_out), _bits32(jv))
                _assert_composition(h, want, f"{kind} K {k} merge {merge}")
                assert not h[:, others].any()  # exact zeros on welded non-representatives
        want, _jv = _composition(ctx, fields[:3], None)
        _assert_composition(ctx.render_vertex_gn_product(fields[:3]), want, f"{kind} NULL weight")
        zero = ctx.render_vertex_gn_product(fields[:3], np.zeros((ry, rx, 2), np.float32))
        assert not zero.any()  # a weight of zeros: exact zeros
    assert others.any() or kind != "soup"


def test_row_ranges_and_cyclic_row_tiles_sum_to_the_whole_frame():
    xyz, cells, rots, rx, ry, bounds = _scene("kuhn3_off_tile")
    alpha, q = mr.scalars(len(cells), 5)
    fields, w = _fields(5, len(xyz), 96), _weight(ry, rx, 97)
    with _ctx(xyz, cells, alpha, q, rots, rx, ry, bounds) as ctx:
        whole, jv_whole = ctx.render_vertex_gn_product(fields, w, want_jv=True)
    cut = 13  # (off the 8-row tile)
    layouts = {"ranges": [(lambda c, b=b, n=n: c.set_row_range(b, n), np.arange(b, b + n)) for b, n in ((0, cut), (cut, ry - cut))],
               "tiles": [(lambda c, r=r: c.set_row_tiles(4, r, 2), np.array([y for y in range(ry) if (y // 4) % 2 == r])) for r in range(2)]}
    for name, parts in layouts.items():
        total = np.zeros_like(whole)
        for place, rows in parts:
            with _ctx(xyz, cells, alpha, q, rots, rx, ry, bounds) as ctx:
                place(ctx)
                part_w = np.ascontiguousarray(w[rows])
                h, jv = ctx.render_vertex_gn_product(fields, part_w, want_jv=True)
                assert np.array_equal(_bits32(jv), _bits32(jv_whole[:, rows]))
                want, _jv = _composition(ctx, fields, part_w)
                _assert_composition(h, want, f"{name} rows {rows[0]}..")
                total += h
        _assert_composition(total, whole, name)


# ---- the composition, "vertex_exact" 1 --------------------------------------------------------------------------------

@pytest.mark.parametrize("cell_order", [0, 1])
@pytest.mark.parametrize("kind", ALL_SCENES)
def test_composition_with_exact_sums_is_bit_for_bit(kind, cell_order):
    ctx, xyz, rx, ry = _open(kind, 6, (("cell_order", cell_order), ("vertex_exact", 1)))
    fields, others = _welded_garbage(xyz, _fields(11, len(xyz), 98), 99)
    w = _weight(ry, rx, 100)
    with ctx:
        for k in (1, 3, 11):
            want, jv = _composition(ctx, fields[:k], w)
            h, jv_out = ctx.render_vertex_gn_product(fields[:k], w, want_jv=True)
            again = ctx.render_vertex_gn_product(fields[:k], w)
            assert np.abs(want).max() > 0
            assert np.array_equal(_bits32(jv_out), _bits32(jv))
            differ = int((_bits64(h) != _bits64(want)).sum())
            assert differ == 0, f"{kind} cell_order {cell_order} K {k}: {differ} values differ from the composition in bits"
            assert np.array_equal(_bits64(again), _bits64(h)), f"{kind} K {k}: a second call gives other bits"
            assert not _bits64(h[:, others]).any()  # +0.0 to the bit
        want, _jv = _composition(ctx, fields[:3], None)
        assert np.array_equal(_bits64(ctx.render_vertex_gn_product(fields[:3])), _bits64(want))


def test_exact_sums_over_row_parts():
    xyz, cells, rots, rx, ry, bounds = _scene("kuhn3_off_tile")
    alpha, q = mr.scalars(len(cells), 7)
    fields, w = _fields(3, len(xyz), 101), _weight(ry, rx, 102)
    parts = [(lambda c: c.set_row_range(0, 13), np.arange(13)), (lambda c: c.set_row_range(13, ry - 13), np.arange(13, ry)),
             (lambda c: c.set_row_tiles(4, 1, 2), np.array([y for y in range(ry) if (y // 4) % 2 == 1]))]
    for place, rows in parts:
        with _ctx(xyz, cells, alpha, q, rots, rx, ry, bounds, (("vertex_exact", 1),)) as ctx:
            place(ctx)
            part_w = np.ascontiguousarray(w[rows])
            want, _jv = _composition(ctx, fields, part_w)
            assert np.abs(want).max() > 0
            assert np.array_equal(_bits64(ctx.render_vertex_gn_product(fields, part_w)), _bits64(want))


# ---- the restatement --------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _matrices(kind, seed):
    xyz, cells, rots, rx, ry, bounds = _scene(kind)
    alpha, q = mr.scalars(len(cells), seed)
    m = ar.ray_matrices(xyz, cells, alpha, q, rots, rx, ry, bounds)
    geo = vr.segment_faces(xyz, cells, rots, rx, ry, bounds)
    return xyz, cells, rots, rx, ry, bounds, alpha, q, m, geo


@pytest.mark.parametrize("kind,exact", [("kuhn3_off_tile", 0), ("kuhn3_off_tile", 1), ("hanging_nodes", 0)])
def test_restatement_on_the_library_s_own_upstream_image(kind, exact):
    xyz, cells, rots, rx, ry, bounds, alpha, q, m, geo = _matrices(kind, 8)
    fields, w = _fields(5, len(xyz), 103), _weight(ry, rx, 104)
    with _ctx(xyz, cells, alpha, q, rots, rx, ry, bounds, (("vertex_exact", exact),)) as ctx:
        h, jv = ctx.render_vertex_gn_product(fields, w, want_jv=True)
        h1 = ctx.render_vertex_gn_product(fields[0], w)
    dz_err = _dz_err(xyz, rots)
    for j, g in enumerate(np.float32(w) * jv):
        _assert_close(h[j], vr.gradients_of(m, geo, cells, len(xyz), rots, g), dz_err, f"{kind} exact {exact} field {j}")
    _assert_close(h1, vr.gradients_of(m, geo, cells, len(xyz), rots, np.float32(w) * jv[0]), dz_err, f"{kind} exact {exact} one field")


# ---- structure --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["kuhn3_off_tile", "hanging_nodes"])
def test_bilinear_form_symmetry_and_semidefiniteness(kind):
    ctx, xyz, rx, ry = _open(kind, 9)
    w = _weight(ry, rx, 105)
    uv = _fields(2, len(xyz), 106)
    with ctx:
        h, jv = ctx.render_vertex_gn_product(uv, w, want_jv=True)
    g = (np.float32(w) * jv).astype(np.float64)  # g[j] = w * jv_j, the fp32 product the library forms
    jv = jv.astype(np.float64)
    form, bar = np.zeros((2, 2)), np.zeros((2, 2))
    for i in range(2):  # <u_i, H u_j> against sum w jv_i jv_j
        for j in range(2):
            form[i, j] = float((uv[i] * h[j]).sum())
            want = float((g[j] * jv[i]).sum())
            bar[i, j] = 2.0 ** -22 * float((np.abs(g[j]) * np.abs(jv[i])).sum())
            print(f"{kind} <u{i}, H u{j}> = {form[i, j]:.12g}, sum w jv jv = {want:.12g}, |difference| {abs(form[i, j] - want):.3g}, bar {bar[i, j]:.3g}")
            assert bar[i, j] > 0 and abs(form[i, j] - want) <= bar[i, j]
    assert abs(form[0, 1] - form[1, 0]) <= bar[0, 1] + bar[1, 0]  # (sum w jv_u jv_v is symmetric up to g's fp32 rounding: inside the bars)
    assert form[0, 0] >= -bar[0, 0] and form[1, 1] >= -bar[1, 1] and (w >= 0).all()


# ---- side effects and refusals ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("exact", [0, 1])
def test_device_form_and_no_trace_left(exact):
    import torch
    xyz, cells, rots, rx, ry, bounds = _scene("kuhn3_off_tile")
    alpha, q = mr.scalars(len(cells), 10)
    fields, w = _fields(9, len(xyz), 107), _weight(ry, rx, 108)
    opts = (("vertex_exact", exact),)
    with _ctx(xyz, cells, alpha, q, rots, rx, ry, bounds, opts) as a, _ctx(xyz, cells, alpha, q, rots, rx, ry, bounds, opts) as b:
        for _ in range(3):  # (three frames: the view cache is in use by the third)
            a.render(), b.render()
        before = a.stats()
        h, jv = a.render_vertex_gn_product(fields, w, want_jv=True)
        assert a.stats() == before
        d_dev, w_dev = torch.tensor(fields, device="cuda"), torch.tensor(w, device="cuda")
        h_dev = torch.full((9, len(xyz), 3), float("nan"), dtype=torch.float64, device="cuda")
        jv_dev = torch.full((9, ry, rx, 2), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        a.render_vertex_gn_product_device(d_dev, w_dev, h_dev, jv_dev)
        assert a.synchronize() == capi.C5_OK
        assert np.array_equal(_bits32(jv_dev.cpu().numpy()), _bits32(jv))
        if exact:
            assert np.array_equal(_bits64(h_dev.cpu().numpy()), _bits64(h))
        else:
            _assert_composition(h_dev.cpu().numpy(), h, "device form")
        a.render_vertex_gn_product_device(d_dev[:1].contiguous(), None, h_dev[:1], None)  # NULL weight, NULL jv_out
        assert a.synchronize() == capi.C5_OK
        _assert_composition(h_dev[:1].cpu().numpy(), a.render_vertex_gn_product(fields[:1]), "device form, one field")
        # the parts afterwards pass on their own: the heads were handed back clean
        want, _jv = _composition(a, fields[:3], w)
        _assert_composition(h[:3], want, "the composition after the product")
        assert a.stats() == before
        for _ in range(3):
            ia, ib = a.render(), b.render()
            assert np.array_equal(ia.view(np.uint32), ib.view(np.uint32))
        assert a.stats()["segments"] == b.stats()["segments"]


def test_bad_arguments_and_outstanding_async_frames_are_refused():
    xyz, cells, rots, rx, ry, bounds = _scene("kuhn3")
    alpha, q = mr.scalars(len(cells), 12)
    fields = _fields(2, len(xyz), 109)
    out = np.zeros((2, len(xyz), 3))
    dp = C.POINTER(C.c_double)
    with _ctx(xyz, cells, alpha, q, rots, rx, ry, bounds) as ctx:
        lib, h = ctx.lib, ctx.handle
        fp_, op = fields.ctypes.data_as(dp), out.ctypes.data_as(dp)
        assert lib.c5_render_vertex_gn_product(h, 0, fp_, None, op, None) == capi.C5_ERR_INVALID
        assert lib.c5_render_vertex_gn_product(h, -1, fp_, None, op, None) == capi.C5_ERR_INVALID
        assert lib.c5_render_vertex_gn_product(h, 2, None, None, op, None) == capi.C5_ERR_INVALID
        assert lib.c5_render_vertex_gn_product(h, 2, fp_, None, None, None) == capi.C5_ERR_INVALID
        assert lib.c5_render_vertex_gn_product_device(h, 2, None, None, None, None) == capi.C5_ERR_INVALID
        assert lib.c5_render_vertex_gn_product_device(h, 0, 1, None, 1, None) == capi.C5_ERR_INVALID
        assert lib.c5_render_vertex_gn_product(None, 2, fp_, None, op, None) == capi.C5_ERR_INVALID
        assert not out.any()
        with pytest.raises(ValueError):
            ctx.render_vertex_gn_product(fields[:, 1:])
        buf = ctx.host_image()
        ctx.render_host_async(buf)
        with pytest.raises(capi.C5Error) as e:
            ctx.render_vertex_gn_product(fields)
        assert e.value.code == capi.C5_ERR_STATE
        assert ctx.render_host_wait() == capi.C5_OK
        ctx.free_host_image(buf)
        good = ctx.render_vertex_gn_product(fields)
        want, _jv = _composition(ctx, fields, None)
        _assert_composition(good, want, "after the refusals")


def test_a_scene_without_cells_gives_zeros():
    xyz = np.array([[1.0, 0.0, 0.0], [1.2, 0.0, 0.0], [1.0, 0.2, 0.0], [1.0, 0.0, 0.2]])
    sx, sc = mg.kuhn_box(2, lo=(0.9, -0.15, 0.3), size=0.3)
    with capi.Context(0) as ctx:
        ctx.upload_grid(xyz, np.zeros((0, 4), np.int32), np.zeros(0), np.zeros(0))
        ctx.set_image(25, 19, B)
        ctx.set_view(ROTS)
        ctx.set_solid(0, sx[sc].reshape(-1, 12))
        d, h = np.ones((3, 4, 3)), np.full((3, 4, 3), np.nan)  # (the binding hands over zeros: the library itself is asked)
        jv = np.full((3, 19, 25, 2), np.nan, np.float32)
        dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
        rc = ctx.lib.c5_render_vertex_gn_product(ctx.handle, 3, d.ctypes.data_as(dp), None, h.ctypes.data_as(dp), jv.ctypes.data_as(fp))
        assert rc == capi.C5_OK and ctx.local_rows == 19
    assert not _bits64(h).any() and not _bits32(jv).any()


# ---- fit.shape_step and autograd ------------------------------------------------------------------------------------------

def _cg_on_the_composition(ctx, residual, w, damping, iters):
    """fit.shape_step's iteration written out on the two renders and a torch multiply: the H of the commit before the
    fused call.  Every line is fit._shape_cg's, in its order, on torch float64 tensors on the GPU."""
    import torch
    from course5_amd import autograd
    device = torch.device("cuda", ctx.device)

    def JtW(img):
        return autograd._vertex_adjoint(ctx, (img if w is None else img * w).contiguous(), device)

    def H(p):
        return JtW(autograd._vertex_tangent(ctx, p.reshape(1, ctx.n_pts, 3).contiguous(), device)[0])

    def dot(a, b):
        return float((a * b).sum())

    g = JtW(residual)
    x, hx = torch.zeros_like(g), torch.zeros_like(g)
    res = -g
    p = res.clone()
    rr = dot(res, res)
    models = []
    for _ in range(iters):
        if not rr > 0.0:
            break
        ap = H(p) + damping * p
        curvature = dot(p, ap)
        if not curvature > 0.0:
            break
        step = rr / curvature
        x += step * p
        hx += step * ap
        res -= step * ap
        models.append(0.5 * dot(x, hx) + dot(x, g))
        rr_next = dot(res, res)
        p = res + (rr_next / rr) * p
        rr = rr_next
    return x, models


@pytest.mark.parametrize("weighted", [True, False])
def test_shape_step_is_the_cg_on_the_composition_bit_for_bit(weighted):
    import torch
    from course5_amd import fit
    xyz, cells = mg.kuhn_box(4, jitter=0.1)
    rx, ry = 80, 60
    alpha, q = mr.scalars(len(cells), 13)
    rng = np.random.default_rng(110)
    moved = xyz + 0.004 * rng.normal(size=xyz.shape)
    with _ctx(moved, cells, alpha, q, ROTS, rx, ry, B, (("vertex_exact", 1),)) as ctx:
        target = ctx.render()
        ctx.update_points(xyz)
        residual = torch.tensor(ctx.render() - target, device="cuda")
        w = torch.tensor(_weight(ry, rx, 111), device="cuda") if weighted else None
        ta, tq = torch.tensor(alpha, device="cuda"), torch.tensor(q, device="cuda")
        d, models = fit.shape_step(ctx, ta, tq, residual, w, damping=1e-3, iters=4)
        want, want_models = _cg_on_the_composition(ctx, residual, w, 1e-3, 4)
        again, _models = fit.shape_step(ctx, ta, tq, residual, w, damping=1e-3, iters=4)
    assert len(models) == 4 and float(d.abs().max()) > 0
    assert models == want_models
    assert np.array_equal(_bits64(d.cpu().numpy()), _bits64(want.cpu().numpy()))
    assert np.array_equal(_bits64(again.cpu().numpy()), _bits64(d.cpu().numpy()))


def test_autograd_operator():
    import torch
    from course5_amd import autograd
    xyz, cells, rots, rx, ry, bounds = _scene("kuhn3_off_tile")
    alpha, q = mr.scalars(len(cells), 14)
    fields, w = _fields(3, len(xyz), 112), _weight(ry, rx, 113)
    with _ctx(xyz, cells, alpha, q, rots, rx, ry, bounds, (("vertex_exact", 1),)) as ctx:
        ta, tq = torch.tensor(alpha, device="cuda"), torch.tensor(q, device="cuda")
        tv, tw = torch.tensor(fields, device="cuda"), torch.tensor(w, device="cuda")
        h = autograd.vertex_gn_product(ctx, ta, tq, tv, tw)
        h1 = autograd.vertex_gn_product(ctx, ta, tq, tv[0])
        assert h.shape == (3, len(xyz), 3) and h.dtype == torch.float64 and h.is_cuda and not h.requires_grad
        assert h1.shape == (len(xyz), 3)
        assert np.array_equal(_bits64(h.cpu().numpy()), _bits64(ctx.render_vertex_gn_product(fields, w)))
        assert np.array_equal(_bits64(h1.cpu().numpy()), _bits64(ctx.render_vertex_gn_product(fields[0])))
        with pytest.raises(ValueError, match="v_xyz must be"):
            autograd.vertex_gn_product(ctx, ta, tq, tv[:, 1:])
        with pytest.raises(ValueError, match="weight must be"):
            autograd.vertex_gn_product(ctx, ta, tq, tv, tw[1:])
        with pytest.raises(RuntimeError, match="operator with no derivative"):
            torch.func.grad(lambda a: autograd.vertex_gn_product(ctx, a, tq, tv[0]).sum())(ta)
        assert np.array_equal(_bits64(autograd.vertex_gn_product(ctx, ta, tq, tv, tw).cpu().numpy()), _bits64(h.cpu().numpy()))

"""Vertex tangent render on the GPU (c5_render_vertex_tangent*) against the numpy restatement
(tests/vertex_tangent_reference.py), the library's own motion tangent (affine fields) and vertex adjoint (its transpose),
and central differences of two real renders through c5_update_points.  Every test opens its own contexts.

Bars.  Against the restatement, the motion test's two: 1e-6 x max |ref| per channel and field, and per element
2^-23 |ref| + 1e-9 scale + dz_err sens + 2^-103 (calibrated in tests/test_vertex_tangent_cpu.py).  Against the motion
tangent: 1e-6 x max per channel.  Duality with the vertex adjoint: 2^-22 x sum_p |g_p| |out_p| (tests/
test_gpu_vertex_adjoint.py's bar).  Batches, row splits, the device form and repeated calls: equal bits."""
import ctypes as C
import types

import numpy as np
import pytest

from course5_amd import capi
from course5_amd import meshgen as mg
from tests import adjoint_reference as ar, derivative_fuzz as fz, motion_reference as mr
from tests import vertex_adjoint_reference as vr, vertex_tangent_reference as vt
from tests.test_gpu_motion import B, ROTS, _ctx, _scene

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _fields(n_pts, k, seed):
    return np.random.default_rng(seed).normal(size=(k, n_pts, 3))


def _assert_close(got, xyz, cells, alpha, q, rots, rx, ry, bounds, fields, what, rows=None, skip=None):
    dz_err = fz.dz_err(types.SimpleNamespace(xyz=xyz, rots=rots))
    refs = vt.image_tangent(xyz, cells, alpha, q, rots, rx, ry, bounds, fields, rows=rows, skip=skip, with_scale=True)
    assert got.shape == (len(fields),) + refs[0][0].shape + (2,)
    for j, (tau_dot, I_dot, ex) in enumerate(refs):
        for ch, name, ref in ((0, "tau_dot", tau_dot), (1, "I_dot", I_dot)):
            g = got[j, ..., ch].astype(np.float64)
            err = np.abs(g - ref)
            top = np.abs(ref).max()
            key = "tau" if ch == 0 else "I"
            tol = 2.0 ** -23 * np.abs(ref) + 1e-9 * ex["scale_" + key] + dz_err * ex["sens_" + key] + 2.0 ** -103
            print(f"{what} field {j} {name}: max error {err.max():.3g} of max {top:.3g}, worst error / element bar {(err / tol).max():.3g}")
            assert np.isfinite(g).all() and top > 0
            assert err.max() <= 1e-6 * top, f"{what} field {j} {name}: max abs error {err.max():.3g} vs max {top:.3g}"
            assert (err <= tol).all(), f"{what} field {j} {name}: {int((err > tol).sum())} elements over their bar, worst {(err / tol).max():.3g}"


def _interpenetrating_boxes():
    xa, ca = mg.kuhn_box(3, lo=(0.6, -0.4, -0.3), size=0.6, jitter=0.1, seed=5)
    xb, cb = mg.kuhn_box(4, lo=(0.85, -0.2, -0.45), size=0.7, jitter=0.1, seed=6)
    return np.vstack([xa, xb]), np.vstack([ca, cb + len(xa)]).astype(np.int32)


@pytest.mark.parametrize("kind", ["kuhn3", "kuhn3_off_tile", "ball", "hanging_nodes"])
def test_walk_against_the_restatement(kind):
    xyz, cells, rots, rx, ry, bounds = _scene(kind)
    alpha, q = mr.scalars(len(cells), 3)
    fields = _fields(len(xyz), 3, 61)
    with _ctx(xyz, cells, alpha, q, rots, rx, ry, bounds, (("cell_order", 0),)) as ctx:
        got = ctx.render_vertex_tangent(fields)
        again = ctx.render_vertex_tangent(fields)
        zero = ctx.render_vertex_tangent(np.zeros_like(xyz))
    assert np.array_equal(_bits(got), _bits(again))  # two calls: equal bits
    assert zero.shape == (ry, rx, 2) and not zero.any()  # a zero field: exactly 0
    _assert_close(got, xyz, cells, alpha, q, rots, rx, ry, bounds, fields, kind)


@pytest.mark.parametrize("kind", ["kuhn3_off_tile", "hanging_nodes"])
def test_affine_fields_give_the_motion_tangent(kind):
    """d_xyz[v] = M^T (A p_v + b), p_v the point in view space: the library's own motion tangent for (A, b)."""
    xyz, cells, rots, rx, ry, bounds = _scene(kind)
    alpha, q = mr.scalars(len(cells), 4)
    affine = np.vstack([capi.rotation_motion(rots, i) for i in range(len(rots))] + [np.random.default_rng(62).normal(size=(2, 12))])
    with _ctx(xyz, cells, alpha, q, rots, rx, ry, bounds) as ctx:
        want = ctx.render_motion_tangent(affine).astype(np.float64)
        ctx.render()
        p = ctx.view_points(len(xyz))
        M = vr.view_matrix(ctx.rots)
        d = np.stack([(p @ f[:9].reshape(3, 3).T + f[9:]) @ M for f in affine])
        got = ctx.render_vertex_tangent(d).astype(np.float64)
    for j in range(len(affine)):
        for ch, name in ((0, "tau_dot"), (1, "I_dot")):
            err, top = np.abs(got[j, ..., ch] - want[j, ..., ch]).max(), np.abs(want[j, ..., ch]).max()
            print(f"{kind} affine field {j} {name}: max error {err:.3g} of max {top:.3g}")
            assert top > 0 and err <= 1e-6 * top


@pytest.mark.parametrize("kind", ["kuhn3_off_tile", "ball", "hanging_nodes"])
def test_duality_with_the_vertex_adjoint(kind):
    """<g, J d> = <J^T g, d> for general per-point fields: the two renders are transposes of each other."""
    xyz, cells, rots, rx, ry, bounds = _scene(kind)
    alpha, q = mr.scalars(len(cells), 8)
    g = np.random.default_rng(63).normal(size=(ry, rx, 2)).astype(np.float32)
    fields = _fields(len(xyz), 4, 64)
    with _ctx(xyz, cells, alpha, q, rots, rx, ry, bounds) as ctx:
        grad = ctx.render_vertex_adjoint(g)
        out = ctx.render_vertex_tangent(fields).astype(np.float64)
    g64 = g.astype(np.float64)
    for j, (d, o) in enumerate(zip(fields, out)):
        lhs, rhs = float((g64 * o).sum()), float((grad * d).sum())
        bar = 2.0 ** -22 * float((np.abs(g64) * np.abs(o)).sum())
        print(f"{kind} field {j}: <g, out> = {lhs:.9g}, <grad_xyz, d> = {rhs:.9g}, difference / bar = {abs(lhs - rhs) / bar:.3g}")
        assert abs(rhs) > 0 and abs(lhs - rhs) <= bar, (j, lhs, rhs, bar)


def test_batches_are_bit_equal_to_single_calls_at_both_widths():
    xyz, cells, rots, rx, ry, bounds = _scene("kuhn3_off_tile")
    alpha, q = mr.scalars(len(cells), 8)
    fields = _fields(len(xyz), 11, 65)
    with _ctx(xyz, cells, alpha, q, rots, rx, ry, bounds) as ctx:
        singles = np.stack([ctx.render_vertex_tangent(f) for f in fields])
        assert np.abs(singles[0]).max() > 0
        for width in (4, 8):
            ctx.set_option("batch_width", width)
            for k in (1, 3, 8, 11):
                got = ctx.render_vertex_tangent(fields[:k])
                assert np.array_equal(_bits(got), _bits(singles[:k])), (width, k)


def test_soup_on_the_fallback_reads_the_representatives_only():
    xyz, cells = mg.kuhn_box(4, jitter=0.1)
    soup_xyz, soup_cells = mg.per_cell_point_copies(xyz, cells)
    alpha, q = mr.scalars(len(cells), 4)
    rep, merged = capi.weld_points(soup_xyz)
    others = rep != np.arange(len(rep))
    assert merged == len(soup_xyz) - len(xyz) and others.sum() == merged
    fields = _fields(len(soup_xyz), 3, 66)[:, rep]  # (a group moves as one: every copy has its representative's row)
    garbage = fields.copy()
    garbage[:, others] = np.random.default_rng(67).normal(size=(3, int(others.sum()), 3)) * 1e6
    with _ctx(soup_xyz, soup_cells, alpha, q, ROTS, 80, 60, options=(("algorithm", 1),)) as ctx:
        got = ctx.render_vertex_tangent(fields)
        assert np.array_equal(_bits(got), _bits(ctx.render_vertex_tangent(fields)))
        assert np.array_equal(_bits(got[1]), _bits(ctx.render_vertex_tangent(fields[1])))
        assert np.array_equal(_bits(got), _bits(ctx.render_vertex_tangent(garbage)))  # the other rows are never read
    _assert_close(got, soup_xyz, soup_cells, alpha, q, ROTS, 80, 60, B, fields, "soup, algorithm 1")


def test_interpenetrating_boxes_across_the_retry():
    xyz, cells = _interpenetrating_boxes()
    alpha, q = mr.scalars(len(cells), 5)
    fields = _fields(len(xyz), 2, 68)
    with _ctx(xyz, cells, alpha, q, ROTS, 80, 60) as ctx:
        got = ctx.render_vertex_tangent(fields)  # the first walk finds the overlap (C5_RETRY, settled inside the call)
        assert np.array_equal(_bits(got), _bits(ctx.render_vertex_tangent(fields)))
    _assert_close(got, xyz, cells, alpha, q, ROTS, 80, 60, B, fields, "overlapping boxes")


def test_solid_pixels_are_zero():
    xyz, cells = mg.kuhn_box(5, jitter=0.1)
    rx, ry = 80, 60
    alpha, q = mr.scalars(len(cells), 6)
    fields = _fields(len(xyz), 2, 69)
    sx, sc = mg.kuhn_box(2, lo=(0.9, -0.15, 0.3), size=0.3)
    with _ctx(xyz, cells, alpha, q, ROTS, rx, ry) as ctx:
        ctx.set_solid(0, sx[sc].reshape(-1, 12))  # colour NaN: solid pixels are NaN in the image
        img = ctx.render()
        got = ctx.render_vertex_tangent(fields)
    skip = np.isnan(img[..., 0])
    assert 20 < skip.sum() < skip.size // 2
    assert not got[:, skip].any()  # exactly 0
    _assert_close(got, xyz, cells, alpha, q, ROTS, rx, ry, B, fields, "solid", skip=skip)


def test_row_ranges_and_cyclic_row_tiles_are_rows_of_the_whole_frame():
    xyz, cells = mg.kuhn_box(5, jitter=0.1)
    rx, ry = 80, 60
    alpha, q = mr.scalars(len(cells), 7)
    fields = _fields(len(xyz), 2, 70)
    with _ctx(xyz, cells, alpha, q, ROTS, rx, ry) as ctx:
        whole = ctx.render_vertex_tangent(fields)
    assert np.abs(whole).max() > 0
    for begin, count in ((0, 23), (23, ry - 23)):
        with _ctx(xyz, cells, alpha, q, ROTS, rx, ry) as ctx:
            ctx.set_row_range(begin, count)
            got = ctx.render_vertex_tangent(fields)
        assert got.shape == (2, count, rx, 2)
        assert np.array_equal(_bits(got), _bits(whole[:, begin:begin + count]))
    for rank in range(2):
        with _ctx(xyz, cells, alpha, q, ROTS, rx, ry) as ctx:
            ctx.set_row_tiles(3, rank, 2)
            got = ctx.render_vertex_tangent(fields)
        rows = np.array([r for r in range(ry) if (r // 3) % 2 == rank])
        assert np.array_equal(_bits(got), _bits(whole[:, rows]))


def test_morton_ordered_cells():
    xyz, cells = mg.kuhn_box(9, jitter=0.1)  # 4 374 cells: kept in Morton order on the device ("cell_order" 1)
    assert len(cells) >= 4096
    rx, ry = 64, 48
    alpha, q = mr.scalars(len(cells), 7)
    fields = _fields(len(xyz), 2, 71)
    with _ctx(xyz, cells, alpha, q, ROTS, rx, ry, options=(("cell_order", 1),)) as ctx:
        got = ctx.render_vertex_tangent(fields)
    _assert_close(got, xyz, cells, alpha, q, ROTS, rx, ry, B, fields, "cell_order 1")


def test_device_form_and_renders_around_it():
    import torch
    xyz, cells = mg.kuhn_box(5, jitter=0.1)
    rx, ry = 160, 120
    alpha, q = mr.scalars(len(cells), 11)
    fields = _fields(len(xyz), 3, 72)
    with _ctx(xyz, cells, alpha, q, ROTS, rx, ry) as a, _ctx(xyz, cells, alpha, q, ROTS, rx, ry) as b:
        for _ in range(3):  # (three frames: the view cache is in use by the third)
            a.render(), b.render()
        before = a.stats()
        got = a.render_vertex_tangent(fields)
        assert a.stats() == before
        d_dev = torch.tensor(fields, device="cuda")
        out_dev = torch.full((3, ry, rx, 2), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        a.render_vertex_tangent_device(d_dev, out_dev)
        assert a.synchronize() == capi.C5_OK
        assert np.array_equal(_bits(out_dev.cpu().numpy()), _bits(got))
        assert a.stats() == before
        for _ in range(3):
            ia, ib = a.render(), b.render()
            assert np.array_equal(ia.view(np.uint32), ib.view(np.uint32))
        assert a.stats()["segments"] == b.stats()["segments"]
        # the same walk whatever happened before: the bits of a context that only rendered
        assert np.array_equal(_bits(got), _bits(b.render_vertex_tangent(fields)))
    assert np.abs(got).max() > 0


def test_bad_arguments_and_outstanding_async_frames_are_refused():
    xyz, cells, rots, rx, ry, bounds = _scene("kuhn3")
    alpha, q = mr.scalars(len(cells), 12)
    d = _fields(len(xyz), 1, 73)
    out = np.zeros((1, ry, rx, 2), dtype=np.float32)
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    with _ctx(xyz, cells, alpha, q, rots, rx, ry, bounds) as ctx:
        lib, h = ctx.lib, ctx.handle
        assert lib.c5_render_vertex_tangent(h, 1, None, out.ctypes.data_as(fp)) == capi.C5_ERR_INVALID
        assert lib.c5_render_vertex_tangent(h, 1, d.ctypes.data_as(dp), None) == capi.C5_ERR_INVALID
        assert lib.c5_render_vertex_tangent(h, 0, d.ctypes.data_as(dp), out.ctypes.data_as(fp)) == capi.C5_ERR_INVALID
        assert lib.c5_render_vertex_tangent_device(h, 1, None, None) == capi.C5_ERR_INVALID
        assert lib.c5_render_vertex_tangent(None, 1, d.ctypes.data_as(dp), out.ctypes.data_as(fp)) == capi.C5_ERR_INVALID
        for bad in (d[0, 1:], d[:, :, :2], np.zeros((0, len(xyz), 3))):
            with pytest.raises(ValueError):
                ctx.render_vertex_tangent(bad)
        buf = ctx.host_image()
        ctx.render_host_async(buf)
        with pytest.raises(capi.C5Error) as e:
            ctx.render_vertex_tangent(d)
        assert e.value.code == capi.C5_ERR_STATE
        assert ctx.render_host_wait() == capi.C5_OK
        ctx.free_host_image(buf)
        assert np.abs(ctx.render_vertex_tangent(d)).max() > 0


def test_against_central_differences_of_two_renders_through_update_points():
    """Two real renders at xyz +- h d through c5_update_points, h = 2.5e-4, compared where the restated cell list of the
    pixel is the same at -h, 0 and +h (the restatement alone excludes 1.25 % of the covered pixels; fp32-rounded restated
    images differ from the tangent by 5.2e-4 (tau) and 3.4e-4 (I) of the maximum there)."""
    xyz, cells, rots, rx, ry, bounds = _scene("kuhn3")
    a, q = mr.scalars(len(cells), 7)
    alpha = 0.6 * a
    d = np.random.default_rng(51).normal(size=xyz.shape)
    h = 2.5e-4
    lists = [ar.ray_matrices(xyz + s * h * d, cells, alpha, q, rots, rx, ry, bounds)["C"] for s in (-1, 0, 1)]
    width = max(c.shape[1] for c in lists)
    pad = [np.pad(c, ((0, 0), (0, width - c.shape[1])), constant_values=-1) for c in lists]
    same = ((pad[0] == pad[1]).all(1) & (pad[2] == pad[1]).all(1)).reshape(ry, rx)
    covered = (pad[1] >= 0).any(1).reshape(ry, rx)
    excluded = 1.0 - same[covered].mean()
    with _ctx(xyz, cells, alpha, q, rots, rx, ry, bounds) as ctx:
        tan = ctx.render_vertex_tangent(d).astype(np.float64)
        imgs = []
        for s in (1, -1):
            ctx.update_points(xyz + s * h * d)
            imgs.append(ctx.render().astype(np.float64))
    fd = (imgs[0] - imgs[1]) / (2 * h)
    print(f"{excluded:.2%} of the covered pixels changed their cell list")
    assert excluded <= 0.05
    use = same & covered
    for ch, name in ((0, "tau"), (1, "I")):
        err = np.abs(fd[..., ch] - tan[..., ch])[use].max()
        top = np.abs(tan[..., ch]).max()
        print(f"{name}: max error {err:.3g} of max {top:.3g} ({err / top:.3g})")
        assert top > 0 and err <= 2e-2 * top

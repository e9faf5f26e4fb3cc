"""Vertex adjoint render on the GPU (c5_render_vertex_adjoint*, c5_update_points) against the numpy restatement
(tests/vertex_adjoint_reference.py), the library's own motion tangent (the two are transposes of each other) and exact
identities.  Every test opens its own contexts.

Bars.  Against the restatement: per component column 1e-6 x max |ref| (tests/test_gpu_adjoint.py's bar), and per component
1e-9 scale_raw + dz_err sens_raw + 2^-970 (tests/derivative_fuzz.py's bar with the vertex adjoint's own scale and chord
sensitivity, calibrated in tests/test_vertex_adjoint_cpu.py).  Run to run:
rtol 1e-12, atol 1e-15 x max (the adjoint's: fp64 atomics in arrival order).  Duality with the motion tangent:
2^-22 x sum_p |g_p| |out_p| - the motion image is fp32, every value rounded to 2^-24 relative, and a factor 4 covers the
fp64 sides."""
import ctypes as C
import types

import numpy as np
import pytest

from course5_amd import capi
from course5_amd import meshgen as mg
from tests import derivative_fuzz as fz, motion_reference as mr, vertex_adjoint_reference as vr
from tests.test_gpu_motion import B, ROTS, _ctx, _scene

pytestmark = pytest.mark.gpu


def _weights(ry, rx, seed):
    return np.random.default_rng(seed).normal(size=(ry, rx, 2)).astype(np.float32)


def _dz_err(xyz, rots):
    return fz.dz_err(types.SimpleNamespace(xyz=xyz, rots=rots))


def _assert_close(got, full, dz_err, what, onto=None):
    """full: vertex_gradients' dict; onto: the representatives its rows are summed on (a soup), bounds included."""
    ref, scale, sens = full["raw"], full["scale_raw"], full["sens_raw"]
    if onto is not None:
        ref, scale, sens = (np.zeros_like(v) for v in (ref, scale, sens))
        for acc, v in ((ref, full["raw"]), (scale, full["scale_raw"]), (sens, full["sens_raw"])):
            np.add.at(acc, onto, v)  # the group's sum on its representative
    assert got.shape == ref.shape and np.isfinite(got).all()
    for k, name in enumerate("xyz"):
        err, top = np.abs(got[:, k] - ref[:, k]).max(), np.abs(ref[:, k]).max()
        print(f"{what} grad_{name}: max error {err:.3g} of max {top:.3g} ({err / top:.3g})")
        assert top > 0 and err <= 1e-6 * top, f"{what} grad_{name}: max abs error {err:.3g} vs max {top:.3g}"
    # ... and every component on its own scale: a point whose gradient is small is held as tightly as the largest
    tol = 1e-9 * scale + dz_err * sens + 2.0 ** -970
    r = np.abs(got - ref) / tol
    print(f"{what}: worst error / element bar {r.max():.3g}")
    assert (r <= 1.0).all(), f"{what}: {int((r > 1).sum())} components over their bar, worst {r.max():.3g} at {np.unravel_index(r.argmax(), r.shape)}"


def _assert_same_run(a, b, parts=1):
    np.testing.assert_allclose(a, b, rtol=parts * 1e-12, atol=parts * 1e-15 * np.abs(b).max())


def _interpenetrating_boxes():
    xa, ca = mg.kuhn_box(3, lo=(0.6, -0.4, -0.3), size=0.6, jitter=0.1, seed=5)
    xb, cb = mg.kuhn_box(4, lo=(0.85, -0.2, -0.45), size=0.7, jitter=0.1, seed=6)
    return np.vstack([xa, xb]), np.vstack([ca, cb + len(xa)]).astype(np.int32)


@pytest.mark.parametrize("kind", ["kuhn3", "kuhn3_off_tile", "ball", "hanging_nodes"])
def test_walk_against_the_restatement(kind):
    xyz, cells, rots, rx, ry, bounds = _scene(kind)
    alpha, q = mr.scalars(len(cells), 3)
    g = _weights(ry, rx, 31)
    with _ctx(xyz, cells, alpha, q, rots, rx, ry, bounds, (("cell_order", 0),)) as ctx:
        got = ctx.render_vertex_adjoint(g)
        again = ctx.render_vertex_adjoint(g)
    _assert_same_run(again, got)
    _assert_close(got, vr.vertex_gradients(xyz, cells, alpha, q, rots, rx, ry, bounds, g), _dz_err(xyz, rots), kind)


def test_soup_on_the_fallback_lands_on_the_representatives():
    xyz, cells = mg.kuhn_box(4, jitter=0.1)
    soup_xyz, soup_cells = mg.per_cell_point_copies(xyz, cells)
    alpha, q = mr.scalars(len(cells), 4)
    g = _weights(60, 80, 32)
    with _ctx(soup_xyz, soup_cells, alpha, q, ROTS, 80, 60, options=(("algorithm", 1),)) as ctx:
        got = ctx.render_vertex_adjoint(g)
        _assert_same_run(ctx.render_vertex_adjoint(g), got)
    rep, merged = capi.weld_points(soup_xyz)
    assert merged == len(soup_xyz) - len(xyz)  # (every point of the soup is welded to some other)
    others = rep != np.arange(len(rep))
    assert others.sum() == merged and not got[others].any()  # exactly 0
    per_copy = vr.vertex_gradients(soup_xyz, soup_cells, alpha, q, ROTS, 80, 60, B, g)
    _assert_close(got, per_copy, _dz_err(soup_xyz, ROTS), "soup, algorithm 1", onto=rep)


def test_interpenetrating_boxes_across_the_retry():
    xyz, cells = _interpenetrating_boxes()
    alpha, q = mr.scalars(len(cells), 5)
    g = _weights(60, 80, 33)
    with _ctx(xyz, cells, alpha, q, ROTS, 80, 60) as ctx:
        got = ctx.render_vertex_adjoint(g)  # the first walk finds the overlap (C5_RETRY, settled inside the call)
        _assert_same_run(ctx.render_vertex_adjoint(g), got)
    _assert_close(got, vr.vertex_gradients(xyz, cells, alpha, q, ROTS, 80, 60, B, g), _dz_err(xyz, ROTS), "overlapping boxes")


def test_solid_pixels_contribute_nothing():
    xyz, cells = mg.kuhn_box(5, jitter=0.1)
    rx, ry = 80, 60
    alpha, q = mr.scalars(len(cells), 6)
    g = _weights(ry, rx, 34)
    sx, sc = mg.kuhn_box(2, lo=(0.9, -0.15, 0.3), size=0.3)
    with _ctx(xyz, cells, alpha, q, ROTS, rx, ry) as ctx:
        ctx.set_solid(0, sx[sc].reshape(-1, 12))  # colour NaN: solid pixels are NaN in the image
        img = ctx.render()
        got = ctx.render_vertex_adjoint(g)
    skip = np.isnan(img[..., 0])
    assert 20 < skip.sum() < skip.size // 2
    _assert_close(got, vr.vertex_gradients(xyz, cells, alpha, q, ROTS, rx, ry, B, g, skip=skip), _dz_err(xyz, ROTS), "solid")


def test_morton_ordered_cells():
    xyz, cells = mg.kuhn_box(9, jitter=0.1)  # 4 374 cells: kept in Morton order on the device ("cell_order" 1)
    assert len(cells) >= 4096
    rx, ry = 64, 48
    alpha, q = mr.scalars(len(cells), 7)
    g = _weights(ry, rx, 35)
    with _ctx(xyz, cells, alpha, q, ROTS, rx, ry, options=(("cell_order", 1),)) as ctx:
        got = ctx.render_vertex_adjoint(g)
    _assert_close(got, vr.vertex_gradients(xyz, cells, alpha, q, ROTS, rx, ry, B, g), _dz_err(xyz, ROTS), "cell_order 1")


def _duality(ctx, n_pts, g, fields, grad):
    """(lhs, rhs, bar) per field: sum_v grad_xyz[v] . M^T (A p_v + b), <g, motion tangent>, 2^-22 sum |g| |out|."""
    out = ctx.render_motion_tangent(fields).astype(np.float64)
    ctx.render()
    p = ctx.view_points(n_pts)
    M = vr.view_matrix(ctx.rots)
    g64 = g.astype(np.float64)
    rows = []
    for f, o in zip(fields, out):
        u = p @ f[:9].reshape(3, 3).T + f[9:]
        rows.append((float((grad * (u @ M)).sum()), float((g64 * o).sum()), 2.0 ** -22 * float((np.abs(g64) * np.abs(o)).sum())))
    return rows


@pytest.mark.parametrize("kind", ["kuhn3_off_tile", "ball", "hanging_nodes"])
def test_duality_with_the_motion_tangent(kind):
    xyz, cells, rots, rx, ry, bounds = _scene(kind)
    alpha, q = mr.scalars(len(cells), 8)
    g = _weights(ry, rx, 36)
    fields = np.vstack([capi.rotation_motion(rots, i) for i in range(len(rots))] + [np.random.default_rng(37).normal(size=(12, 12))])
    with _ctx(xyz, cells, alpha, q, rots, rx, ry, bounds) as ctx:
        grad = ctx.render_vertex_adjoint(g)
        rows = _duality(ctx, len(xyz), g, fields, grad)
    for j, (lhs, rhs, bar) in enumerate(rows):
        print(f"{kind} field {j}: <grad, u> = {lhs:.9g}, <g, motion tangent> = {rhs:.9g}, difference / bar = {abs(lhs - rhs) / bar:.3g}")
        assert abs(rhs) > 0 and abs(lhs - rhs) <= bar, (j, lhs, rhs, bar)


def test_the_pose_gradient_is_render_view_s():
    import torch
    from course5_amd import autograd
    xyz, cells, rots, rx, ry, bounds = _scene("kuhn3")
    alpha, q = mr.scalars(len(cells), 9)
    g = _weights(ry, rx, 38)
    fields = np.array([capi.rotation_motion(rots, i) for i in range(len(rots))])
    with _ctx(xyz, cells, alpha, q, rots, rx, ry, bounds) as ctx:
        grad = ctx.render_vertex_adjoint(g)
        rows = _duality(ctx, len(xyz), g, fields, grad)
        angles = torch.tensor(rots[:, 1].copy(), requires_grad=True)
        img = autograd.render_view(ctx, torch.tensor(alpha), torch.tensor(q), angles)
        (img * torch.tensor(g, device="cuda")).sum().backward()
    for (lhs, _rhs, bar), want in zip(rows, angles.grad.numpy()):
        print(f"pose: <grad, rotation field> = {lhs:.9g}, render_view's backward = {want:.9g}, difference / bar = {abs(lhs - want) / bar:.3g}")
        assert abs(want) > 0 and abs(lhs - want) <= bar


def test_row_ranges_and_cyclic_row_tiles_sum_to_the_whole_frame():
    xyz, cells = mg.kuhn_box(5, jitter=0.1)
    rx, ry = 80, 60
    alpha, q = mr.scalars(len(cells), 10)
    g = _weights(ry, rx, 39)
    with _ctx(xyz, cells, alpha, q, ROTS, rx, ry) as ctx:
        whole = ctx.render_vertex_adjoint(g)
    total = np.zeros_like(whole)
    for begin, count in ((0, 23), (23, ry - 23)):
        with _ctx(xyz, cells, alpha, q, ROTS, rx, ry) as ctx:
            ctx.set_row_range(begin, count)
            total += ctx.render_vertex_adjoint(g[begin:begin + count])
    _assert_same_run(total, whole, parts=2)
    total = np.zeros_like(whole)
    for rank in range(2):
        with _ctx(xyz, cells, alpha, q, ROTS, rx, ry) as ctx:
            ctx.set_row_tiles(3, rank, 2)
            rows = np.array([r for r in range(ry) if (r // 3) % 2 == rank])
            total += ctx.render_vertex_adjoint(g[rows])
    _assert_same_run(total, whole, parts=2)


def test_zero_weights_device_form_and_renders_around_it():
    import torch
    xyz, cells = mg.kuhn_box(5, jitter=0.1)
    rx, ry = 160, 120
    alpha, q = mr.scalars(len(cells), 11)
    g = _weights(ry, rx, 40)
    with _ctx(xyz, cells, alpha, q, ROTS, rx, ry) as a, _ctx(xyz, cells, alpha, q, ROTS, rx, ry) as b:
        for _ in range(3):  # (three frames: the view cache is in use by the third)
            a.render(), b.render()
        before = a.stats()
        got = a.render_vertex_adjoint(g)
        assert a.stats() == before
        zero = a.render_vertex_adjoint(np.zeros_like(g))
        assert zero.shape == (len(xyz), 3) and not zero.any()  # exactly 0
        g_dev = torch.tensor(g, device="cuda")
        out_dev = torch.full((len(xyz), 3), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        a.render_vertex_adjoint_device(g_dev, out_dev)
        assert a.synchronize() == capi.C5_OK
        _assert_same_run(out_dev.cpu().numpy(), got)
        for _ in range(3):
            ia, ib = a.render(), b.render()
            assert np.array_equal(ia.view(np.uint32), ib.view(np.uint32))
        assert a.stats()["segments"] == b.stats()["segments"]
    assert np.abs(got).max() > 0


def test_bad_arguments_and_outstanding_async_frames_are_refused():
    xyz, cells, rots, rx, ry, bounds = _scene("kuhn3")
    alpha, q = mr.scalars(len(cells), 12)
    g = _weights(ry, rx, 41)
    out = np.zeros((len(xyz), 3))
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    with _ctx(xyz, cells, alpha, q, rots, rx, ry, bounds) as ctx:
        lib, h = ctx.lib, ctx.handle
        assert lib.c5_render_vertex_adjoint(h, None, out.ctypes.data_as(dp)) == capi.C5_ERR_INVALID
        assert lib.c5_render_vertex_adjoint(h, g.ctypes.data_as(fp), None) == capi.C5_ERR_INVALID
        assert lib.c5_render_vertex_adjoint_device(h, None, None) == capi.C5_ERR_INVALID
        assert lib.c5_render_vertex_adjoint(None, g.ctypes.data_as(fp), out.ctypes.data_as(dp)) == capi.C5_ERR_INVALID
        with pytest.raises(ValueError):
            ctx.render_vertex_adjoint(g[1:])
        buf = ctx.host_image()
        ctx.render_host_async(buf)
        with pytest.raises(capi.C5Error) as e:
            ctx.render_vertex_adjoint(g)
        assert e.value.code == capi.C5_ERR_STATE
        assert ctx.render_host_wait() == capi.C5_OK
        ctx.free_host_image(buf)
        assert np.abs(ctx.render_vertex_adjoint(g)).max() > 0


# ---- c5_update_points -------------------------------------------------------------------------------------------------

def _jittered(xyz, cells, seed):
    """The points moved by up to 1e-3 of the shortest edge: no new coincidences."""
    e = xyz[cells[:, [0, 0, 0, 1, 1, 2]]] - xyz[cells[:, [1, 2, 3, 2, 3, 3]]]
    edge = np.sqrt((e ** 2).sum(-1)).min()
    return xyz + 1e-3 * edge * np.random.default_rng(seed).uniform(-1.0, 1.0, xyz.shape)


def _bits(img):
    return np.ascontiguousarray(img).view(np.uint32)


@pytest.mark.parametrize("kind", ["kuhn3", "ball", "kuhn9_morton", "kuhn9_row_range"])
def test_update_points_renders_the_bits_of_a_fresh_upload(kind):
    options, rows = (), None
    if kind.startswith("kuhn9"):
        xyz, cells = mg.kuhn_box(9, jitter=0.1)  # 4 374 cells: Morton order, block spheres of 256 cells
        rots, rx, ry, bounds, options = ROTS, 96, 72, B, (("cell_order", 1),)
        rows = (50, 22) if kind == "kuhn9_row_range" else None  # (a part of the rows: "block_cull" judges by the spheres)
    else:
        xyz, cells, rots, rx, ry, bounds = _scene(kind)
    alpha, q = mr.scalars(len(cells), 13)
    new = _jittered(xyz, cells, 42)
    with _ctx(xyz, cells, alpha, q, rots, rx, ry, bounds, options) as a, _ctx(new, cells, alpha, q, rots, rx, ry, bounds, options) as b:
        for ctx in (a, b):
            if rows:
                ctx.set_row_range(*rows)
        old = a.render()
        a.render()  # (the view cache holds the old points' data)
        a.update_points(new)
        got, want = a.render(), b.render()
        assert np.array_equal(_bits(got), _bits(want))
        assert not np.array_equal(_bits(got), _bits(old))
        assert a.stats()["segments"] == b.stats()["segments"]
        # the derivative renders see the new points too
        g = _weights(got.shape[0], rx, 43)
        _assert_same_run(a.render_vertex_adjoint(g), b.render_vertex_adjoint(g))
        # and back again
        a.update_points(xyz)
        assert np.array_equal(_bits(a.render()), _bits(old))


def test_update_points_refuses_a_wrong_count_and_a_nan():
    xyz, cells, rots, rx, ry, bounds = _scene("kuhn3")
    alpha, q = mr.scalars(len(cells), 14)
    with _ctx(xyz, cells, alpha, q, rots, rx, ry, bounds) as ctx:
        old = ctx.render()
        bad = xyz.copy()
        bad[5, 1] = np.nan
        for pts in (xyz[:-1], bad, np.vstack([xyz, xyz[:1]])):
            with pytest.raises(capi.C5Error) as e:
                ctx.update_points(pts)
            assert e.value.code == capi.C5_ERR_INVALID
            assert np.array_equal(_bits(ctx.render()), _bits(old))
        assert ctx.lib.c5_update_points(ctx.handle, None, len(xyz)) == capi.C5_ERR_INVALID


@pytest.mark.parametrize("kind", ["kuhn3_off_tile", "ball"])
def test_the_wave_merged_walk_gives_the_same_sums(kind):
    """"vertex_merge" 1 (the default): the lanes of a wavefront in one cell are summed in LDS before the atomics; 0: every
    lane adds its own.  Another order of the same fp64 sums: the run-to-run bar."""
    xyz, cells, rots, rx, ry, bounds = _scene(kind)
    alpha, q = mr.scalars(len(cells), 15)
    g = _weights(ry, rx, 44)
    with _ctx(xyz, cells, alpha, q, rots, rx, ry, bounds) as ctx:
        merged = ctx.render_vertex_adjoint(g)
        ctx.set_option("vertex_merge", 0)
        plain = ctx.render_vertex_adjoint(g)
    assert np.abs(plain).max() > 0
    _assert_same_run(merged, plain)

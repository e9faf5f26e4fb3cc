"""Batched vertex adjoint render on the GPU (c5_render_vertex_adjoint_batch*) against the numpy restatement applied image
by image (tests/vertex_adjoint_reference.py; tests/test_vertex_adjoint_batch_cpu.py holds that yardstick to linearity and
duality), against the single call slice by slice, and against the library's own vertex tangent (its transpose).  The
scenes are tests/test_gpu_vertex_adjoint.py's at the smallest sizes that still have more than one 8 x 8 tile each way;
every test opens its own contexts.

Bars, tests/test_gpu_vertex_adjoint.py's.  Against the restatement: per component column 1e-6 x max |ref|, and per
component 1e-9 scale_raw + dz_err sens_raw + 2^-970.  Against the single call (and run to run, device against host,
"vertex_merge" 0): rtol 1e-12, atol 1e-15 x max - every contribution of a slice is the double the single call adds, in
another order.  Row splits: the same with parts = 2.  Duality with the vertex tangent: 2^-22 x sum_p |g_p| |out_p|."""
import ctypes as C
import functools
import types

import numpy as np
import pytest

from course5_amd import capi
from course5_amd import meshgen as mg
from tests import adjoint_reference as ar, derivative_fuzz as fz, motion_reference as mr, vertex_adjoint_reference as vr
from tests.test_gpu_motion import B, ROTS, SMALL_BOUNDS, SMALL_ROTS, _ctx

pytestmark = pytest.mark.gpu
KS = (1, 2, 3, 4, 5, 8, 9, 11)


def _scene(kind):
    if kind == "kuhn3":  # three by two tiles, exactly
        xyz, cells = mg.kuhn_box(3, jitter=0.2)
        return xyz, cells, SMALL_ROTS, 24, 16, SMALL_BOUNDS
    if kind == "kuhn3_off_tile":  # a column and three rows into the last tiles
        xyz, cells = mg.kuhn_box(3, jitter=0.2)
        return xyz, cells, SMALL_ROTS, 25, 19, SMALL_BOUNDS
    if kind == "ball":
        xyz, cells = mg.ball(12)
        return xyz, cells, ROTS, 50, 37, B
    xyz, cells, _ = mg.refined_interface(3, 2, 3, jitter=0.1, warp=0.08)
    return xyz, cells, ROTS, 60, 45, B


def _images(k, ry, rx, seed, at=None):
    """k upstream images: random fp32; number 1 tau-only, 2 I-only, 3 all zero, 4 non-zero at one pixel (`at`, default the
    middle one: most lanes of its wavefront take part with nothing to add) - as far as k goes."""
    g = np.random.default_rng(seed).normal(size=(k, ry, rx, 2)).astype(np.float32)
    if k > 1:
        g[1, ..., 1] = 0.0
    if k > 2:
        g[2, ..., 0] = 0.0
    if k > 3:
        g[3] = 0.0
    if k > 4:
        at = at or (ry // 2, rx // 2)
        one = g[4][at].copy()
        g[4] = 0.0
        g[4][at] = one
    return g


def _dz_err(xyz, rots):
    return fz.dz_err(types.SimpleNamespace(xyz=xyz, rots=rots))


def _assert_close(got, full, dz_err, what, onto=None):
    """full: gradients_of's dict; onto: the representatives its rows are summed on (a soup), bounds included."""
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
    tol = 1e-9 * scale + dz_err * sens + 2.0 ** -970
    r = np.abs(got - ref) / tol
    print(f"{what}: worst error / element bar {r.max():.3g}")
    assert (r <= 1.0).all(), f"{what}: {int((r > 1).sum())} components over their bar, worst {r.max():.3g} at {np.unravel_index(r.argmax(), r.shape)}"


def _assert_same_run(a, b, parts=1):
    np.testing.assert_allclose(a, b, rtol=parts * 1e-12, atol=parts * 1e-15 * np.abs(b).max())


def _assert_slices(batch, images, xyz, cells, m, geo, rots, what, onto=None, skip=None, singles=None):
    """Every slice against the restatement (where that is all zero - an image of zeros, one pixel that no ray of the grid
    starts from - exactly 0.0) and, where given, against the single call."""
    assert batch.shape == (len(images), len(xyz), 3)
    dz_err = _dz_err(xyz, rots)
    assert images[0].any()
    for k, g in enumerate(images):
        ref = vr.gradients_of(m, geo, cells, len(xyz), rots, g, skip)
        assert ref["raw"].any() or k > 2
        if not ref["raw"].any():
            assert not batch[k].any(), f"{what} image {k}: nothing to differentiate must give exact zeros"
        else:
            _assert_close(batch[k], ref, dz_err, f"{what} image {k}", onto)
        if singles is not None:
            _assert_same_run(batch[k], singles[k])


@functools.lru_cache(maxsize=None)
def _matrices(kind, seed):
    """The scene, its scalars and the restatement's matrices, built once and shared (never written to)."""
    xyz, cells, rots, rx, ry, bounds = _scene(kind)
    alpha, q = mr.scalars(len(cells), seed)
    m = ar.ray_matrices(xyz, cells, alpha, q, rots, rx, ry, bounds)
    geo = vr.segment_faces(xyz, cells, rots, rx, ry, bounds)
    return xyz, cells, rots, rx, ry, bounds, alpha, q, m, geo


def _interpenetrating_boxes():
    xa, ca = mg.kuhn_box(3, lo=(0.6, -0.4, -0.3), size=0.6, jitter=0.1, seed=5)
    xb, cb = mg.kuhn_box(4, lo=(0.85, -0.2, -0.45), size=0.7, jitter=0.1, seed=6)
    return np.vstack([xa, xb]), np.vstack([ca, cb + len(xa)]).astype(np.int32)


@pytest.mark.parametrize("kind", ["kuhn3", "kuhn3_off_tile", "ball", "hanging_nodes"])
def test_walk_against_the_restatement_and_the_single_call(kind):
    xyz, cells, rots, rx, ry, bounds, alpha, q, m, geo = _matrices(kind, 3)
    covered = np.argwhere(m["valid"].any(1).reshape(ry, rx))
    at = tuple(covered[np.abs(covered - (ry // 2, rx // 2)).sum(1).argmin()])  # the covered pixel nearest the middle
    images = _images(5, ry, rx, 71, at)
    with _ctx(xyz, cells, alpha, q, rots, rx, ry, bounds, (("cell_order", 0),)) as ctx:
        got = ctx.render_vertex_adjoint_batch(images)
        again = ctx.render_vertex_adjoint_batch(images)
        singles = [ctx.render_vertex_adjoint(g) for g in images]
    _assert_same_run(again, got)
    assert np.abs(got[4]).max() > 0  # (the one pixel is covered)
    _assert_slices(got, images, xyz, cells, m, geo, rots, kind, singles=singles)


@pytest.mark.parametrize("width", [0, 4, 8])
def test_every_batch_size_and_width_against_the_single_call(width):
    """K = 5, 9 and 11 run as chunks of 4 + 1, 8 + 1 and 8 + 3 (4 + 4 + 1, 4 + 4 + 3 at width 4); K = 3 at width 8 leaves five
    columns of the kernel unused; K = 1 IS the single call."""
    xyz, cells, rots, rx, ry, bounds, alpha, q, m, geo = _matrices("kuhn3_off_tile", 8)
    images = _images(max(KS), ry, rx, 72)
    with _ctx(xyz, cells, alpha, q, rots, rx, ry, bounds) as ctx:
        singles = np.stack([ctx.render_vertex_adjoint(g) for g in images])
        assert np.abs(singles[0]).max() > 0 and not singles[3].any()
        ctx.set_option("batch_width", width)
        for k in KS:
            got = ctx.render_vertex_adjoint_batch(images[:k])
            assert got.shape == (k, len(xyz), 3)
            for j in range(k):
                _assert_same_run(got[j], singles[j])
            if k > 3:
                assert not got[3].any()  # exactly 0
        one = ctx.render_vertex_adjoint_batch(images[0])  # one image without the batch axis
        assert one.shape == (1, len(xyz), 3)
        _assert_same_run(one[0], singles[0])


@pytest.mark.parametrize("kind", ["kuhn3_off_tile", "hanging_nodes"])
def test_duality_with_the_vertex_tangent(kind):
    xyz, cells, rots, rx, ry, bounds, alpha, q, _m, _geo = _matrices(kind, 8)
    images = _images(5, ry, rx, 73)
    fields = np.random.default_rng(74).normal(size=(4, len(xyz), 3))
    with _ctx(xyz, cells, alpha, q, rots, rx, ry, bounds) as ctx:
        grads = ctx.render_vertex_adjoint_batch(images)
        outs = ctx.render_vertex_tangent(fields).astype(np.float64)
    for k, (g, grad) in enumerate(zip(images.astype(np.float64), grads)):
        for j, (d, o) in enumerate(zip(fields, outs)):
            lhs, rhs = float((g * o).sum()), float((grad * d).sum())
            bar = 2.0 ** -22 * float((np.abs(g) * np.abs(o)).sum())
            print(f"{kind} image {k} field {j}: <g, out> = {lhs:.9g}, <grad_xyz, d> = {rhs:.9g}, |difference| = {abs(lhs - rhs):.3g}, bar {bar:.3g}")
            assert abs(lhs - rhs) <= bar, (k, j, lhs, rhs, bar)
            assert abs(rhs) > 0 or k > 2
            assert g.any() or (lhs == 0.0 and rhs == 0.0)


def test_soup_on_the_bin_sort_lists_lands_on_the_representatives():
    xyz, cells = mg.kuhn_box(3, jitter=0.2)
    soup_xyz, soup_cells = mg.per_cell_point_copies(xyz, cells)
    rx, ry = 25, 19
    alpha, q = mr.scalars(len(cells), 4)
    images = _images(5, ry, rx, 75)
    with _ctx(soup_xyz, soup_cells, alpha, q, SMALL_ROTS, rx, ry, SMALL_BOUNDS, (("algorithm", 1),)) as ctx:
        got = ctx.render_vertex_adjoint_batch(images)
        singles = [ctx.render_vertex_adjoint(g) for g in images]
    rep, merged = capi.weld_points(soup_xyz)
    others = rep != np.arange(len(rep))
    assert others.sum() == merged > 0 and not got[:, others].any()  # exactly 0 in every slice
    m = ar.ray_matrices(soup_xyz, soup_cells, alpha, q, SMALL_ROTS, rx, ry, SMALL_BOUNDS)
    geo = vr.segment_faces(soup_xyz, soup_cells, SMALL_ROTS, rx, ry, SMALL_BOUNDS)
    _assert_slices(got, images, soup_xyz, soup_cells, m, geo, SMALL_ROTS, "soup, algorithm 1", onto=rep, singles=singles)


def test_interpenetrating_boxes_across_the_retry():
    xyz, cells = _interpenetrating_boxes()
    rx, ry = 80, 60  # (tests/test_gpu_vertex_adjoint.py's frame: the one known to overflow the first entry pool)
    alpha, q = mr.scalars(len(cells), 5)
    images = _images(5, ry, rx, 76)
    with _ctx(xyz, cells, alpha, q, ROTS, rx, ry) as ctx:
        got = ctx.render_vertex_adjoint_batch(images)  # the first walk finds the overlap (C5_RETRY, settled inside the call)
        singles = [ctx.render_vertex_adjoint(g) for g in images]
        _assert_same_run(ctx.render_vertex_adjoint_batch(images), got)
    m = ar.ray_matrices(xyz, cells, alpha, q, ROTS, rx, ry, B)
    geo = vr.segment_faces(xyz, cells, ROTS, rx, ry, B)
    _assert_slices(got, images, xyz, cells, m, geo, ROTS, "overlapping boxes", singles=singles)


def test_solid_pixels_contribute_nothing():
    xyz, cells = mg.kuhn_box(5, jitter=0.1)
    rx, ry = 40, 30
    alpha, q = mr.scalars(len(cells), 6)
    images = _images(3, ry, rx, 77)
    sx, sc = mg.kuhn_box(2, lo=(0.9, -0.15, 0.3), size=0.3)
    with _ctx(xyz, cells, alpha, q, ROTS, rx, ry) as ctx:
        ctx.set_solid(0, sx[sc].reshape(-1, 12))  # colour NaN: solid pixels are NaN in the image
        img = ctx.render()
        got = ctx.render_vertex_adjoint_batch(images)
        singles = [ctx.render_vertex_adjoint(g) for g in images]
    skip = np.isnan(img[..., 0])
    assert 5 < skip.sum() < skip.size // 2
    m = ar.ray_matrices(xyz, cells, alpha, q, ROTS, rx, ry, B)
    geo = vr.segment_faces(xyz, cells, ROTS, rx, ry, B)
    _assert_slices(got, images, xyz, cells, m, geo, ROTS, "solid", skip=skip, singles=singles)


def test_morton_ordered_cells():
    xyz, cells = mg.kuhn_box(9, jitter=0.1)  # 4 374 cells: kept in Morton order on the device ("cell_order" 1)
    assert len(cells) >= 4096
    rx, ry = 33, 26
    alpha, q = mr.scalars(len(cells), 7)
    images = _images(5, ry, rx, 78)
    with _ctx(xyz, cells, alpha, q, ROTS, rx, ry, options=(("cell_order", 1),)) as ctx:
        got = ctx.render_vertex_adjoint_batch(images)
        singles = [ctx.render_vertex_adjoint(g) for g in images]
    m = ar.ray_matrices(xyz, cells, alpha, q, ROTS, rx, ry, B)
    geo = vr.segment_faces(xyz, cells, ROTS, rx, ry, B)
    _assert_slices(got, images, xyz, cells, m, geo, ROTS, "cell_order 1", singles=singles)


def test_row_ranges_and_cyclic_row_tiles_sum_to_the_whole_frame():
    xyz, cells, rots, rx, ry, bounds, alpha, q, _m, _geo = _matrices("kuhn3_off_tile", 10)
    images = _images(5, ry, rx, 79)
    with _ctx(xyz, cells, alpha, q, rots, rx, ry, bounds) as ctx:
        whole = ctx.render_vertex_adjoint_batch(images)
    total = np.zeros_like(whole)
    for begin, count in ((0, 5), (5, ry - 5)):
        with _ctx(xyz, cells, alpha, q, rots, rx, ry, bounds) as ctx:
            ctx.set_row_range(begin, count)
            total += ctx.render_vertex_adjoint_batch(images[:, begin:begin + count])
    _assert_same_run(total, whole, parts=2)
    total = np.zeros_like(whole)
    for rank in range(2):
        with _ctx(xyz, cells, alpha, q, rots, rx, ry, bounds) as ctx:
            ctx.set_row_tiles(4, rank, 2)
            rows = np.array([r for r in range(ry) if (r // 4) % 2 == rank])
            total += ctx.render_vertex_adjoint_batch(images[:, rows])
    _assert_same_run(total, whole, parts=2)
    assert np.abs(whole[0]).max() > 0 and not whole[3].any()


def test_no_trace_left_and_the_device_form():
    import torch
    xyz, cells, rots, rx, ry, bounds, alpha, q, m, geo = _matrices("kuhn3_off_tile", 11)
    images = _images(9, ry, rx, 80)
    with _ctx(xyz, cells, alpha, q, rots, rx, ry, bounds) as a, _ctx(xyz, cells, alpha, q, rots, rx, ry, bounds) as b:
        for _ in range(3):  # (three frames: the view cache is in use by the third)
            a.render(), b.render()
        before = a.stats()
        got = a.render_vertex_adjoint_batch(images)
        assert a.stats() == before
        # a single call after the batch passes its own bar: the heads were handed back clean
        single = a.render_vertex_adjoint(images[0])
        _assert_close(single, vr.gradients_of(m, geo, cells, len(xyz), rots, images[0]), _dz_err(xyz, rots), "single after a batch")
        _assert_same_run(got[0], single)
        g_dev = torch.tensor(images, device="cuda")
        out_dev = torch.full((len(images), len(xyz), 3), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        a.render_vertex_adjoint_batch_device(g_dev, out_dev)
        assert a.synchronize() == capi.C5_OK
        _assert_same_run(out_dev.cpu().numpy(), got)
        assert not out_dev[3].any().item()  # exactly 0, the NaN overwritten
        for _ in range(3):
            ia, ib = a.render(), b.render()
            assert np.array_equal(ia.view(np.uint32), ib.view(np.uint32))
        assert a.stats()["segments"] == b.stats()["segments"]


def test_bad_arguments_and_outstanding_async_frames_are_refused():
    xyz, cells, rots, rx, ry, bounds, alpha, q, _m, _geo = _matrices("kuhn3", 12)
    images = _images(2, ry, rx, 81)
    out = np.zeros((2, len(xyz), 3))
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    with _ctx(xyz, cells, alpha, q, rots, rx, ry, bounds) as ctx:
        lib, h = ctx.lib, ctx.handle
        gp, op = images.ctypes.data_as(fp), out.ctypes.data_as(dp)
        assert lib.c5_render_vertex_adjoint_batch(h, 0, gp, op) == capi.C5_ERR_INVALID
        assert lib.c5_render_vertex_adjoint_batch(h, -1, gp, op) == capi.C5_ERR_INVALID
        assert lib.c5_render_vertex_adjoint_batch(h, 2, None, op) == capi.C5_ERR_INVALID
        assert lib.c5_render_vertex_adjoint_batch(h, 2, gp, None) == capi.C5_ERR_INVALID
        assert lib.c5_render_vertex_adjoint_batch_device(h, 2, None, None) == capi.C5_ERR_INVALID
        assert lib.c5_render_vertex_adjoint_batch_device(h, 0, 1, 1) == capi.C5_ERR_INVALID
        assert lib.c5_render_vertex_adjoint_batch(None, 2, gp, op) == capi.C5_ERR_INVALID
        with pytest.raises(ValueError):
            ctx.render_vertex_adjoint_batch(images[:, 1:])
        buf = ctx.host_image()
        ctx.render_host_async(buf)
        with pytest.raises(capi.C5Error) as e:
            ctx.render_vertex_adjoint_batch(images)
        assert e.value.code == capi.C5_ERR_STATE
        assert ctx.render_host_wait() == capi.C5_OK
        ctx.free_host_image(buf)
        assert np.abs(ctx.render_vertex_adjoint_batch(images)).max() > 0


def test_vertex_merge_off_changes_nothing_about_the_batch():
    """The batch always merges: "vertex_merge" 0 is the single call's option."""
    xyz, cells, rots, rx, ry, bounds, alpha, q, _m, _geo = _matrices("kuhn3_off_tile", 15)
    images = _images(5, ry, rx, 82)
    with _ctx(xyz, cells, alpha, q, rots, rx, ry, bounds) as ctx:
        merged = ctx.render_vertex_adjoint_batch(images)
        ctx.set_option("vertex_merge", 0)
        plain = ctx.render_vertex_adjoint_batch(images)
    assert np.abs(plain).max() > 0
    _assert_same_run(merged, plain)

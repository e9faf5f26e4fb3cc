"""Motion tangent render on the GPU (c5_render_motion_tangent*, capi.Context.render_view_tangent) against the numpy
restatement (tests/motion_reference.py), exact identities and central differences of two real renders.

Two bars against the restatement: 1e-6 x max |ref| per channel and field (the project's tangent bar), and per
element 2^-23 |ref| + 1e-9 scale + dz_err sens + 2^-103 (tests/derivative_fuzz.py's bar with the motion's own scale and
chord sensitivity, calibrated in tests/test_motion_cpu.py).  Every test opens its own contexts."""
import types

import numpy as np
import pytest

from course5_amd import capi
from course5_amd import meshgen as mg
from tests import adjoint_reference as ar, derivative_fuzz as fz, motion_reference as mr

pytestmark = pytest.mark.gpu
B = mg.REFERENCE_BOUNDS
SMALL_BOUNDS = (1.9, 0.1, 0.9, -0.9)
SMALL_ROTS = np.array([[0.0, 0.31, 0.0], [1.0, 0.22, 1.0]])
ROTS = mg.view_rotations(0.13, 0.21)


def _fields(rots, seed, extra=2):
    """Every angle of the view, `extra` random affine fields, the z-scale and a z-translation."""
    rng = np.random.default_rng(seed)
    f = [capi.rotation_motion(rots, i) for i in range(len(rots))] + [rng.normal(size=12) for _ in range(extra)]
    return np.array(f + [mr.Z_SCALE, mr.Z_TRANSLATION])


def _ctx(xyz, cells, alpha, q, rots, rx, ry, bounds=B, options=()):
    ctx = capi.Context(0)
    for k, v in options:
        ctx.set_option(k, v)
    ctx.upload_grid(xyz, cells, alpha, q)
    ctx.set_image(rx, ry, bounds)
    ctx.set_view(rots)
    return ctx


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_close(got, xyz, cells, alpha, q, rots, rx, ry, bounds, fields, what, rows=None, skip=None):
    dz_err = fz.dz_err(types.SimpleNamespace(xyz=xyz, rots=rots))
    refs = mr.image_motion(xyz, cells, alpha, q, rots, rx, ry, bounds, fields, rows=rows, skip=skip, with_scale=True)
    assert got.shape == (len(fields),) + refs[0][0].shape + (2,)
    moving = 0
    for j, (tau_dot, I_dot, ex) in enumerate(refs):
        for ch, name, ref in ((0, "tau_dot", tau_dot), (1, "I_dot", I_dot)):
            g = got[j, ..., ch].astype(np.float64)
            err = np.abs(g - ref)
            top = np.abs(ref).max()
            key = "tau" if ch == 0 else "I"
            tol = 2.0 ** -23 * np.abs(ref) + 1e-9 * ex["scale_" + key] + dz_err * ex["sens_" + key] + 2.0 ** -103
            print(f"{what} field {j} {name}: max error {err.max():.3g} of max {top:.3g}, worst error / element bar {(err / tol).max():.3g}")
            assert np.isfinite(g).all()
            assert err.max() <= 1e-6 * top, f"{what} field {j} {name}: max abs error {err.max():.3g} vs max {top:.3g}"
            assert (err <= tol).all(), f"{what} field {j} {name}: {int((err > tol).sum())} elements over their bar, worst {(err / tol).max():.3g}"
            moving += top > 0
    assert moving >= 2 * (len(fields) - 1)  # (only the z-translation is all zeros)


def _scene(kind):
    if kind == "kuhn3":
        xyz, cells = mg.kuhn_box(3, jitter=0.2)
        return xyz, cells, SMALL_ROTS, 48, 36, SMALL_BOUNDS
    if kind == "kuhn3_off_tile":
        xyz, cells = mg.kuhn_box(3, jitter=0.2)
        return xyz, cells, SMALL_ROTS, 50, 37, SMALL_BOUNDS
    if kind == "ball":
        xyz, cells = mg.ball(12)
        return xyz, cells, ROTS, 150, 112, B
    xyz, cells, _ = mg.refined_interface(3, 2, 3, jitter=0.1, warp=0.08)
    return xyz, cells, ROTS, 120, 90, B


@pytest.mark.parametrize("kind", ["kuhn3", "kuhn3_off_tile", "ball", "hanging_nodes"])
def test_walk_against_the_restatement(kind):
    xyz, cells, rots, rx, ry, bounds = _scene(kind)
    alpha, q = mr.scalars(len(cells), 3)
    fields = _fields(rots, 21)
    with _ctx(xyz, cells, alpha, q, rots, rx, ry, bounds, (("cell_order", 0),)) as ctx:
        got = ctx.render_motion_tangent(fields)
        again = ctx.render_motion_tangent(fields)
        entries = None
        if kind == "ball":
            ctx.render()
            st = ctx.stats()
            entries = st["entries"], st["covered_pixels"]
    assert np.array_equal(_bits(got), _bits(again))  # two calls: equal bits
    assert not got[-1].any()  # a z-translation moves no chord: exactly 0
    if entries:
        assert entries[0] > entries[1]  # (re-entries: more boundary entries than covered pixels)
    _assert_close(got, xyz, cells, alpha, q, rots, rx, ry, bounds, fields, kind)


def test_soup_on_the_fallback_and_interpenetrating_boxes():
    xyz, cells = mg.kuhn_box(4, jitter=0.1)
    soup_xyz, soup_cells = mg.per_cell_point_copies(xyz, cells)
    alpha, q = mr.scalars(len(cells), 4)
    fields = _fields(ROTS, 22, extra=1)
    with _ctx(soup_xyz, soup_cells, alpha, q, ROTS, 80, 60, options=(("algorithm", 1),)) as ctx:
        got = ctx.render_motion_tangent(fields)
        assert np.array_equal(_bits(got), _bits(ctx.render_motion_tangent(fields)))
        assert np.array_equal(_bits(got[1]), _bits(ctx.render_motion_tangent(fields[1])))
    assert not got[-1].any()
    _assert_close(got, soup_xyz, soup_cells, alpha, q, ROTS, 80, 60, B, fields, "soup, algorithm 1")
    # two interpenetrating boxes: the first walk finds them (C5_RETRY, settled inside the call)
    xa, ca = mg.kuhn_box(3, lo=(0.6, -0.4, -0.3), size=0.6, jitter=0.1, seed=5)
    xb, cb = mg.kuhn_box(4, lo=(0.85, -0.2, -0.45), size=0.7, jitter=0.1, seed=6)
    xyz2, cells2 = np.vstack([xa, xb]), np.vstack([ca, cb + len(xa)]).astype(np.int32)
    alpha, q = mr.scalars(len(cells2), 5)
    with _ctx(xyz2, cells2, alpha, q, ROTS, 80, 60) as ctx:
        got = ctx.render_motion_tangent(fields)
    _assert_close(got, xyz2, cells2, alpha, q, ROTS, 80, 60, B, fields, "overlapping boxes")


def test_solid_pixels_are_zero():
    xyz, cells = mg.kuhn_box(5, jitter=0.1)
    rx, ry = 80, 60
    alpha, q = mr.scalars(len(cells), 6)
    fields = _fields(ROTS, 23, extra=1)
    sx, sc = mg.kuhn_box(2, lo=(0.9, -0.15, 0.3), size=0.3)
    with _ctx(xyz, cells, alpha, q, ROTS, rx, ry) as ctx:
        ctx.set_solid(0, sx[sc].reshape(-1, 12))  # colour NaN: solid pixels are NaN in the image
        img = ctx.render()
        got = ctx.render_motion_tangent(fields)
    skip = np.isnan(img[..., 0])
    assert 20 < skip.sum() < skip.size // 2
    assert not got[:, skip].any()
    _assert_close(got, xyz, cells, alpha, q, ROTS, rx, ry, B, fields, "solid", skip=skip)


def test_row_ranges_and_cyclic_row_tiles():
    xyz, cells = mg.kuhn_box(5, jitter=0.1)
    rx, ry = 80, 60
    alpha, q = mr.scalars(len(cells), 7)
    fields = _fields(ROTS, 24, extra=1)
    parts = []
    for begin, count in ((0, 23), (23, ry - 23)):
        with _ctx(xyz, cells, alpha, q, ROTS, rx, ry) as ctx:
            ctx.set_row_range(begin, count)
            parts.append(ctx.render_motion_tangent(fields))
            assert parts[-1].shape == (len(fields), count, rx, 2)
    _assert_close(np.concatenate(parts, axis=1), xyz, cells, alpha, q, ROTS, rx, ry, B, fields, "two row ranges")
    for rank in range(2):
        with _ctx(xyz, cells, alpha, q, ROTS, rx, ry) as ctx:
            ctx.set_row_tiles(3, rank, 2)
            got = ctx.render_motion_tangent(fields)
        rows = np.array([r for r in range(ry) if (r // 3) % 2 == rank])
        _assert_close(got, xyz, cells, alpha, q, ROTS, rx, ry, B, fields, f"row tiles, rank {rank}", rows=rows)


def test_batches_are_bit_equal_to_single_calls_at_both_widths():
    xyz, cells, rots, rx, ry, bounds = _scene("kuhn3_off_tile")
    alpha, q = mr.scalars(len(cells), 8)
    fields = np.vstack([_fields(rots, 25, extra=6), np.random.default_rng(9).normal(size=(1, 12))])
    assert len(fields) == 11
    with _ctx(xyz, cells, alpha, q, rots, rx, ry, bounds) as ctx:
        singles = np.stack([ctx.render_motion_tangent(f) for f in fields])
        assert np.abs(singles[0]).max() > 0
        for width in (4, 8):
            ctx.set_option("batch_width", width)
            for k in (1, 3, 8, 11):
                got = ctx.render_motion_tangent(fields[:k])
                assert np.array_equal(_bits(got), _bits(singles[:k])), (width, k)


def test_z_scale_is_the_tangent_along_the_scalars_themselves():
    """u = (0, 0, z) stretches every chord at its own rate, which is alpha -> (1 + t) alpha, Q -> (1 + t) Q where no alpha
    is clamped: I_dot = render_tangent(alpha, q)'s, tau_dot = tau (DESIGN 4.5's identities and their bar)."""
    xyz, cells = mg.kuhn_box(5, jitter=0.1)
    a, q = mr.scalars(len(cells), 9)
    alpha = 0.6 * a
    with _ctx(xyz, cells, alpha, q, ROTS, 160, 120) as ctx:
        got = ctx.render_motion_tangent(mr.Z_SCALE).astype(np.float64)
        want_I = ctx.render_tangent(alpha, q)[..., 1].astype(np.float64)
        want_tau = ctx.render()[..., 0].astype(np.float64)
    assert np.abs(want_I).max() > 0 and np.abs(want_tau).max() > 0
    for g, w, name in ((got[..., 1], want_I, "I"), (got[..., 0], want_tau, "tau")):
        bad = np.abs(g - w) > 1e-5 * np.abs(w) + 1e-6 * np.abs(w).max()
        assert not bad.any(), f"{name}: {int(bad.sum())} pixels"


@pytest.mark.parametrize("opts", [(), (("depth_split", 2),), (("integration", 1),)], ids=["default", "split", "ftb"])
def test_render_after_a_motion_tangent_is_bit_identical(opts):
    xyz, cells = mg.kuhn_box(5, jitter=0.1)
    alpha, q = mr.scalars(len(cells), 10)
    fields = _fields(ROTS, 26)
    with _ctx(xyz, cells, alpha, q, ROTS, 160, 120, options=opts) as a, _ctx(xyz, cells, alpha, q, ROTS, 160, 120, options=opts) as b:
        for _ in range(3):  # (three frames: the view cache is in use by the third)
            a.render(), b.render()
        before = a.stats()
        first = a.render_motion_tangent(fields)
        assert a.stats() == before
        assert a.synchronize() == capi.C5_OK
        for _ in range(3):
            ia, ib = a.render(), b.render()
            assert np.array_equal(ia.view(np.uint32), ib.view(np.uint32))
        assert a.stats()["segments"] == b.stats()["segments"]
        # the same walk whatever the walk options say: the same bits as a context that never rendered
        assert np.array_equal(_bits(first), _bits(b.render_motion_tangent(fields)))
    with _ctx(xyz, cells, alpha, q, ROTS, 160, 120) as c:
        assert np.array_equal(_bits(first), _bits(c.render_motion_tangent(fields)))


def test_async_frames_outstanding_are_refused_and_bad_arguments():
    xyz, cells, rots, rx, ry, bounds = _scene("kuhn3")
    alpha, q = mr.scalars(len(cells), 11)
    with _ctx(xyz, cells, alpha, q, rots, rx, ry, bounds) as ctx:
        buf = ctx.host_image()
        ctx.render_host_async(buf)
        with pytest.raises(capi.C5Error) as e:
            ctx.render_motion_tangent(mr.Z_SCALE)
        assert e.value.code == capi.C5_ERR_STATE
        assert ctx.render_host_wait() == capi.C5_OK
        ctx.free_host_image(buf)
        with pytest.raises(ValueError):
            ctx.render_motion_tangent(np.zeros(11))
        assert ctx.render_view_tangent().shape == (2, ry, rx, 2)


@pytest.mark.parametrize("index", [0, 1])
def test_view_tangent_against_central_differences_of_two_renders(index):
    xyz, cells, rots, rx, ry, bounds = _scene("kuhn3")
    a, q = mr.scalars(len(cells), 7)
    alpha = 0.6 * a
    h = 1e-3
    lists = []
    for s in (-1, 0, 1):
        r = rots.copy()
        r[index, 1] += s * h
        lists.append(ar.ray_matrices(xyz, cells, alpha, q, r, rx, ry, bounds)["C"])
    width = max(c.shape[1] for c in lists)
    pad = [np.pad(c, ((0, 0), (0, width - c.shape[1])), constant_values=-1) for c in lists]
    same = ((pad[0] == pad[1]).all(1) & (pad[2] == pad[1]).all(1)).reshape(ry, rx)
    covered = (pad[1] >= 0).any(1).reshape(ry, rx)
    excluded = 1.0 - same[covered].mean()
    with _ctx(xyz, cells, alpha, q, rots, rx, ry, bounds) as ctx:
        tan = ctx.render_view_tangent()[index].astype(np.float64)
        imgs = []
        for s in (1, -1):
            r = rots.copy()
            r[index, 1] += s * h
            ctx.set_view(r)
            imgs.append(ctx.render().astype(np.float64))
    fd = (imgs[0] - imgs[1]) / (2 * h)
    print(f"angle {index}: {excluded:.2%} of the covered pixels changed their cell list")
    assert excluded <= 0.05
    use = same & covered
    for ch, name in ((0, "tau"), (1, "I")):
        err = np.abs(fd[..., ch] - tan[..., ch])[use].max()
        top = np.abs(tan[..., ch]).max()
        print(f"angle {index} {name}: max error {err:.3g} of max {top:.3g}")
        assert top > 0 and err <= 2e-2 * top

"""Ray shape Jacobian on the GPU (c5_ray_shape_jacobian_fill*, c5_face_gradients*; capi.Context.ray_shape_jacobian,
autograd.ray_shape_jacobian, fit.ExplicitShapeJacobian, fit.shape_step_preconditioned).

  per element   every dI_ddz and every barycentric coordinate against the numpy restatement on the bars
                tests/shape_jacobian_reference.py derives (1e-9 scale + dz_err sens + 2^-970); faces exactly, but for the
                sides the restatement marks as ties (at most 1 % of them: tests/test_shape_jacobian_cpu.py holds the
                restatement itself under that cap);
  rows          a row of the assembled J_I / J_tau against c5_render_vertex_adjoint of the one-hot image at that pixel, on the
                vertex adjoint's run-to-run bar (rtol 1e-12, atol 1e-15 x max: tests/test_gpu_vertex_adjoint.py);
  product       J d against c5_render_vertex_tangent's fp32 image, 2^-22 sum |J| |d| per pixel (the duality bar);
  bit identities, the guard, and the fit's operators and preconditioner.

The fit's operators against the library's: per component column 1e-6 x max |ref|, the project's adjoint bar
(tests/test_gpu_adjoint.py) - the library's product rounds J p to float32 on the way, the explicit one does not.  The
diagonal against unit-vector products: diag_i = sum_p w J_pi^2 has positive terms only and the library rounds every J_pi to
float32 (2^-24) and multiplies by w in float32 (2^-24): 2^-22 diag_i with the fp64 sides' factor 2.

Scenes: tests/shape_jacobian_reference.py's, at most 28 x 21 pixels.  Every reference is computed once and shared."""
import ctypes as C
import functools
import types

import numpy as np
import pytest

from course5_amd import capi
from course5_amd import meshgen as mg
from course5_amd import sharding
from tests import derivative_fuzz as fz, motion_reference as mr, shape_jacobian_reference as sj

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b):
    return all(x.shape == y.shape and np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def _scene(kind):
    s = types.SimpleNamespace(kind=kind, **sj.scene(kind))
    s.alpha, s.q = mr.scalars(len(s.cells), 3)
    s.dz_err = fz.dz_err(types.SimpleNamespace(xyz=s.xyz, rots=s.rots))
    return s


def _ctx(s, options=None):
    ctx = capi.Context(0)
    for k, v in (s.options if options is None else options):
        ctx.set_option(k, v)
    ctx.upload_grid(s.xyz, s.cells, s.alpha, s.q)
    ctx.set_image(s.rx, s.ry, s.bounds)
    ctx.set_view(s.rots)
    if s.solid is not None:
        ctx.set_solid(0, s.solid)  # colour NaN: solid pixels are NaN in the image
    return ctx


@functools.lru_cache(maxsize=None)
def _exported(kind, options=None):
    """(row_ptr, col, dz, dI_ddz, faces, bary, face_points, dw_dxyz) of the scene, and the NaN mask of its render."""
    s = _scene(kind)
    with _ctx(s, options) as ctx:
        skip = np.isnan(ctx.render()[..., 0])
        return ctx.ray_shape_jacobian(), skip


@functools.lru_cache(maxsize=None)
def _reference(kind):
    s = _scene(kind)
    skip = _exported(kind)[1] if s.solid is not None else None
    return sj.shape_arrays(s.xyz, s.cells, s.alpha, s.q, s.rots, s.rx, s.ry, s.bounds, s.dz_err, skip=skip)


def _dense(ctx, s):
    """(J_tau, J_I) [n_px, 3 n_pts] on the host from autograd.ray_shape_jacobian."""
    import torch
    from course5_amd import autograd
    J_tau, J_I = autograd.ray_shape_jacobian(ctx, torch.tensor(s.alpha), torch.tensor(s.q))
    assert J_tau.layout == torch.sparse_csr and J_tau.is_cuda and tuple(J_I.shape) == (ctx.local_rows * s.rx, 3 * len(s.xyz))
    return J_tau.to_dense().cpu().numpy(), J_I.to_dense().cpu().numpy()


# ---- 1. per element ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", sj.SCENES)
def test_every_element_against_the_restatement(kind):
    s = _scene(kind)
    (row_ptr, col, dz, dI, faces, bary, fpts, dw), _skip = _exported(kind)
    ref = _reference(kind)
    n_px = s.rx * s.ry
    assert row_ptr.shape == (n_px + 1,) and len(col) == len(dI) == len(faces) == len(bary) == row_ptr[-1] == len(ref["col"]) > 200
    pix = np.repeat(np.arange(n_px), np.diff(row_ptr))
    og, orf = np.lexsort((col, pix)), np.lexsort((ref["col"], ref["pixel"]))
    assert np.array_equal(pix[og], ref["pixel"][orf]) and np.array_equal(col[og], ref["col"][orf])
    r = fz.ratio(dI[og], ref["dI_ddz"][orf], ref["scale_dI"][orf], ref["sens_dI"][orf], s.dz_err)
    print(f"{kind}: {len(col)} segments; dI_ddz worst error / bar {r.max():.3g}")
    assert (r <= 1.0).all(), f"{int((r > 1).sum())} of {len(r)} dI_ddz over their bar, worst {r.max():.3g}"
    idle = dI[og][~ref["active"][orf]]  # explicit zeros, +0.0 on the walk and on the lists alike
    assert len(idle) > 0 and (idle == 0).all() and not np.signbit(idle).any() and np.abs(dI).max() > 0
    # the faces: exact but for the restatement's ties; found everywhere on these scenes
    got_f = np.stack([faces[og] & 3, (faces[og] >> 2) & 3], 1)
    want_f = np.stack([ref["faces"][orf] & 3, (ref["faces"][orf] >> 2) & 3], 1)
    tie = ref["tie"][orf]
    assert ((faces >> 4) == 3).all() and tie.mean() <= sj.TIE_CAP
    assert np.array_equal(got_f[~tie], want_f[~tie]), f"{int((got_f != want_f)[~tie].sum())} faces differ off the ties"
    same = (got_f == want_f)[:, :, None] & np.ones(3, bool)
    rb = fz.ratio(bary[og], ref["bary"][orf], ref["scale_bary"][orf], ref["sens_bary"][orf], s.dz_err)
    print(f"{kind}: barycentrics worst error / bar {rb[same].max():.3g}; ties {tie.mean():.3%}")
    assert (rb[same] <= 1.0).all(), f"{int((rb[same] > 1).sum())} barycentrics over their bar, worst {rb[same].max():.3g}"
    # the faces' points and gradients
    assert np.array_equal(fpts, ref["face_points"] if kind != "soup" else capi.weld_points(s.xyz)[0][ref["face_points"]])
    ok = ~ref["edge_on"]
    assert not dw[~ok].any()
    assert np.allclose(dw[ok], ref["dw_dxyz"][ok], rtol=1e-9, atol=1e-12 * np.abs(ref["dw_dxyz"]).max())


def test_an_inactive_segment_stores_plus_zero_on_the_walk_and_on_the_lists():
    """Negative and zero raw alphas: inactive cells (a < DBL_EPSILON), explicit +0.0 on both paths, bit for bit."""
    for kind in ("kuhn3_off_tile", "soup"):
        s = types.SimpleNamespace(**vars(_scene(kind)))
        seen = np.unique(_exported(kind)[0][1])  # (the cells some ray crosses)
        idle = seen[:: max(1, len(seen) // 12)]
        assert len(idle) >= 10
        s.alpha = s.alpha.copy()
        s.alpha[idle] = -0.5
        s.alpha[idle[::3]] = 0.0
        with _ctx(s) as ctx:
            rp, col, dz, dI, faces, bary, _fp, _dw = ctx.ray_shape_jacobian()
        at = np.isin(col, idle)
        print(f"{kind}: {int(at.sum())} segments of {len(idle)} inactive cells")
        assert at.sum() >= len(idle) and not dI[at].view(np.uint64).any()  # +0.0: no sign bit, no NaN
        assert np.isfinite(dI).all() and np.abs(dI[~at]).max() > 0 and ((faces >> 4) == 3).all()


def test_faces_edge_on_to_the_rays_have_zero_gradients_and_the_rows_still_hold():
    s = _scene("edge_on")
    (row_ptr, col, dz, dI, faces, bary, fpts, dw), _skip = _exported("edge_on")
    want_fp, want_dw, edge_on = sj.face_gradients(s.xyz, s.cells, s.rots)
    assert edge_on.sum() == 96 and edge_on.size == 192 and row_ptr[-1] > 200
    assert np.array_equal(fpts, want_fp) and np.array_equal(~dw.any(axis=2), edge_on)  # exact zeros there, and only there
    assert np.allclose(dw[~edge_on], want_dw[~edge_on], rtol=1e-9, atol=1e-12)
    # no chord runs between edge-on faces: both faces of every segment are found, and neither is one of them
    assert ((faces >> 4) == 3).all() and not edge_on[col, faces & 3].any() and not edge_on[col, (faces >> 2) & 3].any()


# ---- 2. rows and products ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", sj.SCENES + ("edge_on",))
def test_rows_are_the_vertex_adjoint_of_one_hot_images_and_j_d_the_vertex_tangent(kind):
    s = _scene(kind)
    n_pts = len(s.xyz)
    with _ctx(s) as ctx:
        J_tau, J_I = _dense(ctx, s)
        rp = ctx.ray_matrix_rows()
        covered = np.nonzero(np.diff(rp) > 0)[0]
        worst = 0.0
        for p in covered[np.linspace(0, len(covered) - 1, 12).astype(int)]:
            for ch, J in ((0, J_tau), (1, J_I)):
                g = np.zeros((s.ry, s.rx, 2), np.float32)
                g.reshape(-1, 2)[p, ch] = 1.0
                want = ctx.render_vertex_adjoint(g)
                got = J[p].reshape(n_pts, 3)
                top = np.abs(want).max()
                assert top > 0
                worst = max(worst, float((np.abs(got - want) / (1e-12 * np.abs(want) + 1e-15 * top)).max()))
        d = np.random.default_rng(51).normal(size=(n_pts, 3))
        img = ctx.render_vertex_tangent(d).astype(np.float64).reshape(-1, 2)
    print(f"{kind}: rows against one-hot vertex adjoints, worst error / run-to-run bar {worst:.3g}")
    assert worst <= 1.0  # (np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-15 max |want|) for every row)
    for ch, J in ((0, J_tau), (1, J_I)):
        got, bar = J @ d.reshape(-1), 2.0 ** -22 * (np.abs(J) @ np.abs(d.reshape(-1)))
        err = np.abs(got - img[:, ch])
        print(f"{kind}: J d channel {ch}: worst error / bar {(err / np.where(bar > 0, bar, 1.0)).max():.3g}")
        assert np.abs(got).max() > 0 and (err <= bar).all()
    if kind == "soup":  # welded non-representatives: empty columns
        rep = capi.weld_points(s.xyz)[0]
        others = np.repeat(rep != np.arange(n_pts), 3)
        assert others.any() and not J_tau[:, others].any() and not J_I[:, others].any()
    if kind == "solid":
        skip = _exported(kind)[1].reshape(-1)
        assert 5 < skip.sum() and not J_I[skip].any() and not J_tau[skip].any()


# ---- 3. bit identities ---------------------------------------------------------------------------------------------------

def test_calls_repeat_forms_agree_and_options_change_nothing():
    import torch
    s = _scene("kuhn3_off_tile")
    whole, _ = _exported("kuhn3_off_tile")
    nnz = int(whole[0][-1])
    with _ctx(s) as ctx:
        assert _same(ctx.ray_shape_jacobian(), whole) and _same(ctx.ray_shape_jacobian(), whole)
        d_rp = torch.tensor(whole[0], device="cuda")
        d_dI = torch.full((nnz,), -7.0, dtype=torch.float64, device="cuda")
        d_f = torch.full((nnz,), 255, dtype=torch.uint8, device="cuda")
        d_b = torch.full((nnz, 2, 3), -7.0, dtype=torch.float64, device="cuda")
        d_fp = torch.full((len(s.cells), 4, 3), -7, dtype=torch.int32, device="cuda")
        d_dw = torch.full((len(s.cells), 4, 3), -7.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        ctx.ray_shape_jacobian_device(d_rp, d_dI, d_f, d_b)
        assert ctx.synchronize() == capi.C5_OK
        ctx.face_gradients_device(d_fp, d_dw)
        assert ctx.synchronize() == capi.C5_OK
        assert _same([t.cpu().numpy() for t in (d_dI, d_f, d_b, d_fp, d_dw)], whole[3:])
        # any one array alone
        only = torch.full((nnz,), -7.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        ctx.ray_shape_jacobian_device(d_rp, only, None, None)
        assert ctx.synchronize() == capi.C5_OK and _same([only.cpu().numpy()], [whole[3]])
    for options in ((("lds_stage", 0),), (("integration", 1),), (("depth_split", 2),), (("adjoint_exact", 1),), (("exact_sums", 1),),
                    (("vertex_exact", 1),), (("vertex_merge", 0),)):
        assert _same(_exported("kuhn3_off_tile", s.options + options)[0], whole), options


def test_both_cell_orders_agree():
    a, b = _exported("morton")[0], _exported("morton", (("cell_order", 0),))[0]
    assert a[0][-1] > 2000 and _same(a, b)


def _rows_held(part, whole, px):
    lengths = np.diff(whole[0])[px]
    if not np.array_equal(np.diff(part[0]), lengths):
        return False
    at = np.repeat(whole[0][px] - part[0][:-1], lengths) + np.arange(part[0][-1])
    return _same(part[1:6], [w[at] for w in whole[1:6]]) and _same(part[6:], whole[6:])


def test_row_ranges_and_row_tiles_are_rows_of_the_whole_frame():
    s = _scene("kuhn3_off_tile")
    whole, _ = _exported("kuhn3_off_tile")
    seen = 0
    with _ctx(s) as ctx:
        for begin, count in ((0, 13), (13, 8)):  # (cut off the 8-row tile)
            ctx.set_row_range(begin, count)
            part = ctx.ray_shape_jacobian()
            px = (np.arange(begin, begin + count)[:, None] * s.rx + np.arange(s.rx)).reshape(-1)
            assert part[0][-1] > 0 and _rows_held(part, whole, px), (begin, count)
            seen += part[0][-1]
    assert seen == whole[0][-1]
    seen = 0
    for rank in range(2):
        with _ctx(s) as ctx:
            ctx.set_row_tiles(4, rank, 2)
            part = ctx.ray_shape_jacobian()
        px = (np.asarray(sharding.local_rows(s.ry, 4, rank, 2))[:, None] * s.rx + np.arange(s.rx)).reshape(-1)
        assert _rows_held(part, whole, px), rank
        seen += part[0][-1]
    assert seen == whole[0][-1]


def test_renders_around_the_calls_are_untouched():
    s = _scene("ball")
    with _ctx(s) as a, _ctx(s) as b:
        for _ in range(3):  # (three frames: the view cache is in use by the third)
            ia, ib = a.render(), b.render()
        before = a.stats()
        j = a.ray_shape_jacobian()
        assert a.stats() == before
        for _ in range(3):
            ja, jb = a.render(), b.render()
            assert np.array_equal(ja.view(np.uint32), ia.view(np.uint32)) and np.array_equal(jb.view(np.uint32), ib.view(np.uint32))
        assert a.stats()["segments"] == b.stats()["segments"] == j[0][-1]
    assert _same(j, _exported("ball")[0])


# ---- 4. the guard -----------------------------------------------------------------------------------------------------

def test_capacity_is_a_guard_and_a_stale_row_ptr_is_reported():
    import torch
    s = _scene("kuhn3_off_tile")
    whole, _ = _exported("kuhn3_off_tile")
    row_ptr, dI, faces, bary = whole[0], whole[3], whole[4], whole[5]
    nnz = int(row_ptr[-1])
    lp, dp, bp = C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    with _ctx(s) as ctx:
        rp = np.ascontiguousarray(row_ptr)
        h_dI, h_f, h_b = np.full(nnz, -7.0), np.full(nnz, 255, np.uint8), np.full((nnz, 2, 3), -7.0)
        assert ctx.lib.c5_ray_shape_jacobian_fill(ctx.handle, rp.ctypes.data_as(lp), nnz - 1, h_dI.ctypes.data_as(dp), h_f.ctypes.data_as(bp),
                                                  h_b.ctypes.data_as(dp)) == capi.C5_ERR_INVALID
        assert str(nnz) in ctx.lib.c5_last_error(ctx.handle).decode()
        assert (h_dI == -7.0).all() and (h_f == 255).all() and (h_b == -7.0).all()
        cap = nnz - 1
        d_rp = torch.tensor(rp, device="cuda")
        d_dI = torch.full((nnz + 64,), -7.0, dtype=torch.float64, device="cuda")
        d_f = torch.full((nnz + 64,), 255, dtype=torch.uint8, device="cuda")
        d_b = torch.full((nnz + 64, 2, 3), -7.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        ctx.ray_shape_jacobian_device(d_rp, d_dI.data_ptr(), d_f.data_ptr(), d_b.data_ptr(), capacity=cap)
        with pytest.raises(capi.C5Error) as e:
            ctx.synchronize()
        assert e.value.code == capi.C5_ERR_STATE and "ray shape jacobian fill" in e.value.message
        got = [d_dI.cpu().numpy(), d_f.cpu().numpy(), d_b.cpu().numpy()]
        assert (got[0][cap:] == -7.0).all() and (got[1][cap:] == 255).all() and (got[2][cap:] == -7.0).all()  # the sentinels past capacity
        assert _same([g[:cap] for g in got], [a[:cap] for a in (dI, faces, bary)])
        assert ctx.synchronize() == capi.C5_OK  # (reported once)
        # other scalars: other values on the same structure, the same faces and barycentrics
        ctx.update_scalars(0.5 * s.alpha + 0.1, s.q[::-1].copy())
        second = ctx.ray_shape_jacobian_fill(row_ptr)
        assert not np.array_equal(second[0], dI) and _same(second[1:], (faces, bary))
        ctx.update_scalars(s.alpha, s.q)
        # a view changed between the rows call and the fill
        ctx.set_view(mg.view_rotations(0.4, -0.3, 0.2))
        with pytest.raises(capi.C5Error) as e:
            ctx.ray_shape_jacobian_fill(row_ptr)
        assert e.value.code == capi.C5_ERR_STATE and "the frame changed" in e.value.message


def test_bad_arguments_and_outstanding_async_frames_are_refused():
    s = _scene("kuhn3_off_tile")
    whole, _ = _exported("kuhn3_off_tile")
    nnz = int(whole[0][-1])
    lp, dp, bp, ip, vp = C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.c_void_p
    rp = np.ascontiguousarray(whole[0])
    a, f, b = np.zeros(nnz), np.zeros(nnz, np.uint8), np.zeros((nnz, 2, 3))
    fpts, dw = np.zeros((len(s.cells), 4, 3), np.int32), np.zeros((len(s.cells), 4, 3))
    with _ctx(s) as ctx:
        lib, h = ctx.lib, ctx.handle
        p_rp, pa, pf, pb = rp.ctypes.data_as(lp), a.ctypes.data_as(dp), f.ctypes.data_as(bp), b.ctypes.data_as(dp)
        assert lib.c5_ray_shape_jacobian_fill(None, p_rp, nnz, pa, pf, pb) == capi.C5_ERR_INVALID
        assert lib.c5_ray_shape_jacobian_fill(h, None, nnz, pa, pf, pb) == capi.C5_ERR_INVALID
        assert lib.c5_ray_shape_jacobian_fill(h, p_rp, nnz, None, None, None) == capi.C5_ERR_INVALID  # all three missing
        assert lib.c5_ray_shape_jacobian_fill(h, p_rp, -1, pa, pf, pb) == capi.C5_ERR_INVALID
        some = rp.ctypes.data  # (a non-null stand-in: the checks come before anything is read or written)
        assert lib.c5_ray_shape_jacobian_fill_device(h, None, nnz, vp(some), vp(some), vp(some)) == capi.C5_ERR_INVALID
        assert lib.c5_ray_shape_jacobian_fill_device(h, vp(some), nnz, None, None, None) == capi.C5_ERR_INVALID
        assert lib.c5_ray_shape_jacobian_fill_device(h, vp(some), -1, vp(some), vp(some), vp(some)) == capi.C5_ERR_INVALID
        assert lib.c5_face_gradients(h, None, dw.ctypes.data_as(dp)) == capi.C5_ERR_INVALID
        assert lib.c5_face_gradients(h, fpts.ctypes.data_as(ip), None) == capi.C5_ERR_INVALID
        assert lib.c5_face_gradients(None, fpts.ctypes.data_as(ip), dw.ctypes.data_as(dp)) == capi.C5_ERR_INVALID
        assert lib.c5_face_gradients_device(h, None, None) == capi.C5_ERR_INVALID
        # any one array alone is enough
        assert lib.c5_ray_shape_jacobian_fill(h, p_rp, nnz, None, pf, None) == capi.C5_OK and np.array_equal(f, whole[4])
        assert lib.c5_ray_shape_jacobian_fill(h, p_rp, nnz, None, None, pb) == capi.C5_OK and np.array_equal(_bits(b), _bits(whole[5]))
        buf = ctx.host_image()
        ctx.render_host_async(buf)
        with pytest.raises(capi.C5Error) as e:
            ctx.ray_shape_jacobian_fill(rp)
        assert e.value.code == capi.C5_ERR_STATE
        with pytest.raises(capi.C5Error) as e:
            ctx.face_gradients()
        assert e.value.code == capi.C5_ERR_STATE
        assert ctx.render_host_wait() == capi.C5_OK
        ctx.free_host_image(buf)
        assert _same(ctx.ray_shape_jacobian(), whole)


def test_a_scene_of_solids_only_has_empty_rows():
    sx, sc = mg.kuhn_box(2, lo=(0.9, -0.15, 0.3), size=0.3)
    rots = mg.view_rotations(0.13, 0.21)
    with capi.Context(0) as ctx:
        ctx.set_solid(0, sx[sc].reshape(-1, 12), 0.5)
        ctx.set_image(28, 21, mg.REFERENCE_BOUNDS)
        ctx.set_view(rots)
        ctx.set_solid_view(0, rots)
        out = ctx.ray_shape_jacobian()
        stale = np.zeros(28 * 21 + 1, np.int64)
        stale[-1] = 3
        with pytest.raises(capi.C5Error) as e:
            ctx.ray_shape_jacobian_fill(stale)
        assert e.value.code == capi.C5_ERR_STATE
    assert not out[0].any() and all(len(a) == 0 for a in out[1:])


# ---- 5. the fit's operators and the preconditioner -----------------------------------------------------------------------

def _column_bar(got, want, what):
    for k, name in enumerate("xyz"):
        err, top = np.abs(got[:, k] - want[:, k]).max(), np.abs(want[:, k]).max()
        print(f"{what} {name}: max error {err:.3g} of max {top:.3g} ({err / top:.3g})")
        assert top > 0 and err <= 1e-6 * top


def test_explicit_operators_against_the_library_s():
    import torch
    from course5_amd import autograd, fit
    s = _scene("kuhn3_off_tile")
    rng = np.random.default_rng(52)
    alpha, q = torch.tensor(s.alpha), torch.tensor(s.q)
    r = torch.tensor(rng.normal(size=(s.ry, s.rx, 2)).astype(np.float32))
    w = torch.tensor(rng.uniform(0.5, 2.0, size=(s.ry, s.rx, 2)).astype(np.float32))
    p = torch.tensor(rng.normal(size=(len(s.xyz), 3)))
    with _ctx(s) as ctx:
        for weight in (None, w):
            ops = fit.ExplicitShapeJacobian(ctx).shape_operators(alpha, q, weight)
            _loss, grad = fit.shape_gradient(ctx, alpha, q, r.cuda(), weight)
            _column_bar(ops.rhs(r).cpu().numpy(), grad.cpu().numpy(), "rhs")
            h = autograd.vertex_gn_product(ctx, alpha, q, p, weight)
            _column_bar(ops.product(p).cpu().numpy(), h.cpu().numpy(), "product")
            loss2, grad2 = fit.shape_gradient(fit.ExplicitShapeJacobian(ctx), alpha, q, r, weight)
            assert abs(loss2 - _loss) <= 1e-12 * abs(_loss) and np.array_equal(grad2.cpu().numpy(), ops.rhs(r).cpu().numpy())


def test_the_diagonal_against_unit_vector_products():
    import torch
    from course5_amd import fit
    xyz, cells = mg.kuhn_box(2, jitter=0.2)
    s = types.SimpleNamespace(xyz=xyz, cells=cells, rots=sj.SMALL_ROTS, rx=27, ry=21, bounds=sj.SMALL_BOUNDS, options=(), solid=None)
    s.alpha, s.q = mr.scalars(len(cells), 4)
    n = 3 * len(xyz)
    assert n == 81
    w = np.random.default_rng(53).uniform(0.5, 2.0, size=(s.ry, s.rx, 2)).astype(np.float32)
    with _ctx(s) as ctx:
        diag = fit.ExplicitShapeJacobian(ctx).shape_operators(torch.tensor(s.alpha), torch.tensor(s.q), torch.tensor(w)).diagonal()
        h = ctx.render_vertex_gn_product(np.eye(n).reshape(n, len(xyz), 3), w)
    want = np.einsum("ii->i", h.reshape(n, n))
    got = diag.cpu().numpy().reshape(-1)
    err = np.abs(got - want)
    print(f"diagonal: {int((want > 0).sum())} of {n} positive, worst error / (2^-22 diag) {(err / np.where(want > 0, 2.0 ** -22 * want, 1.0)).max():.3g}")
    assert (want > 0).sum() > n // 2 and (err <= 2.0 ** -22 * want).all()


def _graded_frame():
    from tests import unstructured_scenes as us
    xyz, cells, alpha, q, rots, _res, limit = us.scene(7002)  # a Kuhn box bisected 57 times toward one of its side planes
    s = types.SimpleNamespace(xyz=xyz, cells=cells, alpha=alpha, q=q, rots=rots, rx=28, ry=21, bounds=fz.B, options=(), solid=None, limit=limit)
    return s


def test_the_preconditioned_step_on_a_graded_layer_stack():
    import torch
    from course5_amd import fit
    s = _graded_frame()
    alpha, q = torch.tensor(s.alpha), torch.tensor(s.q)
    with _ctx(s) as ctx:
        ctx.set_alpha_limit(s.limit)
        ctx.update_scalars(s.alpha, 1.2 * s.q + 0.05)
        target = ctx.render()
        ctx.update_scalars(s.alpha, s.q)
        r = torch.tensor(ctx.render() - target)
        assert float(r.abs().max()) > 0
        ex = fit.ExplicitShapeJacobian(ctx)
        d = ex.shape_operators(alpha, q, None).diagonal()
        d_plain, m_plain = fit.shape_step(ex, alpha, q, r, iters=10)
        d_pre, m_pre = fit.shape_step_preconditioned(ex, alpha, q, r, iters=10)
        P = fit.ShapePrior(ctx, 1e-3)
        d_pp, m_pp = fit.shape_step_preconditioned(fit.WithShapePrior(ex, P), alpha, q, r, iters=10)
        _d_np, m_np = fit.shape_step(fit.WithShapePrior(ex, P), alpha, q, r, iters=10)
        with pytest.raises(ValueError, match="ExplicitShapeJacobian"):
            fit.shape_step_preconditioned(ctx, alpha, q, r.cuda())
        free = torch.ones(len(s.xyz), dtype=torch.bool)
        free[::3] = False
        d_free, _m = fit.shape_step_preconditioned(ex, alpha, q, r, iters=4, free=free)
    pos = d[d > 0]
    print(f"graded stack: diag(J^T J) spans {float(pos.min()):.3g} .. {float(pos.max()):.3g}; model after 10 iterations: "
          f"plain {m_plain[-1]:.9g}, preconditioned {m_pre[-1]:.9g}; with the shape prior: plain {m_np[-1]:.9g}, preconditioned {m_pp[-1]:.9g}")
    assert len(m_plain) == len(m_pre) == 10 and m_pre[-1] < 0
    assert m_pre[-1] <= m_plain[-1]
    assert len(m_pp) == 10 and m_pp[-1] <= m_np[-1]
    assert torch.isfinite(d_pre).all() and float(d_pre.abs().max()) > 0 and float(d_pp.abs().max()) > 0 and float(d_plain.abs().max()) > 0
    assert not d_free[~free].any() and float(d_free[free].abs().max()) > 0


def _shape_cg_as_it_was(JtWr, H, damping, iters):
    """fit._shape_cg before it took a preconditioner (free None), written out: what the default must still run, bit for bit."""
    import torch

    def dot(a, b):
        return float((a * b).sum())

    g = JtWr()
    x = torch.zeros_like(g)
    hx = torch.zeros_like(g)
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


def test_the_default_step_is_the_step_it_was_bit_for_bit():
    import torch
    from course5_amd import autograd, fit
    s = _scene("kuhn3_off_tile")
    rng = np.random.default_rng(54)
    alpha, q = torch.tensor(s.alpha), torch.tensor(s.q)
    r = torch.tensor(rng.normal(size=(s.ry, s.rx, 2)).astype(np.float32)).cuda()
    w = torch.tensor(rng.uniform(0.5, 2.0, size=(s.ry, s.rx, 2)).astype(np.float32)).cuda()
    with _ctx(s, s.options + (("vertex_exact", 1),)) as ctx:
        d0, m0 = fit.shape_step(ctx, alpha, q, r, w, iters=5)
        d1, m1 = fit.shape_step(ctx, alpha, q, r, w, iters=5)
        device = torch.device("cuda", 0)
        want, mw = _shape_cg_as_it_was(lambda: autograd._vertex_adjoint(ctx, (r * w).contiguous(), device),
                                       lambda p: autograd._vertex_gn_product(ctx, p.reshape(1, len(s.xyz), 3).contiguous(), w, device)[0], 1e-3, 5)
    assert len(m0) == 5 and m0 == m1 == mw
    assert torch.equal(d0, d1) and torch.equal(d0, want) and float(d0.abs().max()) > 0

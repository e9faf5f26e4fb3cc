"""The ray shape Jacobian's numpy restatement (tests/shape_jacobian_reference.py) against the vertex adjoint's restatement
and central differences, the coalesced operators of course5_amd.fit over the restated arrays against the dense matrix, and
shape_step's preconditioned iteration on a dense stand-in.  No GPU.

Bars.  Two fp64 evaluations of the same sum in another order: 1e-12 x the sum of the terms' absolute values
(tests/test_vertex_adjoint_cpu.py).  Central differences at h = 1e-6: 1e-6 x max |grad| per component (the same file)."""
import re
import os
import types

import numpy as np
import pytest
import torch

from course5_amd import autograd, capi, fit, meshgen as mg
from tests import adjoint_reference as ar, derivative_fuzz as fz, motion_reference as mr
from tests import shape_jacobian_reference as sj, vertex_adjoint_reference as vr

BOUNDS, ROTS = sj.SMALL_BOUNDS, sj.SMALL_ROTS
RX, RY = 28, 21
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def box():
    xyz, cells = mg.kuhn_box(3, jitter=0.2)
    alpha, q = mr.scalars(len(cells), 7)
    dz_err = fz.dz_err(types.SimpleNamespace(xyz=xyz, rots=ROTS))
    m = ar.ray_matrices(xyz, cells, alpha, q, ROTS, RX, RY, BOUNDS)
    geo = vr.segment_faces(xyz, cells, ROTS, RX, RY, BOUNDS)
    a = sj.arrays_of(m, geo, xyz, cells, ROTS, dz_err)
    a["face_points"], a["dw_dxyz"], a["edge_on"] = sj.face_gradients(xyz, cells, ROTS)
    n_pts = len(xyz)
    J_I, J_tau = sj.dense_jacobian(a, n_pts, a["dI_ddz"]), sj.dense_jacobian(a, n_pts, a["alpha"])
    return types.SimpleNamespace(xyz=xyz, cells=cells, alpha=alpha, q=q, m=m, geo=geo, a=a, n_pts=n_pts, J_I=J_I, J_tau=J_tau)


def _operators(s, weight=None):
    a = s.a
    csr = autograd.assemble_shape_jacobian(a["row_ptr"], a["col"], s.alpha, a["dI_ddz"], a["faces"], a["bary"], a["face_points"],
                                           a["dw_dxyz"], s.n_pts)
    return fit.ShapeJacobianOperators(*csr, s.n_pts, weight)


def test_header_binding_and_python_surface():
    text = open(os.path.join(ROOT, "include", "course5_hip.h")).read()
    for name, args in (
            ("c5_ray_shape_jacobian_fill", r"c5_context\* ctx, const int64_t\* row_ptr_host, int64_t capacity, double\* dI_ddz_host,\s+"
                                           r"uint8_t\* faces_host, double\* bary_host"),
            ("c5_ray_shape_jacobian_fill_device", r"c5_context\* ctx, const void\* row_ptr_dev, int64_t capacity, void\* dI_ddz_dev,\s+"
                                                  r"void\* faces_dev, void\* bary_dev"),
            ("c5_face_gradients", r"c5_context\* ctx, int32_t\* face_points_host, double\* dw_dxyz_host"),
            ("c5_face_gradients_device", r"c5_context\* ctx, void\* face_points_dev, void\* dw_dxyz_dev")):
        assert re.search(r"int " + name + r"\(" + args + r"\);", text), name
        assert name in capi.EXPORTS
    for name in ("ray_shape_jacobian", "ray_shape_jacobian_device", "ray_shape_jacobian_fill", "face_gradients", "face_gradients_device"):
        assert callable(getattr(capi.Context, name))
    assert "ray_shape_jacobian" in autograd.__all__ and callable(autograd.ray_shape_jacobian)
    assert callable(fit.ExplicitShapeJacobian) and callable(fit.shape_step_preconditioned)


def test_rows_are_the_vertex_adjoint_of_one_hot_images_in_all_192_components(box):
    s = box
    assert s.J_I.shape == (RX * RY, 64, 3)
    covered = np.nonzero(np.diff(s.a["row_ptr"]) > 0)[0]
    pixels = covered[np.linspace(0, len(covered) - 1, 16).astype(int)]
    worst = 0.0
    for p in pixels:
        for ch, J in ((0, s.J_tau), (1, s.J_I)):
            g = np.zeros((RY, RX, 2))
            g.reshape(-1, 2)[p, ch] = 1.0
            ref = vr.gradients_of(s.m, s.geo, s.cells, s.n_pts, ROTS, g)
            err, bar = np.abs(J[p] - ref["raw"]), 1e-12 * ref["scale_raw"]
            assert np.abs(ref["raw"]).max() > 0 and (err <= bar).all(), (p, ch, float((err / np.where(bar > 0, bar, 1)).max()))
            worst = max(worst, float((err / np.where(bar > 0, bar, 1.0)).max()))
    # ... and by linearity every pixel at once
    g = np.random.default_rng(11).normal(size=(RY, RX, 2))
    ref = vr.gradients_of(s.m, s.geo, s.cells, s.n_pts, ROTS, g)
    got = np.einsum("p,pvk->vk", g.reshape(-1, 2)[:, 0], s.J_tau) + np.einsum("p,pvk->vk", g.reshape(-1, 2)[:, 1], s.J_I)
    assert (np.abs(got - ref["raw"]) <= 1e-12 * ref["scale_raw"]).all()
    print(f"one-hot rows: worst error / (1e-12 sum |terms|) = {worst:.3g}")


def test_against_central_differences_of_every_component(box):
    s = box
    g = np.random.default_rng(12).normal(size=(RY, RX, 2)).astype(np.float32).astype(np.float64)
    got = np.einsum("p,pvk->vk", g.reshape(-1, 2)[:, 0], s.J_tau) + np.einsum("p,pvk->vk", g.reshape(-1, 2)[:, 1], s.J_I)
    h = 1e-6
    fd = np.zeros_like(got)
    for v in range(s.n_pts):
        for k in range(3):
            vals = []
            for sign in (1, -1):
                p = s.xyz.copy()
                p[v, k] += sign * h
                vals.append(vr.loss(p, s.cells, s.alpha, s.q, ROTS, RX, RY, BOUNDS, g))
            fd[v, k] = (vals[0] - vals[1]) / (2 * h)
    top, err = np.abs(got).max(), np.abs(fd - got)
    print(f"central differences: worst error {err.max():.3g} of max {top:.3g} ({err.max() / top:.3g})")
    assert top > 0 and (err <= 1e-6 * top).all()


def test_operators_over_the_restated_arrays_against_the_dense_matrix(box):
    s = box
    rng = np.random.default_rng(13)
    w = rng.uniform(0.5, 2.0, size=(RY, RX, 2)).astype(np.float32)
    w64 = w.astype(np.float64).reshape(-1, 2)
    Jt, Ji = s.J_tau.reshape(RX * RY, -1), s.J_I.reshape(RX * RY, -1)
    for weight, wt, wi in ((None, np.ones(RX * RY), np.ones(RX * RY)), (w, w64[:, 0], w64[:, 1])):
        ops = _operators(s, None if weight is None else torch.tensor(weight))
        want = (wt[:, None] * Jt * Jt).sum(0) + (wi[:, None] * Ji * Ji).sum(0)  # diag(J^T W J): positive terms
        got = ops.diagonal().numpy().reshape(-1)
        assert want.max() > 0 and np.allclose(got, want, rtol=1e-12, atol=0.0)
        p = rng.normal(size=(s.n_pts, 3))
        hp = Jt.T @ (wt * (Jt @ p.reshape(-1))) + Ji.T @ (wi * (Ji @ p.reshape(-1)))
        terms = np.abs(Jt).T @ (wt * (np.abs(Jt) @ np.abs(p.reshape(-1)))) + np.abs(Ji).T @ (wi * (np.abs(Ji) @ np.abs(p.reshape(-1))))
        assert (np.abs(ops.product(torch.tensor(p)).numpy().reshape(-1) - hp) <= 1e-12 * terms).all()
        r = rng.normal(size=(RY, RX, 2)).astype(np.float32)
        g = (r if weight is None else r * weight).astype(np.float64).reshape(-1, 2)
        rhs = Jt.T @ g[:, 0] + Ji.T @ g[:, 1]
        terms = np.abs(Jt).T @ np.abs(g[:, 0]) + np.abs(Ji).T @ np.abs(g[:, 1])
        assert (np.abs(ops.rhs(torch.tensor(r)).numpy().reshape(-1) - rhs) <= 1e-12 * terms).all()
    # the coalesced structure: every (pixel, coordinate) once, columns of one row ascending
    assert (np.diff(ops.crow.numpy()) >= 0).all() and ops.crow[-1] == len(ops.cols)
    key = np.repeat(np.arange(RX * RY), np.diff(ops.crow.numpy())) * (3 * s.n_pts) + ops.cols.numpy()
    assert (np.diff(key) > 0).all()


@pytest.mark.parametrize("kind", sj.SCENES)
def test_the_restatement_s_ties_stay_under_the_cap(kind):
    sc = sj.scene(kind)
    alpha, q = mr.scalars(len(sc["cells"]), 3)
    dz_err = fz.dz_err(types.SimpleNamespace(xyz=sc["xyz"], rots=sc["rots"]))
    a = sj.shape_arrays(sc["xyz"], sc["cells"], alpha, q, sc["rots"], sc["rx"], sc["ry"], sc["bounds"], dz_err)
    share = a["tie"].mean()
    print(f"{kind}: {len(a['col'])} segments on {int((np.diff(a['row_ptr']) > 0).sum())} of {sc['rx'] * sc['ry']} pixels, ties {share:.3%}")
    assert len(a["col"]) > 200 and share <= sj.TIE_CAP
    lam = a["bary"]
    assert np.abs(lam.sum(2) - 1.0).max() <= 1e-9 and (a["sens_bary"] > 0).all() and np.isfinite(a["sens_bary"]).all()


def test_preconditioned_cg_reaches_the_unpreconditioned_solution():
    rng = np.random.default_rng(14)
    n_pts = 12
    n = 3 * n_pts
    A = rng.normal(size=(2 * n, n))
    s = 10.0 ** rng.uniform(-3, 3, n)  # columns whose scales span six orders: what a graded grid does to diag(J^T W J)
    Hm = torch.tensor((A * s).T @ (A * s))
    g = torch.tensor(rng.normal(size=n) * s).reshape(n_pts, 3)
    damping = 1e-9
    H = lambda p: (Hm @ p.reshape(-1)).reshape(n_pts, 3)  # noqa: E731
    want = torch.linalg.solve(Hm + damping * torch.eye(n, dtype=torch.float64), -g.reshape(-1)).reshape(n_pts, 3)
    plain, m_plain = fit._shape_cg(lambda: g.clone(), H, damping, 40 * n, None, n_pts)
    pre, m_pre = fit._shape_cg(lambda: g.clone(), H, damping, 40 * n, None, n_pts, diagonal=lambda: torch.diagonal(Hm).reshape(n_pts, 3))
    model = lambda x: float(0.5 * x.reshape(-1) @ (Hm @ x.reshape(-1)) + damping * 0.5 * (x * x).sum() + (x * g).sum())  # noqa: E731
    best = model(want)
    print(f"model at the solution {best:.9g}; plain CG {model(plain):.9g} after {len(m_plain)}, preconditioned {model(pre):.9g} after {len(m_pre)}; "
          f"after 10 iterations: plain {m_plain[9]:.6g}, preconditioned {m_pre[9]:.6g}")
    assert abs(model(pre) - best) <= 1e-9 * abs(best) and abs(model(plain) - best) <= 1e-6 * abs(best)
    assert len(m_pre) <= len(m_plain) and m_pre[9] <= m_plain[9]
    assert torch.allclose(pre, want, rtol=1e-6, atol=1e-6 * float(want.abs().max()))
    # fixed rows stay fixed, with and without the preconditioner
    free = torch.ones(n_pts, dtype=torch.bool)
    free[[2, 5]] = False
    x, _ = fit._shape_cg(lambda: g.clone(), H, damping, 50, free, n_pts, diagonal=lambda: torch.diagonal(Hm).reshape(n_pts, 3))
    assert not x[~free].any() and x[free].abs().max() > 0
    # without a diagonal the iteration is the one it was: the same bits as the loop written out
    x2, m2 = fit._shape_cg(lambda: g.clone(), H, damping, 7, None, n_pts)
    x3, m3 = fit._shape_cg(lambda: g.clone(), H, damping, 7, None, n_pts, None)
    assert torch.equal(x2, x3) and m2 == m3


def test_the_preconditioned_step_needs_operators_with_a_diagonal():
    plain = types.SimpleNamespace(n_pts=4)
    with pytest.raises(ValueError, match="ExplicitShapeJacobian"):
        fit.shape_step_preconditioned(plain, None, None, None)
    ops = types.SimpleNamespace(rhs=lambda r: torch.zeros(4, 3, dtype=torch.float64), product=lambda p: p)
    own = types.SimpleNamespace(n_pts=4, shape_operators=lambda alpha, q, weight: ops)
    with pytest.raises(ValueError, match="ExplicitShapeJacobian"):
        fit.shape_step_preconditioned(own, None, None, None)
    d, models = fit.shape_step(own, None, None, None)  # (the default asks for no diagonal)
    assert not d.any() and models == []

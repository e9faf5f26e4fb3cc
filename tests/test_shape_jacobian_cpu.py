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


def _plain_cg_written_out(g, H, damping, iters, keep):
    """shape_step's plain CG, line for line (keep: float64 [n_pts, 1] of 0 / 1, or None)."""
    fixed = lambda v: v if keep is None else v * keep  # noqa: E731
    dot = lambda a, b: float((a * b).sum())  # noqa: E731
    g = fixed(g)
    x, hx, res, models = torch.zeros_like(g), torch.zeros_like(g), -g, []
    p = res.clone()
    rr = dot(res, res)
    for _ in range(iters):
        if not rr > 0.0:
            break
        ap = fixed(H(p)) + damping * p
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


def _preconditioned_cg_written_out(g, H, damping, iters, keep, diagonal):
    """shape_step_preconditioned's CG, line for line."""
    fixed = lambda v: v if keep is None else v * keep  # noqa: E731
    dot = lambda a, b: float((a * b).sum())  # noqa: E731
    g = fixed(g)
    x, hx, res, models = torch.zeros_like(g), torch.zeros_like(g), -g, []
    m = diagonal + damping
    m_inv = fixed(torch.where(m > 0, 1.0 / torch.where(m > 0, m, torch.ones_like(m)), torch.zeros_like(m)))
    z = res * m_inv
    p = z.clone()
    rz = dot(res, z)
    for _ in range(iters):
        if not rz > 0.0:
            break
        ap = fixed(H(p)) + damping * p
        curvature = dot(p, ap)
        if not curvature > 0.0:
            break
        step = rz / curvature
        x += step * p
        hx += step * ap
        res -= step * ap
        models.append(0.5 * dot(x, hx) + dot(x, g))
        z = res * m_inv
        rz_next = dot(res, z)
        p = z + (rz_next / rz) * p
        rz = rz_next
    return x, models


@pytest.mark.parametrize("n_pts", [1, 4, 12])
def test_both_iterations_are_the_loops_written_out_bit_for_bit(n_pts):
    """Both of fit._shape_cg's iterations, with `free` None and set and damping 0 and 1e-3, against the two loops above:
    torch.equal steps and equal models.  On one point two more systems take the loops' exits: H = 2 I, whose first step is
    exact and leaves a residual of 0 (rz > 0 fails), and H = 0, a direction without curvature while damping is 0."""
    rng = np.random.default_rng(15 + n_pts)
    n = 3 * n_pts
    A = rng.normal(size=(2 * n, n)) * 10.0 ** rng.uniform(-2, 2, n)
    systems = [("random", torch.tensor(A.T @ A))]
    if n_pts == 1:
        systems += [("2 I", 2.0 * torch.eye(n, dtype=torch.float64)), ("0", torch.zeros((n, n), dtype=torch.float64))]
    g = torch.tensor(rng.normal(size=(n_pts, 3)))
    free = torch.ones(n_pts, dtype=torch.bool)
    free[::3] = n_pts == 1  # (the only point stays free; of several, every third is fixed)
    assert free.any() and free.all() == (n_pts == 1)
    for name, Hm in systems:
        diag = torch.diagonal(Hm).reshape(n_pts, 3)
        H = lambda p: (Hm @ p.reshape(-1)).reshape(n_pts, 3)  # noqa: E731
        for fr in (None, free):
            keep = None if fr is None else fr.to(torch.float64).reshape(-1, 1)
            for damping in (0.0, 1e-3):
                x, models = fit._shape_cg(lambda: g.clone(), H, damping, 25, fr, n_pts)
                want, want_models = _plain_cg_written_out(g.clone(), H, damping, 25, keep)
                assert torch.equal(x, want) and models == want_models, (name, "plain")
                xp, models_p = fit._shape_cg(lambda: g.clone(), H, damping, 25, fr, n_pts, diagonal=lambda: diag)
                want, want_models = _preconditioned_cg_written_out(g.clone(), H, damping, 25, keep, diag)
                assert torch.equal(xp, want) and models_p == want_models, (name, "preconditioned")
                if fr is not None:
                    assert not x[~fr].any() and not xp[~fr].any()
                if damping == 0.0:
                    steps = {"random": None, "2 I": 1, "0": 0}[name]
                    assert steps is None or (len(models), len(models_p)) == (steps, steps), name
                assert name == "0" and damping == 0.0 or (len(models) >= 1 and len(models_p) >= 1)


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


# ---- the operators bit for bit: every product is the gather, the multiply and the segmented sum written out ---------------

def _written_out_cases(box):
    csr = autograd.assemble_shape_jacobian(box.a["row_ptr"], box.a["col"], box.alpha, box.a["dI_ddz"], box.a["faces"], box.a["bary"],
                                           box.a["face_points"], box.a["dw_dxyz"], box.n_pts)
    rng = np.random.default_rng(16)
    yield ("box",) + tuple(torch.as_tensor(t) for t in csr) + (box.n_pts, rng.uniform(0.5, 2.0, size=(RY, RX, 2)).astype(np.float32))
    # no nonzero at all; and an empty first row, an empty last row, an empty row between and coordinates (0, 3, 7, 8) no row names
    for kind, crow, cols, n_pts in (("empty", [0, 0, 0, 0, 0], [], 2), ("gaps", [0, 0, 2, 2, 5, 6, 6], [4, 1, 2, 5, 1, 4], 3)):
        crow, cols = torch.tensor(crow, dtype=torch.int64), torch.tensor(cols, dtype=torch.int64)
        yield (kind, crow, cols, torch.tensor(rng.normal(size=len(cols))), torch.tensor(rng.normal(size=len(cols))), n_pts,
               rng.uniform(0.5, 2.0, size=(len(crow) - 1, 2)).astype(np.float32))


def test_every_product_is_the_segmented_sum_written_out_bit_for_bit(box):
    from tests import operators_written_out as wo
    for kind, crow, cols, v_tau, v_I, n_pts, w in _written_out_cases(box):
        n_px = len(crow) - 1
        m = wo.ByRowAndColumn(crow, cols, 3 * n_pts)
        rng = np.random.default_rng(17)
        p = torch.tensor(rng.normal(size=(n_pts, 3)))
        r = rng.normal(size=(n_px, 2)).astype(np.float32)
        jt = lambda g_tau, g_I: (m.to_columns(v_tau, g_tau) + m.to_columns(v_I, g_I)).reshape(n_pts, 3)  # noqa: E731
        for weight in (None, w):
            ops = fit.ShapeJacobianOperators(crow, cols, v_tau, v_I, n_pts, None if weight is None else torch.from_numpy(weight))
            tau, I = m.to_rows(v_tau, p.reshape(-1)), m.to_rows(v_I, p.reshape(-1))
            got = ops.jv(p)
            assert got[0].shape == (n_px,) and torch.equal(got[0], tau) and torch.equal(got[1], I), (kind, "jv")
            w_tau, w_I = wo.weights(weight, n_px)
            got = ops.product(p)
            assert got.shape == (n_pts, 3) and torch.equal(got, jt(tau if weight is None else w_tau * tau, I if weight is None else w_I * I)), (kind, "product")
            g_tau, g_I = torch.tensor(rng.normal(size=n_px)), torch.tensor(rng.normal(size=n_px))
            assert torch.equal(ops.jt(g_tau, g_I), jt(g_tau, g_I)), (kind, "jt")
            assert torch.equal(ops.rhs(torch.from_numpy(r)), jt(*wo.weighted_image(r, weight))), (kind, "rhs")
            diag = ops.diagonal()
            assert torch.equal(diag, (m.to_columns(v_tau * v_tau, w_tau) + m.to_columns(v_I * v_I, w_I)).reshape(n_pts, 3)), (kind, "diagonal")
            if kind == "gaps":  # the rows and coordinates nothing names are exact zeros, the others are not
                named = torch.zeros(3 * n_pts, dtype=torch.bool)
                named[cols] = True
                assert not diag.reshape(-1)[~named].any() and (diag.reshape(-1)[named] > 0).all()
                assert not ops.jv(p)[1][[0, 2, 5]].any()


def test_the_messages_of_the_four_checks(box):
    ops = _operators(box)
    crow, cols, v_tau, v_I, n = ops.crow, ops.cols, ops.v_tau, ops.v_I, box.n_pts
    for a, b, c in ((cols[:-1], v_tau, v_I), (cols, v_tau[:-1], v_I), (cols, v_tau, v_I[:-1])):
        with pytest.raises(ValueError, match=re.escape(f"cols, v_tau and v_I must hold crow's {len(cols)} elements each")):
            fit.ShapeJacobianOperators(crow, a, b, c, n)
    top = int(cols.max())
    with pytest.raises(ValueError, match=re.escape(f"cols must name coordinates 0 .. {3 * (top // 3) - 1}")):
        fit.ShapeJacobianOperators(crow, cols, v_tau, v_I, top // 3)
    bad = cols.clone()
    bad[0] = -1
    with pytest.raises(ValueError, match=re.escape(f"cols must name coordinates 0 .. {3 * n - 1}")):
        fit.ShapeJacobianOperators(crow, bad, v_tau, v_I, n)
    with pytest.raises(ValueError, match=re.escape(f"weight must hold two values for each of the {RX * RY} pixels")):
        fit.ShapeJacobianOperators(crow, cols, v_tau, v_I, n, torch.zeros(RX * RY + 1, 2))
    with pytest.raises(ValueError, match=re.escape(f"residual must hold two values for each of the {RX * RY} pixels")):
        ops.rhs(torch.zeros(RX * RY - 1, 2))


# ---- what shape_gradient and shape_step ask of a context, and in which order -------------------------------------------

N_PTS, ROWS, RES_X = 3, 2, 3


class _Calls:
    """A stand-in for the library under a plain context (the four functions of autograd the shape fit goes through, on the
    CPU, over a dense J) and for a shape prior; every call is written down."""

    def __init__(self, monkeypatch=None):
        rng = np.random.default_rng(18)
        self.J = torch.tensor(rng.normal(size=(ROWS * RES_X * 2, 3 * N_PTS)))
        self.log = []
        self.ctx = types.SimpleNamespace(n_pts=N_PTS, local_rows=ROWS, res_x=RES_X, device=0, points=torch.tensor(rng.normal(size=(N_PTS, 3))))
        if monkeypatch is not None:
            import contextlib
            monkeypatch.setattr(torch.cuda, "device", lambda device: contextlib.nullcontext())
            monkeypatch.setattr(autograd, "_gn_enter", self.enter)
            monkeypatch.setattr(autograd, "_vertex_adjoint", self.vertex_adjoint)
            monkeypatch.setattr(autograd, "_vertex_gn_product", self.vertex_gn_product)

    def enter(self, ctx, alpha, q, what):
        self.log.append(("enter", what, alpha, q))
        return torch.device("cpu")

    def vertex_adjoint(self, ctx, g, device):
        assert ctx is self.ctx and g.dtype == torch.float32 and g.is_contiguous() and tuple(g.shape) == (ROWS, RES_X, 2)
        self.log.append(("vertex_adjoint", g.clone()))
        return (self.J.T @ g.reshape(-1).to(torch.float64)).reshape(N_PTS, 3)

    def vertex_gn_product(self, ctx, v, w, device):
        assert ctx is self.ctx and v.dtype == torch.float64 and v.is_contiguous() and tuple(v.shape) == (1, N_PTS, 3)
        self.log.append(("vertex_gn_product", v.clone(), None if w is None else w.clone()))
        jv = self.J @ v.reshape(-1)
        return (self.J.T @ (jv if w is None else w.reshape(-1).to(torch.float64) * jv)).reshape(1, N_PTS, 3)

    # the prior (fit.ShapePrior's three operators)
    def value_gradient(self, xyz):
        self.log.append(("prior.value_gradient", xyz))
        return torch.tensor([2.5], dtype=torch.float64), 0.25 * xyz

    def product(self, xyz, v):
        self.log.append(("prior.product", xyz, v.clone()))
        return 0.5 * v

    def diagonal(self, xyz):
        self.log.append(("prior.diagonal", xyz))
        return torch.full((N_PTS, 3), 0.5, dtype=torch.float64)

    def names(self):
        return [c[0] for c in self.log]


def _images():
    rng = np.random.default_rng(19)
    return (torch.tensor(rng.normal(size=(ROWS, RES_X, 2)).astype(np.float32)), torch.tensor(rng.uniform(0.5, 2.0, (ROWS, RES_X, 2)).astype(np.float32)))


@pytest.mark.parametrize("weighted", [False, True])
def test_a_plain_context_s_gradient_and_step_call_the_library_as_they_did(monkeypatch, weighted):
    s = _Calls(monkeypatch)
    r, w = _images()
    w = w if weighted else None
    g = (r * w).contiguous() if weighted else r
    alpha, q = torch.zeros(5), torch.ones(5)
    # the gradient: the scalars, then ONE vertex adjoint on w r (float32)
    loss, grad = fit.shape_gradient(s.ctx, alpha, q, r, w)
    assert [c[:2] for c in s.log] == [("enter", "shape_gradient"), ("vertex_adjoint", s.log[1][1])]
    assert s.log[0][2] is alpha and s.log[0][3] is q and torch.equal(s.log[1][1], g)
    assert loss == 0.5 * float((g.to(torch.float64) * r.to(torch.float64)).sum())
    assert torch.equal(grad, s.vertex_adjoint(s.ctx, g, None))
    # ... with a prior: the same, then the prior's value and gradient at the points the context holds
    s.log.clear()
    loss_p, grad_p = fit.shape_gradient(fit.WithShapePrior(s.ctx, s), alpha, q, r, w)
    assert s.names() == ["enter", "vertex_adjoint", "prior.value_gradient"] and s.log[2][1] is s.ctx.points
    assert loss_p == loss + 2.5 and torch.equal(grad_p, grad + 0.25 * s.ctx.points)
    # the step: the scalars, the vertex adjoint on w r, then one vertex Gauss-Newton product per iteration, with the weights
    s.log.clear()
    d, models = fit.shape_step(s.ctx, alpha, q, r, w, damping=1e-3, iters=3)
    assert s.names() == ["enter", "vertex_adjoint"] + ["vertex_gn_product"] * 3 and len(models) == 3
    assert s.log[0][1] == "shape_step" and torch.equal(s.log[1][1], g)
    assert torch.equal(s.log[2][1].reshape(N_PTS, 3), -grad)  # (the first direction: the residual of d = 0)
    assert all((c[2] is None) if w is None else torch.equal(c[2], w) for c in s.log[2:])
    want, want_models = _plain_cg_written_out(grad.clone(), lambda p: s.vertex_gn_product(s.ctx, p.reshape(1, N_PTS, 3).contiguous(), w, None)[0],
                                              1e-3, 3, None)
    assert torch.equal(d, want) and models == want_models
    # ... with a prior: its gradient after the adjoint, its product after every library product
    s.log.clear()
    d, models = fit.shape_step(fit.WithShapePrior(s.ctx, s), alpha, q, r, w, damping=1e-3, iters=2)
    assert s.names() == ["enter", "vertex_adjoint", "prior.value_gradient"] + ["vertex_gn_product", "prior.product"] * 2
    assert len(models) == 2 and all(c[1] is s.ctx.points for c in s.log if c[0].startswith("prior."))
    # a residual of another shape is refused with the text it was
    for call in (fit.shape_gradient, fit.shape_step):
        with pytest.raises(ValueError, match=re.escape(f"residual must be [{ROWS}, {RES_X}, 2], not [{ROWS}, {RES_X}]")):
            call(s.ctx, alpha, q, r[..., 0], w)
    # and the preconditioned step raises before anything reaches the library
    s.log.clear()
    with pytest.raises(ValueError, match="ExplicitShapeJacobian"):
        fit.shape_step_preconditioned(s.ctx, alpha, q, r, w)
    assert s.log == []


def test_a_context_s_own_shape_operators_are_called_as_they_were():
    s = _Calls()
    r, w = _images()
    Jt, Ji = s.J[0::2], s.J[1::2]

    class Ops:
        def rhs(self, residual):
            s.log.append(("rhs", residual))
            return (s.J.T @ (residual * w).reshape(-1).to(torch.float64)).reshape(N_PTS, 3)

        def product(self, p):
            s.log.append(("product", p.clone()))
            return (s.J.T @ (w.reshape(-1).to(torch.float64) * (s.J @ p.reshape(-1)))).reshape(N_PTS, 3)

        def diagonal(self):
            s.log.append(("diagonal",))
            w64 = w.reshape(-1, 2).to(torch.float64)
            return ((w64[:, :1] * Jt * Jt).sum(0) + (w64[:, 1:] * Ji * Ji).sum(0)).reshape(N_PTS, 3)

    def shape_operators(alpha, q, weight):
        s.log.append(("shape_operators", alpha, q, weight))
        return Ops()

    own = types.SimpleNamespace(n_pts=N_PTS, points=s.ctx.points, shape_operators=shape_operators)
    alpha, q = torch.zeros(5), torch.ones(5)
    loss, grad = fit.shape_gradient(own, alpha, q, r, w)
    assert s.names() == ["shape_operators", "rhs"] and all(a is b for a, b in zip(s.log[0][1:], (alpha, q, w))) and s.log[1][1] is r
    assert loss == 0.5 * float(((r * w).to(torch.float64) * r.to(torch.float64)).sum())
    s.log.clear()
    d, models = fit.shape_step(own, alpha, q, r, w, iters=3)
    assert s.names() == ["shape_operators", "rhs", "product", "product", "product"] and len(models) == 3
    assert torch.equal(s.log[2][1], -grad)
    s.log.clear()
    d, models = fit.shape_step_preconditioned(own, alpha, q, r, w, iters=2)
    assert s.names() == ["shape_operators", "rhs", "diagonal", "product", "product"] and len(models) == 2
    want, want_models = _preconditioned_cg_written_out(grad.clone(), Ops().product, 1e-3, 2, None, Ops().diagonal())
    assert torch.equal(d, want) and models == want_models
    # with a prior every operator of the context is followed by the prior's, at the points the context holds
    s.log.clear()
    d, models = fit.shape_step_preconditioned(fit.WithShapePrior(own, s), alpha, q, r, w, iters=2)
    assert s.names() == ["shape_operators", "rhs", "prior.value_gradient", "diagonal", "prior.diagonal"] + ["product", "prior.product"] * 2
    s.log.clear()
    loss_p, grad_p = fit.shape_gradient(fit.WithShapePrior(own, s), alpha, q, r, w)
    assert s.names() == ["shape_operators", "rhs", "prior.value_gradient"]
    assert loss_p == loss + 2.5 and torch.equal(grad_p, grad + 0.25 * s.ctx.points)

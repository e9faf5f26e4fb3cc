"""autograd.render_mesh(..., forward_xyz=True) (forward mode in the grid's points) and fit.shape_step on the GPU, against
the library's own calls."""
import numpy as np
import pytest

from course5_amd import capi
from course5_amd import meshgen as mg
from tests import motion_reference as mr

pytestmark = pytest.mark.gpu
BOUNDS = (1.9, 0.1, 0.9, -0.9)
ROTS = np.array([[0.0, 0.31, 0.0], [1.0, 0.22, 1.0]])
RX, RY = 50, 37


@pytest.fixture()
def scene():
    import torch  # noqa: F401  (before the library's first call: capi's docstring)
    xyz, cells = mg.kuhn_box(3, jitter=0.2)
    alpha, q = mr.scalars(len(cells), 7)
    ctx = capi.Context(0)
    ctx.upload_grid(xyz, cells, alpha, q)
    ctx.set_image(RX, RY, BOUNDS)
    ctx.set_view(ROTS)
    yield ctx, xyz, alpha, q
    ctx.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _close(got, want, rtol=1e-12):
    """Equal to the order of the atomics (the adjoint's run-to-run bar)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.abs(want).max() > 0
    np.testing.assert_allclose(got, want, rtol=rtol, atol=1e-15 * np.abs(want).max())


def test_jvp_forward_ad_and_jacfwd_in_the_points(scene):
    import torch
    import torch.autograd.forward_ad as fwAD
    from course5_amd import autograd
    ctx, xyz, alpha, q = scene
    rng = np.random.default_rng(5)
    p, a, qq = torch.tensor(xyz), torch.tensor(alpha), torch.tensor(q)
    d = rng.normal(size=xyz.shape)
    d_alpha = rng.normal(size=len(alpha))
    frame = ctx.render()
    want = ctx.render_vertex_tangent(d)
    want_a = ctx.render_tangent(d_alpha, None)
    assert np.abs(want).max() > 0

    out, tan = torch.func.jvp(lambda x: autograd.render_mesh(ctx, x, a, qq, forward_xyz=True), (p,), (torch.tensor(d),))
    assert np.array_equal(out.cpu().numpy(), frame)
    assert tan.dtype == torch.float32 and tan.is_cuda and np.array_equal(_bits(tan.cpu().numpy()), _bits(want))

    # xyz and alpha together: the fp32 sum of the two library images
    out, tan = torch.func.jvp(lambda x, s: autograd.render_mesh(ctx, x, s, qq, forward_xyz=True), (p, a),
                              (torch.tensor(d), torch.tensor(d_alpha)))
    assert np.array_equal(_bits(tan.cpu().numpy()), _bits(want_a + want))

    # forward_ad's dual tensors
    with fwAD.dual_level():
        img = autograd.render_mesh(ctx, fwAD.make_dual(p, torch.tensor(d)), a, qq, forward_xyz=True)
        primal, tangent = fwAD.unpack_dual(img)
        assert np.array_equal(primal.cpu().numpy(), frame)
        assert np.array_equal(_bits(tangent.cpu().numpy()), _bits(want))
    with fwAD.dual_level():
        img = autograd.render_mesh(ctx, fwAD.make_dual(p, torch.tensor(d)), fwAD.make_dual(a, torch.tensor(d_alpha)), qq, forward_xyz=True)
        assert np.array_equal(_bits(fwAD.unpack_dual(img).tangent.cpu().numpy()), _bits(want_a + want))

    # jacfwd over a 5-parameter linear map theta -> xyz0 + sum theta_i D_i: ONE batched call's images
    D = rng.normal(size=(5,) + xyz.shape)
    Dt = torch.tensor(D)
    J = torch.func.jacfwd(lambda th: autograd.render_mesh(ctx, p + torch.einsum("i,ivk->vk", th, Dt), a, qq, forward_xyz=True))(
        torch.zeros(5, dtype=torch.float64))
    assert J.shape == (RY, RX, 2, 5)
    assert np.array_equal(_bits(J.movedim(-1, 0).cpu().numpy()), _bits(ctx.render_vertex_tangent(D)))


def test_reverse_mode_is_unchanged_and_second_derivatives_raise(scene):
    import torch
    from course5_amd import autograd
    ctx, xyz, alpha, q = scene
    g = np.random.default_rng(2).normal(size=(RY, RX, 2)).astype(np.float32)
    want_xyz = ctx.render_vertex_adjoint(g)
    want_a, want_q = ctx.render_adjoint(g)
    gt = torch.tensor(g, device="cuda")
    p = torch.tensor(xyz, requires_grad=True)
    a = torch.tensor(alpha, requires_grad=True)
    qq = torch.tensor(q, requires_grad=True)
    (autograd.render_mesh(ctx, p, a, qq, forward_xyz=True) * gt).sum().backward()
    _close(p.grad.numpy(), want_xyz)
    _close(a.grad.numpy(), want_a)
    _close(qq.grad.numpy(), want_q)
    a, qq = torch.tensor(alpha), torch.tensor(q)
    losses = torch.tensor(np.random.default_rng(4).normal(size=(2, RY, RX, 2)).astype(np.float32).astype(np.float64), device="cuda")
    f = lambda x: (autograd.render_mesh(ctx, x, a, qq, forward_xyz=True).to(torch.float64) * losses).sum(dim=(1, 2, 3))  # noqa: E731
    J = torch.func.jacrev(f)(torch.tensor(xyz))
    assert J.shape == (2, len(xyz), 3)
    for k in range(2):
        _close(J[k].cpu().numpy(), ctx.render_vertex_adjoint(losses[k].cpu().numpy()))
    with pytest.raises(RuntimeError, match="second derivatives are not supported"):
        torch.func.hessian(lambda x: autograd.render_mesh(ctx, x, a, qq, forward_xyz=True).sum())(torch.tensor(xyz))
    # the default is what it was: forward mode in the points raises
    with pytest.raises(RuntimeError, match="forward mode in the points is not supported"):
        torch.func.jvp(lambda x: autograd.render_mesh(ctx, x, a, qq), (torch.tensor(xyz),), (torch.ones(len(xyz), 3, dtype=torch.float64),))


def test_shape_step_recovers_displaced_interior_points():
    """One fit.shape_step on kuhn_box(4), 80 x 60, the target rendered from points whose interior is displaced by 1e-3 N(0,
    1).  The loss is checked at the FULL step d: the fp64 restatement of this scene (a dense J from
    tests/vertex_tangent_reference.py, the same CG) falls from 0.0578 to 0.0016 there (0.0165 at d / 2, 0.0335 at d / 4)."""
    import torch
    from course5_amd import autograd, fit
    xyz, cells = mg.kuhn_box(4, jitter=0.1)
    alpha, q = mr.scalars(len(cells), 9)
    rots, bounds, rx, ry = mg.view_rotations(0.13, 0.21), mg.REFERENCE_BOUNDS, 80, 60
    lo, hi = xyz.min(0), xyz.max(0)
    interior = ((xyz > lo + 1e-9) & (xyz < hi - 1e-9)).all(1)
    assert interior.sum() == 27
    true = xyz.copy()
    true[interior] += 1e-3 * np.random.default_rng(81).normal(size=(27, 3))
    a, qq = torch.tensor(alpha), torch.tensor(q)
    damping = 1e-3
    with capi.Context(0) as ctx:
        ctx.upload_grid(xyz, cells, alpha, q)
        ctx.set_image(rx, ry, bounds)
        ctx.set_view(rots)
        target = autograd.render_mesh(ctx, torch.tensor(true), a, qq).clone()

        def residual(p):
            return autograd.render_mesh(ctx, torch.tensor(p), a, qq) - target

        r = residual(xyz)
        before = 0.5 * float((r.double() ** 2).sum())
        d, models = fit.shape_step(ctx, a, qq, r, free=interior)
        assert d.shape == (len(xyz), 3) and d.dtype == torch.float64 and d.is_cuda
        d = d.cpu().numpy()
        print("shape_step models:", " ".join(f"{m:.6g}" for m in models))
        assert 1 <= len(models) <= 10
        assert all(y <= x for x, y in zip(models, models[1:])) and models[-1] < 0
        assert not d[~interior].any() and np.abs(d[interior]).max() > 0  # the fixed rows: exactly 0

        # the linear system's residual, from one independent tangent / adjoint pair: CG from zero cannot increase it
        keep = interior[:, None]
        g = ctx.render_vertex_adjoint(r.cpu().numpy()) * keep
        hd = ctx.render_vertex_adjoint(ctx.render_vertex_tangent(d)) * keep
        lin, rhs = np.linalg.norm(hd + damping * d + g), np.linalg.norm(g)
        print(f"|(H + damping I) d + g| = {lin:.6g}, |g| = {rhs:.6g}")
        assert rhs > 0 and lin <= rhs
        loss, grad = fit.shape_gradient(ctx, a, qq, r)
        assert abs(loss - before) <= 1e-12 * before
        assert float((grad.cpu().numpy() * d).sum()) < 0  # a descent direction

        after = 0.5 * float((residual(xyz + d).double() ** 2).sum())
        print(f"loss {before:.6g} -> {after:.6g}")
        assert after < before

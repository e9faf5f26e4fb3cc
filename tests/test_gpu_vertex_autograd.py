"""autograd.render_mesh (the frame as a differentiable function of the grid's points) and fit.shape_gradient on the GPU,
against the library's own calls dotted in fp64."""
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


def _close(got, want, rtol=1e-12):
    """Equal to the order of the atomics (the adjoint's run-to-run bar)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.abs(want).max() > 0
    np.testing.assert_allclose(got, want, rtol=rtol, atol=1e-15 * np.abs(want).max())


def test_backward_in_all_three_inputs_and_subsets(scene):
    import torch
    from course5_amd import autograd
    ctx, xyz, alpha, q = scene
    g = np.random.default_rng(2).normal(size=(RY, RX, 2)).astype(np.float32)
    frame = ctx.render()
    want_xyz = ctx.render_vertex_adjoint(g)
    want_a, want_q = ctx.render_adjoint(g)
    gt = torch.tensor(g, device="cuda")

    p = torch.tensor(xyz, requires_grad=True)
    a = torch.tensor(alpha, requires_grad=True)
    qq = torch.tensor(q, device="cuda", requires_grad=True)
    img = autograd.render_mesh(ctx, p, a, qq)
    assert np.array_equal(img.detach().cpu().numpy(), frame)  # (the points are the uploaded ones: nothing was sent)
    (img * gt).sum().backward()
    assert p.grad.dtype == torch.float64 and not p.grad.is_cuda and p.grad.shape == (len(xyz), 3)
    _close(p.grad.numpy(), want_xyz)
    _close(a.grad.numpy(), want_a)
    _close(qq.grad.cpu().numpy(), want_q)

    # subsets of needs_input_grad: only what is asked for is computed and returned
    p = torch.tensor(xyz, requires_grad=True)
    (autograd.render_mesh(ctx, p, torch.tensor(alpha), torch.tensor(q)) * gt).sum().backward()
    _close(p.grad.numpy(), want_xyz)
    a = torch.tensor(alpha, requires_grad=True)
    (autograd.render_mesh(ctx, torch.tensor(xyz), a, torch.tensor(q)) * gt).sum().backward()
    _close(a.grad.numpy(), want_a)

    # moved points go to the context; jacrev loops the single call
    moved = xyz + 1e-3 * np.random.default_rng(3).uniform(-1, 1, xyz.shape)
    pm = torch.tensor(moved, requires_grad=True)
    img = autograd.render_mesh(ctx, pm, torch.tensor(alpha), torch.tensor(q))
    assert np.array_equal(ctx.points, moved) and not np.array_equal(img.detach().cpu().numpy(), frame)
    (img * gt).sum().backward()
    _close(pm.grad.numpy(), ctx.render_vertex_adjoint(g))
    losses = torch.tensor(np.random.default_rng(4).normal(size=(2, RY, RX, 2)).astype(np.float32).astype(np.float64), device="cuda")
    f = lambda x: (autograd.render_mesh(ctx, x, torch.tensor(alpha), torch.tensor(q)).to(torch.float64) * losses).sum(dim=(1, 2, 3))  # noqa: E731
    J = torch.func.jacrev(f)(torch.tensor(moved))
    assert J.shape == (2, len(xyz), 3)
    for k in range(2):
        _close(J[k].cpu().numpy(), ctx.render_vertex_adjoint(losses[k].cpu().numpy()))


def test_forward_mode_in_the_points_and_second_derivatives_raise(scene):
    import torch
    from course5_amd import autograd
    ctx, xyz, alpha, q = scene
    p, a, qq = torch.tensor(xyz), torch.tensor(alpha), torch.tensor(q)
    with pytest.raises(RuntimeError, match="forward mode in the points is not supported"):
        torch.func.jvp(lambda x: autograd.render_mesh(ctx, x, a, qq), (p,), (torch.ones_like(p),))
    # tangents on the scalars go through the tangent render, as in render
    d_alpha = torch.tensor(np.random.default_rng(5).normal(size=len(alpha)))
    out, tan = torch.func.jvp(lambda s: autograd.render_mesh(ctx, p, s, qq), (a,), (d_alpha,))
    assert np.array_equal(tan.cpu().numpy(), ctx.render_tangent(d_alpha.numpy(), None))
    # forward over reverse meets the forward-mode error first; reverse over reverse the second-order one
    with pytest.raises(RuntimeError, match="forward mode in the points is not supported"):
        torch.func.hessian(lambda x: autograd.render_mesh(ctx, x, a, qq).sum())(p)
    x = torch.tensor(xyz, requires_grad=True)
    (grad,) = torch.autograd.grad(autograd.render_mesh(ctx, x, a, qq).sum(), x, create_graph=True)
    with pytest.raises(RuntimeError, match="second derivatives are not supported"):
        grad.sum().backward()
    # points replaced since the forward pass: refused, as a changed view is
    img = autograd.render_mesh(ctx, x, a, qq)
    ctx.update_points(xyz + 1e-4)
    with pytest.raises(RuntimeError, match="changed since the forward pass"):
        img.sum().backward()


def test_gradient_descent_on_displaced_interior_points_decreases_the_loss(scene):
    import torch
    from course5_amd import autograd, fit
    ctx, xyz, alpha, q = scene
    a, qq = torch.tensor(alpha), torch.tensor(q)
    target = autograd.render_mesh(ctx, torch.tensor(xyz), a, qq).clone()
    lo, hi = xyz.min(0), xyz.max(0)
    interior = ((xyz > lo + 1e-9) & (xyz < hi - 1e-9)).all(1)
    assert interior.sum() == 8
    pts = xyz.copy()
    pts[interior] += 0.02 * np.random.default_rng(6).uniform(-1, 1, (int(interior.sum()), 3))

    def loss_at(p):
        r = autograd.render_mesh(ctx, torch.tensor(p), a, qq) - target
        return 0.5 * float((r.double() ** 2).sum()), r

    loss, r = loss_at(pts)
    first, step, history = loss, None, [loss]
    for _ in range(10):
        got, grad = fit.shape_gradient(ctx, a, qq, r)
        assert abs(got - loss) <= 1e-12 * loss
        d = grad.cpu().numpy() * interior[:, None]
        if step is None:
            step = 0.01 / np.abs(d).max()  # the first trial moves a point by a hundredth of the box at the most
        while True:  # the step size by halving
            trial = pts - step * d
            new, r_new = loss_at(trial)
            if new < loss or step < 1e-30:
                break
            step *= 0.5
        assert new < loss, history
        pts, loss, r = trial, new, r_new
        history.append(loss)
    print("shape fit:", " ".join(f"{v:.6g}" for v in history))
    assert all(b < a_ for a_, b in zip(history, history[1:])) and history[-1] < first

"""autograd.render_view (the frame as a differentiable function of the view's angles) and fit.view_step on the GPU, against
the library's motion tangent images dotted in fp64."""
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
    yield ctx, alpha, q
    ctx.close()


def _close(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.abs(want).max() > 0
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (got, want)


def test_backward_jvp_jacfwd_and_jacrev_in_the_angles(scene):
    import torch
    from course5_amd import autograd
    ctx, alpha, q = scene
    a, qq = torch.tensor(alpha), torch.tensor(q, device="cuda")
    angles = torch.tensor(ROTS[:, 1].copy(), requires_grad=True)
    rng = np.random.default_rng(2)
    g = rng.normal(size=(RY, RX, 2)).astype(np.float32)
    t = rng.normal(size=2)
    imgs = ctx.render_view_tangent().astype(np.float64)  # [2, RY, RX, 2]
    frame = ctx.render()

    img = autograd.render_view(ctx, a, qq, angles)
    assert np.array_equal(img.detach().cpu().numpy(), frame)
    (img * torch.tensor(g, device="cuda")).sum().backward()
    assert angles.grad.dtype == torch.float64 and not angles.grad.is_cuda
    _close(angles.grad.numpy(), (imgs * g.astype(np.float64)).sum(axis=(1, 2, 3)))

    f = lambda th: autograd.render_view(ctx, a, qq, th)  # noqa: E731
    out, tan = torch.func.jvp(f, (angles.detach(),), (torch.tensor(t),))
    assert np.array_equal(out.cpu().numpy(), frame)
    # one affine field: sum_i t_i field_i
    want = ctx.render_motion_tangent(t.reshape(1, -1) @ ctx.view_fields())[0]
    assert np.array_equal(tan.cpu().numpy(), want)
    both = (t[0] * imgs[0] + t[1] * imgs[1])
    assert np.abs(tan.cpu().numpy() - both).max() <= 1e-5 * np.abs(both).max()

    J = torch.func.jacfwd(f)(angles.detach())  # [RY, RX, 2, 2]: one batched call
    assert np.array_equal(J.cpu().numpy(), np.moveaxis(ctx.render_view_tangent(), 0, -1))
    # float32 values held as float64: the frame is float32, so the cast's backward hands render_view float32 cotangents
    losses = torch.tensor(rng.normal(size=(3, RY, RX, 2)).astype(np.float32).astype(np.float64), device="cuda")
    Jr = torch.func.jacrev(lambda th: (f(th).to(torch.float64) * losses).sum(dim=(1, 2, 3)))(angles.detach())  # [3, 2]
    _close(Jr.cpu().numpy(), np.einsum("kyxc,nyxc->kn", losses.cpu().numpy(), imgs))


def test_scalar_gradients_are_renders_own_and_second_derivatives_raise(scene):
    import torch
    from course5_amd import autograd
    ctx, alpha, q = scene
    g = torch.tensor(np.random.default_rng(3).normal(size=(RY, RX, 2)).astype(np.float32), device="cuda")
    grads = []
    for fn in (lambda a, b: autograd.render_view(ctx, a, b, torch.tensor(ROTS[:, 1].copy())), lambda a, b: autograd.render(ctx, a, b)):
        a = torch.tensor(alpha, requires_grad=True)
        qq = torch.tensor(q, requires_grad=True)
        (fn(a, qq) * g).sum().backward()
        grads.append((a.grad.numpy(), qq.grad.numpy()))
    for got, want in zip(grads[0], grads[1]):
        assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()  # (the adjoint's atomics: DESIGN 4.6's bar)
    a, qq = torch.tensor(alpha), torch.tensor(q)
    f = lambda th: autograd.render_view(ctx, a, qq, th).sum()  # noqa: E731
    with pytest.raises(RuntimeError, match="second derivatives are not supported"):
        torch.func.hessian(f)(torch.tensor(ROTS[:, 1].copy()))
    th = torch.tensor(ROTS[:, 1].copy(), requires_grad=True)
    (grad,) = torch.autograd.grad(f(th), th, create_graph=True)
    with pytest.raises(RuntimeError, match="second derivatives are not supported"):
        grad.sum().backward()
    # a changed view is refused, as by render
    img = autograd.render_view(ctx, a, qq, th)
    ctx.set_view(ROTS)
    with pytest.raises(RuntimeError, match="changed since the forward pass"):
        img.sum().backward()


def test_view_step_moves_towards_the_true_angles(scene):
    import torch
    from course5_amd import autograd, fit
    ctx, alpha, q = scene
    a, qq = torch.tensor(alpha), torch.tensor(q)
    true = torch.tensor(ROTS[:, 1].copy())
    target = autograd.render_view(ctx, a, qq, true).clone()
    angles = true + torch.tensor([0.01, -0.01])
    residual = autograd.render_view(ctx, a, qq, angles) - target
    loss0 = float((residual.double() ** 2).sum())
    d, model = fit.view_step(ctx, a, qq, angles, residual)
    new = angles + d.cpu()
    loss1 = float(((autograd.render_view(ctx, a, qq, new) - target).double() ** 2).sum())
    err0, err1 = float((angles - true).abs().max()), float((new - true).abs().max())
    print(f"view_step: loss {loss0:.6g} -> {loss1:.6g} (model {model:.6g}), angle error {err0:.3g} -> {err1:.3g} rad")
    assert model < 0
    assert loss1 < loss0 and err1 < err0

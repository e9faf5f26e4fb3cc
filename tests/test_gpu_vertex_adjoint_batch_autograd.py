"""autograd.render_mesh under vmap: a batch of cotangents on the image (torch.func.jacrev, vmap over a vjp) is ONE batched
vertex adjoint render (c5_render_vertex_adjoint_batch_device), equal to the stacked single calls at the run-to-run bar
(rtol 1e-12, atol 1e-15 x max: fp64 atomics in another order); a plain backward stays one single call."""
import numpy as np
import pytest

from course5_amd import capi
from course5_amd import meshgen as mg
from tests import motion_reference as mr

pytestmark = pytest.mark.gpu
BOUNDS = (1.9, 0.1, 0.9, -0.9)
ROTS = np.array([[0.0, 0.31, 0.0], [1.0, 0.22, 1.0]])
RX, RY = 25, 19


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


def _close(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.abs(want).max() > 0
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-15 * np.abs(want).max())


def _count_calls(ctx):
    """Wraps the two device forms on the instance; returns the dict of their call counts."""
    calls = {"single": 0, "batch": 0}
    single, batch = ctx.render_vertex_adjoint_device, ctx.render_vertex_adjoint_batch_device

    def counted_single(*a, **k):
        calls["single"] += 1
        return single(*a, **k)

    def counted_batch(*a, **k):
        calls["batch"] += 1
        return batch(*a, **k)

    ctx.render_vertex_adjoint_device, ctx.render_vertex_adjoint_batch_device = counted_single, counted_batch
    return calls


def _losses(k, seed):
    return np.random.default_rng(seed).normal(size=(k, RY, RX, 2)).astype(np.float32)


@pytest.mark.parametrize("k", [3, 9])
def test_jacrev_is_one_batched_call(scene, k):
    import torch
    from course5_amd import autograd
    ctx, xyz, alpha, q = scene
    g = _losses(k, 4)
    want = np.stack([ctx.render_vertex_adjoint(gk) for gk in g])
    losses = torch.tensor(g.astype(np.float64), device="cuda")
    f = lambda x: (autograd.render_mesh(ctx, x, torch.tensor(alpha), torch.tensor(q)).to(torch.float64) * losses).sum(dim=(1, 2, 3))  # noqa: E731
    calls = _count_calls(ctx)
    J = torch.func.jacrev(f)(torch.tensor(xyz))
    assert calls == {"single": 0, "batch": 1}
    assert J.shape == (k, len(xyz), 3)
    for j in range(k):
        _close(J[j].cpu().numpy(), want[j])


def test_vmap_over_the_vjp_is_one_batched_call(scene):
    import torch
    from course5_amd import autograd
    ctx, xyz, alpha, q = scene
    g = _losses(5, 5)
    want = np.stack([ctx.render_vertex_adjoint(gk) for gk in g])
    _img, vjp = torch.func.vjp(lambda x: autograd.render_mesh(ctx, x, torch.tensor(alpha), torch.tensor(q)), torch.tensor(xyz))
    calls = _count_calls(ctx)
    (got,) = torch.func.vmap(vjp)(torch.tensor(g, device="cuda"))
    assert calls == {"single": 0, "batch": 1}
    assert got.shape == (5, len(xyz), 3)
    for j in range(5):
        _close(got[j].cpu().numpy(), want[j])


def test_a_plain_backward_is_still_one_single_call(scene):
    import torch
    from course5_amd import autograd
    ctx, xyz, alpha, q = scene
    g = _losses(1, 6)[0]
    want = ctx.render_vertex_adjoint(g)
    p = torch.tensor(xyz, requires_grad=True)
    img = autograd.render_mesh(ctx, p, torch.tensor(alpha), torch.tensor(q))
    calls = _count_calls(ctx)
    (img * torch.tensor(g, device="cuda")).sum().backward()
    assert calls == {"single": 1, "batch": 0}
    _close(p.grad.numpy(), want)


def test_forward_mode_and_second_order_errors_are_unchanged(scene):
    import torch
    from course5_amd import autograd
    ctx, xyz, alpha, q = scene
    p, a, qq = torch.tensor(xyz), torch.tensor(alpha), torch.tensor(q)
    with pytest.raises(RuntimeError, match="forward mode in the points is not supported"):
        torch.func.jvp(lambda x: autograd.render_mesh(ctx, x, a, qq), (p,), (torch.ones_like(p),))
    with pytest.raises(RuntimeError, match="forward mode in the points is not supported"):
        torch.func.hessian(lambda x: autograd.render_mesh(ctx, x, a, qq).sum())(p)
    x = torch.tensor(xyz, requires_grad=True)
    (grad,) = torch.autograd.grad(autograd.render_mesh(ctx, x, a, qq).sum(), x, create_graph=True)
    with pytest.raises(RuntimeError, match="second derivatives are not supported"):
        grad.sum().backward()

"""autograd.shape_prior, fit.ShapePrior / fit.WithShapePrior in fit.shape_gradient and fit.shape_step, and
fit.shape_line_search, on the GPU.

The fit's scene follows tests/test_gpu_prior_fit.py: kuhn_box(4) (384 cells, 125 points) under view_rotations(0.1, 0.07, 0.05),
a 13 x 21 image whose bounds are cut so that a part of the grid is crossed by no ray - its points are the null space the
prior is there for.  The rest shape is the box; the points the context holds are the box with the surface of the crossed
part (the crossed points that share a cell with an uncrossed one) displaced by 5 % of the cell size.  Which cells are
crossed comes from the restatement's segment lists on the CPU.  Contexts run with "vertex_exact" 1 wherever bits are
compared."""
import math

import numpy as np
import pytest
import torch

from course5_amd import autograd, capi, fit
from course5_amd import meshgen as mg
from tests import adjoint_reference as ar
from tests import shape_prior_reference as sr

pytestmark = pytest.mark.gpu
EPS, K = sr.EPS, sr.K
VIEW = mg.view_rotations(0.1, 0.07, 0.05)
RX, RY = 13, 21
BOUNDS = (1.2, 0.5, 0.2, -0.6)  # {x_max, x_min, y_max, y_min}: the box projects onto [0.39, 1.61] x [-0.72, 0.72]
LAM, KAPPA = 1e-2, 1.5


def _bits(a):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else a
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


# ---- autograd.shape_prior ------------------------------------------------------------------------------------------------------
class _Small:
    def __init__(self):
        self.X, self.cells = mg.kuhn_box(4, jitter=0.1)
        self.n_pts = len(self.X)
        self.vert = sr.welded_cells(self.X, self.cells)
        self.x = sr.displaced(self.X, self.vert)
        self.v = np.random.default_rng(3).normal(size=(self.n_pts, 3))

    def ctx(self):
        ctx = capi.Context(0)
        ctx.upload_grid(self.X, self.cells, np.ones(len(self.cells)), np.ones(len(self.cells)))
        assert ctx.shape_prior_rest(self.X) == 0
        return ctx


@pytest.mark.parametrize("stream", ["default", "side"])
@pytest.mark.parametrize("energy", [sr.DIRICHLET, sr.NEO_HOOKEAN])
def test_autograd_shape_prior(energy, stream):
    """On torch's default (null) stream every call is waited for; on a stream of torch's own the calls are only enqueued and
    that stream orders them with the torch operations around them.  The same bits either way."""
    s = _Small()
    P = capi.ShapePrior(energy, 0.75, KAPPA)
    side = torch.cuda.Stream() if stream == "side" else None
    with s.ctx() as ctx:
        value, _n, grad = ctx.shape_prior_gradient(P, s.x)
        hv = ctx.shape_prior_product(P, s.x, s.v)
        with torch.cuda.stream(side):
            _autograd_checks(ctx, s, P, value, grad, hv, waits=side is None)
        torch.cuda.synchronize()
        ctx.set_stream(0)


def _autograd_checks(ctx, s, P, value, grad, hv, waits):
    x = _dev(s.x).requires_grad_()
    v = _dev(s.v)
    calls = []
    for name in ("shape_prior_gradient_device", "shape_prior_product_device", "synchronize"):
        inner = getattr(ctx, name)
        setattr(ctx, name, lambda *args, _inner=inner, _name=name: (calls.append(_name), _inner(*args))[1])

    def made(*names):
        """The library calls since the last look: each followed by a wait on the null stream, by none on a real one."""
        got, want = list(calls), [n for name in names for n in ((name, "synchronize") if waits else (name,))]
        del calls[:]
        return got == want

    def f(x_):
        return autograd.shape_prior(ctx, x_, P)

    def np_(t):
        return t.detach().cpu().numpy()

    # torch.autograd.grad: one c5_shape_prior_gradient_device, and no further call
    r = f(x)
    assert r.dtype == torch.float64 and r.shape == () and float(r.detach()) == value
    (g,) = torch.autograd.grad(r, (x,))
    assert made("shape_prior_gradient_device")
    assert _same(np_(g), grad)
    # reverse over reverse: one c5_shape_prior_product_device
    (g,) = torch.autograd.grad(f(x), (x,), create_graph=True)
    (h,) = torch.autograd.grad((g * v).sum(), (x,))
    assert made("shape_prior_gradient_device", "shape_prior_product_device")
    assert _same(np_(h), hv)
    # torch.func
    grad_f = torch.func.grad(f)
    g = grad_f(x.detach())
    assert made("shape_prior_gradient_device")
    assert _same(np_(g), grad)
    g, h = torch.func.jvp(grad_f, (x.detach(),), (v,))
    assert made("shape_prior_gradient_device", "shape_prior_product_device")
    assert _same(np_(g), grad) and _same(np_(h), hv)
    # the value's own jvp is grad R . v, and reverse over forward finds the Hessian product behind it
    r, r_dot = torch.func.jvp(f, (x.detach(),), (v,))
    assert made("shape_prior_gradient_device")
    assert abs(float(r_dot) - float((s.v * grad).sum())) <= (3 * s.n_pts + 8) * EPS * np.abs(s.v * grad).sum()
    h = torch.func.grad(lambda x_: torch.func.jvp(f, (x_,), (v,))[1])(x.detach())
    assert made("shape_prior_gradient_device", "shape_prior_product_device")
    assert _same(np_(h), hv)
    # what is not there raises, in the shape prior's own words: forward over forward, beyond the second derivative, vmap
    with pytest.raises(RuntimeError, match=r"autograd\.shape_prior: torch\.func\.jvp of a jvp"):
        torch.func.jvp(lambda a_: torch.func.jvp(f, (a_,), (v,))[1], (x.detach(),), (v,))
    (g,) = torch.autograd.grad(f(x), (x,), create_graph=True)
    (h,) = torch.autograd.grad((g * v).sum(), x, create_graph=True)
    with pytest.raises(RuntimeError, match=r"autograd\.shape_prior: derivatives beyond the second are not supported"):
        torch.autograd.grad(h.sum(), x)
    with pytest.raises(RuntimeError, match=r"autograd\.shape_prior: vmap"):
        torch.func.vmap(f)(torch.stack([x.detach(), x.detach()]))


def test_fit_shape_prior_is_the_c_calls():
    s = _Small()
    with s.ctx() as ctx:
        for energy, name in ((sr.DIRICHLET, "dirichlet"), (sr.NEO_HOOKEAN, "neo_hookean")):
            P = fit.ShapePrior(ctx, 0.75, energy=name, kappa=KAPPA, rest=s.X)
            assert P.n_degenerate == 0
            raw = capi.ShapePrior(energy, 0.75, KAPPA)
            value, _n, grad = ctx.shape_prior_gradient(raw, s.x)
            got_value, got_grad = P.value_gradient(torch.tensor(s.x))
            assert float(got_value[0]) == value and _same(got_grad, grad)
            assert _same(P.product(s.x, s.v), ctx.shape_prior_product(raw, s.x, s.v))
            assert _same(P.diagonal(s.x), ctx.shape_prior_diagonal(raw, s.x))
            ratio, n_inv = P.quality(s.x)
            want = ctx.shape_prior_quality(s.x)
            assert _same(ratio, want[0]) and n_inv == want[1] == 0 and P.feasible(s.x)
        # rest=False keeps the rest shape the context has; rest=None takes the points it holds
        ctx.update_points(s.x)
        kept = fit.ShapePrior(ctx, 0.75, kappa=KAPPA, rest=False)
        assert float(kept.value_gradient(s.x)[0][0]) == value
        taken = fit.ShapePrior(ctx, 0.75, kappa=KAPPA, rest=None)
        v0, s0 = sr.value(*ctx.shape_prior_rest_data()[:2], s.vert, s.x, sr.NEO_HOOKEAN, KAPPA, 0.75, with_scale=True)
        assert abs(float(taken.value_gradient(s.x)[0][0])) <= K * EPS * s0
        ctx.set_stream(0)


# ---- shape_line_search -----------------------------------------------------------------------------------------------------------------
def test_shape_line_search_backs_off_until_no_cell_is_inverted():
    s = _Small()
    with s.ctx() as ctx:
        P = fit.ShapePrior(ctx, 1.0, rest=False)
        # a direction that pushes one interior point far through its neighbours at t = 1
        lo, hi = s.X.min(0), s.X.max(0)
        inner = np.flatnonzero(((s.X > lo + 1e-9) & (s.X < hi - 1e-9)).all(1))
        d = np.zeros_like(s.X)
        d[inner[13]] = (0.9, -0.7, 0.8)
        assert P.quality(s.X + d)[1] > 0 and P.feasible(s.X)
        calls = []
        inner_quality = ctx.shape_prior_quality_device
        ctx.shape_prior_quality_device = lambda *a: (calls.append("quality"), inner_quality(*a))[1]
        rendered = ctx.frame_state
        t = fit.shape_line_search(ctx, P, s.X, torch.tensor(d))
        assert 0.0 < t < 1.0 and t == 0.5 ** (len(calls) - 1) and len(calls) >= 2
        ratio, n_inv = P.quality(s.X + t * d)
        assert n_inv == 0 and float(ratio.min()) > 0 and P.quality(s.X + 2 * t * d)[1] > 0  # (the step before it was refused)
        assert ctx.frame_state == rendered  # (no render, no update_points)
        assert fit.shape_line_search(ctx, P, s.X, 0.01 * d) == 1.0
        with pytest.raises(ValueError):
            fit.shape_line_search(capi.Context.__new__(capi.Context), P, s.X, d)
        ctx.set_stream(0)


# ---- the fit ---------------------------------------------------------------------------------------------------------------------------
class _Scene:
    def __init__(self):
        self.X, self.cells = mg.kuhn_box(4)
        self.n, self.n_pts = len(self.cells), len(self.X)
        rng = np.random.default_rng(21)
        self.alpha, self.q = rng.uniform(0.5, 2.0, self.n), rng.uniform(0.2, 1.0, self.n)
        self.weight = np.abs(rng.normal(size=(RY, RX, 2))).astype(np.float32) + 0.1
        cells = np.asarray(self.cells, dtype=np.int64)

        def crossed_points(xyz):
            _pix, cell, _zh, _dz = ar.segment_lists(xyz, self.cells, VIEW, RX, RY, BOUNDS)
            crossed = np.zeros(self.n, dtype=bool)
            crossed[np.unique(cell)] = True
            pts = np.zeros(self.n_pts, dtype=bool)
            pts[np.unique(cells[crossed])] = True
            return crossed, pts

        crossed, pts = crossed_points(self.X)
        # the surface of the crossed part: crossed points that share a cell with an uncrossed point
        mixed = (~pts[cells]).any(axis=1) & pts[cells].any(axis=1)
        surface = np.zeros(self.n_pts, dtype=bool)
        surface[np.unique(cells[mixed])] = True
        surface &= pts
        h = sr.local_size(self.X, cells)
        push = np.stack([np.sin(5.0 * self.X[:, 1] + 1.0), np.cos(4.0 * self.X[:, 2]), np.sin(3.0 * self.X[:, 0] + 2.0)], axis=1) / math.sqrt(3.0)
        self.cur = self.X + np.where(surface[:, None], 0.05 * h[:, None] * push, 0.0)
        self.surface = surface
        # what the rays see of the points the context holds
        self.crossed, self.seen = crossed_points(self.cur)
        touched = (surface[cells]).any(axis=1)
        beside = np.zeros(self.n_pts, dtype=bool)
        beside[np.unique(cells[touched])] = True
        self.beside = beside & ~self.seen  # no cell of theirs is crossed, and they share a cell with a displaced point
        with self.ctx() as ctx:
            target = ctx.render()  # (the rest shape's frame)
            ctx.update_points(self.cur)
            self.residual = ctx.render() - target
        assert np.abs(self.residual).max() > 0

    def ctx(self, exact=True, place=None, points=None):
        ctx = capi.Context(0)
        ctx.upload_grid(self.X, self.cells, self.alpha, self.q)
        ctx.set_image(RX, RY, BOUNDS)
        ctx.set_view(VIEW)
        if place:
            ctx.set_row_range(*place)
        ctx.set_option("vertex_exact", 1 if exact else 0)
        if points is not None:
            ctx.update_points(points)
        return ctx

    def tensors(self):
        return torch.tensor(self.alpha), torch.tensor(self.q), torch.tensor(self.residual), torch.tensor(self.weight)


@pytest.fixture(scope="module")
def scene():
    return _Scene()


def test_the_scene_leaves_points_unseen(scene):
    print(f"{(~scene.seen).sum()} of {scene.n_pts} points have no crossed cell, {scene.surface.sum()} are displaced, "
          f"{scene.beside.sum()} unseen points share a cell with a displaced one")
    assert (~scene.seen).sum() >= 10 and scene.surface.sum() >= 5 and scene.beside.sum() >= 5
    assert not (scene.surface & ~scene.seen).any()


def test_without_a_prior_unseen_points_stay_put_and_with_one_they_move(scene):
    alpha, q, residual, weight = scene.tensors()
    with scene.ctx(points=scene.cur) as ctx:
        # the control: today's behaviour
        d0, models0 = fit.shape_step(ctx, alpha, q, residual, weight, iters=10)
        d0 = d0.cpu().numpy()
        assert (d0[~scene.seen] == 0).all() and np.abs(d0[scene.seen]).max() > 0 and len(models0) > 1
        loss0, grad0 = fit.shape_gradient(ctx, alpha, q, residual, weight)
        # with the prior (the rest shape: the box, given explicitly - the context holds the displaced points)
        P = fit.ShapePrior(ctx, LAM, kappa=KAPPA, rest=scene.X)
        d, models = fit.shape_step(fit.WithShapePrior(ctx, P), alpha, q, residual, weight, iters=10)
        d = d.cpu().numpy()
        assert (d[scene.beside] != 0).any(axis=1).all()
        assert len(models) > 1 and all(b <= a for a, b in zip(models, models[1:])) and models[0] < 0
        assert np.isfinite(d).all()
        # the loss and the gradient gain R and grad R at the points the context holds
        loss, grad = fit.shape_gradient(fit.WithShapePrior(ctx, P), alpha, q, residual, weight)
        value, _n, g = ctx.shape_prior_gradient(P.prior, scene.cur)
        assert value > 0 and loss == loss0 + value and _same(grad, grad0.cpu().numpy() + g)
        # the same bits again, and the context's own step is untouched by the prior's having been there
        d_again, models_again = fit.shape_step(fit.WithShapePrior(ctx, P), alpha, q, residual, weight, iters=10)
        assert _same(d_again, d) and models_again == models
        d1, models1 = fit.shape_step(ctx, alpha, q, residual, weight, iters=10)
        assert _same(d1, d0) and models1 == models0
        # the step does not invert a cell, and the line search says so
        assert fit.shape_line_search(ctx, P, scene.cur, d) == 1.0
        ctx.set_stream(0)


def test_the_first_cg_iterate_rebuilt_from_public_calls(scene):
    """x_1 = (r^T r / p^T A p) p with r = -(J^T W r + grad R), p = r and A = J^T W J + damping I + Hess R; against
    shape_step's, 1e-10 of its norm (the two dot products over 375 terms are taken in another order: n x 2^-52 is 1e-13)."""
    alpha, q, residual, weight = scene.tensors()
    damping = 1e-3
    with scene.ctx(points=scene.cur) as ctx:
        P = fit.ShapePrior(ctx, LAM, kappa=KAPPA, rest=scene.X)
        got, models = fit.shape_step(fit.WithShapePrior(ctx, P), alpha, q, residual, weight, damping=damping, iters=1)
        got = got.cpu().numpy()
        g = ctx.render_vertex_adjoint(scene.residual * scene.weight) + ctx.shape_prior_gradient(P.prior, scene.cur)[2]
        r = -g
        hp = autograd.vertex_gn_product(ctx, alpha, q, torch.tensor(r), weight).cpu().numpy() + ctx.shape_prior_product(P.prior, scene.cur, r)
        ap = hp + damping * r
        step = (r * r).sum() / (r * ap).sum()
        want = step * r
        err = np.linalg.norm(got - want) / np.linalg.norm(want)
        print(f"first iterate: relative difference {err:.3g}")
        assert err <= 1e-10 and len(models) == 1
        assert models[0] == pytest.approx(0.5 * (want * (step * ap)).sum() + (want * g).sum(), rel=1e-9)
        ctx.set_stream(0)


def test_row_shards_get_the_prior_once(scene):
    alpha, q, residual, weight = scene.tensors()
    with scene.ctx(points=scene.cur) as single:
        P = fit.ShapePrior(single, LAM, kappa=KAPPA, rest=scene.X)
        want, want_models = fit.shape_step(fit.WithShapePrior(single, P), alpha, q, residual, weight, iters=4)
        want_loss, want_grad = fit.shape_gradient(fit.WithShapePrior(single, P), alpha, q, residual, weight)
        doubled, _m = fit.shape_step(fit.WithShapePrior(single, fit.ShapePrior(single, 2 * LAM, kappa=KAPPA, rest=False)), alpha, q, residual,
                                     weight, iters=4)
        want, want_grad, doubled = want.cpu().numpy(), want_grad.cpu().numpy(), doubled.cpu().numpy()
        single.set_stream(0)
    assert not _same(doubled, want) and np.abs(doubled - want).max() > 1e-6 * np.abs(want).max()
    parts = [(scene.ctx(place=(b, n), points=scene.cur), np.arange(b, b + n)) for b, n in ((0, 13), (13, 8))]
    try:
        shards = fit.RowShards(parts)
        Ps = fit.ShapePrior(parts[0][0], LAM, kappa=KAPPA, rest=scene.X)
        got, models = fit.shape_step(fit.WithShapePrior(shards, Ps), alpha, q, residual, weight, iters=4)
        assert _same(got, want) and models == want_models
        loss, grad = fit.shape_gradient(fit.WithShapePrior(shards, Ps), alpha, q, residual, weight)
        assert loss == want_loss and _same(grad, want_grad)
    finally:
        for c, _rows in parts:
            c.set_stream(0)
            c.close()

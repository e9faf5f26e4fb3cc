"""fit.gn_step / fit.newton_step with a smoothness prior (fit.SmoothnessPrior, fit.WithPrior).

The scene: kuhn_box(4) (384 cells) under view_rotations(0.1, 0.07, 0.05), a 13 x 21 image whose bounds are cut so that a
third of the cells is crossed by no ray - the null space the prior is there for.  Which cells those are comes from the
restatement's segment lists on the CPU.  Contexts run with "exact_sums" 1 wherever bits are compared."""
import numpy as np
import pytest
import torch

from course5_amd import autograd, capi, fit
from course5_amd import meshgen as mg
from tests import adjoint_reference as ar
from tests import prior_reference as pr

pytestmark = pytest.mark.gpu
VIEW = mg.view_rotations(0.1, 0.07, 0.05)
RX, RY = 13, 21
BOUNDS = (1.2, 0.5, 0.2, -0.6)  # {x_max, x_min, y_max, y_min}: the box projects onto [0.39, 1.61] x [-0.72, 0.72]
LAMBDA_Q = 1e-2


class _Scene:
    def __init__(self):
        self.xyz, self.cells = mg.kuhn_box(4)
        self.n = n = len(self.cells)
        rng = np.random.default_rng(21)
        self.alpha, self.q = rng.uniform(0.5, 2.0, n), rng.uniform(0.2, 1.0, n)
        _pix, cell, _zh, _dz = ar.segment_lists(self.xyz, self.cells, VIEW, RX, RY, BOUNDS)
        self.crossed = np.zeros(n, dtype=bool)
        self.crossed[np.unique(cell)] = True
        self.adj = pr.adjacency(self.xyz, self.cells)
        self.weight = np.abs(rng.normal(size=(RY, RX, 2))).astype(np.float32) + 0.1
        with self.ctx() as ctx:
            ctx.update_scalars(self.alpha, self.q * (1.0 + 0.2 * rng.normal(size=n)))
            target = ctx.render()
            ctx.update_scalars(self.alpha, self.q)
            self.residual = ctx.render() - target
        assert np.abs(self.residual).max() > 0

    def ctx(self, exact=True, place=None):
        ctx = capi.Context(0)
        ctx.upload_grid(self.xyz, self.cells, self.alpha, self.q)
        ctx.set_image(RX, RY, BOUNDS)
        ctx.set_view(VIEW)
        if place:
            ctx.set_row_range(*place)
        if exact:
            ctx.set_option("exact_sums", 1)
        return ctx

    def tensors(self):
        return torch.tensor(self.alpha), torch.tensor(self.q), torch.tensor(self.residual), torch.tensor(self.weight)


@pytest.fixture(scope="module")
def scene():
    return _Scene()


def _q_step(step):
    (d_alpha, d_q), models = step
    assert d_alpha is None
    return d_q.cpu().numpy(), models


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def test_the_scene_leaves_cells_uncrossed(scene):
    share = 1.0 - scene.crossed.mean()
    print(f"{share:.1%} of the cells are crossed by no ray")
    assert 0.10 <= share <= 0.60


def test_without_a_prior_uncrossed_cells_stay_put_and_with_one_they_move(scene):
    alpha, q, residual, weight = scene.tensors()
    with scene.ctx() as ctx:
        # 1. the control: today's behaviour
        d, models = _q_step(fit.gn_step(ctx, alpha, q, residual, weight, fit=("q",), iters=10))
        assert (d[~scene.crossed] == 0).all() and np.abs(d[scene.crossed]).max() > 0 and len(models) > 1
        # 6. prior=None is the call that omits it, bit for bit
        d_none, models_none = _q_step(fit.gn_step(ctx, alpha, q, residual, weight, fit=("q",), iters=10, prior=None))
        assert _same(d_none, d) and models_none == models
        # 2. a quadratic prior on q
        P = fit.SmoothnessPrior(ctx, lambda_q=LAMBDA_Q)
        d, models = _q_step(fit.gn_step(ctx, alpha, q, residual, weight, fit=("q",), iters=10, prior=P))
        beside = ~scene.crossed & (scene.crossed[np.where(scene.adj >= 0, scene.adj, 0)] & (scene.adj >= 0)).any(axis=1)
        assert beside.sum() > 10 and (d[beside] != 0).all()
        assert len(models) == 10 and all(b <= a for a, b in zip(models, models[1:])) and models[0] < 0
        # the same through the context, and never twice
        d_with, models_with = _q_step(fit.gn_step(fit.WithPrior(ctx, P), alpha, q, residual, weight, fit=("q",), iters=10))
        assert _same(d_with, d) and models_with == models
        with pytest.raises(ValueError, match="once"):
            fit.gn_step(fit.WithPrior(ctx, P), alpha, q, residual, weight, prior=P)
        # a field named in fit whose lambda is 0 gets no term; a field with a lambda that is not fitted does not enter
        (da, dq), _m = fit.gn_step(ctx, alpha, q, residual, weight, fit=("alpha", "q"), iters=3, prior=P)
        (da0, dq0), _m = fit.gn_step(ctx, alpha, q, residual, weight, fit=("alpha", "q"), iters=3)
        assert (da.cpu().numpy()[~scene.crossed] == 0).all() and not _same(dq.cpu().numpy(), dq0.cpu().numpy())
        Pa = fit.SmoothnessPrior(ctx, lambda_alpha=1.0)
        d_a, models_a = _q_step(fit.gn_step(ctx, alpha, q, residual, weight, fit=("q",), iters=10, prior=Pa))
        assert _same(d_a, d_none) and models_a == models_none


def test_one_iteration_is_the_first_cg_iterate_rebuilt_from_public_calls(scene):
    """x_1 = (r^T z / p^T A p) p with r = -(J^T W r + grad P), z = r / (diag H + diag Hess P), p = z and A = H + damping
    diag H + Hess P; against gn_step's, 1e-10 of its norm (the two dot products over 384 terms are taken in another order:
    n x 2^-52 is 1e-13; the adjoint's atomics less)."""
    alpha, q, residual, weight = scene.tensors()
    damping = 0.1
    with scene.ctx(exact=False) as ctx:
        P = fit.SmoothnessPrior(ctx, lambda_q=LAMBDA_Q)
        got, models = _q_step(fit.gn_step(ctx, alpha, q, residual, weight, fit=("q",), damping=damping, iters=1, prior=P))
        prior = P.prior
        g = ctx.render_adjoint(scene.residual * scene.weight)[1] + ctx.prior_gradient(prior, None, scene.q)[2]
        d = autograd.gn_diagonal(ctx, alpha, q, weight)[1].cpu().numpy()
        dm = d + ctx.prior_diagonal(prior, None, scene.q)[1]
        r = -g
        z = np.where(dm > 0, r / np.where(dm > 0, dm, 1.0), 0.0)
        hp = autograd.gn_product(ctx, alpha, q, None, torch.tensor(z), weight)[1].cpu().numpy() + ctx.prior_product(prior, None, scene.q, None, z)[1]
        want = (r @ z) / (z @ (hp + damping * d * z)) * z
        err = np.linalg.norm(got - want) / np.linalg.norm(want)
        print(f"first iterate: relative difference {err:.3g}")
        assert err <= 1e-10
        assert models[0] == pytest.approx(0.5 * want @ ((r @ z) / (z @ (hp + damping * d * z)) * hp) + want @ g, rel=1e-9)


def test_row_shards_get_the_prior_once(scene):
    alpha, q, residual, weight = scene.tensors()
    with scene.ctx() as single:
        P = fit.SmoothnessPrior(single, lambda_q=LAMBDA_Q)
        want, want_models = _q_step(fit.gn_step(single, alpha, q, residual, weight, fit=("q",), iters=4, prior=P))
        doubled, _m = _q_step(fit.gn_step(single, alpha, q, residual, weight, fit=("q",), iters=4,
                                          prior=fit.SmoothnessPrior(single, lambda_q=2 * LAMBDA_Q)))
    assert not _same(doubled, want) and np.abs(doubled - want).max() > 1e-6 * np.abs(want).max()
    parts = [(scene.ctx(exact=False, place=(b, n)), np.arange(b, b + n)) for b, n in ((0, 13), (13, 8))]
    try:
        shards = fit.RowShards(parts)
        Ps = fit.SmoothnessPrior(parts[0][0], lambda_q=LAMBDA_Q)
        got, models = _q_step(fit.gn_step(shards, alpha, q, residual, weight, fit=("q",), iters=4, prior=Ps))
        assert _same(got, want) and models == want_models
    finally:
        for c, _rows in parts:
            c.close()


def test_newton_step_with_a_pseudo_huber_prior(scene):
    alpha, q, residual, weight = scene.tensors()
    with scene.ctx() as ctx:
        P = fit.SmoothnessPrior(ctx, lambda_alpha=1e-2, lambda_q=LAMBDA_Q, penalty="pseudo_huber", delta_alpha=0.3, delta_q=0.1)
        (da, dq), models = fit.newton_step(fit.WithPrior(ctx, P), alpha, q, residual, weight, fit=("alpha", "q"), iters=5)
        assert models and models[0] < 0
        assert np.isfinite(da.cpu().numpy()).all() and np.isfinite(dq.cpu().numpy()).all()
        (da0, dq0), _m = fit.newton_step(ctx, alpha, q, residual, weight, fit=("alpha", "q"), iters=5)
        assert (dq0.cpu().numpy()[~scene.crossed] == 0).all() and (dq.cpu().numpy()[~scene.crossed] != 0).any()


def test_a_step_on_a_stream_of_torch_s_own_is_the_default_stream_s(scene):
    """On torch's default (null) stream the prior's calls are waited for; under a torch.cuda.Stream they are only enqueued,
    between the torch operations of CG on that stream.  The same bits."""
    alpha, q, residual, weight = scene.tensors()
    with scene.ctx() as ctx:
        P = fit.SmoothnessPrior(ctx, lambda_alpha=1e-2, lambda_q=LAMBDA_Q, penalty="pseudo_huber", delta_alpha=0.3, delta_q=0.1)
        (da, dq), models = fit.gn_step(ctx, alpha, q, residual, weight, fit=("alpha", "q"), iters=5, prior=P)
        want = (da.cpu().numpy(), dq.cpu().numpy())
        with torch.cuda.stream(torch.cuda.Stream()):
            (da, dq), models_side = fit.gn_step(ctx, alpha, q, residual, weight, fit=("alpha", "q"), iters=5, prior=P)
            got = (da.cpu().numpy(), dq.cpu().numpy())
        torch.cuda.synchronize()
        ctx.set_stream(0)
        assert _same(got[0], want[0]) and _same(got[1], want[1]) and models_side == models and len(models) == 5

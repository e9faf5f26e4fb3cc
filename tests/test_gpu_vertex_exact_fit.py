"""A shape fit on exact vertex adjoint sums (option "vertex_exact", fit.RowShards.shape_operators) on the GPU:
fit.shape_gradient and fit.shape_step on one context, over row shards of two row ranges and over two ranks of cyclic
4-row tiles give the same bits - loss, gradient, step and every model value - from run to run and after
RowShards.update_points; the step stays within 1e-8 of the largest element of the atomic mode's.  All contexts sit on one
device."""
import numpy as np
import pytest

from course5_amd import capi, sharding
from course5_amd import meshgen as mg
from tests import motion_reference as mr

pytestmark = pytest.mark.gpu
RX, RY = 29, 21
B = mg.REFERENCE_BOUNDS
ROTS = mg.view_rotations(0.13, 0.21)
ITERS = 4


def _bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, np.float64).view(np.int64)


class _Fit:
    def __init__(self):
        self.xyz, self.cells = mg.kuhn_box(4, jitter=0.1)
        self.alpha, self.q = mr.scalars(len(self.cells), 9)
        lo, hi = self.xyz.min(0), self.xyz.max(0)
        self.free = ((self.xyz > lo + 1e-9) & (self.xyz < hi - 1e-9)).all(1)
        assert self.free.sum() == 27
        rng = np.random.default_rng(81)
        self.true = self.xyz.copy()
        self.true[self.free] += 1e-3 * rng.normal(size=(27, 3))
        self.weight = (0.5 + np.abs(rng.normal(size=(RY, RX, 2)))).astype(np.float32)
        self.ctxs = []

    def ctx(self, exact=True, place=None):
        ctx = capi.Context(0)
        self.ctxs.append(ctx)
        ctx.upload_grid(self.xyz, self.cells, self.alpha, self.q)
        ctx.set_image(RX, RY, B)
        ctx.set_view(ROTS)
        ctx.set_option("vertex_exact", 1 if exact else 0)
        rows = np.arange(RY) if place is None else place(ctx)
        return ctx, rows

    def close(self):
        for c in self.ctxs:
            c.close()


@pytest.fixture()
def setup():
    import torch  # noqa: F401  (before the library's first call)
    s = _Fit()
    yield s
    s.close()


def _ways(s):
    """(name, the object fit is given) three ways: one context, two row ranges, two ranks of 4-row tiles."""
    from course5_amd import fit
    one, _ = s.ctx()
    ranges = fit.RowShards([s.ctx(place=lambda c, b=b, n=n: (c.set_row_range(b, n), np.arange(b, b + n))[1]) for b, n in ((0, 13), (13, 8))])
    tiles = fit.RowShards([s.ctx(place=lambda c, r=r: (c.set_row_tiles(4, r, 2), sharding.local_rows(RY, 4, r, 2))[1]) for r in range(2)])
    return one, (("one context", one), ("rows [0,13)+[13,21)", ranges), ("4-row tiles of two ranks", tiles))


def _residual(ctx, target):
    import torch
    return torch.tensor(ctx.render() - target)


def _fit_once(obj, s, r):
    import torch
    from course5_amd import fit
    a, q, w = torch.tensor(s.alpha), torch.tensor(s.q), torch.tensor(s.weight)
    loss, grad = fit.shape_gradient(obj, a, q, r, w)
    d, models = fit.shape_step(obj, a, q, r, w, iters=ITERS, free=s.free)
    return loss, grad, d, models


def _assert_same(got, want, what):
    assert got[0] == want[0], what
    assert np.array_equal(_bits(got[1]), _bits(want[1])), what
    assert np.array_equal(_bits(got[2]), _bits(want[2])), what
    assert got[3] == want[3], what


def test_three_ways_one_step_and_a_second_after_update_points(setup):
    s = setup
    one, ways = _ways(s)
    one.update_points(s.true)
    target = one.render()
    one.update_points(s.xyz)
    r = _residual(one, target)
    assert float(r.abs().max()) > 0

    first = _fit_once(one, s, r)
    loss, grad, d, models = first
    print("loss", loss, "models:", " ".join(f"{m:.9g}" for m in models))
    assert loss > 0 and 1 <= len(models) <= ITERS and all(y <= x for x, y in zip(models, models[1:])) and models[-1] < 0
    d_np = d.cpu().numpy()
    assert not d_np[~s.free].view(np.int64).any() and np.abs(d_np[s.free]).max() > 0  # the fixed rows: exactly 0
    assert float((grad.cpu().numpy() * d_np).sum()) < 0
    _assert_same(_fit_once(one, s, r), first, "one context, run again")
    for name, obj in ways[1:]:
        _assert_same(_fit_once(obj, s, r), first, name)

    # the atomic mode's step: the same to 1e-8 of its largest element
    plain, _ = s.ctx(exact=False)
    d_atomic = _fit_once(plain, s, r)[2].cpu().numpy()
    gap = np.abs(d_np - d_atomic).max()
    print(f"largest |d_exact - d_atomic| {gap:.3g} of max {np.abs(d_atomic).max():.3g}")
    assert gap <= 1e-8 * np.abs(d_atomic).max()

    # the outer loop: new points to every context, a second step
    moved = s.xyz + d_np
    one.update_points(moved)
    r2 = _residual(one, target)
    second = _fit_once(one, s, r2)
    assert second[0] < first[0]  # (the loss fell)
    for name, obj in ways[1:]:
        obj.update_points(moved)
        _assert_same(_fit_once(obj, s, r2), second, name + ", second step")

"""Tangent render on the GPU (c5_render_tangent*, course5_amd.autograd's jvp) against the numpy restatement
(tests/tangent_reference.py), the adjoint (dot-product test) and exact identities.  Every test opens its own contexts."""
import types

import numpy as np
import pytest

from course5_amd import capi
from course5_amd import meshgen as mg
from tests import tangent_reference as tr

pytestmark = pytest.mark.gpu
B = mg.REFERENCE_BOUNDS


def _scalars(n, seed):
    """alpha ~ U[0, 4) (the 2.5 clamp) with exact zeros, nothing in [eps, 1e-6); Q ~ U[0, 1)."""
    rng = np.random.default_rng(seed)
    alpha = rng.uniform(0.0, 4.0, n)
    alpha[rng.random(n) < 0.05] = 0.0
    alpha[(alpha > 0) & (alpha < 1e-6)] = 1e-6
    return alpha, rng.uniform(0.0, 1.0, n)


def _directions(n, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=n), rng.normal(size=n)


def _ctx(xyz, cells, alpha, q, rots, rx, ry, options=()):
    ctx = capi.Context(0)
    for k, v in options:
        ctx.set_option(k, v)
    ctx.upload_grid(xyz, cells, alpha, q)
    ctx.set_image(rx, ry, B)
    ctx.set_view(rots)
    return ctx


def _assert_close(got, want, what):
    for ch, name in ((0, "tau_dot"), (1, "I_dot")):
        w = want[ch]
        err = np.abs(got[..., ch].astype(np.float64) - w).max()
        assert err <= 1e-6 * np.abs(w).max(), f"{what}: {name} max abs error {err:.3g} vs max {np.abs(w).max():.3g}"


def _check(xyz, cells, rots, rx=160, ry=120, seed=3, options=()):
    alpha, q = _scalars(len(cells), seed)
    da, dq = _directions(len(cells), seed + 1)
    with _ctx(xyz, cells, alpha, q, rots, rx, ry, options) as ctx:
        got = ctx.render_tangent(da, dq)
    want = tr.image_tangent(xyz, cells, alpha, q, rots, rx, ry, B, da, dq)[:2]
    assert np.abs(want[1]).max() > 0
    return got, want


@pytest.fixture(scope="module")
def kuhn():
    xyz, cells = mg.kuhn_box(9, jitter=0.1)  # 4 374 cells: Morton order on ("cell_order"), caller order is tested
    return xyz, cells, mg.view_rotations(0.13, 0.21)


def test_kuhn_box_against_the_restatement_whatever_the_walk_options(kuhn):
    xyz, cells, rots = kuhn
    got0, want = _check(xyz, cells, rots)
    _assert_close(got0, want, "default")
    for opts in ((("integration", 1),), (("depth_split", 2),), (("lds_stage", 0), ("tile", 0)), (("cell_order", 0),)):
        got, _ = _check(xyz, cells, rots, options=opts)
        # the same walk whatever the options, and no atomics: the same bits
        assert np.array_equal(got.view(np.uint32), got0.view(np.uint32)), opts


@pytest.mark.parametrize("grid", ["ball", "slabs", "refined"])
def test_reentries_entry_chains_and_hanging_nodes(grid):
    if grid == "ball":
        xyz, cells = mg.ball(16, 0.45)
    elif grid == "slabs":
        from tests.test_gpu_parity import _stacked_slabs
        xyz, cells, _, _ = _stacked_slabs()
    else:
        xyz, cells, _ = mg.refined_interface(3, 2, 3, jitter=0.1, warp=0.08)
    got, want = _check(xyz, cells, mg.view_rotations(0.13, 0.21))
    _assert_close(got, want, grid)


def test_soup_and_overlapping_grid_on_the_fallback():
    rots = mg.view_rotations(0.13, 0.21)
    xyz, cells = mg.kuhn_box(4, jitter=0.1)
    soup_xyz, soup_cells = mg.per_cell_point_copies(xyz, cells)
    got, want = _check(soup_xyz, soup_cells, rots, options=(("algorithm", 1),))
    _assert_close(got, want, "soup, algorithm 1")
    # two interpenetrating boxes: the first walk finds them (C5_RETRY, settled by c5_render_tangent itself)
    xa, ca = mg.kuhn_box(3, lo=(0.6, -0.4, -0.3), size=0.6, jitter=0.1, seed=5)
    xb, cb = mg.kuhn_box(4, lo=(0.85, -0.2, -0.45), size=0.7, jitter=0.1, seed=6)
    xyz2, cells2 = np.vstack([xa, xb]), np.vstack([ca, cb + len(xa)]).astype(np.int32)
    got, want = _check(xyz2, cells2, rots)
    _assert_close(got, want, "overlapping boxes")


def test_solid_pixels_are_zero(kuhn):
    xyz, cells, rots = kuhn
    rx, ry = 160, 120
    alpha, q = _scalars(len(cells), 4)
    da, dq = _directions(len(cells), 14)
    sx, sc = mg.kuhn_box(2, lo=(0.9, -0.15, 0.3), size=0.3)
    solid = sx[sc].reshape(-1, 12)
    with _ctx(xyz, cells, alpha, q, rots, rx, ry) as ctx:
        ctx.set_solid(0, solid)  # colour NaN: solid pixels are NaN in the image
        img = ctx.render()
        got = ctx.render_tangent(da, dq)
    skip = np.isnan(img[..., 0])
    assert 100 < skip.sum() < skip.size // 2
    assert not got[skip].any()
    want = tr.image_tangent(xyz, cells, alpha, q, rots, rx, ry, B, da, dq, skip=skip)[:2]
    _assert_close(got, want, "solid")


def test_null_directions_reproducibility_and_row_ranges(kuhn):
    xyz, cells, rots = kuhn
    rx, ry = 160, 120
    alpha, q = _scalars(len(cells), 5)
    da, dq = _directions(len(cells), 15)
    zero = np.zeros(len(cells))
    with _ctx(xyz, cells, alpha, q, rots, rx, ry) as ctx:
        full = ctx.render_tangent(da, dq)
        again = ctx.render_tangent(da, dq)
        assert np.array_equal(full.view(np.uint32), again.view(np.uint32))
        assert np.array_equal(ctx.render_tangent(None, dq), ctx.render_tangent(zero, dq))
        assert np.array_equal(ctx.render_tangent(da, None), ctx.render_tangent(da, zero))
        nothing = ctx.render_tangent(None, None)
        assert nothing.shape == (ry, rx, 2) and not nothing.any()
        assert np.abs(ctx.render_tangent(da, None)[..., 0]).max() > 0 and not ctx.render_tangent(None, dq)[..., 0].any()
    parts = []
    for begin, count in ((0, 47), (47, ry - 47)):
        with _ctx(xyz, cells, alpha, q, rots, rx, ry) as ctx:
            ctx.set_row_range(begin, count)
            part = ctx.render_tangent(da, dq)
            assert part.shape == (count, rx, 2)
            parts.append(part)
    stacked = np.concatenate(parts, axis=0).astype(np.float64)
    for ch in range(2):
        assert np.abs(stacked[..., ch] - full[..., ch]).max() <= 1e-6 * np.abs(full[..., ch]).max()


@pytest.mark.parametrize("opts", [(), (("depth_split", 2),), (("integration", 1),)], ids=["default", "split", "ftb"])
def test_render_after_a_tangent_is_bit_identical(kuhn, opts):
    xyz, cells, rots = kuhn
    alpha, q = _scalars(len(cells), 6)
    da, dq = _directions(len(cells), 16)
    with _ctx(xyz, cells, alpha, q, rots, 160, 120, opts) as a, _ctx(xyz, cells, alpha, q, rots, 160, 120, opts) as b:
        for _ in range(3):  # (three frames: the view cache is in use by the third)
            a.render(), b.render()
        before = a.stats()
        a.render_tangent(da, dq)
        assert a.stats() == before
        assert a.synchronize() == capi.C5_OK
        for _ in range(3):
            ia, ib = a.render(), b.render()
            assert np.array_equal(ia.view(np.uint32), ib.view(np.uint32))
        assert a.stats()["segments"] == b.stats()["segments"]


def test_torch_forward_mode_matches_render_tangent(kuhn):
    import torch
    import torch.autograd.forward_ad as fwAD
    from course5_amd import autograd
    xyz, cells, rots = kuhn
    alpha, q = _scalars(len(cells), 7)
    da, dq = _directions(len(cells), 17)
    with _ctx(xyz, cells, alpha, q, rots, 160, 120) as ctx:
        a = torch.tensor(alpha, dtype=torch.float32)
        qq = torch.tensor(q, dtype=torch.float64, device="cuda")
        ta = torch.tensor(da, dtype=torch.float32)                   # CPU, float32
        tq = torch.tensor(dq, dtype=torch.float64, device="cuda")    # GPU, float64
        with fwAD.dual_level():
            img = autograd.render(ctx, fwAD.make_dual(a, ta), fwAD.make_dual(qq, tq))
            primal, tangent = fwAD.unpack_dual(img)
        assert tangent.dtype == torch.float32 and tangent.is_cuda and tangent.shape == (120, 160, 2)
        ctx.update_scalars(a.double().numpy(), q)
        assert np.array_equal(primal.cpu().numpy(), ctx.render())
        want = ctx.render_tangent(ta.double().numpy(), dq)
        assert np.array_equal(tangent.cpu().numpy(), want)
        # only alpha carries a tangent: q's is zero
        with fwAD.dual_level():
            t_a = fwAD.unpack_dual(autograd.render(ctx, fwAD.make_dual(a, ta), qq)).tangent
        assert np.array_equal(t_a.cpu().numpy(), ctx.render_tangent(ta.double().numpy(), None))
        # torch.func.jvp: the same
        out, t = torch.func.jvp(lambda x, y: autograd.render(ctx, x, y), (a, qq), (ta, tq))
        assert np.array_equal(t.cpu().numpy(), want) and np.array_equal(out.cpu().numpy(), primal.cpu().numpy())
        # reverse mode still works beside it
        a_req = a.clone().requires_grad_(True)
        autograd.render(ctx, a_req, qq).sum().backward()
        assert a_req.grad is not None and a_req.grad.shape == a.shape


def test_jvp_uploads_its_own_scalars_and_refuses_a_changed_view(kuhn):
    import torch
    from course5_amd import autograd
    xyz, cells, rots = kuhn
    alpha, q = _scalars(len(cells), 8)
    da, dq = _directions(len(cells), 18)
    ta, tq = torch.tensor(da).cuda(), torch.tensor(dq).cuda()
    with _ctx(xyz, cells, alpha, q, rots, 160, 120) as ctx:
        a, qq = torch.tensor(alpha), torch.tensor(q)
        fctx = types.SimpleNamespace()
        out = autograd._Render.forward(ctx, a, qq)
        autograd._Render.setup_context(fctx, (ctx, a, qq), out)
        want = ctx.render_tangent(da, dq)
        autograd.render(ctx, a * 0.5, qq)  # another forward replaces the context's scalars
        got = autograd._Render.jvp(fctx, None, ta, tq)
        assert np.array_equal(got.cpu().numpy(), want)
        ctx.set_view(mg.view_rotations(0.2, 0.1))
        with pytest.raises(RuntimeError, match="changed since the forward pass"):
            autograd._Render.jvp(fctx, None, ta, tq)


@pytest.fixture(scope="module")
def c3():
    xyz, cells, alpha, q = mg.workload("c3")
    alpha = alpha.copy()
    alpha[(alpha >= np.finfo(np.float64).eps) & (alpha < 1e-6)] = 1e-6
    ctx = _ctx(xyz, cells, alpha, q, mg.view_rotations(**mg.BENCH_VIEW), 2400, 1800)
    yield ctx, alpha, q
    ctx.close()


def test_c3_dot_product_with_the_adjoint(c3):
    ctx, alpha, q = c3
    rng = np.random.default_rng(31)
    g = rng.random((1800, 2400, 2)).astype(np.float32)
    v_a = alpha * rng.uniform(-0.5, 1.5, len(alpha))
    v_q = q * rng.uniform(-0.5, 1.5, len(q))
    Jv = ctx.render_tangent(v_a, v_q).astype(np.float64)
    ga, gq = ctx.render_adjoint(g)
    lhs = float((g.astype(np.float64) * Jv).sum())
    rhs = float(ga @ v_a + gq @ v_q)
    assert abs(lhs - rhs) <= 1e-5 * abs(rhs), (lhs, rhs)


def test_c3_linearity_identities(c3):
    """I is linear in Q and tau in alpha: (0, Q) gives I_dot = I, (alpha, 0) gives tau_dot = tau."""
    ctx, alpha, q = c3
    img = ctx.render().astype(np.float64)
    I_dot = ctx.render_tangent(None, q)[..., 1].astype(np.float64)
    tau_dot = ctx.render_tangent(alpha, None)[..., 0].astype(np.float64)
    for got, want, name in ((I_dot, img[..., 1], "I"), (tau_dot, img[..., 0], "tau")):
        bad = np.abs(got - want) > 1e-5 * np.abs(want) + 1e-6 * np.abs(want).max()
        assert not bad.any(), f"{name}: {int(bad.sum())} pixels"


def test_c3_central_differences_of_two_renders(c3):
    ctx, alpha, q = c3
    rng = np.random.default_rng(32)
    h = 1e-2
    u = rng.uniform(-1.0, 1.0, len(alpha))
    # a relative step; cells whose step would cross the clamp do not move (the image is not smooth there)
    d_alpha = np.where(np.abs(alpha - 2.5) > 2 * h * alpha, alpha * u, 0.0)
    d_q = q * rng.uniform(-1.0, 1.0, len(q))
    tan = ctx.render_tangent(d_alpha, d_q).astype(np.float64)
    imgs = []
    for s in (1, -1):
        ctx.update_scalars(alpha + s * h * d_alpha, q + s * h * d_q)
        imgs.append(ctx.render().astype(np.float64))
    ctx.update_scalars(alpha, q)
    fd = (imgs[0] - imgs[1]) / (2 * h)
    for ch in range(2):
        strong = np.abs(tan[..., ch]) >= 0.2 * np.abs(tan[..., ch]).max()
        assert strong.sum() > 1000
        rel = np.abs(fd[..., ch][strong] - tan[..., ch][strong]) / np.abs(tan[..., ch][strong])
        assert rel.max() <= 1e-3, (ch, rel.max())

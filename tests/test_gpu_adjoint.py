"""Adjoint render on the GPU (c5_render_adjoint*, course5_amd.autograd, course --contribution) against the numpy helper
(tests/adjoint_reference.py) and exact identities.  Every test opens its own contexts: the session's gpu_ctx is left
as it is."""
import os
import subprocess

import numpy as np
import pytest

from course5_amd import capi
from course5_amd import meshgen as mg
from tests import adjoint_reference as ar

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COURSE = os.path.join(ROOT, "course5_amd", "course")
B = mg.REFERENCE_BOUNDS


def _scalars(n, seed):
    """alpha ~ U[0, 4) (the 2.5 clamp) with exact zeros, nothing in [eps, 1e-6); Q ~ U[0, 1)."""
    rng = np.random.default_rng(seed)
    alpha = rng.uniform(0.0, 4.0, n)
    alpha[rng.random(n) < 0.05] = 0.0
    alpha[(alpha > 0) & (alpha < 1e-6)] = 1e-6
    return alpha, rng.uniform(0.0, 1.0, n)


def _ctx(xyz, cells, alpha, q, rots, rx, ry, options=()):
    ctx = capi.Context(0)
    for k, v in options:
        ctx.set_option(k, v)
    ctx.upload_grid(xyz, cells, alpha, q)
    ctx.set_image(rx, ry, B)
    ctx.set_view(rots)
    return ctx


def _assert_close(got, want, what):
    for g, w, name in zip(got, want, ("grad_alpha", "grad_q")):
        err = np.abs(g - w).max()
        assert err <= 1e-6 * np.abs(w).max(), f"{what}: {name} max abs error {err:.3g} vs max {np.abs(w).max():.3g}"


def _check(xyz, cells, rots, rx=160, ry=120, seed=3, options=(), weights=None):
    alpha, q = _scalars(len(cells), seed)
    w = np.random.default_rng(seed + 1).normal(size=(ry, rx, 2)) if weights is None else weights
    w = w.astype(np.float32)
    with _ctx(xyz, cells, alpha, q, rots, rx, ry, options) as ctx:
        got = ctx.render_adjoint(w)
    want = ar.image_gradients(xyz, cells, alpha, q, rots, rx, ry, B, w.astype(np.float64))[:2]
    return got, want


@pytest.fixture(scope="module")
def kuhn():
    xyz, cells = mg.kuhn_box(9, jitter=0.1)  # 4 374 cells: Morton order on ("cell_order"), caller order is tested
    return xyz, cells, mg.view_rotations(0.13, 0.21)


def test_kuhn_box_against_the_helper_whatever_the_walk_options(kuhn):
    xyz, cells, rots = kuhn
    got0, want = _check(xyz, cells, rots)
    _assert_close(got0, want, "default")
    for opts in ((("integration", 1),), (("depth_split", 2),), (("lds_stage", 0), ("tile", 0))):
        got, _ = _check(xyz, cells, rots, options=opts)
        _assert_close(got, want, str(opts))
        for g, g0 in zip(got, got0):  # the same walk whatever the options: equal to the atomics' rounding
            np.testing.assert_allclose(g, g0, rtol=1e-12, atol=1e-15 * np.abs(g0).max())


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
    # two interpenetrating boxes: the first walk finds them (C5_RETRY, settled by c5_render_adjoint itself)
    xa, ca = mg.kuhn_box(3, lo=(0.6, -0.4, -0.3), size=0.6, jitter=0.1, seed=5)
    xb, cb = mg.kuhn_box(4, lo=(0.85, -0.2, -0.45), size=0.7, jitter=0.1, seed=6)
    xyz2, cells2 = np.vstack([xa, xb]), np.vstack([ca, cb + len(xa)]).astype(np.int32)
    got, want = _check(xyz2, cells2, rots)
    _assert_close(got, want, "overlapping boxes")


def test_solid_pixels_contribute_nothing(kuhn):
    xyz, cells, rots = kuhn
    rx, ry = 160, 120
    alpha, q = _scalars(len(cells), 4)
    sx, sc = mg.kuhn_box(2, lo=(0.9, -0.15, 0.3), size=0.3)
    solid = sx[sc].reshape(-1, 12)
    w = np.random.default_rng(9).normal(size=(ry, rx, 2)).astype(np.float32)
    with _ctx(xyz, cells, alpha, q, rots, rx, ry) as ctx:
        ctx.set_solid(0, solid)  # colour NaN: solid pixels are NaN in the image
        img = ctx.render()
        got = ctx.render_adjoint(w)
    skip = np.isnan(img[..., 0])
    assert 100 < skip.sum() < skip.size // 2
    want = ar.image_gradients(xyz, cells, alpha, q, rots, rx, ry, B, w.astype(np.float64), skip=skip)[:2]
    _assert_close(got, want, "solid")


def test_row_ranges_add_up_to_the_whole_image(kuhn):
    xyz, cells, rots = kuhn
    rx, ry = 160, 120
    alpha, q = _scalars(len(cells), 5)
    w = np.random.default_rng(11).normal(size=(ry, rx, 2)).astype(np.float32)
    with _ctx(xyz, cells, alpha, q, rots, rx, ry) as whole:
        full = whole.render_adjoint(w)
    parts = []
    for begin, count in ((0, 47), (47, ry - 47)):
        with _ctx(xyz, cells, alpha, q, rots, rx, ry) as ctx:
            ctx.set_row_range(begin, count)
            parts.append(ctx.render_adjoint(w[begin:begin + count]))
    _assert_close((parts[0][0] + parts[1][0], parts[0][1] + parts[1][1]), full, "two row ranges")


@pytest.mark.parametrize("opts", [(), (("depth_split", 2),), (("integration", 1),)], ids=["default", "split", "ftb"])
def test_render_after_an_adjoint_is_bit_identical(kuhn, opts):
    xyz, cells, rots = kuhn
    alpha, q = _scalars(len(cells), 6)
    w = np.ones((120, 160, 2), np.float32)
    with _ctx(xyz, cells, alpha, q, rots, 160, 120, opts) as a, _ctx(xyz, cells, alpha, q, rots, 160, 120, opts) as b:
        for _ in range(3):  # (three frames: the view cache is in use by the third)
            a.render(), b.render()
        a.render_adjoint(w)
        for _ in range(3):
            ia, ib = a.render(), b.render()
            assert np.array_equal(ia.view(np.uint32), ib.view(np.uint32))
        assert a.stats()["segments"] == b.stats()["segments"]


def test_torch_autograd_matches_render_adjoint_and_refuses_a_changed_view(kuhn):
    import torch
    from course5_amd import autograd
    xyz, cells, rots = kuhn
    alpha, q = _scalars(len(cells), 7)
    W = torch.from_numpy(np.random.default_rng(13).normal(size=(120, 160, 2)).astype(np.float32)).cuda()
    with _ctx(xyz, cells, alpha, q, rots, 160, 120) as ctx:
        a = torch.tensor(alpha, dtype=torch.float32, requires_grad=True)  # (dtype and device of the inputs come back)
        qq = torch.tensor(q, dtype=torch.float64, device="cuda", requires_grad=True)
        img = autograd.render(ctx, a, qq)
        assert np.array_equal(img.detach().cpu().numpy(), (ctx.update_scalars(a.detach().double().numpy(), q), ctx.render())[1])
        # another forward with other scalars in between: the backward uploads its own again
        autograd.render(ctx, a.detach() * 0.5, qq.detach())
        (img * W).sum().backward()
        assert a.grad.dtype == torch.float32 and a.grad.device.type == "cpu" and qq.grad.dtype == torch.float64 and qq.grad.is_cuda
        ctx.update_scalars(a.detach().double().numpy(), q)
        ga, gq = ctx.render_adjoint(W.cpu().numpy())
        np.testing.assert_allclose(a.grad.numpy(), ga.astype(np.float32), rtol=1e-5, atol=1e-6 * np.abs(ga).max())
        np.testing.assert_allclose(qq.grad.cpu().numpy(), gq, rtol=1e-9, atol=1e-12 * np.abs(gq).max())
        img2 = autograd.render(ctx, a, qq)
        ctx.set_view(mg.view_rotations(0.2, 0.1))
        with pytest.raises(RuntimeError, match="changed since the forward pass"):
            img2.sum().backward()


def test_c3_frame_identities_and_finite_differences():
    xyz, cells, alpha, q = mg.workload("c3")
    rots = mg.view_rotations(**mg.BENCH_VIEW)
    rx, ry = 2400, 1800
    with _ctx(xyz, cells, alpha, q, rots, rx, ry) as ctx:
        img = ctx.render().astype(np.float64)
        w = np.zeros((ry, rx, 2), np.float32)
        w[..., 0] = 1
        ga_tau, _ = ctx.render_adjoint(w)
        w[..., 0], w[..., 1] = 0, 1
        ga, gq = ctx.render_adjoint(w)
        # tau is linear in alpha, I in Q
        tau_sum, I_sum = img[..., 0].sum(), img[..., 1].sum()
        assert abs(np.dot(alpha, ga_tau) - tau_sum) <= 1e-5 * abs(tau_sum)
        assert abs(np.dot(q, gq) - I_sum) <= 1e-5 * abs(I_sum)
        # d sum(I) / d alpha of the cells with the largest gradients, against central differences of two renders
        unclamped = alpha < 2.5 * (1 - 1e-3)
        cand = np.argsort(-np.abs(ga) * unclamped)[:20]
        for c in cand:
            h = 1e-3 * alpha[c]
            sums = []
            for s in (1, -1):
                a2 = alpha.copy()
                a2[c] += s * h
                ctx.update_scalars(a2, q)
                sums.append(ctx.render()[..., 1].astype(np.float64).sum())
            fd = (sums[0] - sums[1]) / (2 * h)
            assert fd == pytest.approx(ga[c], rel=0.02), (c, fd, ga[c])


def test_cli_contribution(tmp_path):
    xyz, cells = mg.kuhn_box(6, jitter=0.1)
    alpha, q = _scalars(len(cells), 8)
    src = tmp_path / "g.vtk"
    mg.write_vtk_binary(str(src), xyz, cells, alpha, q)
    args = ["-x", "240", "-y", "180", "-X", "0.1", "-Y", "0.07", "--no_solids", "-j", "4"]
    r = subprocess.run([COURSE, "-f", str(src), "-d", str(tmp_path / "a.vti"), "--contribution", str(tmp_path / "c.vtk")] + args,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r2 = subprocess.run([COURSE, "-f", str(tmp_path / "c.vtk"), "-d", str(tmp_path / "b.vti")] + args,
                        capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0, r2.stderr
    assert (tmp_path / "a.vti").read_bytes() == (tmp_path / "b.vti").read_bytes()
    # Contribution sums to the image's sum of I
    contrib = _cell_array(tmp_path / "c.vtk", "Contribution")
    with _ctx(xyz, cells, alpha, q, mg.view_rotations(0.1, 0.07), 240, 180) as ctx:
        I_sum = ctx.render()[..., 1].astype(np.float64).sum()
    assert abs(contrib.sum() - I_sum) <= 1e-5 * abs(I_sum)
    assert np.array_equal(_cell_array(tmp_path / "c.vtk", "AbsorpCoef"), alpha)


def _cell_array(path, name):
    """A big-endian double CELL_DATA SCALARS array of a binary legacy .vtk."""
    raw = open(path, "rb").read()
    at = raw.index(f"SCALARS {name} double 1\nLOOKUP_TABLE default\n".encode())
    head = raw[:at]
    n = int(head[head.rindex(b"CELL_DATA ") + 10:].split(b"\n")[0])
    start = at + len(f"SCALARS {name} double 1\nLOOKUP_TABLE default\n")
    return np.frombuffer(raw, dtype=">f8", count=n, offset=start).astype(np.float64)

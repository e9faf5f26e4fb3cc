"""The Hessian-vector render on the GPU (c5_render_hvp*, course5_amd.autograd.hvp, course5_amd.fit.newton_product /
newton_step) against the numpy restatement (tests/hvp_reference.py, itself pinned to 80 digits in tests/test_hvp_cpu.py),
and against the library's own adjoint.

Bars, none fitted to what the GPU returns:
  per array     max |got - ref| <= 1e-6 x max |ref|: the family's coarse bar;
  per element   |got - ref| <= 1e-9 x scale + dz_err x sens + 2^-970, with hvp_of's scale and sens and
                derivative_fuzz.dz_err / ratio;
  symmetry      |<u, H v> - <v, H u>| <= 1e-9 (sum |u_i (H v)_i| + sum |v_i (H u)_i|);
  differences   central differences of c5_render_adjoint at the step settled on the CPU (tests/test_hvp_cpu.py: relative
                1e-4) within ten times what the restatement's own difference showed there, of the largest element.
The worst measured ratios are in profiles/hvp_fuzz.md.  Every test opens its own contexts.
"""
import ctypes as C
import types

import numpy as np
import pytest

from course5_amd import capi
from course5_amd import meshgen as mg
from tests import adjoint_reference as ar
from tests import hvp_reference as hr
from tests.derivative_fuzz import dz_err, ratio
from tests.test_gpu_tangent import _ctx, _scalars
from tests.test_hvp_cpu import FD_SHOWN, fd_directions, fd_step, newton_scene, small_scene

pytestmark = pytest.mark.gpu
B = mg.REFERENCE_BOUNDS
ROTS = mg.view_rotations(0.13, 0.21)
LIMIT = 2.5
EPS = float(np.finfo(np.float64).eps)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _draw(n, seed):
    """alpha over zero, below DBL_EPSILON, above the limit and the rest U[0, limit) (chords of up to a quarter of the box:
    a dz on both sides of 1/8); Q U[0, 1); a direction and an upstream image's seed."""
    rng = np.random.default_rng(seed)
    alpha = rng.uniform(0.0, LIMIT, n)
    cls = rng.random(n)
    alpha[cls < 0.05] = 0.0
    alpha[(cls >= 0.05) & (cls < 0.10)] = 10.0 ** rng.uniform(-300.0, -17.0, int(((cls >= 0.05) & (cls < 0.10)).sum()))
    alpha[cls >= 0.88] = LIMIT * (2.0 - rng.uniform(0.0, 1.0, int((cls >= 0.88).sum())))
    alpha[(alpha >= EPS) & (alpha < 1e-6)] = 1e-6
    return alpha, rng.uniform(0.0, 1.0, n), rng.normal(size=n), rng.normal(size=n), rng


def _image(rng, ry, rx):
    g = rng.normal(size=(ry, rx, 2)).astype(np.float32)
    g[ry // 3: ry // 3 + 2, : rx // 2] = 0.0  # (a patch of exact zeros: rays that are not walked)
    return g


def _hold(got, ref, x, e, what):
    """Both bars, for (h_alpha, h_q)."""
    for name, g, r in (("alpha", got[0], ref[0]), ("q", got[1], ref[1])):
        top = np.abs(r).max()
        err = np.abs(g - r).max()
        el = ratio(g, r, x["scale_" + name], x["sens_" + name], e)
        print(f"{what} h_{name}: max |diff| / max |ref| = {err / top if top else 0:.3g} (bar 1e-6), worst element error / bar {el.max():.3g}")
        if top == 0:  # (the Q-Q block is zero: a direction in Q alone has h_q identically 0)
            assert name == "q" and "NULL d_alpha" in what and not np.asarray(g).any(), (what, name)
            continue
        assert err <= 1e-6 * top, (what, name, err, top)
        assert (el <= 1.0).all(), (what, name, float(el.max()), int(np.argmax(el)))


def _scene(kind):
    if kind == "box4":
        (xyz, cells), (rx, ry) = mg.kuhn_box(4, jitter=0.1), (37, 29)
    elif kind == "box9":
        (xyz, cells), (rx, ry) = mg.kuhn_box(9, jitter=0.1), (24, 16)
    elif kind == "ball":
        (xyz, cells), (rx, ry) = mg.ball(16, 0.45), (40, 30)
    else:
        (xyz, cells), (rx, ry) = mg.refined_interface()[:2], (40, 30)
    return xyz, cells, rx, ry


def _reference(xyz, cells, alpha, q, rx, ry, rows=None):
    return ar.ray_matrices(xyz, cells, alpha, q, ROTS, rx, ry, B, LIMIT, rows)


@pytest.mark.parametrize("kind", ["box4", "box9", "ball", "refined"])
def test_against_the_restatement(kind):
    xyz, cells, rx, ry = _scene(kind)
    n = len(cells)
    alpha, q, va, vq, rng = _draw(n, 71)
    g = _image(rng, ry, rx)
    e = dz_err(types.SimpleNamespace(xyz=xyz, rots=ROTS))
    m = _reference(xyz, cells, alpha, q, rx, ry)
    with _ctx(xyz, cells, alpha, q, ROTS, rx, ry) as ctx:
        for da, dq, what in ((va, vq, "both"), (None, vq, "NULL d_alpha"), (va, None, "NULL d_q")):
            got = ctx.render_hvp(da, dq, g)
            ha, hq, x = hr.hvp_of(m, n, da, dq, g, with_scale=True)
            _hold(got, (ha, hq), x, e, f"{kind} {what}")
        # a NULL h_q, a NULL h_alpha
        ha, hq, x = hr.hvp_of(m, n, va, vq, g, with_scale=True)
        only_a, none = ctx.render_hvp(va, vq, g, fit=("alpha",))
        assert none is None
        none, only_q = ctx.render_hvp(va, vq, g, fit=("q",))
        assert none is None
        _hold((only_a, only_q), (ha, hq), x, e, f"{kind} one output at a time")


def test_solid_rows_and_caller_order():
    xyz, cells, rx, ry = _scene("box4")
    n = len(cells)
    alpha, q, va, vq, rng = _draw(n, 72)
    g = _image(rng, ry, rx)
    e = dz_err(types.SimpleNamespace(xyz=xyz, rots=ROTS))
    # a solid over part of the grid
    with _ctx(xyz, cells, alpha, q, ROTS, rx, ry) as ctx:
        sx, sc = mg.kuhn_box(2, lo=(0.9, -0.15, 0.3), size=0.3)
        ctx.set_solid(0, sx[sc].reshape(-1, 12))
        skip = np.isnan(ctx.render()[..., 0])
        assert 10 < skip.sum() < skip.size // 2
        got = ctx.render_hvp(va, vq, g)
    m = _reference(xyz, cells, alpha, q, rx, ry)
    ha, hq, x = hr.hvp_of(m, n, va, vq, g, skip, with_scale=True)
    _hold(got, (ha, hq), x, e, "solid")
    # two row ranges add up to the whole image's result; each is its rows' restatement
    ha, hq, x = hr.hvp_of(m, n, va, vq, g, with_scale=True)
    total = [np.zeros(n), np.zeros(n)]
    for begin, count in ((0, 11), (11, ry - 11)):
        with _ctx(xyz, cells, alpha, q, ROTS, rx, ry) as ctx:
            ctx.set_row_range(begin, count)
            part = ctx.render_hvp(va, vq, np.ascontiguousarray(g[begin:begin + count]))
        rows = np.arange(begin, begin + count)
        pa, pq, px = hr.hvp_of(_reference(xyz, cells, alpha, q, rx, ry, rows), n, va, vq, g[rows], with_scale=True)
        _hold(part, (pa, pq), px, e, f"rows {begin}..{begin + count}")
        total[0] += part[0]
        total[1] += part[1]
    _hold(total, (ha, hq), x, e, "two row ranges, summed")
    # the caller's order with "cell_order" on (the default) and off
    for order in (1, 0):
        with _ctx(xyz, cells, alpha, q, ROTS, rx, ry, (("cell_order", order),)) as ctx:
            _hold(ctx.render_hvp(va, vq, g), (ha, hq), x, e, f"cell_order {order}")


def test_on_the_fallback_and_across_the_retry():
    rx, ry = 37, 29
    xyz, cells = mg.kuhn_box(4, jitter=0.1)
    soup_xyz, soup_cells = mg.per_cell_point_copies(xyz, cells)
    n = len(soup_cells)
    alpha, q, va, vq, rng = _draw(n, 73)
    g = _image(rng, ry, rx)
    e = dz_err(types.SimpleNamespace(xyz=soup_xyz, rots=ROTS))
    ha, hq, x = hr.hvp_of(_reference(soup_xyz, soup_cells, alpha, q, rx, ry), n, va, vq, g, with_scale=True)
    with _ctx(soup_xyz, soup_cells, alpha, q, ROTS, rx, ry, (("algorithm", 1),)) as ctx:
        _hold(ctx.render_hvp(va, vq, g), (ha, hq), x, e, "soup, algorithm 1")
    # two interpenetrating boxes (tests/test_gpu_adjoint.py: test_soup_and_overlapping_grid_on_the_fallback, its meshes and
    # scalars): the first call's walk finds them (C5_RETRY, settled by c5_render_hvp itself)
    xa, ca = mg.kuhn_box(3, lo=(0.6, -0.4, -0.3), size=0.6, jitter=0.1, seed=5)
    xb, cb = mg.kuhn_box(4, lo=(0.85, -0.2, -0.45), size=0.7, jitter=0.1, seed=6)
    xyz2, cells2 = np.vstack([xa, xb]), np.vstack([ca, cb + len(xa)]).astype(np.int32)
    n = len(cells2)
    alpha, q = _scalars(n, 3)
    rng = np.random.default_rng(74)
    va, vq = rng.normal(size=(2, n))
    g = _image(rng, ry, rx)
    e = dz_err(types.SimpleNamespace(xyz=xyz2, rots=ROTS))
    ha, hq, x = hr.hvp_of(_reference(xyz2, cells2, alpha, q, rx, ry), n, va, vq, g, with_scale=True)
    with _ctx(xyz2, cells2, alpha, q, ROTS, rx, ry) as ctx:
        _hold(ctx.render_hvp(va, vq, g), (ha, hq), x, e, "overlapping boxes")


def test_device_form_and_torch_operator():
    import torch
    from course5_amd import autograd
    xyz, cells, rx, ry = _scene("box4")
    n = len(cells)
    alpha, q, va, vq, rng = _draw(n, 75)
    g = _image(rng, ry, rx)
    e = dz_err(types.SimpleNamespace(xyz=xyz, rots=ROTS))
    ha, hq, x = hr.hvp_of(_reference(xyz, cells, alpha, q, rx, ry), n, va, vq, g, with_scale=True)
    with _ctx(xyz, cells, alpha, q, ROTS, rx, ry) as ctx:
        t = lambda a, dt=torch.float64: torch.tensor(a, dtype=dt, device="cuda")  # noqa: E731
        out_a = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
        out_q = out_a.clone()
        ctx.render_hvp_device(t(va), t(vq), t(g, torch.float32), out_a, out_q)
        assert ctx.synchronize() == capi.C5_OK
        dev = out_a.cpu().numpy(), out_q.cpu().numpy()
        _hold(dev, (ha, hq), x, e, "_device")
        out_q.fill_(float("nan"))
        ctx.render_hvp_device(t(va), t(vq), t(g, torch.float32), out_a, None)  # (a NULL h_q: nothing of it is written)
        assert ctx.synchronize() == capi.C5_OK and bool(torch.isnan(out_q).all())
        # autograd.hvp is render_hvp_device with the scalars it is given
        ctx.update_scalars(alpha * 0.5, q)
        a_t, q_t = t(alpha), t(q)
        ta, tq = autograd.hvp(ctx, a_t, q_t, t(va), t(vq), t(g, torch.float32))
        assert ta.shape == tq.shape == (n,) and ta.is_cuda and ta.dtype == torch.float64 and not ta.requires_grad
        for got, want, scale in ((ta.cpu().numpy(), dev[0], x["scale_alpha"]), (tq.cpu().numpy(), dev[1], x["scale_q"])):
            assert (np.abs(got - want) <= 1e-9 * scale + 2.0 ** -970).all()
        ta0, _ = autograd.hvp(ctx, a_t.clone().requires_grad_(True), q_t, torch.tensor(va), None, torch.tensor(g))  # (host tensors)
        assert ta0.grad_fn is None and not ta0.requires_grad
        with pytest.raises(RuntimeError, match="second derivatives are not supported"):
            torch.func.grad(lambda v: autograd.hvp(ctx, v, q_t, t(va), None, t(g, torch.float32))[0].sum())(a_t)
        with pytest.raises(ValueError):
            autograd.hvp(ctx, a_t, q_t, None, None, t(g, torch.float32))
        with pytest.raises(ValueError):
            autograd.hvp(ctx, a_t, q_t, t(va)[:-1], None, t(g, torch.float32))
        # autograd.render still refuses second derivatives, word for word
        with pytest.raises(RuntimeError, match="second derivatives are not supported"):
            torch.func.hessian(lambda v: autograd.render(ctx, v, q_t)[..., 1].sum())(a_t)


def test_identities_on_the_librarys_own_results():
    xyz, cells, rx, ry = _scene("box4")
    n = len(cells)
    alpha, q, va, vq, rng = _draw(n, 76)
    ua, uq = rng.normal(size=(2, n))
    g = _image(rng, ry, rx)
    m = _reference(xyz, cells, alpha, q, rx, ry)
    with _ctx(xyz, cells, alpha, q, ROTS, rx, ry) as ctx:
        # symmetry
        hv, hu = ctx.render_hvp(va, vq, g), ctx.render_hvp(ua, uq, g)
        lhs = float(ua @ hv[0] + uq @ hv[1])
        rhs = float(va @ hu[0] + vq @ hu[1])
        bar = 1e-9 * float(np.abs(ua * hv[0]).sum() + np.abs(uq * hv[1]).sum() + np.abs(va * hu[0]).sum() + np.abs(vq * hu[1]).sum())
        print(f"<u, H v> = {lhs:.15g}, <v, H u> = {rhs:.15g}, |difference| / bar = {abs(lhs - rhs) / bar:.3g}")
        assert abs(lhs - rhs) <= bar
        # I is linear in Q: the direction (0, Q) with g = (0, g_I) gives the adjoint's grad_alpha, and h_q identically 0
        g_I = g.copy()
        g_I[..., 0] = 0.0
        ha, hq = ctx.render_hvp(None, q, g_I)
        ga, _gq = ctx.render_adjoint(g_I)
        scale = ar.gradients_of(m, n, g_I, with_scale=True)[4]["scale_alpha"]
        print(f"hvp(v = (0, Q)) against the adjoint: worst |diff| / (1e-9 scale) = {(np.abs(ha - ga) / (1e-9 * scale + 2.0 ** -970)).max():.3g}")
        assert (np.abs(ha - ga) <= 1e-9 * scale + 2.0 ** -970).all() and np.abs(ga).max() > 0
        assert not hq.any()
        # a direction that moves only clamped or inactive cells
        d = np.where((alpha > LIMIT) | (alpha < EPS), rng.normal(size=n), 0.0)
        assert (d != 0).sum() > 10
        ha, hq = ctx.render_hvp(d, None, g)
        assert not ha.any() and not hq.any()
        # a zero channel 1 while channel 0 is not
        g_tau = g.copy()
        g_tau[..., 1] = 0.0
        ha, hq = ctx.render_hvp(va, vq, g_tau)
        assert g_tau.any() and not ha.any() and not hq.any()


def test_central_differences_of_the_librarys_own_adjoint():
    s = small_scene()
    g = s["g"].astype(np.float32)
    with _ctx(s["xyz"], s["cells"], s["alpha"], s["q"], ROTS, s["rx"], s["ry"]) as ctx:
        for va, vq in fd_directions(s):
            h = fd_step(s["alpha"], s["q"], va, vq)
            grads = []
            for sign in (1.0, -1.0):
                ctx.update_scalars(s["alpha"] + (sign * h * va if va is not None else 0.0), s["q"] + (sign * h * vq if vq is not None else 0.0))
                grads.append(ctx.render_adjoint(g))
            ctx.update_scalars(s["alpha"], s["q"])
            ha, hq = ctx.render_hvp(va, vq, g)
            fd = [(grads[0][k] - grads[1][k]) / (2.0 * h) for k in range(2)]
            top = max(np.abs(ha).max(), np.abs(hq).max())
            err = max(np.abs(fd[0] - ha).max(), np.abs(fd[1] - hq).max()) / top
            print(f"central difference of c5_render_adjoint (h = {h:.3g}), alpha {va is not None} q {vq is not None}: {err:.3g} of the "
                  f"largest element (bar {10 * FD_SHOWN:g})")
            assert top > 0 and err <= 10 * FD_SHOWN


@pytest.mark.parametrize("opts", [(), (("depth_split", 2),), (("integration", 1),)], ids=["default", "split", "ftb"])
def test_render_after_an_hvp_is_bit_identical_and_stats_stay(opts):
    xyz, cells, rx, ry = _scene("box9")
    alpha, q, va, vq, rng = _draw(len(cells), 77)
    g = _image(rng, ry, rx)
    with _ctx(xyz, cells, alpha, q, ROTS, rx, ry, opts) as a, _ctx(xyz, cells, alpha, q, ROTS, rx, ry, opts) as b:
        for call in (lambda: a.render_hvp(va, vq, g), lambda: a.render_hvp(None, vq, g, fit=("alpha",))):
            for _ in range(3):  # (three frames: the view cache is in use by the third)
                a.render(), b.render()
            before = a.stats()
            call()
            assert a.stats() == before
            assert a.synchronize() == capi.C5_OK
            for _ in range(3):
                assert np.array_equal(_bits(a.render()), _bits(b.render()))
            assert a.stats()["segments"] == b.stats()["segments"]


def test_invalid_arguments_and_outstanding_frames():
    xyz, cells, rx, ry = _scene("box4")
    n = len(cells)
    alpha, q, _va, _vq, _rng = _draw(n, 78)
    with _ctx(xyz, cells, alpha, q, ROTS, rx, ry) as ctx:
        lib, h = ctx.lib, ctx.handle
        d = np.zeros(n)
        img = np.zeros((ry, rx, 2), np.float32)
        fp = img.ctypes.data_as(C.POINTER(C.c_float))
        dp = d.ctypes.data_as(C.POINTER(C.c_double))
        assert lib.c5_render_hvp(h, None, None, fp, dp, dp) == capi.C5_ERR_INVALID  # both directions NULL
        assert lib.c5_render_hvp(h, dp, dp, fp, None, None) == capi.C5_ERR_INVALID  # both outputs NULL
        assert lib.c5_render_hvp(h, dp, dp, None, dp, dp) == capi.C5_ERR_INVALID    # grad_out is required
        assert lib.c5_render_hvp(None, dp, dp, fp, dp, dp) == capi.C5_ERR_INVALID
        import torch
        cell_t = torch.zeros(n, dtype=torch.float64, device="cuda").data_ptr()
        img_t = torch.zeros((ry, rx, 2), dtype=torch.float32, device="cuda").data_ptr()
        assert lib.c5_render_hvp_device(h, None, None, img_t, cell_t, cell_t) == capi.C5_ERR_INVALID
        assert lib.c5_render_hvp_device(h, cell_t, cell_t, img_t, None, None) == capi.C5_ERR_INVALID
        assert lib.c5_render_hvp_device(h, cell_t, cell_t, None, cell_t, cell_t) == capi.C5_ERR_INVALID
        # refused while frames of c5_render_host_async are outstanding
        frame = ctx.host_image()
        assert lib.c5_render_host_async(h, frame.ctypes.data_as(C.POINTER(C.c_float))) == capi.C5_OK
        assert lib.c5_render_hvp(h, dp, dp, fp, dp, dp) == capi.C5_ERR_STATE
        assert lib.c5_render_hvp_device(h, cell_t, cell_t, img_t, cell_t, cell_t) == capi.C5_ERR_STATE
        assert lib.c5_render_host_wait(h) == capi.C5_OK
        ctx.free_host_image(frame)
        ctx.render_hvp(d, None, img)  # (the context is still good)


def test_newton_product_and_one_newton_step_for_alpha():
    import torch
    from course5_amd import autograd, fit
    s = newton_scene()
    n = s["n"]
    with _ctx(s["xyz"], s["cells"], s["alpha0"], s["q"], ROTS, s["rx"], s["ry"]) as ctx:
        a0, q = torch.tensor(s["alpha0"], device="cuda"), torch.tensor(s["q"], device="cuda")
        W = torch.tensor(s["weight"], device="cuda")
        target = autograd.render(ctx, torch.tensor(s["alpha_true"], device="cuda"), q).clone()
        residual = autograd.render(ctx, a0, q) - target

        def loss(alpha):
            r = (autograd.render(ctx, alpha, q) - target).double()
            return 0.5 * float((W.double() * r * r).sum())

        # newton_product = gn_product + hvp(grad_img = W r)
        rng = np.random.default_rng(79)
        va, vq = (torch.tensor(v, device="cuda") for v in rng.normal(size=(2, n)))
        na, nq = fit.newton_product(ctx, a0, q, residual, va, vq, W)
        ga, gq = autograd.gn_product(ctx, a0, q, va, vq, W)
        ha, hq = autograd.hvp(ctx, a0, q, va, vq, (W * residual).contiguous())
        for got, x, y in ((na, ga, ha), (nq, gq, hq)):
            assert bool(((got - (x + y)).abs() <= 1e-9 * (x.abs() + y.abs()) + 2.0 ** -970).all())
        assert float(ha.abs().max()) > 0
        # one Newton step for alpha (two CG iterations: tests/test_hvp_cpu.py, newton_scene) does not increase the loss, and
        # it is not the Gauss-Newton step
        loss0 = loss(a0)
        (d_newton, none), models = fit.newton_step(ctx, a0, q, residual, W, fit=("alpha",), iters=2)
        (d_gn, _), _gn_models = fit.gn_step(ctx, a0, q, residual, W, fit=("alpha",), iters=2)
        assert none is None and d_newton.shape == (n,)
        loss1, loss_gn = loss(a0 + d_newton), loss(a0 + d_gn)
        differ = float((d_newton - d_gn).norm() / d_gn.norm())
        print(f"loss {loss0:.6g} -> {loss1:.6g} after one Newton step ({len(models)} CG iterations), {loss_gn:.6g} after the "
              f"Gauss-Newton step; |d_newton - d_gn| / |d_gn| = {differ:.3g}")
        assert loss1 <= loss0
        assert differ > 1e-3

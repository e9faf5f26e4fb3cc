"""Hessian-vector render, no GPU: the numpy restatement (tests/hvp_reference.py) pinned to two 80-digit references
(tests/hvp_reference_mp.py) on the scenes of tests/test_derivative_references_cpu.py and to identities of its own, the C ABI
declarations and bindings, the wrappers' argument checks, and fit.newton_step on numpy operators.

Bar of the 80-digit pin: |numpy - mpmath| <= 64 x 2^-52 x scale per element, scale the element's absolute-sum scale
(DBL_MIN where it is smaller), the bar the other restatements are held to.  Worst ratios seen over the ten scenes (up to
200 sampled pixels each, every cell they touch, three directions): against the formulas as written 45 for h_alpha (seed
2016, a "threshold" scene: S_aa in closed form just above a dz = 1/8, where 2 S_a and dz^2 E cancel to 1/24 of their size)
and 1.67 for h_q (seed 2000); against the central difference of the adjoint at step 1e-25 the same to three digits - the
two references agree far below the bar.

THE STEP of the fp64 central differences (test_central_difference_of_the_restatements_own_gradient, and on the GPU
tests/test_gpu_hvp.py): relative 1e-4, that is h = 1e-4 x max(|alpha|, |Q|) / max|v|, as the issue proposes; the
restatement's own difference agrees with hvp_of within 2.4e-9 of its largest element there (bar 1e-6; FD_SHOWN).
"""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from course5_amd import capi
from course5_amd import meshgen as mg
from tests import adjoint_reference as ar
from tests.fake_library import bare_context
from tests import hvp_reference as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
B = mg.REFERENCE_BOUNDS
ROTS = mg.view_rotations(0.13, 0.21)
SEEDS = (2027, 2014, 2016, 2009, 2000, 2019, 2020, 2004, 2011, 2002)  # tests/test_derivative_references_cpu.py: SEEDS
N_PIXELS = 200
FD_STEP = 1e-4
FD_SHOWN = 2.5e-9  # what the restatement's own central difference shows at FD_STEP (module docstring); the GPU's margin is 10 x


def fd_step(alpha, q, va, vq, rel=FD_STEP):
    """The central differences' step: rel x the largest scalar over the largest component of the direction."""
    top = max(float(np.abs(v).max()) for v in (va, vq) if v is not None)
    return rel * max(float(np.abs(alpha).max()), float(np.abs(q).max())) / top


# ---- against 80 digits ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", SEEDS)
def test_restatement_against_80_digits(seed, oracle_port):
    from tests import derivative_fuzz as df
    from tests import derivative_reference_mp as dm
    from tests import hvp_reference_mp as hm
    """The pin covers the three modes of the fuzz scenes: among SEEDS 2027, 2014 and 2016 are "threshold" scenes (S_aa in
    closed form just above a dz = 1/8, cells at 0.125 / dz and its neighbouring doubles), 2009 and 2000 "underflow" scenes
    (T and E through the subnormals), the rest plain - the scenes tests/test_gpu_second_order_fuzz.py holds the kernel to."""
    s = df.derivative_scene(seed)
    assert df.qualify(s, oracle_port) is None
    rx, ry = s.res
    n = len(s.cells)
    pix, cell, _zh, dz = s.segments[:4]
    covered = np.unique(pix)
    pixels = covered if len(covered) <= N_PIXELS else np.sort(np.random.default_rng([seed, 2]).choice(covered, N_PIXELS, replace=False))
    seg = dm.Segments(pix, cell, dz, s.alpha, s.q, s.limit, pixels)
    chosen = np.zeros(rx * ry, bool)
    chosen[pixels] = True
    g = np.where(chosen[:, None], s.g[0].reshape(-1, 2).astype(np.float64), 0.0)
    m = ar.ray_matrices(s.xyz, s.cells, s.alpha, s.q, s.rots, rx, ry, B, s.limit)
    rng = np.random.default_rng([seed, 3])
    da = rng.normal(size=n) if s.d_alpha is None else s.d_alpha[0]
    dq = rng.normal(size=n) if s.d_q is None else s.d_q[0]
    worst = {}
    for va, vq in ((da, dq), (da, None), (None, dq)):
        ha, hq, x = hr.hvp_of(m, n, va, vq, g, with_scale=True)
        want = hm.hvp(seg, n, va, vq, g[pixels])
        by_difference = hm.hvp_by_difference(seg, n, va, vq, g[pixels])
        for name in ("scale_alpha", "scale_q"):
            np.testing.assert_allclose(x[name], want[name], rtol=1e-9, atol=2.0 ** -970, err_msg=name)
        for what, got, refs, scale in (("h_alpha", ha, (want["alpha"], by_difference[0]), x["scale_alpha"]),
                                       ("h_q", hq, (want["q"], by_difference[1]), x["scale_q"])):
            for which, ref in zip(("as written", "difference"), refs):
                r = np.abs(got - ref) / (2.0 ** -52 * np.maximum(scale, 2.0 ** -1022))
                worst[what, which] = max(worst.get((what, which), 0.0), float(r.max()))
    print(f"seed {seed} ({seg.n_segments} segments on {len(pixels)} pixels at 80 digits): "
          + ", ".join(f"{k[0]} {k[1]} {v:.3g}" for k, v in worst.items()) + "  [x 2^-52 x scale]")
    for k, v in worst.items():
        assert v <= 64, (k, v)


@pytest.mark.parametrize("block", range(8))
def test_restatement_is_finite_on_the_fuzz_seeds_of_the_gpu_sweep(block, oracle_port):
    """hvp_of with direction 0 and g[0] on the 40 seeds of tests/test_gpu_second_order_fuzz.py (8 blocks of 5; the covered
    pixels of the whole image): every result, scale and sensitivity is finite - the "underflow" scenes run T and E through
    the subnormals - and h_alpha is not identically zero (the fewest non-zero elements: 1 in seed 3029, 21 in seed 3006)."""
    from tests import derivative_fuzz as df
    for seed in range(3000 + 5 * block, 3005 + 5 * block):
        s = df.derivative_scene(seed)
        assert df.qualify(s, oracle_port) is None
        rx, ry = s.res
        rows = np.unique(s.segments[0] // rx)  # (a row without a segment adds nothing)
        m = ar.ray_matrices(s.xyz, s.cells, s.alpha, s.q, s.rots, rx, ry, B, s.limit, rows)
        cov, mc, _ = df.covered_only(m, {})
        da = None if s.d_alpha is None else s.d_alpha[0]
        dq = None if s.d_q is None else s.d_q[0]
        ha, hq, x = hr.hvp_of(mc, len(s.cells), da, dq, s.g[0][rows].reshape(-1, 2)[cov], with_scale=True)
        assert np.isfinite(ha).all() and np.isfinite(hq).all(), seed
        assert set(x) == {"scale_alpha", "scale_q", "sens_alpha", "sens_q"} and all(np.isfinite(v).all() for v in x.values()), seed
        print(f"seed {seed} ({s.mode}): {int((ha != 0).sum())} non-zero elements of h_alpha, {int((hq != 0).sum())} of h_q")
        assert (ha != 0).any(), seed


# ---- identities on the restatement ----------------------------------------------------------------------------------

def small_scene():
    """Kuhn box 3 at 24 x 18, limit 2.5, with the special scalars on cells the image sees: a clamped alpha, inactive
    cells, cells whose a dz lies in the series range, and the rest on both sides of a dz = 1/8.  (Also the scene of the
    GPU's central differences, tests/test_gpu_hvp.py: the step's truncation error is this scene's.)"""
    xyz, cells = mg.kuhn_box(3, jitter=0.1)
    n = len(cells)
    rng = np.random.default_rng(41)
    alpha = rng.uniform(0.05, 2.0, n)
    q = rng.uniform(0.1, 1.0, n)
    alpha[5], alpha[11], alpha[17], alpha[23], alpha[29] = 3.7, 0.5 * EPS, 0.0, 0.02, 1e-5
    rx, ry = 24, 18
    g = rng.normal(size=(ry, rx, 2))
    return dict(xyz=xyz, cells=cells, alpha=alpha, q=q, rx=rx, ry=ry, n=n, g=g, frozen=np.array([5]), inactive=np.array([11, 17]))


def fd_directions(s, seed=45):
    """Three directions (both fields, alpha only, q only) for the central differences: d_alpha zero on the cells a finite
    step would carry across the activity threshold (an inactive alpha has no column and the step would wake it up; one
    within the step of DBL_EPSILON would be put to sleep: cell 29 at 1e-5)."""
    rng = np.random.default_rng(seed)
    out = []
    for use_a, use_q in ((True, True), (True, False), (False, True)):
        va = rng.normal(size=s["n"]) if use_a else None
        vq = rng.normal(size=s["n"]) if use_q else None
        if va is not None:
            va[s["alpha"] < 1e-3] = 0.0
        out.append((va, vq))
    return out


def newton_scene():
    """The 4-box at 37 x 29 with a fit of alpha to the intensity image (weights 0 on tau, which is linear in alpha and
    would drown the curvature, 1 on I) in mid-course: alpha_0 = alpha_true x U[0.8, 1.2), all of it below the limit and
    active.  Chosen so that the exact Hessian and the Gauss-Newton one differ: along the gradient the curvature term is
    a few per cent of the Gauss-Newton product (test_the_newton_scene_has_curvature_the_gauss_newton_product_leaves_out),
    and two CG iterations of either step lower the loss (test_newton_step_on_the_restatements_operators: one view does not
    determine 384 cells, and a longer CG run follows the nearly flat directions of either Hessian out of the range where the
    quadratic model holds - with the spread 0.4 or with three iterations both steps INCREASE the loss on the restatement)."""
    xyz, cells = mg.kuhn_box(4, jitter=0.1)
    n = len(cells)
    rng = np.random.default_rng(61)
    alpha_true = rng.uniform(0.3, 1.7, n)
    q = rng.uniform(0.2, 1.0, n)
    alpha0 = alpha_true * rng.uniform(0.8, 1.2, n)
    weight = np.zeros((29, 37, 2), np.float32)
    weight[..., 1] = 1.0
    return dict(xyz=xyz, cells=cells, alpha_true=alpha_true, alpha0=alpha0, q=q, rx=37, ry=29, n=n, weight=weight)


@pytest.fixture(scope="module")
def small():
    s = small_scene()
    m = ar.ray_matrices(s["xyz"], s["cells"], s["alpha"], s["q"], ROTS, s["rx"], s["ry"], B, 2.5)
    x = (m["a"] * m["D"])[m["active"]]
    assert (x < 0.125).sum() > 50 and (x >= 0.125).sum() > 50
    assert {5, 11, 17, 23, 29} <= set(m["C"][m["valid"]].tolist())
    s["m"] = m
    return s


def test_symmetry(small):
    s = small
    rng = np.random.default_rng(42)
    u = rng.normal(size=(2, s["n"]))
    v = rng.normal(size=(2, s["n"]))
    hu = hr.hvp_of(s["m"], s["n"], u[0], u[1], s["g"])
    hv = hr.hvp_of(s["m"], s["n"], v[0], v[1], s["g"])
    lhs = u[0] @ hv[0] + u[1] @ hv[1]
    rhs = v[0] @ hu[0] + v[1] @ hu[1]
    bar = 1e-12 * sum(float(np.abs(a * b).sum()) for a, b in ((u[0], hv[0]), (u[1], hv[1]), (v[0], hu[0]), (v[1], hu[1])))
    assert abs(lhs - rhs) <= bar


def test_a_direction_in_q_gives_the_adjoint_because_I_is_linear_in_q(small):
    s = small
    g = s["g"].copy()
    g[..., 0] = 0.0
    ha, hq = hr.hvp_of(s["m"], s["n"], None, s["q"], g)
    ga, _gq, _tau, _I, x = ar.gradients_of(s["m"], s["n"], g, with_scale=True)
    assert np.array_equal(hq, np.zeros(s["n"]))
    assert (np.abs(ha - ga) <= 1e-12 * x["scale_alpha"]).all()
    assert np.abs(ga).max() > 0


def test_clamped_or_inactive_directions_and_a_zero_channel_give_zero(small):
    s = small
    d = np.zeros(s["n"])
    d[s["frozen"]] = 3.0
    d[s["inactive"]] = -2.0
    ha, hq = hr.hvp_of(s["m"], s["n"], d, None, s["g"])
    assert not ha.any() and not hq.any()
    # a clamped cell has no row either, an inactive one neither row
    v = np.random.default_rng(43).normal(size=(2, s["n"]))
    ha, hq = hr.hvp_of(s["m"], s["n"], v[0], v[1], s["g"])
    assert not ha[s["frozen"]].any() and not ha[s["inactive"]].any() and not hq[s["inactive"]].any()
    assert hq[s["frozen"]].any()
    g = s["g"].copy()
    g[..., 1] = 0.0
    ha, hq, x = hr.hvp_of(s["m"], s["n"], v[0], v[1], g, with_scale=True)
    assert not ha.any() and not hq.any() and not any(t.any() for t in x.values())


def test_skipped_pixels_and_row_parts(small):
    s = small
    v = np.random.default_rng(44).normal(size=(2, s["n"]))
    skip = np.zeros((s["ry"], s["rx"]), bool)
    skip[:, : s["rx"] // 2] = True
    g0 = s["g"].copy()
    g0[skip] = 0.0
    a = hr.hvp_of(s["m"], s["n"], v[0], v[1], s["g"], skip)
    b = hr.hvp_of(s["m"], s["n"], v[0], v[1], g0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    whole = hr.hvp_of(s["m"], s["n"], v[0], v[1], s["g"])
    parts = [hr.hvp_of(ar.ray_matrices(s["xyz"], s["cells"], s["alpha"], s["q"], ROTS, s["rx"], s["ry"], B, 2.5, rows=r),
                       s["n"], v[0], v[1], s["g"][r]) for r in (np.arange(0, 7), np.arange(7, s["ry"]))]
    for k in range(2):
        assert np.abs(parts[0][k] + parts[1][k] - whole[k]).max() <= 1e-12 * np.abs(whole[k]).max()


def test_central_difference_of_the_restatements_own_gradient(small):
    s = small
    g = s["g"]
    for va, vq in fd_directions(s):
        h = fd_step(s["alpha"], s["q"], va, vq)
        grads = []
        for sign in (1.0, -1.0):
            alpha = s["alpha"] + (sign * h * va if va is not None else 0.0)
            q = s["q"] + (sign * h * vq if vq is not None else 0.0)
            grads.append(ar.image_gradients(s["xyz"], s["cells"], alpha, q, ROTS, s["rx"], s["ry"], B, g)[:2])
        fd = [(grads[0][k] - grads[1][k]) / (2.0 * h) for k in range(2)]
        ha, hq = hr.hvp_of(s["m"], s["n"], va, vq, g)
        top = max(np.abs(ha).max(), np.abs(hq).max())
        err = max(np.abs(fd[0] - ha).max(), np.abs(fd[1] - hq).max()) / top
        print(f"central difference at relative step {FD_STEP:g} (h = {h:.3g}), alpha {va is not None} q {vq is not None}: "
              f"{err:.3g} of the largest element")
        assert err <= FD_SHOWN
    assert FD_SHOWN <= 1e-6


def test_the_newton_scene_has_curvature_the_gauss_newton_product_leaves_out():
    from tests import gn_reference as gr
    s = newton_scene()
    n, rx, ry = s["n"], s["rx"], s["ry"]
    m0 = ar.ray_matrices(s["xyz"], s["cells"], s["alpha0"], s["q"], ROTS, rx, ry, B, 2.5)
    m1 = ar.ray_matrices(s["xyz"], s["cells"], s["alpha_true"], s["q"], ROTS, rx, ry, B, 2.5)
    r = np.stack(ar.forward_of(m0), axis=-1) - np.stack(ar.forward_of(m1), axis=-1)
    wr = s["weight"] * r
    g = ar.gradients_of(m0, n, wr)[0]  # J^T W r: the first CG direction but for the preconditioner
    terms = gr.segment_terms(s["xyz"], s["cells"], s["alpha0"], s["q"], ROTS, rx, ry, B)
    gn = gr.product(terms, rx * ry, n, g, None, s["weight"])[0]
    curv = hr.hvp_of(m0, n, g, None, wr)[0]
    share = np.linalg.norm(curv) / np.linalg.norm(gn)
    print(f"|sum w r Hess(I) v| / |J^T W J v| along the gradient: {share:.3g}")
    assert share > 0.02


class _RestatementOperators:
    """fit's operator hook on the numpy restatements: the frame of newton_scene() at alpha, on the CPU."""

    def __init__(self, s, alpha):
        from tests import gn_reference as gr
        self.s, self.gr, self.n_px = s, gr, s["rx"] * s["ry"]
        self.m = ar.ray_matrices(s["xyz"], s["cells"], alpha, s["q"], ROTS, s["rx"], s["ry"], B, 2.5)
        self.terms = gr.segment_terms(s["xyz"], s["cells"], alpha, s["q"], ROTS, s["rx"], s["ry"], B)
        self.image = np.stack(ar.forward_of(self.m), axis=-1)

    def gn_operators(self, alpha, q, weight):
        return self

    @staticmethod
    def _np(t):
        return None if t is None else t.numpy().astype(np.float64)

    @staticmethod
    def _pair(a, b):
        import torch
        return torch.tensor(a), torch.tensor(b)

    def rhs(self, residual):
        return self._pair(*ar.gradients_of(self.m, self.s["n"], self.s["weight"] * self._np(residual))[:2])

    def diagonal(self):
        return self._pair(*self.gr.diagonal(self.terms, self.n_px, self.s["n"], self.s["weight"]))

    def product(self, va, vq):
        return self._pair(*self.gr.product(self.terms, self.n_px, self.s["n"], self._np(va), self._np(vq), self.s["weight"])[:2])

    def hvp(self, va, vq, grad_img):
        return self._pair(*hr.hvp_of(self.m, self.s["n"], self._np(va), self._np(vq), self._np(grad_img)))


def test_newton_step_on_the_restatements_operators():
    """The scene of the GPU's Newton step (tests/test_gpu_hvp.py), driven through the gn_operators hook on the CPU: two CG
    iterations lower the loss, and the Newton step is not the Gauss-Newton step."""
    import torch
    from course5_amd import fit
    s = newton_scene()
    W = s["weight"].astype(np.float64)
    target = _RestatementOperators(s, s["alpha_true"]).image
    ops = _RestatementOperators(s, s["alpha0"])
    residual = torch.tensor(ops.image - target)

    def loss(alpha):
        return 0.5 * float((W * (_RestatementOperators(s, alpha).image - target) ** 2).sum())

    a0, q = torch.tensor(s["alpha0"]), torch.tensor(s["q"])
    (d_newton, none), models = fit.newton_step(ops, a0, q, residual, torch.tensor(s["weight"]), fit=("alpha",), iters=2)
    (d_gn, _), _models = fit.gn_step(ops, a0, q, residual, torch.tensor(s["weight"]), fit=("alpha",), iters=2)
    loss0, loss1, loss_gn = loss(s["alpha0"]), loss(s["alpha0"] + d_newton.numpy()), loss(s["alpha0"] + d_gn.numpy())
    differ = float((d_newton - d_gn).norm() / d_gn.norm())
    print(f"loss {loss0:.6g} -> {loss1:.6g} (Newton, {len(models)} iterations), {loss_gn:.6g} (Gauss-Newton); "
          f"|d_newton - d_gn| / |d_gn| = {differ:.3g}")
    assert none is None and len(models) == 2
    assert loss1 < loss0 and differ > 1e-3


# ---- the C ABI and the bindings ---------------------------------------------------------------------------------------

def _header():
    text = open(os.path.join(ROOT, "include", "course5_hip.h")).read()
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def test_header_declares_the_two_calls():
    h = _header()
    for decl in (
        "int c5_render_hvp(c5_context* ctx, const double* d_alpha_host, const double* d_q_host, const float* grad_out_host, "
        "double* h_alpha_host, double* h_q_host);",
        "int c5_render_hvp_device(c5_context* ctx, const void* d_alpha_dev, const void* d_q_dev, const void* grad_out_dev, "
        "void* h_alpha_dev, void* h_q_dev);",
    ):
        assert decl in h, decl
    assert "#define C5_ABI_VERSION 2" in h


def test_library_and_bindings_have_them():
    lib = ctypes.CDLL(capi.LIB_PATH)
    exported = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("c5_render_hvp", "c5_render_hvp_device"):
        assert re.search(rf" T {name}$", exported, re.M), name
        assert hasattr(lib, name) and name in capi.EXPORTS
    assert lib.c5_abi_version() == 2
    for name in ("render_hvp", "render_hvp_device"):
        assert callable(getattr(capi.Context, name)), name
    from course5_amd import autograd, fit
    assert "hvp" in autograd.__all__ and "hvp()" in autograd.render.__doc__
    assert list(inspect.signature(autograd.hvp).parameters) == ["ctx", "alpha", "q", "v_alpha", "v_q", "grad_img"]
    assert list(inspect.signature(fit.newton_product).parameters) == ["ctx", "alpha", "q", "residual", "v_alpha", "v_q", "weight"]
    p = inspect.signature(fit.newton_step).parameters
    assert list(p) == ["ctx", "alpha", "q", "residual", "weight", "fit", "damping", "iters"]
    assert p["fit"].default == ("q",) and p["damping"].default == 0.0 and p["iters"].default == 10


def test_the_forward_kernels_are_untouched():
    from course5_amd import build
    assert build.DEVICE_SOURCES == ("device_types.hpp", "kernels.hpp", "walk_common.hpp", "walk_plan.hpp", "tile_of_block_body.hpp", "walk_steps.hpp", "walk_stamps.hpp",
                                    "exact_kernels.hip", "walk_kernels.hip", "setup_kernels.hip")
    assert build.kernel_source_hash() == "63c90aeb24365e47"  # (re-stamped with next_entry: profiles/component_fuzz.md)


def test_argument_checks_raise_before_the_library():
    ctx = bare_context()
    g = np.zeros((5, 6, 2), np.float32)
    with pytest.raises(ValueError, match=r"one value per cell \(7\)"):
        ctx.render_hvp(np.zeros(8), None, g)
    with pytest.raises(ValueError, match=r"one value per cell \(7\)"):
        ctx.render_hvp(np.zeros(7), np.zeros((1, 7)), g)
    with pytest.raises(ValueError, match="give d_alpha and / or d_q"):
        ctx.render_hvp(None, None, g)
    with pytest.raises(ValueError, match="grad_out is required"):
        ctx.render_hvp(np.zeros(7), None, None)
    with pytest.raises(ValueError, match=r"grad_out must be \[5, 6, 2\]"):
        ctx.render_hvp(np.zeros(7), None, np.zeros((5, 6)))
    with pytest.raises(ValueError, match="fit must name"):
        ctx.render_hvp(np.zeros(7), None, g, fit=())
    with pytest.raises(ValueError, match="give d_alpha and / or d_q"):
        ctx.render_hvp_device(None, None, 1, 2, 3)
    with pytest.raises(ValueError, match="give h_alpha and / or h_q"):
        ctx.render_hvp_device(1, None, 1, None, None)
    with pytest.raises(ValueError, match="grad_out is required"):
        ctx.render_hvp_device(1, None, None, 2, 3)
    import torch
    with pytest.raises(ValueError, match="expected a contiguous"):
        ctx.render_hvp_device(torch.zeros(7, dtype=torch.float64), None, 1, 2, 3)  # (not on the GPU)


# ---- fit.newton_step on numpy operators -----------------------------------------------------------------------------

class _DenseContext:
    """A mock context: a dense J [m, 2 n], weights, and a symmetric K [2 n, 2 n] standing for sum_p (W r)_p Hess(img_p)."""

    def __init__(self, J, w, K):
        import torch
        self.J, self.w, self.K, self.n = torch.tensor(J), torch.tensor(w), torch.tensor(K), J.shape[1] // 2
        self.hvps = 0

    def gn_operators(self, alpha, q, weight):
        return self

    def _v(self, va, vq):
        import torch
        return torch.cat([torch.zeros(self.n, dtype=torch.float64) if t is None else t for t in (va, vq)])

    def rhs(self, residual):
        g = self.J.T @ (self.w * residual)
        return g[:self.n], g[self.n:]

    def diagonal(self):
        d = (self.J * self.J * self.w[:, None]).sum(0)
        return d[:self.n], d[self.n:]

    def product(self, va, vq):
        h = self.J.T @ (self.w * (self.J @ self._v(va, vq)))
        return h[:self.n], h[self.n:]

    def hvp(self, va, vq, grad_img):
        self.hvps += 1
        self.seen_grad = grad_img
        h = self.K @ self._v(va, vq)
        return h[:self.n], h[self.n:]


def _problem(seed, n=12, m=60):
    rng = np.random.default_rng(seed)
    J = rng.normal(size=(m, 2 * n)) * rng.uniform(0.2, 3.0, 2 * n)
    return J, rng.uniform(0.1, 2.0, m), rng.normal(size=m), rng


def _cg(A, g, d, iters):
    """The iteration newton_step documents, dense: Jacobi-preconditioned CG that stops at the first direction without
    positive curvature (the first direction itself if it is the first)."""
    x, r = np.zeros_like(g), -g
    z = r / d
    p, rz = z.copy(), r @ z
    for it in range(iters):
        ap = A @ p
        if not p @ ap > 0:
            return (p if it == 0 else x), it
        step = rz / (p @ ap)
        x, r = x + step * p, r - step * ap
        z = r / d
        rz, rz_old = r @ z, rz
        p = z + (rz / rz_old) * p
    return x, iters


@pytest.mark.parametrize("fit_fields", [("alpha", "q"), ("alpha",), ("q",)])
def test_newton_step_on_an_spd_operator_is_gn_step(fit_fields):
    import torch
    from course5_amd import fit
    J, w, r, rng = _problem(51)
    n = J.shape[1] // 2
    zero = torch.zeros(n, dtype=torch.float64)
    for K in (np.zeros((2 * n, 2 * n)), (lambda a: 0.05 * (a @ a.T))(rng.normal(size=(2 * n, 2 * n)))):
        ctx = _DenseContext(J, w, K)
        iters = 2 * n + 10
        (da, dq), models = fit.newton_step(ctx, zero, zero, torch.tensor(r), fit=fit_fields, iters=iters)
        got = np.concatenate([t.numpy() for t in (da, dq) if t is not None])
        assert (da is None) == ("alpha" not in fit_fields) and (dq is None) == ("q" not in fit_fields)
        assert ctx.hvps == len(models) and np.array_equal(ctx.seen_grad.numpy(), r.astype(np.float32))
        if not K.any():
            (ga, gq), gn_models = fit.gn_step(ctx, zero, zero, torch.tensor(r), fit=fit_fields, iters=iters)
            want = np.concatenate([t.numpy() for t in (ga, gq) if t is not None])
            assert np.array_equal(got, want) and models == gn_models
        cols = np.r_[np.arange(n) if "alpha" in fit_fields else [], n + np.arange(n) if "q" in fit_fields else []].astype(int)
        Js = J[:, cols]
        H = Js.T @ (w[:, None] * Js) + K[np.ix_(cols, cols)]
        want = np.linalg.solve(H, -(Js.T @ (w * r)))
        assert np.abs(got - want).max() <= 1e-8 * np.abs(want).max()


def test_newton_product_is_the_sum_and_weighs_the_residual():
    import torch
    from course5_amd import fit
    J, w, r, rng = _problem(52)
    n = J.shape[1] // 2
    K = rng.normal(size=(2 * n, 2 * n))
    K = K + K.T
    ctx = _DenseContext(J, w, K)
    v = torch.tensor(rng.normal(size=2 * n))
    weight = torch.tensor(rng.uniform(0.5, 1.5, len(r)))
    ha, hq = fit.newton_product(ctx, torch.zeros(n), torch.zeros(n), torch.tensor(r), v[:n], v[n:], weight)
    want = J.T @ (w * (J @ v.numpy())) + K @ v.numpy()
    assert np.allclose(np.concatenate([ha.numpy(), hq.numpy()]), want, rtol=1e-12, atol=0)
    assert np.array_equal(ctx.seen_grad.numpy(), r.astype(np.float32) * weight.numpy().astype(np.float32))


@pytest.mark.parametrize("shift,first", [(-50.0, True), (-0.6, False)])
def test_newton_step_stops_at_negative_curvature(shift, first):
    """An indefinite operator: H_gn + shift x diag(H_gn).  At -50 the very first direction has negative curvature and the
    step is that direction (preconditioned steepest descent); at -0.6 the iteration runs into one later and returns the
    iterate it had."""
    import torch
    from course5_amd import fit
    J, w, r, _rng = _problem(53)
    n = J.shape[1] // 2
    H = J.T @ (w[:, None] * J)
    K = shift * np.diag(np.diag(H))
    assert np.linalg.eigvalsh(H + K).min() < 0
    g, d = J.T @ (w * r), np.diag(H).copy()
    want, done = _cg(H + K, g, d, 2 * n + 10)
    assert (done == 0) == first and done < 2 * n
    ctx = _DenseContext(J, w, K)
    zero = torch.zeros(n, dtype=torch.float64)
    (da, dq), models = fit.newton_step(ctx, zero, zero, torch.tensor(r), fit=("alpha", "q"), iters=2 * n + 10)
    got = np.concatenate([da.numpy(), dq.numpy()])
    assert len(models) == done and ctx.hvps == done + 1
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()
    if first:
        assert np.allclose(got, -g / d, rtol=1e-12, atol=0) and got @ g < 0  # a descent direction


def test_newton_step_refuses_bad_arguments():
    import torch
    from course5_amd import fit
    z = torch.zeros(3, dtype=torch.float64)
    for kw in (dict(fit=()), dict(fit=("tau",)), dict(fit=("q", "q")), dict(damping=-1.0), dict(iters=0)):
        with pytest.raises(ValueError):
            fit.newton_step(None, z, z, z, **kw)

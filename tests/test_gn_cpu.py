"""Gauss-Newton renders, no GPU: the C ABI declarations and bindings, the numpy restatement (tests/gn_reference.py) pinned
to the adjoint's and the tangent's, fit.gn_step against a dense solve, and `course --sensitivity`'s parse-time checks."""
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
from tests import gn_reference as gr
from tests import tangent_reference as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COURSE = os.path.join(ROOT, "course5_amd", "course")
EPS = np.finfo(np.float64).eps
B = mg.REFERENCE_BOUNDS
ROTS = mg.view_rotations(0.13, 0.21)


def _header():
    text = open(os.path.join(ROOT, "include", "course5_hip.h")).read()
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def test_header_declares_the_four_calls():
    h = _header()
    for decl in (
        "int c5_render_gn_product(c5_context* ctx, int n_dirs, const double* d_alpha_host, const double* d_q_host, "
        "const float* weight_host, double* h_alpha_host, double* h_q_host, float* jv_out_host);",
        "int c5_render_gn_product_device(c5_context* ctx, int n_dirs, const void* d_alpha_dev, const void* d_q_dev, "
        "const void* weight_dev, void* h_alpha_dev, void* h_q_dev, void* jv_out_dev);",
        "int c5_render_gn_diagonal(c5_context* ctx, const float* weight_host, double* diag_alpha_host, double* diag_q_host);",
        "int c5_render_gn_diagonal_device(c5_context* ctx, const void* weight_dev, void* diag_alpha_dev, void* diag_q_dev);",
    ):
        assert decl in h, decl
    assert "#define C5_ABI_VERSION 2" in h


def test_library_and_bindings_have_them():
    lib = ctypes.CDLL(capi.LIB_PATH)
    for name in ("c5_render_gn_product", "c5_render_gn_product_device", "c5_render_gn_diagonal", "c5_render_gn_diagonal_device"):
        assert hasattr(lib, name), name
        assert name in capi.EXPORTS
    for name in ("render_gn_product", "render_gn_product_device", "render_gn_diagonal", "render_gn_diagonal_device"):
        assert callable(getattr(capi.Context, name)), name
    from course5_amd import autograd, fit
    assert callable(autograd.gn_product) and callable(autograd.gn_diagonal) and callable(fit.gn_step)
    params = inspect.signature(fit.gn_step).parameters
    assert list(params)[:4] == ["ctx", "alpha", "q", "residual"]
    assert params["fit"].default == ("q",) and params["damping"].default == 0.0 and params["precondition"].default is True


def test_argument_checks_raise_before_the_library():
    ctx = bare_context()
    good = np.zeros((2, 7))
    with pytest.raises(ValueError, match=r"directions must be \[K, 7\]"):
        ctx.render_gn_product(np.zeros(7), None)
    with pytest.raises(ValueError, match=r"directions must be \[K, 7\]"):
        ctx.render_gn_product(good, np.zeros((2, 8)))
    with pytest.raises(ValueError, match="same number of directions"):
        ctx.render_gn_product(good, np.zeros((3, 7)))
    with pytest.raises(ValueError, match="same number of directions"):
        ctx.render_gn_product(None, None)
    with pytest.raises(ValueError, match=r"weight must be \[5, 6, 2\]"):
        ctx.render_gn_product(good, good, weight=np.zeros((5, 6)))
    with pytest.raises(ValueError, match="fit must name"):
        ctx.render_gn_product(good, good, fit=())
    with pytest.raises(ValueError, match=r"weight must be \[5, 6, 2\]"):
        ctx.render_gn_diagonal(np.zeros((6, 5, 2)))
    with pytest.raises(ValueError, match="give d_alpha and / or d_q"):
        ctx.render_gn_product_device(None, None, None, 1, 2, n=2)
    with pytest.raises(ValueError, match="give h_alpha and / or h_q"):
        ctx.render_gn_product_device(1, None, None, None, None, n=2)


def test_device_sources_hash_and_abi_version_stay():
    from course5_amd import build
    assert build.DEVICE_SOURCES == ("device_types.hpp", "kernels.hpp", "walk_common.hpp", "walk_plan.hpp", "tile_of_block_body.hpp", "walk_steps.hpp", "walk_stamps.hpp",
                                    "exact_kernels.hip", "walk_kernels.hip", "setup_kernels.hip")
    assert build.kernel_source_hash() == "63c90aeb24365e47"  # (re-stamped with next_entry: profiles/component_fuzz.md)
    assert ctypes.CDLL(capi.LIB_PATH).c5_abi_version() == 2


def test_the_derivative_kernels_are_three_translation_units():
    from course5_amd import build
    listed = [name for name, _ in build.LIB_SOURCES]
    for name in sorted(os.listdir(build.CSRC)):
        if name.endswith((".hip", ".cpp")):
            assert listed.count(name) == 1, name
    assert not os.path.exists(os.path.join(build.CSRC, "adjoint_kernels.hip"))
    flags = dict(build.LIB_SOURCES)
    for name in ("scalar_derivative_kernels.hip", "geometry_derivative_kernels.hip", "ray_matrix_kernels.hip"):
        assert "-munsafe-fp-atomics" in flags[name], name


# ---- the restatement ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small():
    """Kuhn box 3 at 24 x 18 with the special scalars on cells the image sees: a clamped alpha, an inactive cell, and
    cells whose alpha x chord lies in the series range (below 1/8)."""
    xyz, cells = mg.kuhn_box(3, jitter=0.1)
    n = len(cells)
    rng = np.random.default_rng(31)
    alpha = rng.uniform(0.3, 2.0, n)
    q = rng.uniform(0.1, 1.0, n)
    alpha[5] = 3.7          # clamped at 2.5: dI/dalpha = 0, dtau/dalpha = dz
    alpha[11] = 0.5 * EPS   # inactive: nothing in I
    alpha[17] = 0.0
    alpha[23] = 0.02        # alpha dz < 1/8 on every chord: the series
    alpha[29] = 1e-5
    rx, ry = 24, 18
    lists = gr.pixel_lists(xyz, cells, ROTS, rx, ry, B)
    seen = {c for segs in lists for c, _z, _d in segs}
    assert {5, 11, 17, 23, 29} <= seen
    assert max(d for segs in lists for c, _z, d in segs if c in (23, 29)) * 0.02 < 0.125
    J = gr.dense_jacobian(lists, alpha, q, n)
    terms = gr.segment_terms(xyz, cells, alpha, q, ROTS, rx, ry, B)
    return dict(xyz=xyz, cells=cells, alpha=alpha, q=q, rx=rx, ry=ry, n=n, J=J, terms=terms, rng=rng)


def _rel(got, want):
    return np.abs(got - want).max() / np.abs(want).max()


def test_a_ray_crosses_a_cell_once(small):
    P, C = small["terms"][:2]
    assert len(np.unique(P * small["n"] + C)) == len(P)


def test_product_is_the_adjoint_of_the_weighted_tangent(small):
    s = small
    n, n_px, J = s["n"], s["rx"] * s["ry"], s["J"]
    rng = np.random.default_rng(32)
    w = rng.uniform(0.0, 2.0, (s["ry"], s["rx"], 2))
    w[: s["ry"] // 3] = 0.0
    for va, vq, weight in ((rng.normal(size=n), rng.normal(size=n), w), (rng.normal(size=n), None, w),
                           (None, rng.normal(size=n), w), (rng.normal(size=n), rng.normal(size=n), None)):
        v = np.concatenate([np.zeros(n) if va is None else va, np.zeros(n) if vq is None else vq])
        W = np.ones(2 * n_px) if weight is None else weight.reshape(-1)
        dense = J.T @ (W * (J @ v))
        ha, hq, jv = gr.product(s["terms"], n_px, n, va, vq, weight)
        # the two restatements of the adjoint and of the tangent, composed
        t = tr.image_tangent(s["xyz"], s["cells"], s["alpha"], s["q"], ROTS, s["rx"], s["ry"], B, va, vq)[:2]
        jv_ref = np.stack(t, axis=-1)
        g = jv_ref if weight is None else weight * jv_ref
        ca, cq = ar.image_gradients(s["xyz"], s["cells"], s["alpha"], s["q"], ROTS, s["rx"], s["ry"], B, g)[:2]
        assert _rel(jv.reshape(-1), J @ v) <= 1e-12 and _rel(jv.reshape(jv_ref.shape), jv_ref) <= 1e-12
        for got in (np.concatenate([ha, hq]), np.concatenate([ca, cq])):
            assert _rel(got, dense) <= 1e-12
        assert _rel(ha, dense[:n]) <= 1e-12 and _rel(hq, dense[n:]) <= 1e-12


def test_diagonal_is_the_dense_diagonal(small):
    s = small
    n, n_px, J = s["n"], s["rx"] * s["ry"], s["J"]
    rng = np.random.default_rng(33)
    w = rng.uniform(0.0, 2.0, (s["ry"], s["rx"], 2))
    w[s["ry"] // 2:] = 0.0
    for weight in (None, w):
        W = np.ones(2 * n_px) if weight is None else weight.reshape(-1)
        dense = np.einsum("pc,p,pc->c", J, W, J)
        da, dq = gr.diagonal(s["terms"], n_px, n, weight)
        assert _rel(da, dense[:n]) <= 1e-12 and _rel(dq, dense[n:]) <= 1e-12
        assert (da >= 0).all() and (dq >= 0).all()
        # the special cells: clamped - only tau's term; inactive - none in I
        P, C, dtau = s["terms"][:3]
        w_tau = np.ones(n_px) if weight is None else weight.reshape(n_px, 2)[:, 0]
        for c in (5, 11, 17):
            assert da[c] == pytest.approx(float((w_tau[P[C == c]] * dtau[C == c] ** 2).sum()), rel=1e-12)
        assert dq[11] == 0.0 and dq[17] == 0.0
        if weight is None:
            assert dq[5] > 0 and dq[23] > 0 and da[23] > 0
            # diag[c] = e_c^T H e_c
            for c in (0, 5, 23, 40):
                e = np.zeros(n)
                e[c] = 1.0
                assert gr.product(s["terms"], n_px, n, e, None)[0][c] == pytest.approx(da[c], rel=1e-12)
                assert gr.product(s["terms"], n_px, n, None, e)[1][c] == pytest.approx(dq[c], rel=1e-12)


def test_rows_and_skipped_pixels(small):
    s = small
    n, rx, ry = s["n"], s["rx"], s["ry"]
    whole = gr.diagonal(s["terms"], rx * ry, n)
    parts = [gr.diagonal(gr.segment_terms(s["xyz"], s["cells"], s["alpha"], s["q"], ROTS, rx, ry, B, rows=r), len(r) * rx, n)
             for r in (np.arange(0, 7), np.arange(7, ry))]
    for k in range(2):
        assert _rel(parts[0][k] + parts[1][k], whole[k]) <= 1e-12
    skip = np.zeros((ry, rx), bool)
    skip[:, : rx // 2] = True
    w = np.ones((ry, rx, 2))
    w[skip] = 0.0
    a = gr.diagonal(gr.segment_terms(s["xyz"], s["cells"], s["alpha"], s["q"], ROTS, rx, ry, B, skip=skip), rx * ry, n)
    b = gr.diagonal(s["terms"], rx * ry, n, w)
    assert _rel(a[0], b[0]) <= 1e-12 and _rel(a[1], b[1]) <= 1e-12


# ---- fit.gn_step ----------------------------------------------------------------------------------------------------

class _DenseContext:
    """A mock context: a dense J [m, 2 n] and weights, its operators in torch on the CPU."""

    def __init__(self, J, w):
        import torch
        self.J, self.w, self.n = torch.tensor(J), torch.tensor(w), J.shape[1] // 2
        self.products = self.diagonals = self.adjoints = 0

    def gn_operators(self, alpha, q, weight):
        assert weight is None
        return self

    def rhs(self, residual):
        self.adjoints += 1
        g = self.J.T @ (self.w * residual)
        return g[:self.n], g[self.n:]

    def diagonal(self):
        self.diagonals += 1
        d = (self.J * self.J * self.w[:, None]).sum(0)
        return d[:self.n], d[self.n:]

    def product(self, va, vq):
        import torch
        self.products += 1
        v = torch.cat([torch.zeros(self.n, dtype=torch.float64) if t is None else t for t in (va, vq)])
        h = self.J.T @ (self.w * (self.J @ v))
        return h[:self.n], h[self.n:]


@pytest.mark.parametrize("precondition", [True, False])
@pytest.mark.parametrize("fit_fields,damping", [(("alpha", "q"), 0.0), (("q",), 0.0), (("alpha",), 0.3), (("alpha", "q"), 0.05)])
def test_gn_step_solves_the_normal_equations(fit_fields, damping, precondition):
    import torch
    from course5_amd import fit
    rng = np.random.default_rng(34)
    n, m = 15, 80  # 30 unknowns with both fields
    J = rng.normal(size=(m, 2 * n)) * rng.uniform(0.2, 3.0, 2 * n)
    w = rng.uniform(0.1, 2.0, m)
    r = rng.normal(size=m)
    cols = np.r_[np.arange(n) if "alpha" in fit_fields else [], n + np.arange(n) if "q" in fit_fields else []].astype(int)
    Js = J[:, cols]
    H = Js.T @ (w[:, None] * Js)
    g = Js.T @ (w * r)
    want = np.linalg.solve(H + damping * np.diag(np.diag(H)), -g)
    ctx = _DenseContext(J, w)
    iters = len(cols) + 10
    (da, dq), models = fit.gn_step(ctx, torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64), torch.tensor(r),
                                   fit=fit_fields, damping=damping, iters=iters, precondition=precondition)
    assert (da is None) == ("alpha" not in fit_fields) and (dq is None) == ("q" not in fit_fields)
    got = np.concatenate([t.numpy() for t in (da, dq) if t is not None])
    assert np.abs(got - want).max() <= 1e-8 * np.abs(want).max()
    assert ctx.adjoints == 1 and ctx.diagonals == 1 and ctx.products == len(models) <= iters
    # the model values are those of the iterates, and CG does not increase them when it minimises the model itself
    assert models[-1] == pytest.approx(0.5 * got @ H @ got + got @ g, rel=1e-9)
    if damping == 0.0:
        assert all(b <= a + 1e-12 * abs(models[0]) for a, b in zip(models, models[1:]))
        assert models[-1] == pytest.approx(-0.5 * g @ np.linalg.solve(H, g), rel=1e-9)
    # one iteration from zero is a steepest-descent step of the (preconditioned) gradient
    (da1, dq1), m1 = fit.gn_step(ctx, torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64), torch.tensor(r),
                                 fit=fit_fields, damping=damping, iters=1, precondition=precondition)
    x1 = np.concatenate([t.numpy() for t in (da1, dq1) if t is not None])
    z = -g / np.diag(H) if precondition else -g
    A = H + damping * np.diag(np.diag(H))
    assert np.allclose(x1, (-(g @ z) / (z @ A @ z)) * z, rtol=1e-10, atol=0) and len(m1) == 1


def test_gn_step_refuses_bad_arguments():
    import torch
    from course5_amd import fit
    z = torch.zeros(3, dtype=torch.float64)
    for kw in (dict(fit=()), dict(fit=("tau",)), dict(fit=("q", "q")), dict(damping=-1.0), dict(iters=0)):
        with pytest.raises(ValueError):
            fit.gn_step(None, z, z, z, **kw)


# ---- course --sensitivity -------------------------------------------------------------------------------------------

def test_course_help_lists_sensitivity():
    out = subprocess.run([COURSE, "--help"], capture_output=True, text=True).stdout
    assert re.search(r"^  --sensitivity arg\s+after the frame", out, re.M)


@pytest.mark.parametrize("extra,message", [
    (["--frames", "3"], "option '--sensitivity' cannot be used with '--frames' above 1"),
    (["--bench", "5"], "option '--sensitivity' cannot be used with '--bench'"),
    (["--devices", "0,1"], "option '--sensitivity' cannot be used with more than one of '--devices'"),
])
def test_sensitivity_rejects_what_it_cannot_do_at_parse_time(tmp_path, extra, message):
    r = subprocess.run([COURSE, "-f", str(tmp_path / "missing.vtk"), "-d", str(tmp_path / "a.vti"),
                        "--sensitivity", str(tmp_path / "s.vtk")] + extra, capture_output=True, text=True)
    assert r.returncode != 0 and message in (r.stdout + r.stderr)

"""The vertex Gauss-Newton product without a GPU: the C ABI's two declarations, the exports and the bindings' argument
checks, the pins that must not move, and its numpy restatement (tests/vertex_gn_reference.py: tangent restatement, one
float32 rounding, one float32 multiply, adjoint restatement) against the dense J^T W J v on kuhn_box(3).

The dense side takes J column by column from the tangent restatement (unit fields).  Both halves are held at the bar of
the two restatements' duality test (tests/test_vertex_tangent_cpu.py), 1e-12 of the sum of the terms' absolute values:
J v = sum_c J[:, c] v_c per pixel BEFORE the rounding to float32, and H v = sum_p J[p, :] g_p per point coordinate on
the restatement's own g = w * float32(J v), the terms those of both sums (the dense |J|^T |g| and the adjoint
restatement's scale_raw: per view-space face term, then |M|) - the float32 rounding stands between the two halves on both sides (taken
from the dense J v instead, a pixel whose fp64 value differs in the last bits may round to the neighbouring float32, 6e-8
of that pixel: a property of the rounding, not of either restatement)."""
import ctypes
import inspect
import os
import re
import types

import numpy as np
import pytest

from course5_amd import build, capi, meshgen as mg
from tests import adjoint_reference as ar, motion_reference as mr
from tests import vertex_adjoint_reference as vr, vertex_gn_reference as gn, vertex_tangent_reference as vt
from tests.fake_library import RecordingLibrary, bare_context

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS = (1.9, 0.1, 0.9, -0.9)
RX, RY = 48, 36
ROTS = np.array([[0.0, 0.31, 0.0], [1.0, 0.22, 1.0]])

DECLARATIONS = (
    "int c5_render_vertex_gn_product(c5_context* ctx, int n_dirs, const double* d_xyz_host, const float* weight_host, "
    "double* h_xyz_host, float* jv_out_host);",
    "int c5_render_vertex_gn_product_device(c5_context* ctx, int n_dirs, const void* d_xyz_dev, const void* weight_dev, "
    "void* h_xyz_dev, void* jv_out_dev);")
NAMES = ("c5_render_vertex_gn_product", "c5_render_vertex_gn_product_device")


# ---- the C ABI and the bindings ---------------------------------------------------------------------------------------

def test_header_library_and_bindings_have_the_two_calls():
    text = open(os.path.join(ROOT, "include", "course5_hip.h")).read()
    h = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    for decl in DECLARATIONS:
        assert decl in h, decl
    comment = re.sub(r"\s+", " ", text).split("vertex Gauss-Newton product")[1]
    for phrase in ("H v = J^T W J v for n_dirs per-point fields", "c5_render_vertex_adjoint_batch on grad_out = weight *",
                   '"vertex_exact" 1: bit for bit', "never launched"):
        assert phrase in comment, phrase
    lib = ctypes.CDLL(capi.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in capi.EXPORTS, name
    for name in ("render_vertex_gn_product", "render_vertex_gn_product_device"):
        assert callable(getattr(capi.Context, name)), name


def test_pins_still_hold():
    from course5_amd import autograd, fit
    assert build.kernel_source_hash() == "63c90aeb24365e47"  # (re-stamped with next_entry: profiles/component_fuzz.md)
    assert "geometry_derivative_kernels.hip" not in build.DEVICE_SOURCES
    assert ctypes.CDLL(capi.LIB_PATH).c5_abi_version() == 2
    assert "#define C5_ABI_VERSION 2" in open(os.path.join(ROOT, "include", "course5_hip.h")).read()
    p = inspect.signature(fit.shape_step).parameters
    assert list(p) == ["ctx", "alpha", "q", "residual", "weight", "damping", "iters", "free"]
    assert (p["weight"].default, p["damping"].default, p["iters"].default, p["free"].default) == (None, 1e-3, 10, None)
    p = inspect.signature(autograd.render_mesh).parameters
    assert list(p) == ["ctx", "xyz", "alpha", "q", "forward_xyz"] and p["forward_xyz"].default is False
    p = inspect.signature(autograd.vertex_gn_product).parameters
    assert list(p) == ["ctx", "alpha", "q", "v_xyz", "weight"] and p["weight"].default is None
    assert "vertex_gn_product" in autograd.__all__
    assert "vertex_gn_product" in autograd.__doc__ and "vertex_gn_product" in fit.__doc__ and "vertex_gn_product" in fit.shape_step.__doc__


def test_argument_checks_before_the_library():
    import torch
    ctx = bare_context()
    for bad in (np.zeros(27), np.zeros((8, 3)), np.zeros((9, 2)), np.zeros((2, 8, 3)), np.zeros((0, 9, 3)), np.zeros((1, 2, 9, 3))):
        with pytest.raises(ValueError, match=r"d_xyz must be \[9, 3\] or \[K, 9, 3\]"):
            ctx.render_vertex_gn_product(bad)
    for bad in (np.zeros((5, 6)), np.zeros((6, 5, 2)), np.zeros((1, 5, 6, 2))):
        with pytest.raises(ValueError, match=r"weight must be \[5, 6, 2\]"):
            ctx.render_vertex_gn_product(np.zeros((9, 3)), weight=bad)
    d, h = torch.zeros((2, 9, 3), dtype=torch.float64), torch.zeros((2, 9, 3), dtype=torch.float64)
    with pytest.raises(ValueError, match="expected a contiguous"):  # (host tensors are not device arrays)
        ctx.render_vertex_gn_product_device(d, None, h)
    with pytest.raises(ValueError, match="h_xyz must be"):
        ctx.render_vertex_gn_product_device(d[0], None, h[0])
    with pytest.raises(ValueError, match="h_xyz must be"):
        ctx.render_vertex_gn_product_device(1234, None, 5678, n=0)
    with pytest.raises(ValueError, match="give d_xyz and h_xyz"):
        ctx.render_vertex_gn_product_device(None, None, 5678, n=2)
    with pytest.raises(AssertionError, match="the library was entered"):  # (a good call does get there)
        ctx.render_vertex_gn_product(np.zeros((9, 3)))


def test_what_reaches_the_library():
    ctx = bare_context()
    ctx.lib = RecordingLibrary()
    h = ctx.render_vertex_gn_product(np.zeros((9, 3)))
    assert h.shape == (9, 3) and h.dtype == np.float64
    h, jv = ctx.render_vertex_gn_product(np.zeros((3, 9, 3)), weight=np.ones((5, 6, 2)), want_jv=True)
    assert h.shape == (3, 9, 3) and jv.shape == (3, 5, 6, 2) and jv.dtype == np.float32
    h, jv = ctx.render_vertex_gn_product(np.zeros((9, 3)), want_jv=True)
    assert h.shape == (9, 3) and jv.shape == (5, 6, 2)
    ctx.render_vertex_gn_product_device(1234, None, 5678, n=2)
    ctx.render_vertex_gn_product_device(1234, 42, 5678, 99, n=11)
    assert ctx.lib.calls == [
        ("c5_render_vertex_gn_product", (None, 1, "ptr", None, "ptr", None)),
        ("c5_render_vertex_gn_product", (None, 3, "ptr", "ptr", "ptr", "ptr")),
        ("c5_render_vertex_gn_product", (None, 1, "ptr", None, "ptr", "ptr")),
        ("c5_render_vertex_gn_product_device", (None, 2, 1234, None, 5678, None)),
        ("c5_render_vertex_gn_product_device", (None, 11, 1234, 42, 5678, 99))]


# ---- the restatement ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scene():
    xyz, cells = mg.kuhn_box(3, jitter=0.2)
    a, q = mr.scalars(len(cells), 7)
    alpha = 0.6 * a  # below the 2.5 clamp
    m = ar.ray_matrices(xyz, cells, alpha, q, ROTS, RX, RY, BOUNDS)
    geo = vr.segment_faces(xyz, cells, ROTS, RX, RY, BOUNDS)
    rng = np.random.default_rng(61)
    fields = rng.normal(size=(3,) + xyz.shape)
    weight = rng.uniform(0.0, 2.0, size=(RY, RX, 2)).astype(np.float32)
    weight[5:9, 10:30] = 0.0
    J = gn.dense_jacobian(m, geo, cells, len(xyz), ROTS)
    return types.SimpleNamespace(xyz=xyz, cells=cells, m=m, geo=geo, fields=fields, weight=weight, J=J)


@pytest.mark.parametrize("weighted", [False, True])
def test_restatement_against_the_dense_product(scene, weighted):
    s, n_pts = scene, len(scene.xyz)
    w = s.weight if weighted else None
    assert s.m["valid"].any(1).sum() > 500 and np.abs(s.J).max() > 0
    for j, d in enumerate(s.fields):
        got = gn.product_of(s.m, s.geo, s.cells, n_pts, ROTS, d, w)
        # J v, before the rounding: the restatement's fp64 image against the dense sum over the columns
        jv64 = np.stack(vt.tangent_of(s.m, s.geo, s.cells, ROTS, d), axis=-1).reshape(-1)
        dense_jv, size_jv = s.J @ d.reshape(-1), np.abs(s.J) @ np.abs(d.reshape(-1))
        err_jv = float((np.abs(jv64 - dense_jv) / np.where(size_jv > 0, size_jv, 1.0)).max())
        assert (np.abs(jv64 - dense_jv) <= 1e-12 * size_jv).all()
        assert np.array_equal(got["jv"].reshape(-1), jv64.astype(np.float32))
        # g: one float32 multiply per channel
        w32 = np.ones((RY, RX, 2), np.float32) if w is None else w
        assert got["g"].dtype == np.float32 and np.array_equal(got["g"], w32 * got["jv"])
        # H v = J^T g: per point coordinate the dense sum over the pixels
        g64 = got["g"].astype(np.float64).reshape(-1)
        # (the terms: the dense sum's |J| |g| and the restatement's own scale_raw - both sums round, each within its terms;
        # a coordinate the view turns away from has dense columns of rounding noise alone and a sum of terms of its own)
        dense_h, size_h = s.J.T @ g64, np.abs(s.J).T @ np.abs(g64) + got["scale_raw"].reshape(-1)
        h = got["raw"].reshape(-1)
        err_h = float((np.abs(h - dense_h) / np.where(size_h > 0, size_h, 1.0)).max())
        print(f"field {j} weighted {weighted}: J v within {err_jv:.3g}, J^T W J v within {err_h:.3g} of the sums of |terms|")
        assert np.abs(h).max() > 0 and (np.abs(h - dense_h) <= 1e-12 * size_h).all()
        # and as one number: <v, H v> = <J v, g>, both bars above at once (sum_c |v_c| size_h_c = sum_p size_jv_p |g_p|);
        # g has the sign of J v where w >= 0, so that is >= 0
        quad, want, bar = float(d.reshape(-1) @ h), float((g64 * jv64).sum()), 2e-12 * float(np.abs(d.reshape(-1)) @ size_h)
        assert abs(quad - want) <= bar and want >= 0.0 and quad >= -bar


def test_zero_weights_and_skip(scene):
    s, n_pts = scene, len(scene.xyz)
    zero = gn.product_of(s.m, s.geo, s.cells, n_pts, ROTS, s.fields[0], np.zeros((RY, RX, 2), np.float32))
    assert not zero["raw"].any() and zero["jv"].any()
    skip = np.zeros((RY, RX), dtype=bool)
    skip[10:20, 15:30] = True
    w = np.ones((RY, RX, 2), np.float32)
    w[skip] = 0.0
    a = gn.product_of(s.m, s.geo, s.cells, n_pts, ROTS, s.fields[0], None, skip)
    b = gn.product_of(s.m, s.geo, s.cells, n_pts, ROTS, s.fields[0], w)
    assert not a["jv"][skip].any() and np.array_equal(a["raw"], b["raw"])

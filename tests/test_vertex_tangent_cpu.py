"""The vertex tangent's numpy restatement (tests/vertex_tangent_reference.py) against central differences of the restated
fp64 image, its duality with the vertex adjoint's restatement, the motion tangent's restatement for affine fields, and the
calibration of the per-element bar the GPU tests use; the C ABI's declarations and the bindings' argument checks.  No GPU.

Measured: central differences at h = 1e-6 within 8.3e-9 (tau) and 5.4e-9 (I) of the maximum; duality to 6e-16 of the sum
of the terms' absolute values."""
import ctypes
import inspect
import os
import re
import types

import numpy as np
import pytest

from course5_amd import build, capi, meshgen as mg
from tests import adjoint_reference as ar, derivative_fuzz as fz, motion_reference as mr
from tests import vertex_adjoint_reference as vr, vertex_tangent_reference as vt
from tests.fake_library import bare_context

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS = (1.9, 0.1, 0.9, -0.9)
RX, RY = 48, 36
ROTS = np.array([[0.0, 0.31, 0.0], [1.0, 0.22, 1.0]])


@pytest.fixture(scope="module")
def scene():
    xyz, cells = mg.kuhn_box(3, jitter=0.2)
    a, q = mr.scalars(len(cells), 7)
    alpha = 0.6 * a  # below the 2.5 clamp
    m = ar.ray_matrices(xyz, cells, alpha, q, ROTS, RX, RY, BOUNDS)
    geo = vr.segment_faces(xyz, cells, ROTS, RX, RY, BOUNDS)
    fields = np.random.default_rng(51).normal(size=(3,) + xyz.shape)
    return types.SimpleNamespace(xyz=xyz, cells=cells, alpha=alpha, q=q, m=m, geo=geo, rots=ROTS, fields=fields)


@pytest.mark.parametrize("j", [0, 1, 2])
def test_restatement_against_central_differences(scene, j):
    s, h = scene, 1e-6
    d = s.fields[j]
    tau_dot, I_dot = vt.tangent_of(s.m, s.geo, s.cells, ROTS, d)
    hi, lo = (ar.ray_matrices(s.xyz + sign * h * d, s.cells, s.alpha, s.q, ROTS, RX, RY, BOUNDS) for sign in (1, -1))
    assert s.m["valid"].any(1).sum() > 500
    for name, got in (("tau", tau_dot), ("I", I_dot)):
        fd = (hi[name] - lo[name]) / (2 * h)
        err, top = np.abs(fd - got.reshape(-1)).max(), np.abs(got).max()  # (no pixel excluded)
        print(f"field {j} {name}_dot: max error {err:.3g} of max {top:.3g} ({err / top:.3g})")
        assert top > 0 and err <= 1e-6 * top


def test_duality_with_the_vertex_adjoint_restatement(scene):
    s = scene
    rng = np.random.default_rng(52)
    for j, d in enumerate(s.fields):
        g = rng.normal(size=(RY, RX, 2)).astype(np.float32)
        ref = vr.gradients_of(s.m, s.geo, s.cells, len(s.xyz), ROTS, g)
        tau_dot, I_dot = vt.tangent_of(s.m, s.geo, s.cells, ROTS, d)
        g64 = g.astype(np.float64)
        lhs = float((ref["raw"] * d).sum())
        terms = np.concatenate([(g64[..., 0] * tau_dot).ravel(), (g64[..., 1] * I_dot).ravel()])
        rhs, size = float(terms.sum()), float(np.abs(terms).sum())
        print(f"field {j}: <J^T g, d> = {lhs:.15g}, <g, J d> = {rhs:.15g}, difference / sum |terms| = {abs(lhs - rhs) / size:.3g}")
        assert abs(rhs) > 0 and abs(lhs - rhs) <= 1e-12 * size


def test_affine_fields_give_the_motion_tangent_restatement(scene):
    s = scene
    geo_m = mr.face_matrices(s.xyz, s.cells, ROTS, RX, RY, BOUNDS)
    M = vr.view_matrix(ROTS)
    p = ar.rotate(s.xyz, ROTS)
    for j, f in enumerate(np.random.default_rng(53).normal(size=(4, 12))):
        u = p @ f[:9].reshape(3, 3).T + f[9:]
        d = u @ M  # d_xyz[v] = M^T (A p_v + b)
        got = vt.tangent_of(s.m, s.geo, s.cells, ROTS, d)
        want = mr.motion_of(s.m, geo_m, f, with_scale=True)
        for name, g, w in (("tau", got[0], want[0]), ("I", got[1], want[1])):
            err, scale = np.abs(g - w), want[2]["scale_" + name]
            print(f"affine field {j} {name}_dot: worst error / scale {(err / np.where(scale > 0, scale, 1.0)).max():.3g}")
            assert np.abs(w).max() > 0 and (err <= 1e-12 * scale).all()


@pytest.mark.parametrize("which", ["box", 3001, 3006])
def test_chord_sensitivity_covers_moved_chords(scene, which):
    """1e-9 scale + dz_err sens covers the restatement re-evaluated with every chord moved by +-F dz_err: the per-element
    bar of tests/test_gpu_vertex_tangent.py and of the geometry sweep, calibrated without the code under test (tests/
    test_motion_cpu.py's way) - on the fixed box and on a "threshold" (3001) and an "underflow" (3006, a soup) scene of the
    sweep with the fields the sweep compares.  The scale bounds the result term by term."""
    if which == "box":
        s, m, geo, rots, fields = scene, scene.m, scene.geo, ROTS, scene.fields
    else:
        s = fz.geometry_scene(which)
        assert s.mode == {3001: "threshold", 3006: "underflow"}[which]
        rots, fields = s.rots, s.v_fields[s.v_compare]
        m = ar.ray_matrices(s.xyz, s.cells, s.alpha, s.q, rots, s.res[0], s.res[1], fz.B, s.limit)
        geo = vr.segment_faces(s.xyz, s.cells, rots, s.res[0], s.res[1], fz.B)
    shape = m["shape"]
    dz_err = fz.dz_err(s)
    rng = np.random.default_rng(3)
    M = vr.view_matrix(rots)
    moves = [np.ones_like(m["D"]), -np.ones_like(m["D"]), rng.choice([-1.0, 1.0], m["D"].shape)]
    worst = 0.0
    for d in fields:
        tau_dot, I_dot, extra = vt.tangent_of(m, geo, s.cells, rots, d, with_scale=True)
        assert (np.abs(tau_dot) <= extra["scale_tau"] * (1 + 1e-12)).all() and (np.abs(I_dot) <= extra["scale_I"] * (1 + 1e-12)).all()
        assert not extra["sens_tau"].any()  # (tau_dot does not hold the chords, and a per-vertex dw not the depth)
        ddz = vt.chord_rates(geo, s.cells, d @ M.T)[0]
        tol = 1e-9 * extra["scale_I"] + dz_err * extra["sens_I"]
        if which == "box":
            assert (extra["sens_I"][m["active"].any(1).reshape(shape)] > 0).all()
        for sign in moves:
            D = np.where(m["valid"], m["D"] + sign * m["F"] * dz_err, 0.0)
            moved_tau, moved_I = mr.recurrence(m, D, ddz)[:2]
            assert np.array_equal(moved_tau.reshape(shape), tau_dot)
            diff = np.abs(moved_I.reshape(shape) - I_dot)
            assert (diff <= tol).all(), (which, float((diff / np.where(tol > 0, tol, 1.0)).max()))
            worst = max(worst, float((diff / np.where(tol > 0, tol, 1.0)).max()))
    print(f"{which}: moved chords, worst change / bar {worst:.3g}")


def test_skip_and_rows(scene):
    s = scene
    skip = np.zeros((RY, RX), dtype=bool)
    skip[10:20, 15:30] = True
    full = vt.tangent_of(s.m, s.geo, s.cells, ROTS, s.fields[0])
    got = vt.image_tangent(s.xyz, s.cells, s.alpha, s.q, ROTS, RX, RY, BOUNDS, s.fields[:1], skip=skip)[0]
    assert not got[0][skip].any() and not got[1][skip].any()
    assert np.array_equal(got[0][~skip], full[0][~skip]) and np.array_equal(got[1][~skip], full[1][~skip])
    rows = np.arange(5, 17)
    part = vt.image_tangent(s.xyz, s.cells, s.alpha, s.q, ROTS, RX, RY, BOUNDS, s.fields[:1], rows=rows)[0]
    assert np.array_equal(part[0], full[0][rows]) and np.array_equal(part[1], full[1][rows])


# ---- the C ABI and the bindings ---------------------------------------------------------------------------------------

def test_header_declares_the_two_calls():
    text = open(os.path.join(ROOT, "include", "course5_hip.h")).read()
    h = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    for decl in ("int c5_render_vertex_tangent(c5_context* ctx, int n_dirs, const double* d_xyz_host, float* out_host);",
                 "int c5_render_vertex_tangent_device(c5_context* ctx, int n_dirs, const void* d_xyz_dev, void* out_dev);"):
        assert decl in h, decl
    comment = re.sub(r"\s+", " ", text)
    assert "WELDED POINTS" in comment.split("vertex tangent render")[1] and "DUALITY" in comment.split("vertex tangent render")[1]


def test_library_and_bindings_have_them():
    lib = ctypes.CDLL(capi.LIB_PATH)
    for name in ("c5_render_vertex_tangent", "c5_render_vertex_tangent_device"):
        assert hasattr(lib, name), name
        assert name in capi.EXPORTS
    for name in ("render_vertex_tangent", "render_vertex_tangent_device"):
        assert callable(getattr(capi.Context, name)), name


def test_pins_still_hold():
    assert build.kernel_source_hash() == "63c90aeb24365e47"  # (re-stamped with next_entry: profiles/component_fuzz.md)
    for name in ("scalar_derivative_kernels.hip", "geometry_derivative_kernels.hip", "ray_matrix_kernels.hip", "deriv_ray.hpp", "deriv_lists.hpp", "deriv_faces.hpp"):
        assert name not in build.DEVICE_SOURCES, name
    assert ctypes.CDLL(capi.LIB_PATH).c5_abi_version() == 2
    assert "#define C5_ABI_VERSION 2" in open(os.path.join(ROOT, "include", "course5_hip.h")).read()


def test_argument_checks_before_the_library():
    import torch
    ctx = bare_context()
    for bad in (np.zeros(27), np.zeros((8, 3)), np.zeros((9, 2)), np.zeros((2, 8, 3)), np.zeros((0, 9, 3)), np.zeros((1, 2, 9, 3))):
        with pytest.raises(ValueError, match=r"d_xyz must be \[9, 3\] or \[K, 9, 3\]"):
            ctx.render_vertex_tangent(bad)
    with pytest.raises(ValueError, match="expected a contiguous"):  # (host tensors are not device arrays)
        ctx.render_vertex_tangent_device(torch.zeros((2, 9, 3), dtype=torch.float64), torch.zeros((2, 5, 6, 2)))
    with pytest.raises(ValueError, match="out must be"):
        ctx.render_vertex_tangent_device(torch.zeros((9, 3), dtype=torch.float64), torch.zeros((5, 6, 2)))
    with pytest.raises(AssertionError, match="the library was entered"):  # (a good call does get there)
        ctx.render_vertex_tangent(np.zeros((9, 3)))


def test_render_mesh_and_shape_step_signatures():
    from course5_amd import autograd, fit
    p = inspect.signature(autograd.render_mesh).parameters
    assert list(p) == ["ctx", "xyz", "alpha", "q", "forward_xyz"] and p["forward_xyz"].default is False
    assert "forward_xyz" in autograd.__doc__ and "forward_xyz" in autograd.render_mesh.__doc__
    p = inspect.signature(fit.shape_step).parameters
    assert list(p) == ["ctx", "alpha", "q", "residual", "weight", "damping", "iters", "free"]
    assert (p["weight"].default, p["damping"].default, p["iters"].default, p["free"].default) == (None, 1e-3, 10, None)
    assert "shape_step" in fit.__doc__

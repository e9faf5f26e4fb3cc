"""The vertex adjoint's numpy restatement (tests/vertex_adjoint_reference.py) against central differences of the restated
fp64 image, against the motion tangent's restatement (the two are transposes of each other) and exact identities.  No GPU.

Bars.  Central differences at h = 1e-6: 1e-6 x max |grad| per component, the project's adjoint bar (the truncation error
h^2 f''' / 6 and the rounding eps |loss| / h are both far below it).  Identities between two fp64 evaluations of the same
sum in another order: 1e-12 x the sum of the terms' absolute values - a few thousand terms at 2^-53 each."""
import types

import numpy as np
import pytest

from course5_amd import meshgen as mg
from tests import adjoint_reference as ar, derivative_fuzz as fz, motion_reference as mr, tangent_reference as tr
from tests import vertex_adjoint_reference as vr

BOUNDS = (1.9, 0.1, 0.9, -0.9)  # tests/test_gpu_motion.py: SMALL_BOUNDS, SMALL_ROTS
RX, RY = 48, 36
ROTS = np.array([[0.0, 0.31, 0.0], [1.0, 0.22, 1.0]])
NO_ROTS = np.zeros((0, 3))


@pytest.fixture(scope="module")
def scene():
    xyz, cells = mg.kuhn_box(3, jitter=0.2)
    alpha, q = mr.scalars(len(cells), 7)
    g = np.random.default_rng(11).normal(size=(RY, RX, 2)).astype(np.float32)
    ref = vr.vertex_gradients(xyz, cells, alpha, q, ROTS, RX, RY, BOUNDS, g)
    return types.SimpleNamespace(xyz=xyz, cells=cells, alpha=alpha, q=q, g=g, ref=ref, view=ar.rotate(xyz, ROTS))


def _central(points, rots, s, v, k, h=1e-6):
    out = []
    for sign in (1, -1):
        p = points.copy()
        p[v, k] += sign * h
        out.append(vr.loss(p, s.cells, s.alpha, s.q, rots, RX, RY, BOUNDS, s.g))
    return (out[0] - out[1]) / (2 * h)


def test_the_faces_are_motion_reference_s(scene):
    s = scene
    geo = vr.segment_faces(s.xyz, s.cells, ROTS, RX, RY, BOUNDS)
    want = mr.face_matrices(s.xyz, s.cells, ROTS, RX, RY, BOUNDS)
    for name in ("C", "Z_out", "GX_out", "GY_out", "Z_in", "GX_in", "GY_in"):
        assert np.array_equal(geo[name], want[name]), name
    valid = geo["C"] >= 0
    for side in ("out", "in"):
        lam = geo["L_" + side][valid]
        assert np.abs(lam.sum(1) - 1.0).max() <= 1e-12
        assert lam.min() >= -1e-12  # (the pixel lies in the face)
        # the barycentric combination of the face's depths is the face's depth at the pixel
        z = s.view[s.cells[geo["C"][valid]][np.arange(len(lam))[:, None], vr.FACES[geo["F_" + side][valid]]], 2]
        assert np.abs((lam * z).sum(1) - geo["Z_" + side][valid]).max() <= 1e-12


def test_view_space_against_central_differences_of_every_component(scene):
    s = scene
    got = s.ref["view"]
    assert got.shape == (64, 3)
    fd = np.array([[_central(s.view, NO_ROTS, s, v, k) for k in range(3)] for v in range(len(s.view))])
    top = np.abs(got).max()
    err = np.abs(fd - got)
    print(f"view space: worst error {err.max():.3g} of max {top:.3g} ({err.max() / top:.3g}), {int((err > 1e-6 * top).sum())} of {err.size} over")
    assert top > 0 and (err <= 1e-6 * top).all()


def test_raw_space_against_central_differences_of_one_point(scene):
    s = scene
    got = s.ref["raw"]
    v = int(np.abs(got).sum(1).argmax())
    fd = np.array([_central(s.xyz, ROTS, s, v, k) for k in range(3)])
    top = np.abs(got).max()
    print(f"raw space, point {v}: error {np.abs(fd - got[v]).max():.3g} of max {top:.3g}")
    assert (np.abs(fd - got[v]) <= 1e-6 * top).all()
    # M^T maps the view-space gradient to the raw-space one: M from the view transform's own differences
    M = vr.view_matrix(ROTS)
    assert np.abs(M @ M.T - np.eye(3)).max() <= 1e-15
    assert np.array_equal(got, s.ref["view"] @ M)


def test_transpose_of_the_motion_tangent(scene):
    s = scene
    fields = np.random.default_rng(12).normal(size=(4, 12))
    images = mr.image_motion(s.xyz, s.cells, s.alpha, s.q, ROTS, RX, RY, BOUNDS, fields)
    g = s.g.astype(np.float64)
    for f, (tau_dot, I_dot) in zip(fields, images):
        u = s.view @ f[:9].reshape(3, 3).T + f[9:]
        lhs = float((s.ref["view"] * u).sum())
        rhs = float((g[..., 0] * tau_dot).sum() + (g[..., 1] * I_dot).sum())
        terms = float((s.ref["scale_view"] * np.abs(u)).sum())
        print(f"<grad, u> = {lhs:.6g}, <g, motion tangent> = {rhs:.6g}, difference / sum |terms| = {abs(lhs - rhs) / terms:.3g}")
        assert abs(lhs) > 0 and abs(lhs - rhs) <= 1e-12 * terms


def test_a_translation_along_the_rays_changes_nothing(scene):
    gz, scale = scene.ref["view"][:, 2], scene.ref["scale_view"][:, 2]
    print(f"sum of grad_z = {gz.sum():.3g}, sum of |terms| = {scale.sum():.3g}")
    assert abs(gz.sum()) <= 1e-12 * scale.sum()
    assert (np.abs(scene.ref["view"]) <= scene.ref["scale_view"] * (1 + 1e-12)).all()


def test_z_scale_is_the_tangent_along_the_scalars_themselves():
    """u = (0, 0, z) stretches every chord at its own rate, which is alpha -> (1 + t) alpha, Q -> (1 + t) Q where no alpha
    is clamped: sum_v z_v grad_z[v] = <g_tau, tau> + <g_I, J (alpha, q)>."""
    xyz, cells = mg.kuhn_box(3, jitter=0.2)
    a, q = mr.scalars(len(cells), 7)
    alpha = 0.6 * a  # below the 2.5 clamp
    g = np.random.default_rng(13).normal(size=(RY, RX, 2)).astype(np.float32).astype(np.float64)
    ref = vr.vertex_gradients(xyz, cells, alpha, q, ROTS, RX, RY, BOUNDS, g)
    z = ar.rotate(xyz, ROTS)[:, 2]
    m = ar.ray_matrices(xyz, cells, alpha, q, ROTS, RX, RY, BOUNDS)
    I_dot = tr.tangent_of(m, len(cells), alpha, q)[1]
    lhs = float(z @ ref["view"][:, 2])
    rhs = float((g[..., 0] * m["tau"].reshape(RY, RX)).sum() + (g[..., 1] * I_dot).sum())
    terms = float(np.abs(z) @ ref["scale_view"][:, 2])
    print(f"z-scale: {lhs:.6g} against {rhs:.6g}, difference / sum |terms| = {abs(lhs - rhs) / terms:.3g}")
    assert abs(lhs) > 0 and abs(lhs - rhs) <= 1e-12 * terms


@pytest.mark.parametrize("which", ["box", 3001, 3006])
def test_chord_sensitivity_covers_moved_chords(scene, which):
    """1e-9 scale_raw + dz_err sens_raw covers the restatement re-evaluated with every chord moved by +-F dz_err: the
    per-element bar of the geometry sweep (tests/derivative_fuzz.py) and of tests/test_gpu_vertex_adjoint.py, calibrated
    without the code under test (tests/test_motion_cpu.py's way) - on the fixed box and on a "threshold" (3001) and an
    "underflow" (3006, a soup) scene of the sweep with their own upstream images."""
    if which == "box":
        s = scene
        rots, images = ROTS, [s.g]
        m = ar.ray_matrices(s.xyz, s.cells, s.alpha, s.q, ROTS, RX, RY, BOUNDS)
        geo = vr.segment_faces(s.xyz, s.cells, ROTS, RX, RY, BOUNDS)
    else:
        s = fz.geometry_scene(which)
        assert s.mode == {3001: "threshold", 3006: "underflow"}[which]
        rots, images = s.rots, s.vg
        m = ar.ray_matrices(s.xyz, s.cells, s.alpha, s.q, rots, s.res[0], s.res[1], fz.B, s.limit)
        geo = vr.segment_faces(s.xyz, s.cells, rots, s.res[0], s.res[1], fz.B)
    dz_err = fz.dz_err(types.SimpleNamespace(xyz=s.xyz, rots=rots))
    rng = np.random.default_rng(3)
    moves = [np.ones_like(m["D"]), -np.ones_like(m["D"]), rng.choice([-1.0, 1.0], m["D"].shape)]
    worst = 0.0
    for g in images:
        ref = vr.gradients_of(m, geo, s.cells, len(s.xyz), rots, g)
        same = vr.gradients_of(vr.with_chords(m, m["D"]), geo, s.cells, len(s.xyz), rots, g)
        assert np.array_equal(same["raw"], ref["raw"])  # (with_chords evaluates what ray_matrices does)
        assert (np.abs(ref["raw"]) <= ref["scale_raw"] * (1 + 1e-12)).all()
        tol = 1e-9 * ref["scale_raw"] + dz_err * ref["sens_raw"]
        if np.abs(np.asarray(g)[..., 1]).max() > 0:
            assert ref["sens_raw"].max() > 0
        else:
            assert not ref["sens_raw"].any()  # (g_tau alpha_k holds no chord)
        for sign in moves:
            D = np.where(m["valid"], m["D"] + sign * m["F"] * dz_err, 0.0)
            diff = np.abs(vr.gradients_of(vr.with_chords(m, D), geo, s.cells, len(s.xyz), rots, g)["raw"] - ref["raw"])
            worst = max(worst, float((diff / np.where(tol > 0, tol, 1.0)).max()))
            assert (diff <= tol).all(), (which, float((diff / np.where(tol > 0, tol, 1.0)).max()))
    print(f"{which}: moved chords, worst change / bar {worst:.3g}")

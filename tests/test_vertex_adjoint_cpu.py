"""The vertex adjoint's numpy restatement (tests/vertex_adjoint_reference.py) against central differences of the restated
fp64 image, against the motion tangent's restatement (the two are transposes of each other) and exact identities.  No GPU.

Bars.  Central differences at h = 1e-6: 1e-6 x max |grad| per component, the project's adjoint bar (the truncation error
h^2 f''' / 6 and the rounding eps |loss| / h are both far below it).  Identities between two fp64 evaluations of the same
sum in another order: 1e-12 x the sum of the terms' absolute values - a few thousand terms at 2^-53 each."""
import types

import numpy as np
import pytest

from course5_amd import meshgen as mg
from tests import adjoint_reference as ar, motion_reference as mr, tangent_reference as tr, vertex_adjoint_reference as vr

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

"""The motion tangent's numpy restatement (tests/motion_reference.py) against central differences of the restated fp64
image, exact identities, c5_rotation_motion against central differences of the view transform, and the calibration of
the per-element bar the GPU tests use.  No GPU."""
import types

import numpy as np
import pytest

from course5_amd import capi, meshgen as mg
from tests import adjoint_reference as ar, derivative_fuzz as fz, motion_reference as mr, tangent_reference as tr

BOUNDS = (1.9, 0.1, 0.9, -0.9)
RX, RY = 48, 36
ROTS = np.array([[0.0, 0.31, 0.0], [1.0, 0.22, 1.0]])


@pytest.fixture(scope="module")
def scene():
    xyz, cells = mg.kuhn_box(3, jitter=0.2)
    a, q = mr.scalars(len(cells), 7)
    alpha = 0.6 * a  # below the 2.5 clamp
    m = ar.ray_matrices(xyz, cells, alpha, q, ROTS, RX, RY, BOUNDS)
    geo = mr.face_matrices(xyz, cells, ROTS, RX, RY, BOUNDS)
    return types.SimpleNamespace(xyz=xyz, cells=cells, alpha=alpha, q=q, m=m, geo=geo, rots=ROTS)


def _lists(m, width):
    c = np.full((m["n_px"], width), -1)
    c[:, :m["C"].shape[1]] = m["C"]
    return c


@pytest.mark.parametrize("index", [0, 1])
def test_restatement_against_central_differences(scene, index):
    s, h = scene, 1e-5
    got = mr.motion_of(s.m, s.geo, capi.rotation_motion(ROTS, index))
    ms = []
    for sign in (-1, 1):
        rots = ROTS.copy()
        rots[index, 1] += sign * h
        ms.append(ar.ray_matrices(s.xyz, s.cells, s.alpha, s.q, rots, RX, RY, BOUNDS))
    width = max(m["C"].shape[1] for m in ms + [s.m])
    same = (_lists(ms[0], width) == _lists(s.m, width)).all(1) & (_lists(ms[1], width) == _lists(s.m, width)).all(1)
    covered = s.m["valid"].any(1)
    assert covered.sum() > 500
    excluded = 1.0 - same[covered].mean()
    print(f"rotation {index}: {int(covered.sum())} covered pixels, {excluded:.2%} changed their cell list")
    assert excluded <= 0.01
    for name, g, key in (("tau", got[0], "tau"), ("I", got[1], "I")):
        fd = (ms[1][key] - ms[0][key]) / (2 * h)
        use = same & covered
        err = np.abs(fd - g.reshape(-1))[use].max()
        print(f"rotation {index} {name}_dot: max error {err:.3g}, max {np.abs(g).max():.3g}")
        assert np.abs(g).max() > 0
        assert err <= 5e-6 * np.abs(g).max()


def test_identities(scene):
    s = scene
    for field in (mr.Z_TRANSLATION, 0.0 * np.array([0, 0, 0, 0, 0, 0, 0, 0, 0, 1.0, 0, 0]), np.zeros(12)):
        tau_dot, I_dot = mr.motion_of(s.m, s.geo, field)
        assert not tau_dot.any() and not I_dot.any()
    tau_dot, I_dot = mr.motion_of(s.m, s.geo, mr.Z_SCALE)
    tau, I = s.m["tau"].reshape(RY, RX), s.m["I"].reshape(RY, RX)
    assert np.abs(tau_dot - tau).max() <= 1e-12 * np.abs(tau).max()
    # dz -> (1 + t) dz is alpha -> (1 + t) alpha, Q -> (1 + t) Q: the tangent along (alpha, q) itself (no alpha is clamped)
    assert not s.m["clamped"].any()
    want = tr.tangent_of(s.m, len(s.alpha), s.alpha, s.q)[1]
    assert np.abs(I_dot - want).max() <= 1e-12 * np.abs(want).max()


def test_rotation_motion_against_central_differences_of_the_view_transform():
    rng = np.random.default_rng(11)
    rots = np.array([[0.0, 0.7, 0.0], [1.0, -0.4, 1.0], [0.0, 1.3, 0.0]])
    pts = rng.uniform(-1.0, 2.0, (50, 3))
    pv = ar.rotate(pts, rots)
    h = 1e-6
    for index in range(3):
        for what in (0, 1):
            f = capi.rotation_motion(rots, index, what)
            lo, hi = rots.copy(), rots.copy()
            lo[index, 1 + what] -= h
            hi[index, 1 + what] += h
            fd = (ar.rotate(pts, hi) - ar.rotate(pts, lo)) / (2 * h)
            u = pv @ f[:9].reshape(3, 3).T + f[9:]
            assert np.abs(u - fd).max() <= 1e-8, (index, what, np.abs(u - fd).max())
            if what == 1 and rots[index, 0] == 0:
                assert not f.any()  # a rotation about the x axis has no x0
            else:
                assert np.abs(f).max() > 0.1
    with pytest.raises(capi.C5Error):
        capi.rotation_motion(rots, 3)


def test_the_convexity_rule_finds_the_paired_faces(scene):
    """What the kernels do at boundary entries and on "algorithm" 1 - the entry face is the deepest of the faces the cell
    lies above, the exit face the shallowest of those it lies below - picks the faces the reference pairs."""
    s = scene
    grids = [(s.xyz, s.cells, ROTS, RX, RY, BOUNDS)]
    xyz, cells = mg.ball(8)
    grids.append((xyz, cells, mg.view_rotations(0.13, 0.21), 60, 45, mg.REFERENCE_BOUNDS))
    for xyz, cells, rots, rx, ry, bounds in grids:
        geo = mr.face_matrices(xyz, cells, rots, rx, ry, bounds)
        valid = geo["C"] >= 0
        assert valid.sum() > 1000
        got = mr.hull_faces(xyz, cells, rots, geo["C"][valid], geo["X"][valid], geo["Y"][valid])
        for g, name in zip(got, ("GX_in", "GY_in", "GX_out", "GY_out")):
            assert np.array_equal(g, geo[name][valid]), name


def _calibration_scene(scene, which):
    """The fixed box, or a scene of the geometry sweep (tests/derivative_fuzz.py) with its own fields: (s, m, geo, fields)."""
    if which == "box":
        rng = np.random.default_rng(3)
        return scene, scene.m, scene.geo, [capi.rotation_motion(ROTS, 0), capi.rotation_motion(ROTS, 1), mr.Z_SCALE, rng.normal(size=12)]
    s = fz.geometry_scene(which)
    assert s.mode == {3001: "threshold", 3006: "underflow"}[which]
    m = ar.ray_matrices(s.xyz, s.cells, s.alpha, s.q, s.rots, s.res[0], s.res[1], fz.B, s.limit)
    return s, m, mr.face_matrices(s.xyz, s.cells, s.rots, s.res[0], s.res[1], fz.B), list(s.motion)


@pytest.mark.parametrize("which", ["box", 3001, 3006])
def test_chord_sensitivity_covers_moved_chords(scene, which):
    """1e-9 scale + dz_err sens covers the restatement re-evaluated with every chord moved by +-F dz_err, and with the two
    depths a field reads (the kappa terms) moved by as much: the per-element bar of tests/test_gpu_motion.py and of the
    geometry sweep, calibrated without the code under test - on the fixed box and on a "threshold" (3001) and an
    "underflow" (3006) scene of the sweep with their own fields (every rotation, the 2^+-20 multiples, the shifts)."""
    s, m, geo, fields = _calibration_scene(scene, which)
    shape = m["shape"]
    dz_err = fz.dz_err(s)
    rng = np.random.default_rng(3)
    moves = [np.ones_like(m["D"]), -np.ones_like(m["D"]), rng.choice([-1.0, 1.0], m["D"].shape)]
    worst = 0.0
    for f in fields:
        tau_dot, I_dot, extra = mr.motion_of(m, geo, f, with_scale=True)
        ddz = mr.chord_rates(geo, f)[0]
        tol_I = 1e-9 * extra["scale_I"] + dz_err * extra["sens_I"]
        tol_tau = 1e-9 * extra["scale_tau"] + dz_err * extra["sens_tau"]
        if np.any(f) and which == "box":
            assert (extra["sens_I"][m["active"].any(1).reshape(shape)] > 0).all()
        for sign in moves:
            D = np.where(m["valid"], m["D"] + sign * m["F"] * dz_err, 0.0)
            moved = mr.recurrence(m, D, ddz)[1].reshape(shape)
            diff = np.abs(moved - I_dot)
            assert (diff <= tol_I).all()
            worst = max(worst, float((diff / np.where(tol_I > 0, tol_I, 1.0)).max()))
            # ... and the depths the field is evaluated at, the far end one way and the near end the other
            there = dict(geo, Z_out=geo["Z_out"] + sign * m["F"] * dz_err, Z_in=geo["Z_in"] - sign * m["F"] * dz_err)
            tau2, I2 = mr.recurrence(m, D, mr.chord_rates(there, f)[0])[:2]
            for got, ref, tol in ((tau2.reshape(shape), tau_dot, tol_tau), (I2.reshape(shape), I_dot, tol_I)):
                diff = np.abs(got - ref)
                worst = max(worst, float((diff / np.where(tol > 0, tol, 1.0)).max()))
                assert (diff <= tol).all(), (which, float((diff / np.where(tol > 0, tol, 1.0)).max()))
    print(f"{which}: moved chords and depths, worst change / bar {worst:.3g}")


def test_course_refuses_view_tangent_for_sweeps_at_parse_time(tmp_path):
    import os
    import subprocess
    course = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "course5_amd", "course")
    out = subprocess.run([course, "--help"], capture_output=True, text=True).stdout
    assert "--view_tangent arg" in out
    r = subprocess.run([course, "-f", "x.vtk", "-d", str(tmp_path / "a.vti"), "--frames", "3", "--view_tangent", str(tmp_path / "t")],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "option '--view_tangent' cannot be used with '--frames' above 1" in r.stdout + r.stderr

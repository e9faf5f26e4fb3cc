"""Adjoint render, no GPU: the numpy helper (tests/adjoint_reference.py) against finite differences and the port oracle,
the C ABI declarations and bindings, and the `course --contribution` option's parse-time checks."""
import os
import re
import subprocess

import numpy as np
import pytest

from course5_amd import capi
from course5_amd import meshgen as mg
from tests import adjoint_reference as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COURSE = os.path.join(ROOT, "course5_amd", "course")
EPS = np.finfo(np.float64).eps


def _random_lists(rng, n_px=40, n_cells=12):
    """Pixels of random segment lists over a few cells with the special values: clamped alpha, alpha = 0, alpha just
    above epsilon, a dz of 1e-6 and a dz of 20 (in units of 1 / alpha)."""
    alpha = rng.uniform(0.2, 2.0, n_cells)
    q = rng.uniform(0.1, 1.0, n_cells)
    alpha[0] = 3.7          # clamped at 2.5
    alpha[1] = 0.0          # inactive
    alpha[2] = 1.5 * EPS    # just above epsilon
    alpha[3] = 2.0          # meets dz = 10: a dz = 20
    alpha[4] = 1.0          # meets dz = 1e-6
    lists = []
    for _ in range(n_px):
        n = int(rng.integers(1, 9))
        cells = rng.integers(0, n_cells, n)
        dz = rng.uniform(0.01, 0.5, n)
        dz[cells == 3] = 10.0
        dz[cells == 4] = 1e-6
        z_hi = np.sort(rng.uniform(-1, 1, n))[::-1]  # the reference's order: descending z_hi
        lists.append(np.column_stack([cells, z_hi, dz]))
    weights = rng.normal(size=(n_px, 2))
    return lists, weights, alpha, q


def _loss(lists, weights, alpha, q):
    return sum(w[0] * t + w[1] * i for w, (t, i) in zip(weights, (ar.forward(s, alpha, q) for s in lists)))


def test_helper_matches_central_differences_of_its_forward():
    rng = np.random.default_rng(7)
    lists, weights, alpha, q = _random_lists(rng)
    ga, gq = ar.gradients(lists, weights, alpha, q, len(alpha))
    for c in range(len(alpha)):
        # Q: the loss is linear in Q - any step is exact up to rounding
        h = 1e-3
        qp, qm = q.copy(), q.copy()
        qp[c] += h
        qm[c] -= h
        fd_q = (_loss(lists, weights, alpha, qp) - _loss(lists, weights, alpha, qm)) / (2 * h)
        assert fd_q == pytest.approx(gq[c], rel=1e-7, abs=1e-9), c
        if c == 1:
            continue  # alpha = 0: inactive, I does not depend on it (a step of any size would switch it on)
        # alpha just above epsilon: one-sided (it must stay active); elsewhere central, relative step
        h = 1e-7 if c == 2 else (1e-3 if c == 4 else 1e-6) * alpha[c]  # (cell 4: dz = 1e-6, a tiny derivative)
        ap = alpha.copy()
        ap[c] += h
        if c == 2:
            fd_a = (_loss(lists, weights, ap, q) - _loss(lists, weights, alpha, q)) / h
            assert fd_a == pytest.approx(ga[c], rel=1e-5, abs=1e-6), c
        else:
            am = alpha.copy()
            am[c] -= h
            fd_a = (_loss(lists, weights, ap, q) - _loss(lists, weights, am, q)) / (2 * h)
            assert fd_a == pytest.approx(ga[c], rel=1e-6, abs=1e-9), c


def test_helper_special_cases():
    """alpha = 0 adds only its tau term; a clamped alpha adds only its tau term (dI/dalpha = 0) but its Q counts; the
    small-argument series agrees with the closed form where both are accurate."""
    seg = np.array([[0, 0.5, 0.3], [1, 0.1, 0.2]])
    alpha, q = np.array([0.0, 3.0]), np.array([0.7, 0.4])
    (c0, dt0, da0, dq0), (c1, dt1, da1, dq1) = ar.pixel_terms(seg, alpha, q)
    assert (c0, dt0, da0, dq0) == (0, 0.3, 0.0, 0.0)
    assert c1 == 1 and dt1 == 0.2 and da1 == 0.0 and dq1 == pytest.approx(-np.expm1(-2.5 * 0.2) / 2.5)
    for x in (0.01, 0.1, 0.124):
        closed = (x * np.exp(-x) + np.expm1(-x)) / x**2
        assert ar._bracket_over_q_dz2(x) == pytest.approx(closed, rel=1e-9)
    assert ar._bracket_over_q_dz2(1e-6) == pytest.approx(-0.5 + 1e-6 / 3, rel=1e-12)


def test_helper_segment_lists_match_the_port_oracle(oracle_port):
    """The helper's own binning (segment_lists) against the oracle: its tau / I images, and the probed lists of a few
    pixels segment for segment."""
    xyz, cells = mg.kuhn_box(4, jitter=0.1)
    alpha, q = mg.scalars(len(cells), seed=3)
    rots = mg.view_rotations(0.13, 0.21)
    rx, ry = 120, 90
    probes = np.array([(i, j) for j in (20, 45, 61) for i in range(30, 90, 7)], dtype=np.int32)
    ref = oracle_port.render(xyz, cells, alpha, q, rots, rx, ry, mg.REFERENCE_BOUNDS, threads=4, probes=probes)
    _, _, tau, I = ar.image_gradients(xyz, cells, alpha, q, rots, rx, ry, mg.REFERENCE_BOUNDS, np.zeros((ry, rx, 2)))
    img = ref["image"].astype(np.float64)
    assert np.abs(tau - img[..., 0]).max() <= 1e-5 * np.abs(img[..., 0]).max()
    assert np.abs(I - img[..., 1]).max() <= 1e-5 * np.abs(img[..., 1]).max()
    pix, cell, zh, dz = ar.segment_lists(xyz, cells, rots, rx, ry, mg.REFERENCE_BOUNDS)
    for (i, j), segs in zip(probes, ref["probes"]):
        mine = pix == j * rx + i
        assert len(segs) == mine.sum()
        # the oracle lists by descending z_hi, the helper by ascending
        assert np.array_equal(segs[::-1, 0].astype(int), cell[mine])
        np.testing.assert_allclose(segs[::-1, 2], dz[mine], rtol=1e-9, atol=1e-12)


def test_header_declares_and_capi_binds_the_adjoint():
    text = open(os.path.join(ROOT, "include", "course5_hip.h")).read()
    for name, args in (("c5_render_adjoint", r"c5_context\* ctx, const float\* grad_out_host, double\* grad_alpha_host, double\* grad_q_host"),
                       ("c5_render_adjoint_device", r"c5_context\* ctx, const void\* grad_out_device, void\* grad_alpha_device, void\* grad_q_device")):
        assert re.search(r"int " + name + r"\(" + args + r"\);", text), name
        assert name in capi.EXPORTS
    lib = capi.load_library()
    assert lib.c5_render_adjoint.restype is not None and len(lib.c5_render_adjoint.argtypes) == 4
    assert len(lib.c5_render_adjoint_device.argtypes) == 4
    assert hasattr(capi.Context, "render_adjoint") and hasattr(capi.Context, "render_adjoint_device")
    from course5_amd import autograd
    assert callable(autograd.render)


def test_course_help_lists_contribution():
    out = subprocess.run([COURSE, "--help"], capture_output=True, text=True, check=True).stdout
    assert re.search(r"^  --contribution arg\s+after the frame", out, re.M)


@pytest.mark.parametrize("extra, message", [
    (["--frames", "3"], "option '--contribution' cannot be used with '--frames' above 1"),
    (["--bench", "5"], "option '--contribution' cannot be used with '--bench'"),
    (["--devices", "0,1"], "option '--contribution' cannot be used with more than one of '--devices'"),
], ids=["frames", "bench", "devices"])
def test_contribution_rejects_what_it_cannot_do_at_parse_time(tmp_path, extra, message):
    """Rejected before anything is read or any GPU is touched (the source file does not even exist)."""
    r = subprocess.run([COURSE, "-f", str(tmp_path / "missing.vtk"), "-d", str(tmp_path / "o.vti"),
                        "--contribution", str(tmp_path / "c.vtk")] + extra, capture_output=True, text=True)
    assert r.returncode == 1
    assert r.stderr.strip() == "course: " + message
    assert not (tmp_path / "c.vtk").exists()

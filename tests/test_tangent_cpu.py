"""Tangent render, no GPU: the numpy restatement (tests/tangent_reference.py) against central differences of the adjoint
helper's forward and, exactly, against its gradients (<g, J v> = <J^T g, v>); the C ABI declarations and bindings; the
torch Function's forward-mode hooks."""
import os
import re
import types

import numpy as np
import pytest

from course5_amd import capi
from course5_amd import meshgen as mg
from tests import adjoint_reference as ar
from tests import tangent_reference as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps


def _random_lists(rng, n_px=40, n_cells=12):
    """Pixels of random segment lists over a few cells with the special values: clamped alpha, alpha = 0, alpha just
    above epsilon, a dz of 10 at alpha 2 and a dz of 1e-6."""
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
        z_hi = np.sort(rng.uniform(-1, 1, n))[::-1]
        lists.append(np.column_stack([cells, z_hi, dz]))
    return lists, alpha, q


def test_restatement_matches_central_differences_of_the_forward():
    rng = np.random.default_rng(21)
    lists, alpha, q = _random_lists(rng)
    # relative directions: every alpha stays on its side of epsilon and of the clamp; alpha = 0 does not move
    d_alpha = alpha * rng.normal(size=len(alpha))
    d_q = q * rng.normal(size=len(q))
    h = 1e-6
    for segs in lists:
        tau_dot, I_dot = tr.pixel_tangent(segs, alpha, q, d_alpha, d_q)
        (tp, ip), (tm, im) = (ar.forward(segs, alpha + s * h * d_alpha, q + s * h * d_q) for s in (1, -1))
        assert (tp - tm) / (2 * h) == pytest.approx(tau_dot, rel=1e-7, abs=1e-12)
        assert (ip - im) / (2 * h) == pytest.approx(I_dot, rel=1e-6, abs=1e-10)


def test_restatement_special_cases():
    """An inactive cell moves tau only; a clamped one moves tau and, through Q, I, but not I through alpha; a chord of
    1e-6 takes the series and agrees with the closed form of a longer one scaled down."""
    seg = np.array([[0, 0.5, 0.3], [1, 0.1, 0.2]])
    alpha, q = np.array([0.0, 3.0]), np.array([0.7, 0.4])
    assert tr.pixel_tangent(seg, alpha, q, np.array([1.0, 0.0]), np.zeros(2)) == (0.3, 0.0)
    assert tr.pixel_tangent(seg, alpha, q, np.array([0.0, 1.0]), np.zeros(2)) == (0.2, 0.0)
    tau_dot, I_dot = tr.pixel_tangent(seg, alpha, q, np.zeros(2), np.array([0.0, 1.0]))
    assert tau_dot == 0.0 and I_dot == pytest.approx(-np.expm1(-2.5 * 0.2) / 2.5)
    # short chord: dI/dalpha = -Q dz^2 / 2 to first order
    seg = np.array([[0, 0.0, 1e-6]])
    _, I_dot = tr.pixel_tangent(seg, np.array([1.0]), np.array([0.5]), np.array([1.0]), np.zeros(1))
    assert I_dot == pytest.approx(-0.5 * 0.5 * 1e-12, rel=1e-5)


def test_dot_product_identity_with_the_adjoint_helper():
    """<g, J v> = <J^T g, v> to rounding, per pixel list and over a whole image."""
    rng = np.random.default_rng(5)
    lists, alpha, q = _random_lists(rng)
    g = rng.normal(size=(len(lists), 2))
    v_a, v_q = rng.normal(size=len(alpha)), rng.normal(size=len(q))
    Jv = np.array([tr.pixel_tangent(s, alpha, q, v_a, v_q) for s in lists])
    ga, gq = ar.gradients(lists, g, alpha, q, len(alpha))
    lhs, rhs = float((g * Jv).sum()), float(ga @ v_a + gq @ v_q)
    assert lhs == pytest.approx(rhs, rel=1e-12, abs=1e-13)

    xyz, cells = mg.kuhn_box(4, jitter=0.1)
    alpha, q = mg.scalars(len(cells), seed=3)
    alpha[::17] = 0.0
    alpha[5::23] = 3.1
    rots = mg.view_rotations(0.13, 0.21)
    rx, ry = 64, 48
    v_a, v_q = rng.normal(size=len(cells)), rng.normal(size=len(cells))
    w = rng.normal(size=(ry, rx, 2))
    tau_dot, I_dot, tau, I = tr.image_tangent(xyz, cells, alpha, q, rots, rx, ry, mg.REFERENCE_BOUNDS, v_a, v_q)
    ga, gq, tau_ref, I_ref = ar.image_gradients(xyz, cells, alpha, q, rots, rx, ry, mg.REFERENCE_BOUNDS, w)
    np.testing.assert_allclose(tau, tau_ref, rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(I, I_ref, rtol=1e-12, atol=1e-15)
    lhs = float((w[..., 0] * tau_dot).sum() + (w[..., 1] * I_dot).sum())
    assert lhs == pytest.approx(float(ga @ v_a + gq @ v_q), rel=1e-11)


def test_image_restatement_matches_the_pixel_one():
    xyz, cells = mg.kuhn_box(3, jitter=0.1)
    alpha, q = mg.scalars(len(cells), seed=8)
    alpha[::7] = 0.0
    alpha[3::11] = 2.9
    rots = mg.view_rotations(0.13, 0.21)
    rx, ry = 40, 30
    rng = np.random.default_rng(2)
    v_a, v_q = rng.normal(size=len(cells)), rng.normal(size=len(cells))
    rows = np.arange(5, 25)
    tau_dot, I_dot, _, _ = tr.image_tangent(xyz, cells, alpha, q, rots, rx, ry, mg.REFERENCE_BOUNDS, v_a, v_q, rows=rows)
    pix, cell, zh, dz = ar.segment_lists(xyz, cells, rots, rx, ry, mg.REFERENCE_BOUNDS)
    covered = 0
    for r_local, r in enumerate(rows):
        for c in range(rx):
            m = pix == r * rx + c
            segs = np.column_stack([cell[m], zh[m], dz[m]])[::-1]  # the reference's order: descending z_hi
            want = tr.pixel_tangent(segs, alpha, q, v_a, v_q) if m.any() else (0.0, 0.0)
            covered += bool(m.any())
            assert tau_dot[r_local, c] == pytest.approx(want[0], rel=1e-12, abs=1e-15)
            assert I_dot[r_local, c] == pytest.approx(want[1], rel=1e-10, abs=1e-15)
    assert covered > 100
    # a NULL direction is a zero one; skipped pixels are 0
    skip = np.zeros((len(rows), rx), bool)
    skip[3:6, 10:20] = True
    t2, i2, _, _ = tr.image_tangent(xyz, cells, alpha, q, rots, rx, ry, mg.REFERENCE_BOUNDS, None, v_q, rows=rows, skip=skip)
    t3, i3, _, _ = tr.image_tangent(xyz, cells, alpha, q, rots, rx, ry, mg.REFERENCE_BOUNDS, np.zeros(len(cells)), v_q,
                                    rows=rows)
    assert not t2.any() and np.array_equal(i2[~skip], i3[~skip]) and not i2[skip].any()


def test_header_declares_and_capi_binds_the_tangent():
    text = open(os.path.join(ROOT, "include", "course5_hip.h")).read()
    for name, args in (("c5_render_tangent", r"c5_context\* ctx, const double\* d_alpha_host, const double\* d_q_host, float\* out_host"),
                       ("c5_render_tangent_device", r"c5_context\* ctx, const void\* d_alpha_dev, const void\* d_q_dev, void\* out_device")):
        assert re.search(r"int " + name + r"\(" + args + r"\);", text), name
        assert name in capi.EXPORTS
    lib = capi.load_library()
    assert lib.c5_render_tangent.restype is not None and len(lib.c5_render_tangent.argtypes) == 4
    assert len(lib.c5_render_tangent_device.argtypes) == 4
    assert hasattr(capi.Context, "render_tangent") and hasattr(capi.Context, "render_tangent_device")


def test_autograd_function_has_forward_mode():
    """torch.func and forward_ad need setup_context and jvp defined on the Function itself (the base class raises)."""
    from course5_amd import autograd
    for name in ("forward", "setup_context", "backward", "jvp"):
        assert name in vars(autograd._Render), name


def test_jvp_refuses_a_changed_frame_before_touching_a_gpu():
    from course5_amd import autograd
    fake = types.SimpleNamespace(frame_state=3, scalars_owner=None)
    fctx = types.SimpleNamespace(c5=fake, state=2, owner=object())
    with pytest.raises(RuntimeError, match="changed since the forward pass; render again before calling jvp"):
        autograd._Render.jvp(fctx, None, None, None)

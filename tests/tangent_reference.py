"""numpy restatement of the tangent render (include/course5_hip.h: c5_render_tangent) from per-pixel segment lists.

A pixel's segments come as rows {tet, z_hi, dz} in the reference's order (tests/adjoint_reference.py): sorted by
descending z_hi, the recurrence run from the last row to the first.  Number them k = 1..n in processing order:
    a_k = min(alpha_k, limit), active_k = !(a_k < DBL_EPSILON), E_k = exp(-a_k dz_k),
    tau_dot = sum_k dz_k dalpha_k                                                        (every segment, raw alpha)
    I_dot_k = E_k I_dot_{k-1} + dQ_k s_k + dalpha'_k (B_k - dz_k E_k I_{k-1})           (active; else I_dot_{k-1})
    s_k = (1 - E_k) / a_k, B_k = Q_k (dz_k E_k / a_k - (1 - E_k) / a_k^2), dalpha'_k = dalpha_k if alpha_k <= limit else 0
with B_k by its series in a_k dz_k below 1/8, as the adjoint's helper has it.  Whole images take their segment lists from
adjoint_reference.segment_lists.
"""
from __future__ import annotations

import math

import numpy as np

from tests import adjoint_reference as ar

EPS = ar.EPS


def pixel_tangent(segs, alpha, q, d_alpha, d_q, limit: float = 2.5) -> tuple[float, float]:
    """(tau_dot, I_dot) of one pixel in fp64."""
    tau_dot = 0.0
    for tet, _z, dz in segs:
        tau_dot += dz * d_alpha[int(tet)]
    I = I_dot = 0.0
    for tet, _z, dz in segs[::-1]:
        c, dz = int(tet), float(dz)
        a = min(alpha[c], limit)
        if a < EPS:
            continue
        E = math.exp(-a * dz)
        s = -math.expm1(-a * dz) / a
        src = d_q[c] * s
        if not alpha[c] > limit:
            src += d_alpha[c] * (q[c] * dz * dz * ar._bracket_over_q_dz2(a * dz) - dz * E * I)
        I_dot = E * I_dot + src
        I = E * I + q[c] * s
    return tau_dot, I_dot


def image_tangent(xyz, cells, alpha, q, rots, res_x, res_y, bounds, d_alpha, d_q, limit: float = 2.5, rows=None, skip=None,
                  with_scale: bool = False):
    """pixel_tangent over whole images, vectorised over the pixels.  d_alpha / d_q: [n_cells] (None: zero); rows: the
    global rows of the output (default: all); skip: optional bool [len(rows), res_x], True = a solid-marked pixel (0).
    Returns (tau_dot, I_dot, tau, I), each fp64 [len(rows), res_x]; with_scale: and tangent_of's dict."""
    m = ar.ray_matrices(xyz, cells, alpha, q, rots, res_x, res_y, bounds, limit, rows)
    return tangent_of(m, len(np.asarray(alpha)), d_alpha, d_q, skip, with_scale)


def tangent_of(m, n_cells: int, d_alpha, d_q, skip=None, with_scale: bool = False):
    """image_tangent from adjoint_reference.ray_matrices' dict (one set of matrices serves many directions).

    with_scale: also a dict of per-pixel bounds (adjoint_reference's docstring): scale_tau = sum dz |d_alpha|, scale_I = the
    recurrence run on |d_q| s + |d_alpha'| (|B| + dz E I_{k-1}), and the chord sensitivities sens_tau = sum F |d_alpha|,
    sens_I = sum_k F_k |T_k (d_q s + d_alpha' (B - dz E I_{k-1}))| / dz_k."""
    d_alpha = np.zeros(n_cells) if d_alpha is None else np.asarray(d_alpha, np.float64)
    d_q = np.zeros(n_cells) if d_q is None else np.asarray(d_q, np.float64)
    C, D, valid, active, E, S, Bk = m["C"], m["D"], m["valid"], m["active"], m["E"], m["S"], m["B"]
    Cc = np.maximum(C, 0)
    dA = np.where(valid, d_alpha[Cc], 0.0)
    dQ = np.where(valid, d_q[Cc], 0.0)
    dA_eff = np.where(m["clamped"], 0.0, dA)
    I_prev = m["I_prev"]
    src = dQ * S + dA_eff * (Bk - D * E * I_prev)
    I_dot = np.zeros(m["n_px"])
    for j in range(D.shape[1]):
        I_dot = np.where(active[:, j], E[:, j] * I_dot + src[:, j], I_dot)
    tau_dot = (D * dA).sum(1)
    tau, I = m["tau"].copy(), m["I"].copy()
    shape = m["shape"]
    extra = None
    if with_scale:
        abs_src = np.abs(dQ) * S + np.abs(dA_eff) * (np.abs(Bk) + D * E * np.abs(I_prev))
        scale_I = np.zeros(m["n_px"])
        for j in range(D.shape[1]):
            scale_I = np.where(active[:, j], E[:, j] * scale_I + abs_src[:, j], scale_I)
        extra = {"scale_tau": (D * np.abs(dA)).sum(1), "scale_I": scale_I, "sens_tau": (m["F"] * np.abs(dA)).sum(1),
                 "sens_I": (np.where(active, np.abs(m["T"] * src), 0.0) * m["F_dz"]).sum(1)}
    if skip is not None:
        sk = np.asarray(skip).reshape(-1)
        tau_dot[sk] = I_dot[sk] = tau[sk] = I[sk] = 0.0
        if extra:
            for v in extra.values():
                v[sk] = 0.0
    out = tau_dot.reshape(shape), I_dot.reshape(shape), tau.reshape(shape), I.reshape(shape)
    return out + ({k: v.reshape(shape) for k, v in extra.items()},) if with_scale else out

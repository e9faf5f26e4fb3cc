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
_SERIES = [(-1.0) ** (m + 1) * (m + 1) / math.factorial(m + 2) for m in range(14)]


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


def image_tangent(xyz, cells, alpha, q, rots, res_x, res_y, bounds, d_alpha, d_q, limit: float = 2.5, rows=None, skip=None):
    """pixel_tangent over whole images, vectorised over the pixels.  d_alpha / d_q: [n_cells] (None: zero); rows: the
    global rows of the output (default: all); skip: optional bool [len(rows), res_x], True = a solid-marked pixel (0).
    Returns (tau_dot, I_dot, tau, I), each fp64 [len(rows), res_x]."""
    rows = np.arange(res_y) if rows is None else np.asarray(rows)
    alpha, q = np.asarray(alpha, np.float64), np.asarray(q, np.float64)
    d_alpha = np.zeros_like(alpha) if d_alpha is None else np.asarray(d_alpha, np.float64)
    d_q = np.zeros_like(q) if d_q is None else np.asarray(d_q, np.float64)
    pix, cell, _zh, dz = ar.segment_lists(xyz, cells, rots, res_x, res_y, bounds)
    row_slot = np.full(res_y, -1)
    row_slot[rows] = np.arange(len(rows))
    sel = row_slot[pix // res_x] >= 0
    lp = (row_slot[pix // res_x] * res_x + pix % res_x)[sel]
    cell, dz = cell[sel], dz[sel]
    n_px = len(rows) * res_x
    # [pixel, k] matrices, k = processing order (deepest first)
    starts = np.searchsorted(lp, np.arange(n_px))
    k = np.arange(len(lp)) - starts[lp]
    M = int(k.max()) + 1 if len(k) else 1
    C = np.full((n_px, M), -1)
    D = np.zeros((n_px, M))
    C[lp, k], D[lp, k] = cell, dz
    valid = C >= 0
    Cc = np.maximum(C, 0)
    a_raw = np.where(valid, alpha[Cc], 0.0)
    Q = np.where(valid, q[Cc], 0.0)
    dA = np.where(valid, d_alpha[Cc], 0.0)
    dQ = np.where(valid, d_q[Cc], 0.0)
    a = np.minimum(a_raw, limit)
    active = valid & ~(a < EPS)
    x = np.where(active, a * D, 0.0)
    E = np.exp(-x)
    with np.errstate(divide="ignore", invalid="ignore"):
        S = np.where(active, -np.expm1(-x) / np.where(active, a, 1.0), 0.0)
        direct = (x * E + np.expm1(-x)) / np.where(x > 0, x * x, 1.0)
    ser = sum(c * x ** m for m, c in enumerate(_SERIES))
    Bk = Q * D * D * np.where(x < 0.125, ser, direct)
    dA_eff = np.where(a_raw > limit, 0.0, dA)
    I = np.zeros(n_px)
    I_dot = np.zeros(n_px)
    for j in range(M):
        act = active[:, j]
        src = dQ[:, j] * S[:, j] + dA_eff[:, j] * (Bk[:, j] - D[:, j] * E[:, j] * I)
        I_dot = np.where(act, E[:, j] * I_dot + src, I_dot)
        I = np.where(act, E[:, j] * I + Q[:, j] * S[:, j], I)
    tau_dot = (D * dA).sum(1)
    tau = (D * a_raw).sum(1)
    if skip is not None:
        s = np.asarray(skip).reshape(-1)
        tau_dot[s] = I_dot[s] = tau[s] = I[s] = 0.0
    shape = (len(rows), res_x)
    return tau_dot.reshape(shape), I_dot.reshape(shape), tau.reshape(shape), I.reshape(shape)

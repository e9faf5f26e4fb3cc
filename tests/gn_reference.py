"""numpy restatement of the Gauss-Newton renders (include/course5_hip.h: c5_render_gn_product, c5_render_gn_diagonal).

J is the Jacobian of the image (tau, I per pixel) with respect to the cells' (alpha, Q).  A tetrahedron is convex, so a
ray crosses a cell in at most one segment and the entry of J for (pixel, cell) is that segment's term of
tests/adjoint_reference.py (pixel_terms): dtau/dalpha = dz, dI/dalpha, dI/dQ.  With per-pixel weights W = (w_tau, w_I):
    H v = J^T W J v,    diag_alpha[c] = sum_p w_tau dz^2 + w_I (dI/dalpha)^2,    diag_q[c] = sum_p w_I (dI/dQ)^2.

Two forms: dense_jacobian, from per-pixel segment lists through adjoint_reference.pixel_terms (small grids: the matrix
itself), and segment_terms / product / diagonal, vectorised over whole images as adjoint_reference.image_gradients is
(the same formulas on [pixel, k] matrices) - tests/test_gn_cpu.py holds the one to the other and both to
image_gradients(weights = w * image_tangent(v)).
"""
from __future__ import annotations

import math

import numpy as np

from tests import adjoint_reference as ar

EPS = ar.EPS


def pixel_lists(xyz, cells, rots, res_x, res_y, bounds):
    """Every pixel's rows {cell, z_hi, dz} in the reference's order (descending z_hi), from segment_lists."""
    pix, cell, zh, dz = ar.segment_lists(xyz, cells, rots, res_x, res_y, bounds)
    lists = [[] for _ in range(res_x * res_y)]
    for p, c, z, d in zip(pix[::-1], cell[::-1], zh[::-1], dz[::-1]):
        lists[int(p)].append((int(c), float(z), float(d)))
    return lists


def dense_jacobian(lists, alpha, q, n_cells: int, limit: float = 2.5) -> np.ndarray:
    """J [2 n_px, 2 n_cells]: row 2p = tau of pixel p, row 2p + 1 = I; column c = alpha_c, n_cells + c = Q_c."""
    J = np.zeros((2 * len(lists), 2 * n_cells))
    for p, segs in enumerate(lists):
        if not segs:
            continue
        for c, dtau, dI_da, dI_dq in ar.pixel_terms(segs, alpha, q, limit):
            J[2 * p, c] += dtau
            J[2 * p + 1, c] += dI_da
            J[2 * p + 1, n_cells + c] += dI_dq
    return J


def segment_terms(xyz, cells, alpha, q, rots, res_x, res_y, bounds, limit: float = 2.5, rows=None, skip=None):
    """Flat arrays over every segment of the pixels of the global rows `rows` (default: all; skip: bool [len(rows),
    res_x], True = solid-marked, nothing): (pixel, cell, dtau/dalpha, dI/dalpha, dI/dQ), pixel = local row * res_x + col.
    The [pixel, k] evaluation of adjoint_reference.image_gradients, the terms kept instead of summed."""
    rows = np.arange(res_y) if rows is None else np.asarray(rows)
    alpha, q = np.asarray(alpha, np.float64), np.asarray(q, np.float64)
    pix, cell, _zh, dz = ar.segment_lists(xyz, cells, rots, res_x, res_y, bounds)
    row_slot = np.full(res_y, -1)
    row_slot[rows] = np.arange(len(rows))
    sel = row_slot[pix // res_x] >= 0
    lp = (row_slot[pix // res_x] * res_x + pix % res_x)[sel]
    cell, dz = cell[sel], dz[sel]
    n_px = len(rows) * res_x
    starts = np.searchsorted(lp, np.arange(n_px))
    k = np.arange(len(lp)) - starts[lp]
    M = int(k.max()) + 1 if len(k) else 1
    C = np.full((n_px, M), -1)
    D = np.zeros((n_px, M))
    C[lp, k], D[lp, k] = cell, dz
    valid = C >= 0
    a_raw = np.where(valid, alpha[np.maximum(C, 0)], 0.0)
    Q = np.where(valid, q[np.maximum(C, 0)], 0.0)
    a = np.minimum(a_raw, limit)
    active = valid & ~(a < EPS)
    x = np.where(active, a * D, 0.0)
    E = np.exp(-x)
    with np.errstate(divide="ignore", invalid="ignore"):
        S = np.where(active, -np.expm1(-x) / np.where(active, a, 1.0), 0.0)
        ser = sum((-1.0) ** (m + 1) * (m + 1) / math.factorial(m + 2) * x ** m for m in range(14))
        direct = (x * E + np.expm1(-x)) / np.where(x > 0, x * x, 1.0)
    br = Q * D * D * np.where(x < 0.125, ser, direct)
    lam = np.cumsum(x, axis=1)
    T = np.exp(-(lam[:, -1:] - lam))
    I_prev = np.zeros_like(D)
    I = np.zeros(n_px)
    for j in range(M):
        I_prev[:, j] = I
        I = np.where(active[:, j], E[:, j] * I + Q[:, j] * S[:, j], I)
    dI_dq = np.where(active, T * S, 0.0)
    dI_da = np.where(active & ~(a_raw > limit), T * (br - D * E * I_prev), 0.0)
    if skip is not None:
        valid = valid & ~np.asarray(skip).reshape(-1)[:, None]
    P = np.broadcast_to(np.arange(n_px)[:, None], C.shape)
    return P[valid], C[valid], D[valid], dI_da[valid], dI_dq[valid]


def _weights(weight, n_px):
    return np.ones((n_px, 2)) if weight is None else np.asarray(weight, np.float64).reshape(n_px, 2)


def product(terms, n_px: int, n_cells: int, v_alpha, v_q, weight=None):
    """(h_alpha, h_q, jv) for one direction (None: zero): jv [n_px, 2] fp64 = J v, h = J^T (weight * jv)."""
    P, C, dtau, dI_da, dI_dq = terms
    va = np.zeros(n_cells) if v_alpha is None else np.asarray(v_alpha, np.float64)
    vq = np.zeros(n_cells) if v_q is None else np.asarray(v_q, np.float64)
    jv = np.zeros((n_px, 2))
    np.add.at(jv[:, 0], P, dtau * va[C])
    np.add.at(jv[:, 1], P, dI_da * va[C] + dI_dq * vq[C])
    g = _weights(weight, n_px) * jv
    ha, hq = np.zeros(n_cells), np.zeros(n_cells)
    np.add.at(ha, C, g[P, 0] * dtau + g[P, 1] * dI_da)
    np.add.at(hq, C, g[P, 1] * dI_dq)
    return ha, hq, jv


def diagonal(terms, n_px: int, n_cells: int, weight=None):
    """(diag_alpha, diag_q) of J^T W J."""
    P, C, dtau, dI_da, dI_dq = terms
    w = _weights(weight, n_px)
    da, dq = np.zeros(n_cells), np.zeros(n_cells)
    np.add.at(da, C, w[P, 0] * dtau ** 2 + w[P, 1] * dI_da ** 2)
    np.add.at(dq, C, w[P, 1] * dI_dq ** 2)
    return da, dq

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

import numpy as np

from tests import adjoint_reference as ar



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


def segment_terms(xyz, cells, alpha, q, rots, res_x, res_y, bounds, limit: float = 2.5, rows=None, skip=None,
                  with_scale: bool = False):
    """Flat arrays over every segment of the pixels of the global rows `rows` (default: all; skip: bool [len(rows),
    res_x], True = solid-marked, nothing): (pixel, cell, dtau/dalpha, dI/dalpha, dI/dQ), pixel = local row * res_x + col.
    The [pixel, k] evaluation of adjoint_reference.image_gradients, the terms kept instead of summed.
    with_scale: two more arrays, |dI/dalpha| with its two parts added in absolute value, T (|B| + dz E I_{k-1}), and the
    segment's factor F of the chord sensitivity (adjoint_reference's docstring)."""
    return terms_of(ar.ray_matrices(xyz, cells, alpha, q, rots, res_x, res_y, bounds, limit, rows), skip, with_scale)


def terms_of(m, skip=None, with_scale: bool = False):
    """segment_terms from adjoint_reference.ray_matrices' dict."""
    C, D, valid, active, E, T = m["C"], m["D"], m["valid"], m["active"], m["E"], m["T"]
    moves = active & ~m["clamped"]
    dI_dq = np.where(active, T * m["S"], 0.0)
    dI_da = np.where(moves, T * (m["B"] - D * E * m["I_prev"]), 0.0)
    if skip is not None:
        valid = valid & ~np.asarray(skip).reshape(-1)[:, None]
    P = np.broadcast_to(np.arange(m["n_px"])[:, None], C.shape)
    out = P[valid], C[valid], D[valid], dI_da[valid], dI_dq[valid]
    if with_scale:
        out += (m["abs_da"][valid], m["F"][valid])
    return out


def _weights(weight, n_px):
    return np.ones((n_px, 2)) if weight is None else np.asarray(weight, np.float64).reshape(n_px, 2)


def product(terms, n_px: int, n_cells: int, v_alpha, v_q, weight=None):
    """(h_alpha, h_q, jv) for one direction (None: zero): jv [n_px, 2] fp64 = J v, h = J^T (weight * jv)."""
    P, C, dtau, dI_da, dI_dq = terms[:5]
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
    P, C, dtau, dI_da, dI_dq = terms[:5]
    w = _weights(weight, n_px)
    da, dq = np.zeros(n_cells), np.zeros(n_cells)
    np.add.at(da, C, w[P, 0] * dtau ** 2 + w[P, 1] * dI_da ** 2)
    np.add.at(dq, C, w[P, 1] * dI_dq ** 2)
    return da, dq


def diagonal_scale(terms, n_px: int, n_cells: int, weight=None):
    """Per-cell bounds for diagonal(): a dict scale_alpha / scale_q (the sums with dI/dalpha's two parts added in absolute
    value before squaring) and sens_alpha / sens_q (sum of 2 F contribution / dz: a squared term goes with dz^2).
    terms: segment_terms(with_scale=True)."""
    P, C, dtau, dI_da, dI_dq, abs_da, F = terms
    w = np.abs(_weights(weight, n_px))
    parts = {"scale_alpha": w[P, 0] * dtau ** 2 + w[P, 1] * abs_da ** 2, "scale_q": w[P, 1] * dI_dq ** 2,
             "sens_alpha": 2.0 * F * (w[P, 0] * dtau ** 2 + w[P, 1] * dI_da ** 2) / dtau, "sens_q": 2.0 * F * w[P, 1] * dI_dq ** 2 / dtau}
    return {name: np.bincount(C, weights=t, minlength=n_cells) for name, t in parts.items()}


def product_header(terms, n_px: int, n_cells: int, v_alpha, v_q, weight=None):
    """product() with the fp32 intermediate of include/course5_hip.h: J v rounded to fp32, one fp32 multiply by the
    weight (None: no multiply), J^T of that in fp64.  Returns (h_alpha, h_q, jv fp32 [n_px, 2], extra); extra: a dict
    scale_alpha / scale_q / sens_alpha / sens_q of the adjoint with the upstream image |w| |J v| (its absolute sums and
    chord sensitivity, as image_gradients(with_scale=True) defines them).  terms: segment_terms(with_scale=True)."""
    P, C, dtau, dI_da, dI_dq, abs_da, F = terms
    _, _, jv = product(terms, n_px, n_cells, v_alpha, v_q, None)
    jv32 = jv.astype(np.float32)
    g32 = jv32 if weight is None else (np.asarray(weight, np.float32).reshape(n_px, 2) * jv32).astype(np.float32)
    g = g32.astype(np.float64)
    ha, hq = np.zeros(n_cells), np.zeros(n_cells)
    np.add.at(ha, C, g[P, 0] * dtau + g[P, 1] * dI_da)
    np.add.at(hq, C, g[P, 1] * dI_dq)
    ag = np.abs(g)
    parts = {"scale_alpha": ag[P, 0] * dtau + ag[P, 1] * abs_da, "scale_q": ag[P, 1] * np.abs(dI_dq),
             "sens_alpha": F * (ag[P, 0] * dtau + np.abs(g[P, 1] * dI_da)) / dtau, "sens_q": F * np.abs(g[P, 1] * dI_dq) / dtau}
    return ha, hq, jv32, {name: np.bincount(C, weights=t, minlength=n_cells) for name, t in parts.items()}

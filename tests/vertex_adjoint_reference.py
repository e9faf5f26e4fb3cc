"""numpy restatement of the vertex adjoint render (include/course5_hip.h: c5_render_vertex_adjoint): the gradient of the
frame with respect to the grid's points, from adjoint_reference.ray_matrices and the faces motion_reference.face_matrices
finds.

With adjoint_reference's numbering (k = 1..n in processing order) a segment's chord dz_k = w_exit - w_entry has
    G_k = d loss / d dz_k = g_tau alpha_k + g_I T_k E_k (Q_k - a_k I_{k-1})      (raw alpha; the second term: active segments)
(motion_reference: tau_dot = sum alpha_k ddz_k, I_dot = sum T_k g_k ddz_k).  A face with view-space vertices P_0, P_1, P_2
has the depth w = sum_i lambda_i z_i at the pixel (x, y), lambda its barycentric coordinates in the projected triangle, and
    dw / d(x_i, y_i, z_i) = lambda_i (-gx, -gy, 1)
with the face's slopes - motion_reference's dw = u_z - gx u_x - gy u_y for u(P) = sum lambda_i u_i.  So
    grad_view[v] = sum over pixels, segments and faces holding v of (+G_k lambda_v [exit] - G_k lambda_v [entry]) (-gx, -gy, 1)
and in the coordinates of the upload grad_xyz[v] = M^T grad_view[v], M the linear part of the view.

SCALE: the same sums with every term replaced by its absolute value (|G_k| from |g_tau| |alpha| + |g_I| T E (|Q| + a |I|)):
what rounding can do to a component.

CHORD SENSITIVITY.  What an error of the chords can do to a component (motion_reference derives the same for I_dot).  The
barycentrics and the slopes come from the vertices and the pixel alone; the chords enter through G_k only, and there
through E alone: G_k = g_tau alpha_k + g_I T_k g_k with g_k = E_k (Q_k - a_k I_{k-1}), T_k = prod_{m > k} E_m.  A chord dz_j
is held
  (i)   for j > k by T_k:                   d G_k / d dz_j = -a_j g_I T_k g_k
  (ii)  for j = k by E_k in g_k:            d G_k / d dz_k = -a_k g_I T_k g_k
  (iii) for j < k by I_{k-1}, which holds I_j:  d I_{k-1} / d dz_j = (prod_{j < m < k} E_m) g_j, and with
        T_k E_k prod_{j < m < k} E_m = T_j:  d G_k / d dz_j = -a_k g_I T_j g_j
(active segments; an inactive one has E = 1 whatever its chord, and g_tau alpha_k holds no chord at all).  Every chord is
known to F_j dz_err, F_j = max(1, |gx| + |gy|) of the steeper of its two faces (adjoint_reference), so term by term
    sens_G_k = |g_I| [T_k |g_k| sum_{j >= k} a_j F_j + a_k sum_{j < k} F_j T_j |g_j|]
and a component's sensitivity is the scale's sum with |G_k| replaced by sens_G_k:
    sens_view[v] = sum over pixels, segments and faces holding v of sens_G_k |lambda_v| |(-gx, -gy, 1)|,  sens_raw = sens_view |M|.
tests/test_vertex_adjoint_cpu.py re-evaluates the restatement with every chord moved by +-F dz_err (with_chords) and finds
the change within 1e-9 scale_raw + dz_err sens_raw.
"""
from __future__ import annotations

import numpy as np

from tests import adjoint_reference as ar

FACES = np.array(ar._FACES)


def view_matrix(rots):
    """M [3, 3]: the linear part of the view, rotate(p) = M p + t."""
    e = ar.rotate(np.vstack([np.zeros((1, 3)), np.eye(3)]), rots)
    return (e[1:] - e[0]).T


def segment_faces(xyz, cells, rots, res_x, res_y, bounds, rows=None):
    """motion_reference.face_matrices' faces again, with what the vertex adjoint needs of them: a dict of [pixel, k]
    matrices in ray_matrices' layout - C cell (-1: none), F_out / F_in the face's index in the cell, GX_*, GY_* its slopes,
    Z_* its depth at the pixel and L_* [pixel, k, 3] the pixel's barycentric coordinates (the face's vertices in
    adjoint_reference._FACES' order); X, Y the pixel's coordinates, so that motion_reference.motion_of takes the dict too."""
    rows = np.arange(res_y) if rows is None else np.asarray(rows)
    cells = np.asarray(cells).reshape(-1, 4)
    pix, cell, zh, dz = ar.segment_lists(xyz, cells, rots, res_x, res_y, bounds)
    X, Y, _sx, _sy = ar.pixel_coordinates(bounds, res_x, res_y)
    x, y = X[pix % res_x], Y[pix // res_x]
    P = ar.rotate(xyz, rots)[cells[cell]]  # [S, 4, 3]
    n = len(pix)
    cover = np.zeros((n, 4), dtype=bool)
    zf, gx, gy, lam = np.zeros((n, 4)), np.zeros((n, 4)), np.zeros((n, 4)), np.zeros((n, 4, 3))
    for f, (ia, ib, ic) in enumerate(ar._FACES):
        A, B, Cc = P[:, ia], P[:, ib], P[:, ic]
        e0 = (B[:, 0] - A[:, 0]) * (y - A[:, 1]) - (B[:, 1] - A[:, 1]) * (x - A[:, 0])
        e1 = (Cc[:, 0] - B[:, 0]) * (y - B[:, 1]) - (Cc[:, 1] - B[:, 1]) * (x - B[:, 0])
        e2 = (A[:, 0] - Cc[:, 0]) * (y - Cc[:, 1]) - (A[:, 1] - Cc[:, 1]) * (x - Cc[:, 0])
        cover[:, f] = ((e0 >= 0) & (e1 >= 0) & (e2 >= 0)) | ((e0 <= 0) & (e1 <= 0) & (e2 <= 0))
        Aa = (B[:, 0] - A[:, 0]) * (Cc[:, 2] - A[:, 2]) - (Cc[:, 0] - A[:, 0]) * (B[:, 2] - A[:, 2])
        Bb = (B[:, 1] - A[:, 1]) * (Cc[:, 2] - A[:, 2]) - (Cc[:, 1] - A[:, 1]) * (B[:, 2] - A[:, 2])
        m = (B[:, 0] - A[:, 0]) * (Cc[:, 1] - A[:, 1]) - (Cc[:, 0] - A[:, 0]) * (B[:, 1] - A[:, 1])
        with np.errstate(divide="ignore", invalid="ignore"):
            gy[:, f], gx[:, f] = Aa / m, -Bb / m
            zf[:, f] = ((y - A[:, 1]) * Aa - (x - A[:, 0]) * Bb) / m + A[:, 2]
            # e1 / m, e2 / m, e0 / m: the weights of A, B and C (the sub-triangle opposite each vertex)
            lam[:, f, 0], lam[:, f, 1], lam[:, f, 2] = e1 / m, e2 / m, e0 / m
    idx = np.arange(n)

    def nearest(z):  # the covering face whose depth at the pixel is z (motion_reference.face_matrices' rule)
        d = np.where(cover & np.isfinite(zf), np.abs(zf - z[:, None]), np.inf)
        f = d.argmin(1)
        return f, zf[idx, f], gx[idx, f], gy[idx, f], lam[idx, f]

    per_seg = nearest(zh) + nearest(zh - dz) + (x, y)
    row_slot = np.full(res_y, -1)
    row_slot[rows] = np.arange(len(rows))
    sel = row_slot[pix // res_x] >= 0
    lp = (row_slot[pix // res_x] * res_x + pix % res_x)[sel]
    n_px = len(rows) * res_x
    k = np.arange(len(lp)) - np.searchsorted(lp, np.arange(n_px))[lp]
    M = int(k.max()) + 1 if len(k) else 1
    out = {"C": np.full((n_px, M), -1)}
    out["C"][lp, k] = cell[sel]
    names = ("F_out", "Z_out", "GX_out", "GY_out", "L_out", "F_in", "Z_in", "GX_in", "GY_in", "L_in", "X", "Y")
    for name, v in zip(names, per_seg):
        out[name] = np.zeros((n_px, M) + v.shape[1:], dtype=v.dtype)
        out[name][lp, k] = v[sel]
    return out


def with_chords(m, D):
    """ray_matrices' dict with the chords D [pixel, k] in place of its own: what gradients_of reads of it (D, E, T, I_prev)
    evaluated again, everything else as it was.  For the calibration of the chord sensitivity."""
    out = dict(m)
    a, Q, active = m["a"], m["Q"], m["active"]
    D = np.where(m["valid"], D, 0.0)
    x = np.where(active, a * D, 0.0)
    E = np.exp(-x)
    S = np.where(active, -np.expm1(-x) / np.where(active, a, 1.0), 0.0)
    I_prev, I = np.zeros_like(D), np.zeros(m["n_px"])
    for j in range(D.shape[1]):
        I_prev[:, j] = I
        I = np.where(active[:, j], E[:, j] * I + Q[:, j] * S[:, j], I)
    out.update(D=D, E=E, S=S, T=ar._transmittance(a, D), I_prev=I_prev, I=I)
    return out


def chord_weights(m, weights, skip=None, with_sens: bool = False):
    """(G, |G|'s bound) [pixel, k] from ray_matrices' dict and the upstream image `weights` [rows, res_x, 2]; with_sens:
    and sens_G (module docstring)."""
    w = np.asarray(weights, np.float64).reshape(m["n_px"], 2).copy()
    if skip is not None:
        w[np.asarray(skip).reshape(-1)] = 0.0
    g_tau, g_I = w[:, :1], w[:, 1:]
    valid, active, a, Q, E, T, I_prev = m["valid"], m["active"], m["a"], m["Q"], m["E"], m["T"], m["I_prev"]
    a_raw = np.where(valid, m["a_raw"], 0.0)
    G = g_tau * a_raw + np.where(active, g_I * T * E * (Q - a * I_prev), 0.0)
    G_abs = np.abs(g_tau) * np.abs(a_raw) + np.where(active, np.abs(g_I) * T * E * (np.abs(Q) + a * np.abs(I_prev)), 0.0)
    if not with_sens:
        return G, G_abs
    Tg = np.where(active, T * np.abs(E * (Q - a * I_prev)), 0.0)      # T_k |g_k|
    aF = np.where(active, a * m["F"], 0.0)
    from_k = aF[:, ::-1].cumsum(1)[:, ::-1]                           # sum_{j >= k} a_j F_j
    FTg = m["F"] * Tg
    before = FTg.cumsum(1) - FTg                                      # sum_{j < k} F_j T_j |g_j|
    return G, G_abs, np.abs(g_I) * (Tg * from_k + np.where(active, a, 0.0) * before)


def gradients_of(m, geo, cells, n_pts, rots, weights, skip=None):
    """The vertex adjoint from ray_matrices' and segment_faces' dicts: a dict view / raw [n_pts, 3] (view space; the
    coordinates of the upload), scale_view / scale_raw, the same sums of absolute values, and sens_view / sens_raw, the
    chord sensitivity (module docstring)."""
    assert np.array_equal(m["C"], geo["C"])
    cells = np.asarray(cells).reshape(-1, 4)
    G, G_abs, G_sens = chord_weights(m, weights, skip, with_sens=True)
    valid = m["valid"]
    c = m["C"][valid]
    gv, sv, xv = np.zeros((n_pts, 3)), np.zeros((n_pts, 3)), np.zeros((n_pts, 3))
    for side, sign in (("out", 1.0), ("in", -1.0)):
        vid = cells[c][np.arange(len(c))[:, None], FACES[geo["F_" + side][valid]]]  # [S, 3]
        lam = geo["L_" + side][valid]                                                   # [S, 3]
        vec = np.stack([-geo["GX_" + side][valid], -geo["GY_" + side][valid], np.ones(len(c))], axis=1)  # [S, 3]
        term = (sign * G[valid])[:, None, None] * lam[:, :, None] * vec[:, None, :]     # [S, vertex, xyz]
        shape = np.abs(lam)[:, :, None] * np.abs(vec)[:, None, :]
        flat = vid.reshape(-1)
        for acc, v in ((gv, term), (sv, G_abs[valid][:, None, None] * shape), (xv, G_sens[valid][:, None, None] * shape)):
            for k in range(3):
                acc[:, k] += np.bincount(flat, weights=v[..., k].reshape(-1), minlength=n_pts)
    M = view_matrix(rots)
    return {"view": gv, "raw": gv @ M, "scale_view": sv, "scale_raw": sv @ np.abs(M), "sens_view": xv, "sens_raw": xv @ np.abs(M)}


def vertex_gradients(xyz, cells, alpha, q, rots, res_x, res_y, bounds, weights, limit: float = 2.5, rows=None, skip=None):
    """gradients_of for one upstream image, the matrices built here.  weights: [len(rows), res_x, 2] (g_tau, g_I) of the
    global rows `rows` (default: all); skip: bool [len(rows), res_x], True = solid-marked (contributes nothing)."""
    m = ar.ray_matrices(xyz, cells, alpha, q, rots, res_x, res_y, bounds, limit, rows)
    geo = segment_faces(xyz, cells, rots, res_x, res_y, bounds, rows)
    return gradients_of(m, geo, cells, len(np.asarray(xyz).reshape(-1, 3)), rots, weights, skip)


def loss(xyz, cells, alpha, q, rots, res_x, res_y, bounds, weights, limit: float = 2.5):
    """<g_tau, tau> + <g_I, I> of the restated fp64 image (for finite differences)."""
    m = ar.ray_matrices(xyz, cells, alpha, q, rots, res_x, res_y, bounds, limit)
    w = np.asarray(weights, np.float64).reshape(m["n_px"], 2)
    return float(w[:, 0] @ m["tau"] + w[:, 1] @ m["I"])


__all__ = ["view_matrix", "segment_faces", "with_chords", "chord_weights", "gradients_of", "vertex_gradients", "loss"]

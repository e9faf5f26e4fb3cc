"""numpy restatement of the motion tangent render (include/course5_hip.h: c5_render_motion_tangent) from per-pixel
segment lists: the frame differentiated with respect to an affine motion u(p) = A p + b of the grid in view space.

A pixel's segments are adjoint_reference.segment_lists' (the reference's binning and pairing); per segment the two faces
the chord runs between are found again from the cell's rotated vertices - the covering faces whose depths at the pixel
are the segment's z_hi and z_hi - dz - with their slopes, z = c + gx x + gy y (line.cpp:158-171: gy = A / m, gx = -B / m).
The rays are parallel to z, so the depth of such a face at the fixed pixel (x, y) moves by
    dw = u_z(P) - gx u_x(P) - gy u_y(P),   P = (x, y, z_face),
and the chord by ddz_k = dw_exit,k - dw_entry,k (exit: the face at z_hi).  With adjoint_reference's numbering (k = 1..n
in processing order, deepest first; a_k the clamped alpha, E_k = exp(-a_k dz_k), I_k = E_k I_{k-1} + Q_k (1 - E_k) / a_k):
    tau_dot = sum_k alpha_k ddz_k                                                (raw alpha, every segment)
    I_dot_k = E_k I_dot_{k-1} + g_k ddz_k,  g_k = dI_k / d dz_k = E_k (Q_k - a_k I_{k-1})   (active; else I_dot_{k-1})
The clamp is on alpha, not on the chord: a clamped cell moves with its chord like any other.

SCALE.  The same sums with ddz replaced by |dw_exit| + |dw_entry| and every term by its absolute value (scale_tau =
sum |alpha_k| (|dw_exit| + |dw_entry|); scale_I: the recurrence on E_k (|Q_k| + a_k |I_{k-1}|) (|dw_exit| + |dw_entry|)):
what rounding can do to the result.

CHORD SENSITIVITY.  What an error of the chords can do.  The result is I_dot = sum_k T_k c_k with c_k = g_k ddz_k and
T_k = prod_{m > k} E_m.  A chord dz_k enters through E_k alone, in three places:
  (i)   T_j for j < k holds E_k:            d/d dz_k = -a_k sum_{j < k} T_j c_j
  (ii)  c_k holds E_k:                      d/d dz_k = -a_k T_k c_k
  (iii) I_{j-1} for j > k holds I_k:        d I_{j-1} / d dz_k = (prod_{k < m < j} E_m) g_k, and c_j = -E_j a_j ddz_j I_{j-1} + ...;
        with T_j E_j prod_{k < m < j} E_m = T_k:   d/d dz_k = -T_k g_k sum_{j > k, active} a_j ddz_j
so  d I_dot / d dz_k = -a_k sum_{j <= k} T_j c_j - T_k g_k sum_{j > k} a_j ddz_j, bounded term by term by
    chord_k = a_k sum_{j <= k} |T_j c_j| + T_k |g_k| sum_{j > k} a_j |ddz_j|.
Besides, a face's own depth enters its dw: d dw / d z_face = kappa = A_zz - gx A_xz - gy A_yz, so an error of the two depths
moves ddz_k by up to |kappa_exit| + |kappa_entry| times it, and the result by T_k |g_k| (tau: |alpha_k|) times that.  With
F_k = max(1, |gx| + |gy|) of the steeper face (adjoint_reference: a depth is known that much worse than the coordinates)
    sens_I   = sum_k F_k [chord_k + T_k |g_k| (|kappa_exit| + |kappa_entry|)]
    sens_tau = sum_k F_k |alpha_k| (|kappa_exit| + |kappa_entry|)                 (tau_dot does not hold the chords)
tests/test_motion_cpu.py re-evaluates the restatement with every chord moved by +-F_k dz_err and finds the change within
1e-9 scale + dz_err sens.
"""
from __future__ import annotations

import numpy as np

from tests import adjoint_reference as ar

EPS = ar.EPS
Z_TRANSLATION = np.array([0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1.0])
Z_SCALE = np.array([0, 0, 0, 0, 0, 0, 0, 0, 1.0, 0, 0, 0])  # u = (0, 0, z): every chord grows at its own rate


def scalars(n: int, seed: int):
    """alpha ~ U[0, 4) with exact zeros, nothing in [eps, 1e-6); Q ~ U[0, 1)."""
    rng = np.random.default_rng(seed)
    alpha = rng.uniform(0.0, 4.0, n)
    alpha[rng.random(n) < 0.05] = 0.0
    alpha[(alpha > 0) & (alpha < 1e-6)] = 1e-6
    return alpha, rng.uniform(0.0, 1.0, n)


def face_matrices(xyz, cells, rots, res_x, res_y, bounds, rows=None):
    """Per segment, laid out as adjoint_reference.ray_matrices lays its own out ([pixel, k], k the processing order, pixel
    = local row * res_x + col over the global rows `rows`): C cell (-1: none), X, Y the pixel's coordinates, and for the
    exit and the entry face Z_out, GX_out, GY_out, Z_in, GX_in, GY_in."""
    rows = np.arange(res_y) if rows is None else np.asarray(rows)
    cells = np.asarray(cells).reshape(-1, 4)
    pix, cell, zh, dz = ar.segment_lists(xyz, cells, rots, res_x, res_y, bounds)
    X, Y, _sx, _sy = ar.pixel_coordinates(bounds, res_x, res_y)
    x, y = X[pix % res_x], Y[pix // res_x]
    P = ar.rotate(xyz, rots)[cells[cell]]  # [S, 4, 3]
    n = len(pix)
    cover = np.zeros((n, 4), dtype=bool)
    zf, gx, gy = np.zeros((n, 4)), np.zeros((n, 4)), np.zeros((n, 4))
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
    idx = np.arange(n)

    def nearest(z):  # the covering face whose depth at the pixel is z
        d = np.where(cover & np.isfinite(zf), np.abs(zf - z[:, None]), np.inf)
        f = d.argmin(1)
        return zf[idx, f], gx[idx, f], gy[idx, f]

    per_seg = (x, y) + nearest(zh) + nearest(zh - dz)
    # ray_matrices' layout
    row_slot = np.full(res_y, -1)
    row_slot[rows] = np.arange(len(rows))
    sel = row_slot[pix // res_x] >= 0
    lp = (row_slot[pix // res_x] * res_x + pix % res_x)[sel]
    n_px = len(rows) * res_x
    k = np.arange(len(lp)) - np.searchsorted(lp, np.arange(n_px))[lp]
    M = int(k.max()) + 1 if len(k) else 1
    out = {"C": np.full((n_px, M), -1)}
    out["C"][lp, k] = cell[sel]
    for name, v in zip(("X", "Y", "Z_out", "GX_out", "GY_out", "Z_in", "GX_in", "GY_in"), per_seg):
        out[name] = np.zeros((n_px, M))
        out[name][lp, k] = v[sel]
    return out


def face_dw(field, gx, gy, x, y, z):
    f = np.asarray(field, np.float64).reshape(12)
    ux = f[0] * x + f[1] * y + f[2] * z + f[9]
    uy = f[3] * x + f[4] * y + f[5] * z + f[10]
    uz = f[6] * x + f[7] * y + f[8] * z + f[11]
    return uz - gx * ux - gy * uy


def chord_rates(geo, field):
    """(ddz, |dw_exit| + |dw_entry|, |kappa_exit| + |kappa_entry|) per segment for one field."""
    f = np.asarray(field, np.float64).reshape(12)
    valid = geo["C"] >= 0
    d_out = face_dw(f, geo["GX_out"], geo["GY_out"], geo["X"], geo["Y"], geo["Z_out"])
    d_in = face_dw(f, geo["GX_in"], geo["GY_in"], geo["X"], geo["Y"], geo["Z_in"])
    kap = np.abs(f[8] - geo["GX_out"] * f[2] - geo["GY_out"] * f[5]) + np.abs(f[8] - geo["GX_in"] * f[2] - geo["GY_in"] * f[5])
    return np.where(valid, d_out - d_in, 0.0), np.where(valid, np.abs(d_out) + np.abs(d_in), 0.0), np.where(valid, kap, 0.0)


def recurrence(m, D, ddz):
    """(tau_dot, I_dot, g, I_prev) per pixel / segment from ray_matrices' dict with the chords D (m["D"], or moved)."""
    a, Q, active = m["a"], m["Q"], m["active"]
    x = np.where(active, a * D, 0.0)
    E = np.exp(-x)
    S = np.where(active, -np.expm1(-x) / np.where(active, a, 1.0), 0.0)
    n_px, M = D.shape
    I, I_dot = np.zeros(n_px), np.zeros(n_px)
    g, I_prev = np.zeros_like(D), np.zeros_like(D)
    for j in range(M):
        I_prev[:, j] = I
        g[:, j] = np.where(active[:, j], E[:, j] * (Q[:, j] - a[:, j] * I), 0.0)
        I_dot = np.where(active[:, j], E[:, j] * I_dot + g[:, j] * ddz[:, j], I_dot)
        I = np.where(active[:, j], E[:, j] * I + Q[:, j] * S[:, j], I)
    tau_dot = (np.where(m["valid"], m["a_raw"], 0.0) * ddz).sum(1)
    return tau_dot, I_dot, g, I_prev


def motion_of(m, geo, field, skip=None, with_scale: bool = False):
    """(tau_dot, I_dot) [rows, res_x] fp64 for one field from ray_matrices' and face_matrices' dicts; with_scale: and a
    dict scale_tau, scale_I, sens_tau, sens_I (module docstring).  skip: bool [rows, res_x], True = solid-marked (0)."""
    assert np.array_equal(m["C"], geo["C"])
    D, a, active, E, T = m["D"], m["a"], m["active"], m["E"], m["T"]
    a_raw = np.where(m["valid"], m["a_raw"], 0.0)
    ddz, absd, kap = chord_rates(geo, field)
    tau_dot, I_dot, g, I_prev = recurrence(m, D, ddz)
    extra = None
    if with_scale:
        g_abs = np.where(active, E * (np.abs(m["Q"]) + a * np.abs(I_prev)), 0.0)
        scale_I = np.zeros(m["n_px"])
        for j in range(D.shape[1]):
            scale_I = np.where(active[:, j], E[:, j] * scale_I + g_abs[:, j] * absd[:, j], scale_I)
        Tg = np.where(active, T * np.abs(g), 0.0)
        contrib = Tg * np.abs(ddz)
        below = np.cumsum(contrib, axis=1)  # sum_{j <= k} |T_j c_j|
        ad = np.where(active, a * np.abs(ddz), 0.0)
        after = ad.sum(1, keepdims=True) - np.cumsum(ad, axis=1)  # sum_{j > k} a_j |ddz_j|
        chord = np.where(active, a * below, 0.0) + Tg * after
        extra = {"scale_tau": (np.abs(a_raw) * absd).sum(1), "scale_I": scale_I,
                 "sens_tau": (m["F"] * np.abs(a_raw) * kap).sum(1), "sens_I": (m["F"] * (chord + Tg * kap)).sum(1)}
    shape = m["shape"]
    if skip is not None:
        sk = np.asarray(skip).reshape(-1)
        tau_dot[sk] = I_dot[sk] = 0.0
        if extra:
            for v in extra.values():
                v[sk] = 0.0
    out = tau_dot.reshape(shape), I_dot.reshape(shape)
    return out + ({k: v.reshape(shape) for k, v in extra.items()},) if with_scale else out


def image_motion(xyz, cells, alpha, q, rots, res_x, res_y, bounds, fields, limit: float = 2.5, rows=None, skip=None,
                 with_scale: bool = False):
    """motion_of for every field of `fields` [K, 12]: a list of its results; the matrices are built once."""
    m = ar.ray_matrices(xyz, cells, alpha, q, rots, res_x, res_y, bounds, limit, rows)
    geo = face_matrices(xyz, cells, rots, res_x, res_y, bounds, rows)
    return [motion_of(m, geo, f, skip, with_scale) for f in np.asarray(fields, np.float64).reshape(-1, 12)]


def hull_faces(xyz, cells, rots, cell, x, y):
    """The rule the kernels find a cell's two faces by where the walk has no plane for them (a tetrahedron is convex): of
    the faces the cell lies ABOVE the one deepest at (x, y) is where the ray enters, of those it lies below the shallowest
    where it leaves; faces edge-on to the rays are never candidates.  Per (cell, x, y): (gx_in, gy_in, gx_out, gy_out)."""
    P = ar.rotate(xyz, rots)[np.asarray(cells).reshape(-1, 4)[cell]]
    opposite = (3, 2, 1, 0)
    n = len(cell)
    best_in, best_out = np.full(n, -np.inf), np.full(n, np.inf)
    out = np.zeros((4, n))
    for f, (ia, ib, ic) in enumerate(ar._FACES):
        A, B, Cc, O = P[:, ia], P[:, ib], P[:, ic], P[:, opposite[f]]
        Aa = (B[:, 0] - A[:, 0]) * (Cc[:, 2] - A[:, 2]) - (Cc[:, 0] - A[:, 0]) * (B[:, 2] - A[:, 2])
        Bb = (B[:, 1] - A[:, 1]) * (Cc[:, 2] - A[:, 2]) - (Cc[:, 1] - A[:, 1]) * (B[:, 2] - A[:, 2])
        m = (B[:, 0] - A[:, 0]) * (Cc[:, 1] - A[:, 1]) - (Cc[:, 0] - A[:, 0]) * (B[:, 1] - A[:, 1])
        with np.errstate(divide="ignore", invalid="ignore"):
            gy, gx = Aa / m, -Bb / m
            z = A[:, 2] + gx * (x - A[:, 0]) + gy * (y - A[:, 1])
            under = A[:, 2] + gx * (O[:, 0] - A[:, 0]) + gy * (O[:, 1] - A[:, 1])
        ok = np.isfinite(gx) & np.isfinite(gy) & np.isfinite(z)
        lower, upper = ok & (O[:, 2] > under), ok & (O[:, 2] < under)
        take = lower & (z > best_in)
        best_in = np.where(take, z, best_in)
        out[0], out[1] = np.where(take, gx, out[0]), np.where(take, gy, out[1])
        take = upper & (z < best_out)
        best_out = np.where(take, z, best_out)
        out[2], out[3] = np.where(take, gx, out[2]), np.where(take, gy, out[3])
    return out


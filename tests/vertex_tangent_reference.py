"""numpy restatement of the vertex tangent render (include/course5_hip.h: c5_render_vertex_tangent): the frame
differentiated along a displacement per grid point, from adjoint_reference.ray_matrices, the faces
vertex_adjoint_reference.segment_faces finds and motion_reference.recurrence.

d_xyz[v] is the velocity of point v in the coordinates of the upload; in view space u_v = M d_xyz[v], M the linear part of
the view.  A face with slopes (gx, gy) and the pixel's barycentric coordinates lambda in its projected triangle moves at
the pixel by
    dw = sum_i lambda_i (u_z - gx u_x - gy u_y)[vertex i of the face]
(motion_reference's dw for u(P) = sum lambda_i u_i; vertex_adjoint_reference's dw / d(x_i, y_i, z_i) = lambda_i (-gx, -gy,
1) read forwards), the chord by ddz_k = dw_exit,k - dw_entry,k, and tau_dot, I_dot are motion_reference.recurrence's.

SCALE: the same sums with every term replaced by its absolute value - |dw| <= sum_i |lambda_i| (|u_z| + |gx| |u_x| +
|gy| |u_y|) per face, ddz by the two faces' sum - as motion_reference forms scale_tau and scale_I.
CHORD SENSITIVITY: motion_reference's with kappa = 0 - a per-vertex dw does not depend on the depth of the point hit, so
an error of the chords enters through E_k alone: sens_tau = 0, sens_I = sum_k F_k chord_k.
"""
from __future__ import annotations

import numpy as np

from tests import adjoint_reference as ar, motion_reference as mr, vertex_adjoint_reference as vr


def chord_rates(geo, cells, u):
    """(ddz, its bound by absolute values) [pixel, k] for the view-space velocities u [n_pts, 3]."""
    cells = np.asarray(cells).reshape(-1, 4)
    valid = geo["C"] >= 0
    c = np.where(valid, geo["C"], 0)
    ddz, absd = np.zeros(c.shape), np.zeros(c.shape)
    for side, sign in (("out", 1.0), ("in", -1.0)):
        vid = np.take_along_axis(cells[c], vr.FACES[geo["F_" + side]], axis=-1)  # [px, k, 3]
        uu = u[vid]                                                               # [px, k, 3 vertices, 3]
        gx, gy, lam = geo["GX_" + side][..., None], geo["GY_" + side][..., None], geo["L_" + side]
        s = uu[..., 2] - gx * uu[..., 0] - gy * uu[..., 1]
        s_abs = np.abs(uu[..., 2]) + np.abs(gx) * np.abs(uu[..., 0]) + np.abs(gy) * np.abs(uu[..., 1])
        ddz += sign * (lam * s).sum(-1)
        absd += (np.abs(lam) * s_abs).sum(-1)
    return np.where(valid, ddz, 0.0), np.where(valid, absd, 0.0)


def tangent_of(m, geo, cells, rots, d_xyz, skip=None, with_scale: bool = False):
    """(tau_dot, I_dot) [rows, res_x] fp64 for one displacement field d_xyz [n_pts, 3] from ray_matrices' and
    segment_faces' dicts; with_scale: and a dict scale_tau, scale_I, sens_tau, sens_I (module docstring).  skip: bool
    [rows, res_x], True = solid-marked (0)."""
    assert np.array_equal(m["C"], geo["C"])
    u = np.asarray(d_xyz, np.float64).reshape(-1, 3) @ vr.view_matrix(rots).T
    ddz, absd = chord_rates(geo, cells, u)
    D, a, active, E, T = m["D"], m["a"], m["active"], m["E"], m["T"]
    a_raw = np.where(m["valid"], m["a_raw"], 0.0)
    tau_dot, I_dot, g, I_prev = mr.recurrence(m, D, ddz)
    extra = None
    if with_scale:
        g_abs = np.where(active, E * (np.abs(m["Q"]) + a * np.abs(I_prev)), 0.0)
        scale_I = np.zeros(m["n_px"])
        for j in range(D.shape[1]):
            scale_I = np.where(active[:, j], E[:, j] * scale_I + g_abs[:, j] * absd[:, j], scale_I)
        Tg = np.where(active, T * np.abs(g), 0.0)
        below = np.cumsum(Tg * np.abs(ddz), axis=1)                  # sum_{j <= k} |T_j c_j|
        ad = np.where(active, a * np.abs(ddz), 0.0)
        after = ad.sum(1, keepdims=True) - np.cumsum(ad, axis=1)     # sum_{j > k} a_j |ddz_j|
        chord = np.where(active, a * below, 0.0) + Tg * after
        extra = {"scale_tau": (np.abs(a_raw) * absd).sum(1), "scale_I": scale_I,
                 "sens_tau": np.zeros(m["n_px"]), "sens_I": (m["F"] * chord).sum(1)}
    shape = m["shape"]
    if skip is not None:
        sk = np.asarray(skip).reshape(-1)
        tau_dot[sk] = I_dot[sk] = 0.0
        if extra:
            for v in extra.values():
                v[sk] = 0.0
    out = tau_dot.reshape(shape), I_dot.reshape(shape)
    return out + ({k: v.reshape(shape) for k, v in extra.items()},) if with_scale else out


def image_tangent(xyz, cells, alpha, q, rots, res_x, res_y, bounds, fields, limit: float = 2.5, rows=None, skip=None,
                  with_scale: bool = False):
    """tangent_of for every field of `fields` [K, n_pts, 3]: a list of its results; the matrices are built once."""
    m = ar.ray_matrices(xyz, cells, alpha, q, rots, res_x, res_y, bounds, limit, rows)
    geo = vr.segment_faces(xyz, cells, rots, res_x, res_y, bounds, rows)
    n = len(np.asarray(xyz).reshape(-1, 3))
    return [tangent_of(m, geo, cells, rots, f, skip, with_scale) for f in np.asarray(fields, np.float64).reshape(-1, n, 3)]


__all__ = ["chord_rates", "tangent_of", "image_tangent"]

"""numpy restatement of the vertex Gauss-Newton product (include/course5_hip.h: c5_render_vertex_gn_product): H v = J^T W J v
as the composition the library defines it by - vertex_tangent_reference.tangent_of (J v, fp64), ONE rounding to float32
(the tangent render's image), one float32 multiply per channel by the weights (g = w * J v, the upstream image), and
vertex_adjoint_reference.gradients_of on g (J^T g, fp64).
"""
from __future__ import annotations

import numpy as np

from tests import adjoint_reference as ar, vertex_adjoint_reference as vr, vertex_tangent_reference as vt


def weighted_image(tau_dot, I_dot, weight=None) -> np.ndarray:
    """g [rows, res_x, 2] float32 = weight * float32(tau_dot, I_dot): the rounding, then one float32 multiply per channel
    (weight None: ones - the multiply by 1.0f changes no bit)."""
    t = np.stack([tau_dot, I_dot], axis=-1).astype(np.float32)
    return t if weight is None else np.asarray(weight, np.float32) * t


def product_of(m, geo, cells, n_pts, rots, d_xyz, weight=None, skip=None):
    """For one field d_xyz [n_pts, 3]: a dict jv (float32 [rows, res_x, 2]: the tangent's image), g (the weighted upstream
    image) and gradients_of's dict for g (raw: H v in the coordinates of the upload; scale_raw, sens_raw: its bounds)."""
    tau_dot, I_dot = vt.tangent_of(m, geo, cells, rots, d_xyz, skip)
    jv = weighted_image(tau_dot, I_dot)
    g = weighted_image(tau_dot, I_dot, weight)
    return {"jv": jv, "g": g, **vr.gradients_of(m, geo, cells, n_pts, rots, g, skip)}


def image_product(xyz, cells, alpha, q, rots, res_x, res_y, bounds, fields, weight=None, limit: float = 2.5, rows=None, skip=None):
    """product_of for every field of `fields` [K, n_pts, 3]: a list of its results; the matrices are built once."""
    m = ar.ray_matrices(xyz, cells, alpha, q, rots, res_x, res_y, bounds, limit, rows)
    geo = vr.segment_faces(xyz, cells, rots, res_x, res_y, bounds, rows)
    n = len(np.asarray(xyz).reshape(-1, 3))
    return [product_of(m, geo, cells, n, rots, f, weight, skip) for f in np.asarray(fields, np.float64).reshape(-1, n, 3)]


def dense_jacobian(m, geo, cells, n_pts, rots) -> np.ndarray:
    """J [rows * res_x * 2, 3 n_pts] fp64: column 3 v + c is the tangent restatement's image (tau_dot, I_dot interleaved as
    the frame's channels) for the unit field that moves point v along coordinate c."""
    J = np.zeros((m["n_px"] * 2, 3 * n_pts))
    for i in range(3 * n_pts):
        e = np.zeros(3 * n_pts)
        e[i] = 1.0
        tau_dot, I_dot = vt.tangent_of(m, geo, cells, rots, e.reshape(n_pts, 3))
        J[:, i] = np.stack([tau_dot, I_dot], axis=-1).reshape(-1)
    return J


__all__ = ["weighted_image", "product_of", "image_product", "dense_jacobian"]

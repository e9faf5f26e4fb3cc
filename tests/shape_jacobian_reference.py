"""numpy restatement of the ray shape Jacobian (include/course5_hip.h: c5_ray_shape_jacobian_fill, c5_face_gradients) from
adjoint_reference.ray_matrices, the faces of vertex_adjoint_reference.segment_faces (motion_reference.face_matrices' rule)
and vertex_adjoint_reference.chord_weights.  No GPU in here.

Per segment k of pixel p in cell c (CSR order: by pixel, deepest segment first):
    dI_ddz[k] = T_k E_k (Q_k - a_k I_{k-1})   (active segments; else 0)        = chord_weights' G for the upstream image (0, 1)
    faces[k]  = exit face | entry face << 2 | 0x30,     bary[k] = the pixel's barycentric coordinates in the two faces
and per cell and face  face_points[c][f] = cells[c][FACES[f]],  dw_dxyz[c][f] = (-gx, -gy, 1) M  (M: view_matrix).

THE BARS of one stored value (tests/derivative_fuzz.py's form, none of it fitted to what the GPU returns):
    dI_ddz:  1e-9 scale + dz_err sens + 2^-970, scale = T E (|Q| + a |I_{k-1}|) and sens = vertex_adjoint_reference's sens_G_k
             for |g_I| = 1 (its module docstring derives it: the chords in front through T_k, the segment's own through E_k,
             the ones behind through I_{k-1}), the geometry sweep's element bar of one G_k.
    bary:    the same form.  lambda_1 = n1 / m with n1 = p q - r s (p = x - ax, q = cy - ay, r = cx - ax, s = y - ay) and
             m = (bx - ax)(cy - ay) - (cx - ax)(by - ay); lambda_2 likewise; lambda_0 = 1 - lambda_1 - lambda_2.  scale: the
             sum of the terms' absolute values, (|p q| + |r s|) / |m| (lambda_0: 1 + both).  A view-space coordinate is
             known to dz_err (derivative_fuzz.dz_err: 16 ulp of the largest), a difference of two to 2 dz_err, so
             |d n1| <= 2 dz_err (|p| + |q| + |r| + |s|), |d m| <= 2 dz_err (sum of its four differences) and
             sens_1 = 2 [(|p| + |q| + |r| + |s|) + |lambda_1| (|bx - ax| + |cy - ay| + |cx - ax| + |by - ay|)] / |m|;
             sens_0 = sens_1 + sens_2.
TIES.  The restatement takes the covering face nearest in depth to the segment's end, the library the deepest face the cell
lies above (the shallowest it lies below): where a pixel lies on the edge two faces of the cell share, both have the
segment's depth there and the choice is rounding's.  A side is marked a tie where another face of the cell passes within
dz_err (F + F') of the chosen face's depth at the pixel, F = max(1, |gx| + |gy|) of either."""
from __future__ import annotations

import numpy as np

from tests import adjoint_reference as ar, vertex_adjoint_reference as vr

FACES = vr.FACES


def face_gradients(xyz, cells, rots):
    """(face_points int [n_cells, 4, 3], dw_dxyz [n_cells, 4, 3], edge_on bool [n_cells, 4]): zeros where m vanishes."""
    cells = np.asarray(cells).reshape(-1, 4)
    P = ar.rotate(xyz, rots)[cells]  # [n, 4, 3]
    M = vr.view_matrix(rots)
    dw = np.zeros((len(cells), 4, 3))
    edge_on = np.zeros((len(cells), 4), dtype=bool)
    for f, (ia, ib, ic) in enumerate(ar._FACES):
        A, B, Cc = P[:, ia], P[:, ib], P[:, ic]
        Aa = (B[:, 0] - A[:, 0]) * (Cc[:, 2] - A[:, 2]) - (Cc[:, 0] - A[:, 0]) * (B[:, 2] - A[:, 2])
        Bb = (B[:, 1] - A[:, 1]) * (Cc[:, 2] - A[:, 2]) - (Cc[:, 1] - A[:, 1]) * (B[:, 2] - A[:, 2])
        m = (B[:, 0] - A[:, 0]) * (Cc[:, 1] - A[:, 1]) - (Cc[:, 0] - A[:, 0]) * (B[:, 1] - A[:, 1])
        with np.errstate(divide="ignore", invalid="ignore"):
            gy, gx = Aa / m, -Bb / m
        ok = np.isfinite(gx) & np.isfinite(gy) & (np.abs(gx) + np.abs(gy) < 2.0 ** 40)
        edge_on[:, f] = ~ok
        vec = np.stack([-np.where(ok, gx, 0.0), -np.where(ok, gy, 0.0), np.ones(len(cells))], axis=1)
        dw[:, f] = np.where(ok[:, None], vec @ M, 0.0)
    return cells[:, FACES], dw, edge_on


def _side_bars(P, f, x, y):
    """(scale, sens) [S, 3] of the barycentric coordinates of (x, y) in face f [S] of the cells with view-space vertices P."""
    idx = np.arange(len(f))
    A, B, Cc = (P[idx, FACES[f][:, i]] for i in range(3))
    bx, by, cx, cy = B[:, 0] - A[:, 0], B[:, 1] - A[:, 1], Cc[:, 0] - A[:, 0], Cc[:, 1] - A[:, 1]
    px, py = x - A[:, 0], y - A[:, 1]
    m = np.abs(bx * cy - cx * by)
    m = np.where(m > 0, m, np.inf)
    l1, l2 = (px * cy - cx * py) / m, (bx * py - px * by) / m
    s_m = np.abs(bx) + np.abs(cy) + np.abs(cx) + np.abs(by)
    sc1 = (np.abs(px * cy) + np.abs(cx * py)) / m
    sc2 = (np.abs(bx * py) + np.abs(px * by)) / m
    se1 = 2.0 * ((np.abs(px) + np.abs(cy) + np.abs(cx) + np.abs(py)) + np.abs(l1) * s_m) / m
    se2 = 2.0 * ((np.abs(bx) + np.abs(py) + np.abs(px) + np.abs(by)) + np.abs(l2) * s_m) / m
    return np.stack([1.0 + sc1 + sc2, sc1, sc2], 1), np.stack([se1 + se2, se1, se2], 1)


def _ties(P, f, x, y, dz_err):
    """bool [S]: another face of the cell passes within dz_err (F + F') of face f's depth at the pixel."""
    n = len(f)
    zf, F = np.full((n, 4), np.inf), np.ones((n, 4))
    for k, (ia, ib, ic) in enumerate(ar._FACES):
        A, B, Cc = P[:, ia], P[:, ib], P[:, ic]
        Aa = (B[:, 0] - A[:, 0]) * (Cc[:, 2] - A[:, 2]) - (Cc[:, 0] - A[:, 0]) * (B[:, 2] - A[:, 2])
        Bb = (B[:, 1] - A[:, 1]) * (Cc[:, 2] - A[:, 2]) - (Cc[:, 1] - A[:, 1]) * (B[:, 2] - A[:, 2])
        m = (B[:, 0] - A[:, 0]) * (Cc[:, 1] - A[:, 1]) - (Cc[:, 0] - A[:, 0]) * (B[:, 1] - A[:, 1])
        with np.errstate(divide="ignore", invalid="ignore"):
            z = ((y - A[:, 1]) * Aa - (x - A[:, 0]) * Bb) / m + A[:, 2]
            s = (np.abs(Aa) + np.abs(Bb)) / np.abs(m)
        ok = np.isfinite(z) & np.isfinite(s)
        zf[:, k], F[:, k] = np.where(ok, z, np.inf), np.where(ok, np.maximum(1.0, s), 1.0)
    idx = np.arange(n)
    z0, F0 = zf[idx, f], F[idx, f]
    near = np.abs(zf - z0[:, None]) <= dz_err * (F + F0[:, None])
    near[idx, f] = False
    return near.any(1)


def arrays_of(m, geo, xyz, cells, rots, dz_err, skip=None):
    """The shape Jacobian's per-segment arrays from ray_matrices' and segment_faces' dicts, flat in CSR order, as a dict:
    row_ptr [n_px + 1], pixel, col, dz, alpha (the cell's raw alpha), dI_ddz, faces (uint8), bary [nnz, 2, 3], active, and
    the bars' terms scale_dI, sens_dI, scale_bary / sens_bary [nnz, 2, 3] and tie [nnz, 2] (module docstring).
    skip: bool per pixel, True = solid-marked: an empty row."""
    assert np.array_equal(m["C"], geo["C"])
    cells = np.asarray(cells).reshape(-1, 4)
    valid, active, a, Q, E, T, I_prev = (m[k] for k in ("valid", "active", "a", "Q", "E", "T", "I_prev"))
    if skip is not None:
        valid = valid & ~np.asarray(skip).reshape(-1)[:, None]
    ones = np.zeros((m["n_px"], 2))
    ones[:, 1] = 1.0
    G, G_abs, G_sens = vr.chord_weights(m, ones, with_sens=True)
    out = {"row_ptr": np.concatenate([[0], np.cumsum(valid.sum(1))]).astype(np.int64),
           "pixel": np.broadcast_to(np.arange(m["n_px"])[:, None], valid.shape)[valid], "col": m["C"][valid], "dz": m["D"][valid],
           "alpha": m["a_raw"][valid], "dI_ddz": G[valid], "scale_dI": G_abs[valid], "sens_dI": G_sens[valid], "active": active[valid]}
    f_out, f_in = geo["F_out"][valid], geo["F_in"][valid]
    out["faces"] = (f_out | (f_in << 2) | 0x30).astype(np.uint8)
    out["bary"] = np.stack([geo["L_out"][valid], geo["L_in"][valid]], axis=1)
    P = ar.rotate(xyz, rots)[cells[out["col"]]]
    x, y = geo["X"][valid], geo["Y"][valid]
    bars = [_side_bars(P, f, x, y) for f in (f_out, f_in)]
    out["scale_bary"] = np.stack([b[0] for b in bars], axis=1)
    out["sens_bary"] = np.stack([b[1] for b in bars], axis=1)
    out["tie"] = np.stack([_ties(P, f, x, y, dz_err) for f in (f_out, f_in)], axis=1)
    return out


def shape_arrays(xyz, cells, alpha, q, rots, res_x, res_y, bounds, dz_err, limit: float = 2.5, rows=None, skip=None):
    """arrays_of with the matrices built here, and face_gradients' two arrays under face_points / dw_dxyz."""
    m = ar.ray_matrices(xyz, cells, alpha, q, rots, res_x, res_y, bounds, limit, rows)
    geo = vr.segment_faces(xyz, cells, rots, res_x, res_y, bounds, rows)
    out = arrays_of(m, geo, xyz, cells, rots, dz_err, skip)
    out["face_points"], out["dw_dxyz"], out["edge_on"] = face_gradients(xyz, cells, rots)
    return out


def dense_jacobian(a, n_pts, values):
    """[n_px, n_pts, 3] from arrays_of's dict (with face_points / dw_dxyz): sum_k values[k] sum_{side, i} (+-bary) dw_dxyz
    scattered to the face's points; values: a["dI_ddz"] for d I / d xyz, a["alpha"] for d tau / d xyz."""
    n_px = len(a["row_ptr"]) - 1
    J = np.zeros((n_px, n_pts, 3))
    faces = a["faces"].astype(np.int64)
    for side, sign, shift, bit in ((0, 1.0, 0, 4), (1, -1.0, 2, 5)):
        f = (faces >> shift) & 3
        on = ((faces >> bit) & 1).astype(np.float64)
        pts = a["face_points"][a["col"], f]   # [nnz, 3]
        g = a["dw_dxyz"][a["col"], f]          # [nnz, 3]
        coef = sign * on * values               # [nnz]
        for i in range(3):
            np.add.at(J, (a["pixel"], pts[:, i]), (coef * a["bary"][:, side, i])[:, None] * g)
    return J


# ---- the scenes of tests/test_gpu_shape_jacobian.py (tests/test_gpu_vertex_adjoint.py's small ones at <= 28 x 21 pixels); the
# CPU test holds the restatement's share of ties on them under the GPU test's cap

SMALL_BOUNDS = (1.9, 0.1, 0.9, -0.9)
SMALL_ROTS = np.array([[0.0, 0.31, 0.0], [1.0, 0.22, 1.0]])
SCENES = ("kuhn3", "kuhn3_off_tile", "ball", "hanging_nodes", "soup", "overlap", "solid", "morton")
TIE_CAP = 0.01


def scene(kind):
    """A dict: xyz, cells, rots, rx, ry, bounds, options (set before the upload), solid (tets [n, 12] or None)."""
    from course5_amd import meshgen as mg
    rots, bounds, rx, ry, options, solid = mg.view_rotations(0.13, 0.21), mg.REFERENCE_BOUNDS, 28, 21, (), None
    if kind in ("kuhn3", "kuhn3_off_tile"):
        xyz, cells = mg.kuhn_box(3, jitter=0.2)
        rots, bounds = SMALL_ROTS, SMALL_BOUNDS
        rx, ry = (24, 16) if kind == "kuhn3" else (27, 21)
        options = (("cell_order", 0),)
    elif kind == "ball":
        xyz, cells = mg.ball(12)
    elif kind == "hanging_nodes":
        xyz, cells, _ = mg.refined_interface(3, 2, 3, jitter=0.1, warp=0.08)
    elif kind == "soup":
        xyz, cells = mg.per_cell_point_copies(*mg.kuhn_box(4, jitter=0.1))
        options = (("algorithm", 1),)
    elif kind == "overlap":
        xa, ca = mg.kuhn_box(3, lo=(0.6, -0.4, -0.3), size=0.6, jitter=0.1, seed=5)
        xb, cb = mg.kuhn_box(4, lo=(0.85, -0.2, -0.45), size=0.7, jitter=0.1, seed=6)
        xyz, cells = np.vstack([xa, xb]), np.vstack([ca, cb + len(xa)]).astype(np.int32)
    elif kind == "solid":
        xyz, cells = mg.kuhn_box(5, jitter=0.1)
        sx, sc = mg.kuhn_box(2, lo=(0.9, -0.15, 0.3), size=0.3)
        solid = sx[sc].reshape(-1, 12)
    elif kind == "morton":
        xyz, cells = mg.kuhn_box(9, jitter=0.1)  # 4 374 cells: kept in Morton order on the device ("cell_order" 1)
        options = (("cell_order", 1),)
    elif kind == "edge_on":
        # an unjittered box under no rotation: the cubes' side faces (96 of the 192) are edge-on to the rays; the pixel
        # columns and rows miss the lattice planes x, y = const, so no ray runs inside a face
        xyz, cells = mg.kuhn_box(2, lo=(0.5, -0.5, -0.5), size=1.0, jitter=0.0)
        rots, bounds = np.zeros((0, 3)), (2.0, 0.0, 1.03, -0.97)
    else:
        raise ValueError(kind)
    return dict(xyz=xyz, cells=cells, rots=rots, rx=rx, ry=ry, bounds=bounds, options=options, solid=solid)


__all__ = ["face_gradients", "arrays_of", "shape_arrays", "dense_jacobian", "scene", "SCENES", "TIE_CAP"]

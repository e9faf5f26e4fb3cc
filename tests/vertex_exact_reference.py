"""The exact vertex adjoint sums (include/course5_hip.h: "exact vertex adjoint sums", option "vertex_exact") restated over
tests/vertex_adjoint_reference.py and tests/exact_sum_reference.py: the per-segment contributions BEFORE they are summed,
their exact sums per (cell, slot) in Python integers, and the four steps that turn them into grad_xyz.

    1. a segment adds +G lambda to the three slots of its exit face and -G lambda to those of its entry face (slot =
       3 face + vertex of the face, faces in adjoint_reference._FACES' order); per (cell, slot) exponent, words, finish
    2. per cell and local vertex the triple (sum -gx_f w, sum -gy_f w, sum w) over the faces holding it, ascending f
    3. per point the triples of its (cell, vertex) incidences, ascending in the cell index
    4. grad_xyz = grad_view M

The slopes here are numpy's, the library's are face_plane's: the restatement meets the library to rounding, not to the
bit - what it pins is the format (additivity over rows, one rounding per slot) and the order of the steps."""
from __future__ import annotations

from fractions import Fraction

import numpy as np

from tests import adjoint_reference as ar
from tests import exact_sum_reference as er
from tests import vertex_adjoint_reference as vr

FACES = vr.FACES


def contributions(m, geo, weights, skip=None):
    """The six contributions of every segment as flat arrays (pixel, cell, slot, value): value = (+-G) * lambda, one fp64
    rounding, exit face first.  pixel: the local pixel of ray_matrices' layout."""
    G, _abs = vr.chord_weights(m, weights, skip)
    valid = m["valid"]
    pix = np.nonzero(valid)[0]
    c = m["C"][valid]
    out = []
    for side, sign in (("out", 1.0), ("in", -1.0)):
        f, lam = geo["F_" + side][valid], geo["L_" + side][valid]
        g = sign * G[valid]
        for k in range(3):
            out.append((pix, c, 3 * f + k, g * lam[:, k]))
    return tuple(np.concatenate([o[i] for o in out]) for i in range(4))


def per_slot(cell, slot, value, n_cells, keep=None):
    """The contributions as lists per (cell, slot): [n_cells][12] lists of floats (zeros left out: they add nothing)."""
    lists = [[[] for _ in range(12)] for _ in range(n_cells)]
    sel = np.ones(len(value), bool) if keep is None else keep
    for c, s, v in zip(cell[sel], slot[sel], value[sel]):
        if v != 0.0:
            lists[int(c)][int(s)].append(float(v))
    return lists


def exponents(lists):
    return np.array([[er.exponent_over(p) for p in row] for row in lists], np.int32)


def words(lists, exps, m):
    return np.array([[er.words(p, int(e), m) for p, e in zip(row, erow)] for row, erow in zip(lists, exps)], np.int64).reshape(len(lists), 12, 2)


def face_w(exps, sums, m):
    """Step 1's end: [n_cells, 12] fp64, one rounding per slot."""
    return np.array([[er.finish(int(e), int(s[0]), int(s[1]), m) for e, s in zip(erow, srow)] for erow, srow in zip(exps, sums)])


def exact_slot_sums(lists):
    """The slots' sums as Fractions (None: an empty slot)."""
    return [[sum((Fraction(v) for v in p), Fraction(0)) if p else None for p in row] for row in lists]


def face_slopes(xyz, cells, rots):
    """(gx, gy, edge_on) [n_cells, 4] of every cell's faces in view space (segment_faces' expressions)."""
    P = ar.rotate(np.asarray(xyz, np.float64).reshape(-1, 3), rots)[np.asarray(cells).reshape(-1, 4)]
    gx, gy = np.zeros(P.shape[:2]), np.zeros(P.shape[:2])
    edge_on = np.zeros(P.shape[:2], bool)
    for f, (ia, ib, ic) in enumerate(ar._FACES):
        A, B, Cc = P[:, ia], P[:, ib], P[:, ic]
        Aa = (B[:, 0] - A[:, 0]) * (Cc[:, 2] - A[:, 2]) - (Cc[:, 0] - A[:, 0]) * (B[:, 2] - A[:, 2])
        Bb = (B[:, 1] - A[:, 1]) * (Cc[:, 2] - A[:, 2]) - (Cc[:, 1] - A[:, 1]) * (B[:, 2] - A[:, 2])
        den = (B[:, 0] - A[:, 0]) * (Cc[:, 1] - A[:, 1]) - (Cc[:, 0] - A[:, 0]) * (B[:, 1] - A[:, 1])
        edge_on[:, f] = den == 0.0
        safe = np.where(edge_on[:, f], 1.0, den)
        gy[:, f], gx[:, f] = Aa / safe, -Bb / safe
    return gx, gy, edge_on


def cell_triples(w, gx, gy, edge_on):
    """Step 2: [n_cells, 4, 3]; separately rounded products and sums, a vertex's faces in ascending order."""
    t = np.zeros((len(w), 4, 3))
    for f in range(4):
        for k in range(3):
            wk = w[:, 3 * f + k]
            use = ~edge_on[:, f] & (wk != 0.0)
            v = FACES[f][k]
            t[:, v, 0] = np.where(use, t[:, v, 0] + (-gx[:, f]) * wk, t[:, v, 0])
            t[:, v, 1] = np.where(use, t[:, v, 1] + (-gy[:, f]) * wk, t[:, v, 1])
            t[:, v, 2] = np.where(use, t[:, v, 2] + wk, t[:, v, 2])
    return t


def point_gather(triples, cells, n_pts):
    """Step 3: [n_pts, 3], a point's incidences added in ascending order of the cell index, from +0.0."""
    gv = np.zeros((n_pts, 3))
    cells = np.asarray(cells).reshape(-1, 4)
    for c in range(len(cells)):
        for k in range(4):
            gv[cells[c, k]] = gv[cells[c, k]] + triples[c, k]
    return gv


def finish(exps, sums, xyz, cells, rots, m):
    """Steps 1 (the finish) to 4: grad_xyz [n_pts, 3] from the exponents and words."""
    n_pts = len(np.asarray(xyz).reshape(-1, 3))
    gv = point_gather(cell_triples(face_w(exps, sums, m), *face_slopes(xyz, cells, rots)), cells, n_pts)
    return gv @ vr.view_matrix(rots)


__all__ = ["contributions", "per_slot", "exponents", "words", "face_w", "exact_slot_sums", "face_slopes", "cell_triples",
           "point_gather", "finish"]

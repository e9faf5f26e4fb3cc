"""80-digit reference of the forward render (c5_render: forward) and of the derivative renders (include/course5_hip.h:
c5_render_tangent, c5_render_adjoint, c5_render_gn_product, c5_render_gn_diagonal) from per-pixel segment lists, in mpmath.

The per-segment terms are evaluated AS THE HEADER AND line.cpp:176-227 STATE THEM - no series, no threshold at
a dz = 1/8, no expm1: at 80 digits the cancellation of (1 - E) / a and of the bracket does not matter down to
alpha = DBL_EPSILON.  For the segments k = 1..n of a pixel in processing order (deepest first):
    a_k = min(alpha_k, limit), active_k = !(a_k < DBL_EPSILON), clamped_k = alpha_k > limit,
    E_k = exp(-a_k dz_k), s_k = (1 - E_k) / a_k, B_k = Q_k (dz_k E_k / a_k - (1 - E_k) / a_k^2),
    I_k = E_k I_{k-1} + Q_k s_k (active; else I_{k-1}), T_k = prod_{j > k, active} E_j, tau = sum dz_k alpha_k (raw alpha),
    dI/dQ_k = T_k s_k (active), dI/dalpha_k = T_k (B_k - dz_k E_k I_{k-1}) (active and not clamped), dtau/dalpha_k = dz_k.
The inputs (dz, alpha, Q, directions, weights) are the doubles the numpy restatements see, taken exactly.

Every result comes with its SCALE, the same sum with every contribution replaced by its absolute value
(|g_tau| dz, |g_I| T s, |g_I| T (|B| + dz E I_{k-1}); for the tangent |d_q| T s + |d_alpha| T (|B| + dz E I_{k-1})), and
its CHORD SENSITIVITY sum_k F_k |contribution_k| / dz_k (F: tests/adjoint_reference.py): what a rounding error and an
error of the chords can do to it.
Results are returned rounded to fp64 (one rounding of the exact sum).

THE GEOMETRY (GeometryRays and what follows it): the renders that differentiate in the grid's points (c5_render_motion_tangent,
c5_render_vertex_tangent, c5_render_vertex_adjoint), from the view-space vertices and the pixel's coordinates - the doubles
the restatements see, taken exactly - with nothing of the restatements' arithmetic: per face the slopes gy = A / m,
gx = -B / m (line.cpp:158-171), the depth at the pixel and the barycentrics e1 / m, e2 / m, e0 / m at 80 digits; the chord
is the difference of the two depths AT 80 DIGITS (not the double the segment lists carry: a restatement is held to this
within its bar with the dz_err term, which is what that term is for); ddz for an affine field (motion_reference's dw at
P = (x, y, z_face)) and for per-point velocities (dw = sum_i lambda_i (u_z - gx u_x - gy u_y)[vertex i]); the recurrence
tau_dot = sum alpha_k ddz_k, I_dot_k = E_k I_dot_{k-1} + E_k (Q_k - a_k I_{k-1}) ddz_k; and G_k = g_tau alpha_k + g_I T_k E_k
(Q_k - a_k I_{k-1}) scattered to the points as +-G_k lambda_v (-gx, -gy, 1), then M^T.  Which two faces of its cell a segment
runs between is taken from the restatement (their indices) and CHECKED here: both cover the pixel and the exit is the
deeper of the two.
"""
from __future__ import annotations

import numpy as np
from mpmath import mp, mpf

DPS = 80
EPS = float(np.finfo(np.float64).eps)


class Segments:
    """The terms of every segment of the chosen pixels.  pix / cell / dz: adjoint_reference.segment_lists' arrays
    (sorted by pixel, then in processing order); pixels: the pixels wanted (default: every pixel with a segment); slope:
    segment_lists(with_slope=True)'s fifth array (default: flat faces, F = 1)."""

    def __init__(self, pix, cell, dz, alpha, q, limit: float, pixels=None, slope=None):
        mp.dps = DPS
        pix, cell, dz = np.asarray(pix), np.asarray(cell), np.asarray(dz, np.float64)
        self.pixels = np.unique(pix) if pixels is None else np.asarray(pixels)
        # per pixel, per segment in processing order: dicts of mpf (c cell, d dz, F, a, Q, E, s, B, I_prev, T, moves; and the
        # derived dI_dq, dI_da, abs_da)
        self.rays = []
        lo = np.searchsorted(pix, self.pixels, side="left")
        hi = np.searchsorted(pix, self.pixels, side="right")
        zero, one = mpf(0), mpf(1)
        self.n_segments = int((hi - lo).sum())
        for b, e in zip(lo, hi):
            ray = []
            I = zero
            for k in range(b, e):
                c = int(cell[k])
                a_raw = float(alpha[c])
                a = min(a_raw, limit)
                t = dict(c=c, d=mpf(float(dz[k])), a_raw=mpf(a_raw), Q=mpf(float(q[c])), active=not a < EPS, moves=False, a=zero, E=one, s=zero,
                         B=zero, I_prev=I, F=mpf(1.0 if slope is None else max(1.0, float(slope[k]))))
                if t["active"]:
                    d, Q, am = t["d"], t["Q"], mpf(a)
                    E = mp.exp(-am * d)
                    s = (one - E) / am
                    t.update(a=am, E=E, s=s, B=Q * (d * E / am - (one - E) / (am * am)), moves=not a_raw > limit)
                    I = E * I + Q * s
                ray.append(t)
            T = one
            for t in reversed(ray):
                d, E, I_prev = t["d"], t["E"], t["I_prev"]
                t.update(T=T, dI_dq=T * t["s"], dI_da=zero, abs_da=zero)
                if t["moves"]:
                    t["dI_da"] = T * (t["B"] - d * E * I_prev)
                    t["abs_da"] = T * (abs(t["B"]) + d * E * abs(I_prev))
                T = T * E
            self.rays.append(ray)


def forward(seg: Segments):
    """The forward render per pixel of seg.pixels: (tau, I, scale_tau, scale_I, sens_tau, sens_I, cancel), fp64 arrays -
    tau = sum dz_k alpha_k (raw alpha), I the recurrence's last value, and the bounds adjoint_reference.forward_of states:
    the absolute sums, the chord sensitivities sum F_k |alpha_k| and sum F_k T_k E_k |Q_k - a_k I_{k-1}|, and the rounding of
    the reference's own step, 8 x 2^-53 sum T_k (|Q_k| + a_k |I_{k-1}|) / a_k."""
    out = np.zeros((7, len(seg.pixels)))
    c8 = mpf(8) * mpf(2) ** -53
    for i, ray in enumerate(seg.rays):
        tau = scale_tau = sens_tau = scale_I = sens_I = cancel = I = mpf(0)
        for t in ray:
            tau += t["d"] * t["a_raw"]
            scale_tau += t["d"] * abs(t["a_raw"])
            sens_tau += t["F"] * abs(t["a_raw"])
            if not t["active"]:
                continue
            a, Q, E, I_prev, T = t["a"], t["Q"], t["E"], t["I_prev"], t["T"]
            I = E * I_prev + Q * t["s"]
            scale_I += T * abs(Q) * t["s"]
            sens_I += t["F"] * T * E * abs(Q - a * I_prev)
            cancel += c8 * T * (abs(Q) + a * abs(I_prev)) / a
        out[:, i] = [float(v) for v in (tau, I, scale_tau, scale_I, sens_tau, sens_I, cancel)]
    return out


def tangent(seg: Segments, d_alpha, d_q):
    """Per pixel of seg.pixels: (tau_dot, I_dot, scale_tau, scale_I, sens_tau, sens_I), fp64 arrays.  None: zero."""
    out = np.zeros((6, len(seg.pixels)))
    for i, ray in enumerate(seg.rays):
        tau_dot = I_dot = scale_tau = scale_I = sens_tau = sens_I = mpf(0)
        for t in ray:
            c, d = t["c"], t["d"]
            da = mpf(0) if d_alpha is None else mpf(float(d_alpha[c]))
            dq = mpf(0) if d_q is None else mpf(float(d_q[c]))
            tau_dot += d * da
            scale_tau += d * abs(da)
            sens_tau += t["F"] * abs(da)
            if not t["active"]:
                continue
            if not t["moves"]:
                da = mpf(0)
            E, I_prev = t["E"], t["I_prev"]
            src = dq * t["s"] + da * (t["B"] - d * E * I_prev)
            sens_I += t["F"] * abs(t["T"] * src) / d
            I_dot = E * I_dot + src
            scale_I = E * scale_I + abs(dq) * t["s"] + abs(da) * (abs(t["B"]) + d * E * abs(I_prev))
        out[:, i] = [float(v) for v in (tau_dot, I_dot, scale_tau, scale_I, sens_tau, sens_I)]
    return out


def _per_cell(seg: Segments, n_cells: int, weights, contributions):
    """Sums contributions(g_tau, g_I, t) -> 6 mpf (alpha, q, their scales, their sensitivities) per cell over the segments
    t of seg's pixels; weights [len(pixels), 2] doubles."""
    acc = {}
    for ray, (g_tau, g_I) in zip(seg.rays, weights):
        g_tau, g_I = mpf(float(g_tau)), mpf(float(g_I))
        for t in ray:
            v = contributions(g_tau, g_I, t)
            a = acc.get(t["c"])
            if a is None:
                acc[t["c"]] = list(v)
            else:
                for j in range(6):
                    a[j] += v[j]
    out = np.zeros((6, n_cells))
    for c, a in acc.items():
        out[:, c] = [float(v) for v in a]
    return dict(zip(("alpha", "q", "scale_alpha", "scale_q", "sens_alpha", "sens_q"), out))


def adjoint(seg: Segments, n_cells: int, weights):
    """grad_alpha / grad_q per cell with scales and sensitivities, for the upstream weights (g_tau, g_I) of seg.pixels."""
    def terms(g_tau, g_I, t):
        return (g_tau * t["d"] + g_I * t["dI_da"], g_I * t["dI_dq"], abs(g_tau) * t["d"] + abs(g_I) * t["abs_da"],
                abs(g_I) * t["dI_dq"], t["F"] * (abs(g_tau * t["d"]) + abs(g_I * t["dI_da"])) / t["d"],
                t["F"] * abs(g_I * t["dI_dq"]) / t["d"])
    return _per_cell(seg, n_cells, weights, terms)


def gn_diagonal(seg: Segments, n_cells: int, weights):
    """diag(J^T W J) per cell with scales and sensitivities; weights (w_tau, w_I) >= 0 of seg.pixels."""
    def terms(w_tau, w_I, t):
        d = t["d"]
        ca, cq = w_tau * d * d + w_I * t["dI_da"] ** 2, w_I * t["dI_dq"] ** 2
        return (ca, cq, abs(w_tau) * d * d + abs(w_I) * t["abs_da"] ** 2, abs(cq), 2 * t["F"] * abs(ca) / d, 2 * t["F"] * abs(cq) / d)
    return _per_cell(seg, n_cells, weights, terms)


def gn_product(seg: Segments, n_cells: int, d_alpha, d_q, weights=None):
    """J^T W (J v) with the header's fp32 intermediate: J v rounded to fp32, one fp32 multiply by the fp32 weight (None:
    none), J^T of that exactly.  Returns (adjoint()'s dict for that upstream image, jv fp32 [len(pixels), 2])."""
    t = tangent(seg, d_alpha, d_q)
    jv32 = np.stack([t[0], t[1]], axis=1).astype(np.float32)
    g32 = jv32 if weights is None else (np.asarray(weights, np.float32) * jv32).astype(np.float32)
    return adjoint(seg, n_cells, g32.astype(np.float64)), jv32


# ---- the geometry ------------------------------------------------------------------------------------------------------

_FACES = ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3))  # plane.cpp:30-37


def _face(P, x, y):
    """(gx, gy, z at the pixel, the three barycentrics, covers) of the face with view-space vertices P [3][3] (mpf)."""
    A, B, C = P
    Aa = (B[0] - A[0]) * (C[2] - A[2]) - (C[0] - A[0]) * (B[2] - A[2])
    Bb = (B[1] - A[1]) * (C[2] - A[2]) - (C[1] - A[1]) * (B[2] - A[2])
    m = (B[0] - A[0]) * (C[1] - A[1]) - (C[0] - A[0]) * (B[1] - A[1])
    e0 = (B[0] - A[0]) * (y - A[1]) - (B[1] - A[1]) * (x - A[0])
    e1 = (C[0] - B[0]) * (y - B[1]) - (C[1] - B[1]) * (x - B[0])
    e2 = (A[0] - C[0]) * (y - C[1]) - (A[1] - C[1]) * (x - C[0])
    covers = (e0 >= 0 and e1 >= 0 and e2 >= 0) or (e0 <= 0 and e1 <= 0 and e2 <= 0)
    gy, gx = Aa / m, -Bb / m
    return dict(gx=gx, gy=gy, z=A[2] + gx * (x - A[0]) + gy * (y - A[1]), lam=(e1 / m, e2 / m, e0 / m), covers=covers)


class GeometryRays:
    """The segments of the chosen pixels with their two faces and their optics at 80 digits (module docstring: the
    geometry).  view [n_pts, 3]: the view-space points; C, X, Y, F_out, F_in: vertex_adjoint_reference.segment_faces'
    [pixel, k] matrices; pixels: the rows of those matrices wanted."""

    def __init__(self, view, cells, geo, alpha, q, limit: float, pixels):
        mp.dps = DPS
        cells = np.asarray(cells).reshape(-1, 4)
        self.pixels = np.asarray(pixels)
        self.rays, self.n_segments, self.steepest = [], 0, 0.0
        zero, one = mpf(0), mpf(1)
        pts = {}

        def point(v):
            if v not in pts:
                pts[v] = tuple(mpf(float(c)) for c in view[v])
            return pts[v]

        for p in self.pixels:
            ray, I = [], zero
            for k in range(geo["C"].shape[1]):
                c = int(geo["C"][p, k])
                if c < 0:
                    break
                x, y = mpf(float(geo["X"][p, k])), mpf(float(geo["Y"][p, k]))
                t = dict(c=c, x=x, y=y)
                for side in ("out", "in"):
                    vid = [int(cells[c][i]) for i in _FACES[int(geo["F_" + side][p, k])]]
                    f = _face([point(v) for v in vid], x, y)
                    assert f["covers"], (int(p), k, side)
                    f["vid"] = vid
                    t[side] = f
                    self.steepest = max(self.steepest, float(abs(f["gx"]) + abs(f["gy"])))
                d = t["out"]["z"] - t["in"]["z"]
                assert d > 0, (int(p), k)
                a_raw = float(alpha[c])
                a = min(a_raw, limit)
                t.update(d=d, a_raw=mpf(a_raw), Q=mpf(float(q[c])), active=not a < EPS, a=zero, E=one, I_prev=I)
                if t["active"]:
                    am = mpf(a)
                    E = mp.exp(-am * d)
                    t.update(a=am, E=E)
                    I = E * I + t["Q"] * (one - E) / am
                ray.append(t)
            T = one
            for t in reversed(ray):
                t["T"] = T
                T = T * t["E"]
            self.rays.append(ray)
            self.n_segments += len(ray)


def _recurrence(ray, ddz):
    """(tau_dot, I_dot) of one ray for the chord rates ddz (one per segment, processing order)."""
    tau_dot = I_dot = mpf(0)
    for t, r in zip(ray, ddz):
        tau_dot += t["a_raw"] * r
        if t["active"]:
            I_dot = t["E"] * I_dot + t["E"] * (t["Q"] - t["a"] * t["I_prev"]) * r
    return tau_dot, I_dot


def motion_tangent(rays: GeometryRays, field):
    """(tau_dot, I_dot) fp64 [len(pixels)] each for the affine field [12] (A row-major, then b)."""
    f = [mpf(float(v)) for v in np.asarray(field, np.float64).reshape(12)]

    def dw(t, face):
        x, y, z = t["x"], t["y"], face["z"]
        ux, uy, uz = (f[3 * r] * x + f[3 * r + 1] * y + f[3 * r + 2] * z + f[9 + r] for r in range(3))
        return uz - face["gx"] * ux - face["gy"] * uy

    out = [_recurrence(ray, [dw(t, t["out"]) - dw(t, t["in"]) for t in ray]) for ray in rays.rays]
    return np.array([[float(a), float(b)] for a, b in out]).reshape(-1, 2).T


def vertex_tangent(rays: GeometryRays, d_xyz, M):
    """(tau_dot, I_dot) fp64 [len(pixels)] each for the displacement field d_xyz [n_pts, 3]; M: the view's linear part."""
    d_xyz = np.asarray(d_xyz, np.float64)
    Mm = [[mpf(float(v)) for v in row] for row in np.asarray(M, np.float64)]
    vel = {}

    def u(v):
        if v not in vel:
            d = [mpf(float(c)) for c in d_xyz[v]]
            vel[v] = tuple(Mm[r][0] * d[0] + Mm[r][1] * d[1] + Mm[r][2] * d[2] for r in range(3))
        return vel[v]

    def dw(face):
        return sum((lam * (u(v)[2] - face["gx"] * u(v)[0] - face["gy"] * u(v)[1]) for lam, v in zip(face["lam"], face["vid"])), mpf(0))

    out = [_recurrence(ray, [dw(t["out"]) - dw(t["in"]) for t in ray]) for ray in rays.rays]
    return np.array([[float(a), float(b)] for a, b in out]).reshape(-1, 2).T


def vertex_adjoint(rays: GeometryRays, weights, n_pts: int, M):
    """grad_xyz fp64 [n_pts, 3] in the coordinates of the upload for the upstream weights (g_tau, g_I) of rays.pixels."""
    acc = {}
    for ray, (g_tau, g_I) in zip(rays.rays, weights):
        g_tau, g_I = mpf(float(g_tau)), mpf(float(g_I))
        for t in ray:
            G = g_tau * t["a_raw"]
            if t["active"]:
                G += g_I * t["T"] * t["E"] * (t["Q"] - t["a"] * t["I_prev"])
            for side, sign in (("out", 1), ("in", -1)):
                face = t[side]
                vec = (-face["gx"], -face["gy"], mpf(1))
                for lam, v in zip(face["lam"], face["vid"]):
                    a = acc.setdefault(v, [mpf(0), mpf(0), mpf(0)])
                    for k in range(3):
                        a[k] += sign * G * lam * vec[k]
    Mm = [[mpf(float(v)) for v in row] for row in np.asarray(M, np.float64)]
    out = np.zeros((n_pts, 3))
    for v, a in acc.items():  # grad_xyz = M^T grad_view
        out[v] = [float(sum(Mm[r][k] * a[r] for r in range(3))) for k in range(3)]
    return out

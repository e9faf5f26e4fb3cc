"""numpy restatement of the adjoint render (include/course5_hip.h: c5_render_adjoint) from per-pixel segment lists.

A pixel's segments come as rows {tet, z_hi, dz} in the reference's order: sorted by descending z_hi (line.cpp:138, what
the port oracle's probes return), the recurrence run from the last row to the first (line.cpp:206), so the first row is
the segment nearest the viewer.  Number them k = 1..n in processing order (row n - k):
    a_k = min(alpha_k, limit), active_k = !(a_k < DBL_EPSILON), E_k = exp(-a_k dz_k),
    I_k = E_k I_{k-1} + Q_k (1 - E_k) / a_k (active), tau = sum dz_k alpha_k, T_k = prod_{j > k} E_j
    dtau/dalpha_k = dz_k, dI/dQ_k = T_k (1 - E_k) / a_k, dI/dalpha_k = T_k [Q_k (dz_k E_k / a_k - (1 - E_k) / a_k^2) - dz_k E_k I_{k-1}]
(dI/d. = 0 for an inactive segment, dI/dalpha = 0 for a clamped one).

SCALE and CHORD SENSITIVITY.  Beside a result the restatements can return two bounds per element (with_scale).  Its scale:
the same sum with every contribution replaced by its absolute value (|g_tau| dz, |g_I| T s, |g_I| T (|B| + dz E I_{k-1})):
what rounding can do to it.  Its chord sensitivity, sum_k F_k |contribution_k| / dz_k: what an error of the chords can do
(a contribution is close to proportional to its chord).  F_k = max(1, |gx| + |gy|) over the two faces the chord runs
between, z = c + gx x + gy y: the depth of a face almost parallel to the rays is known that much worse than its
coordinates, to whoever evaluates it (segment_lists(with_slope=True)).

Whole images take their segment lists from segment_lists, the reference's binning and pairing restated in numpy: the port
oracle's probes give the same lists (tests/test_adjoint_cpu.py checks them pixel by pixel) but re-bin the grid once per
probed pixel, too slow for every pixel of an image.
"""
from __future__ import annotations

import math

import numpy as np

EPS = np.finfo(np.float64).eps


def _bracket_over_q_dz2(x: float) -> float:
    """(x e^-x - (1 - e^-x)) / x^2 by its series (-1/2 + x/3 - x^2/8 + ...) for small x, as written otherwise."""
    if x < 0.125:
        return sum((-1.0) ** (m + 1) * (m + 1) / math.factorial(m + 2) * x ** m for m in range(14))
    return (x * math.exp(-x) + math.expm1(-x)) / (x * x)


def forward(segs, alpha, q, limit: float = 2.5) -> tuple[float, float]:
    """(tau, I) of one pixel in fp64 (the rearranged recurrence, for finite differences)."""
    tau, I = 0.0, 0.0
    for tet, _z, dz in segs:
        tau += dz * alpha[int(tet)]
    for tet, _z, dz in segs[::-1]:
        c = int(tet)
        a = min(alpha[c], limit)
        if a < EPS:
            continue
        I = math.exp(-a * dz) * I + q[c] * (-math.expm1(-a * dz)) / a
    return tau, I


def pixel_terms(segs, alpha, q, limit: float = 2.5):
    """Per segment (in the rows' order): (cell, dtau/dalpha, dI/dalpha, dI/dQ)."""
    n = len(segs)
    out = [None] * n
    a_eff = [min(alpha[int(s[0])], limit) for s in segs]
    active = [not (a < EPS) for a in a_eff]
    # T of row i = prod over the rows before it (nearer the viewer) of E
    T = np.ones(n)
    for i in range(1, n):
        T[i] = T[i - 1] * (math.exp(-a_eff[i - 1] * segs[i - 1][2]) if active[i - 1] else 1.0)
    I = 0.0
    for i in range(n - 1, -1, -1):
        c, dz = int(segs[i][0]), float(segs[i][2])
        a, Q = a_eff[i], q[c]
        dI_da = dI_dq = 0.0
        if active[i]:
            E = math.exp(-a * dz)
            s = -math.expm1(-a * dz) / a
            dI_dq = T[i] * s
            if not alpha[c] > limit:
                dI_da = T[i] * (Q * dz * dz * _bracket_over_q_dz2(a * dz) - dz * E * I)
            I = E * I + Q * s
        out[i] = (c, dz, dI_da, dI_dq)
    return out


def gradients(probes, weights, alpha, q, n_cells: int, limit: float = 2.5):
    """grad_alpha, grad_q [n_cells] from segment lists `probes` (one per pixel) and the pixels' weights (g_tau, g_I)."""
    ga = np.zeros(n_cells)
    gq = np.zeros(n_cells)
    for segs, (g_tau, g_I) in zip(probes, weights):
        if len(segs) == 0 or (g_tau == 0.0 and g_I == 0.0):
            continue
        for c, dtau, dI_da, dI_dq in pixel_terms(segs, alpha, q, limit):
            ga[c] += g_tau * dtau + g_I * dI_da
            gq[c] += g_I * dI_dq
    return ga, gq


def rotate(xyz, rots):
    """The view transform (tetra.cpp:44-62, applied in order; angles in radians as c5_set_view takes them)."""
    p = np.array(xyz, dtype=np.float64).reshape(-1, 3)
    for axis, angle, x0 in np.asarray(rots, dtype=np.float64).reshape(-1, 3):
        co, si = math.cos(angle), math.sin(angle)
        if int(axis) == 0:
            y, z = p[:, 1].copy(), p[:, 2].copy()
            p[:, 1], p[:, 2] = y * co - z * si, y * si + z * co
        else:
            x, z = p[:, 0] - x0, p[:, 2].copy()
            p[:, 0], p[:, 2] = x * co - z * si + x0, x * si + z * co
    return p


_FACES = ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3))  # plane.cpp:30-37


def pixel_coordinates(bounds, res_x, res_y, running: bool = True):
    """(X [res_x], Y [res_y], step_x, step_y): the pixel centres as the reference and the library form them, RUNNING SUMS
    x_{i+1} = x_i + step (plane.cpp:301-314; csrc/context.hip: c5_set_image), not x_min + i step: after a few hundred
    additions the two differ by tens of ulps, which a face of slope F turns into F times that in its depth.  The geometry
    sweep (tests/derivative_fuzz.py) found the restatements on x_min + i step: images of 300 - 500 pixels a side had up to
    1.5 x the chord bar between the library's chords and segment_lists', every one of them the pixel's coordinate.
    running=False gives those older coordinates (derivative_fuzz.derivative_scene draws its alpha from them still, so
    that the scenes of a seed stay what they were)."""
    b = np.asarray(bounds, dtype=np.float64)
    sx, sy = (b[0] - b[1]) / (res_x - 1.0), (b[2] - b[3]) / (res_y - 1.0)
    if not running:
        return b[1] + sx * np.arange(res_x), b[3] + sy * np.arange(res_y), sx, sy
    X = np.add.accumulate(np.concatenate([[b[1]], np.full(res_x - 1, sx)]))  # (accumulate adds in order)
    Y = np.add.accumulate(np.concatenate([[b[3]], np.full(res_y - 1, sy)]))
    return X, Y, sx, sy


def segment_lists(xyz, cells, rots, res_x, res_y, bounds, with_slope: bool = False, running: bool = True):
    """Every pixel's segments, as the reference bins and pairs them (plane.cpp:184-192, line.cpp:99-138): a cell whose
    projection holds the pixel centre (two covering faces; four: two pairs in face order) gives {cell, z_hi, dz}.
    Returns (pixel, cell, z_hi, dz) arrays sorted by pixel and then by ASCENDING z_hi - the order the recurrence runs
    in (line.cpp:206); pixel = row * res_x + col over the full image.  with_slope: a fifth array, the larger |dz/dx| + |dz/dy|
    of the segment's two faces.  running: pixel_coordinates'."""
    P = rotate(xyz, rots)[np.asarray(cells).reshape(-1, 4)]  # [C, 4, 3]
    b = np.asarray(bounds, dtype=np.float64)
    X, Y, sx, sy = pixel_coordinates(b, res_x, res_y, running)
    lo, hi = P[:, :, :2].min(1), P[:, :, :2].max(1)
    c0 = np.clip(np.floor((lo[:, 0] - b[1]) / sx) - 1, 0, res_x - 1).astype(np.int64)
    c1 = np.clip(np.ceil((hi[:, 0] - b[1]) / sx) + 1, 0, res_x - 1).astype(np.int64)
    r0 = np.clip(np.floor((lo[:, 1] - b[3]) / sy) - 1, 0, res_y - 1).astype(np.int64)
    r1 = np.clip(np.ceil((hi[:, 1] - b[3]) / sy) + 1, 0, res_y - 1).astype(np.int64)
    nx, ny = c1 - c0 + 1, r1 - r0 + 1
    cnt = nx * ny
    cid = np.repeat(np.arange(len(P)), cnt)
    local = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    ii = c0[cid] + local % nx[cid]
    jj = r0[cid] + local // nx[cid]
    x, y = X[ii], Y[jj]
    cover = np.zeros((len(cid), 4), dtype=bool)
    zf = np.zeros((len(cid), 4))
    sf = np.zeros((len(cid), 4))
    for f, (ia, ib, ic) in enumerate(_FACES):
        A, B, Cc = P[cid, ia], P[cid, ib], P[cid, ic]
        e0 = (B[:, 0] - A[:, 0]) * (y - A[:, 1]) - (B[:, 1] - A[:, 1]) * (x - A[:, 0])
        e1 = (Cc[:, 0] - B[:, 0]) * (y - B[:, 1]) - (Cc[:, 1] - B[:, 1]) * (x - B[:, 0])
        e2 = (A[:, 0] - Cc[:, 0]) * (y - Cc[:, 1]) - (A[:, 1] - Cc[:, 1]) * (x - Cc[:, 0])
        cover[:, f] = ((e0 >= 0) & (e1 >= 0) & (e2 >= 0)) | ((e0 <= 0) & (e1 <= 0) & (e2 <= 0))
        # line.cpp:158-171
        Aa = (B[:, 0] - A[:, 0]) * (Cc[:, 2] - A[:, 2]) - (Cc[:, 0] - A[:, 0]) * (B[:, 2] - A[:, 2])
        Bb = (B[:, 1] - A[:, 1]) * (Cc[:, 2] - A[:, 2]) - (Cc[:, 1] - A[:, 1]) * (B[:, 2] - A[:, 2])
        m = (B[:, 0] - A[:, 0]) * (Cc[:, 1] - A[:, 1]) - (Cc[:, 0] - A[:, 0]) * (B[:, 1] - A[:, 1])
        with np.errstate(divide="ignore", invalid="ignore"):
            zf[:, f] = ((y - A[:, 1]) * Aa - (x - A[:, 0]) * Bb) / m + A[:, 2]
            sf[:, f] = (np.abs(Aa) + np.abs(Bb)) / np.abs(m)
    n_cov = cover.sum(1)
    out = []
    for want in (2, 4):
        sel = n_cov == want
        order = np.argsort(~cover[sel], axis=1, kind="stable")  # covering faces first, in face order
        z = np.take_along_axis(zf[sel], order, axis=1)
        sl = np.take_along_axis(sf[sel], order, axis=1)
        for k in range(want // 2):
            za, zb = z[:, 2 * k], z[:, 2 * k + 1]
            zh = np.maximum(za, zb)
            out.append((jj[sel] * res_x + ii[sel], cid[sel], zh, zh - np.minimum(za, zb), np.maximum(sl[:, 2 * k], sl[:, 2 * k + 1])))
    pix, cell, zh, dz, slope = (np.concatenate([o[k] for o in out]) for k in range(5))
    keep = dz > 0
    pix, cell, zh, dz, slope = pix[keep], cell[keep], zh[keep], dz[keep], slope[keep]
    o = np.lexsort((zh, pix))
    return (pix[o], cell[o], zh[o], dz[o], slope[o]) if with_slope else (pix[o], cell[o], zh[o], dz[o])


def _transmittance(a, D):
    """T_k = exp(-sum_{j > k} a_j dz_j) over [pixel, k] matrices, the sum taken from the viewer's end (k = M - 1) in
    double-double: exp turns an error of its argument u into a relative error of that size, and u is not small where it
    matters (a cell seen through an optical depth of 500 has all its terms at e^-500: 2^-53 u from the rounding of the
    products a dz alone would be 500 x 2^-53 of that cell's gradient).  As Lambda - Lambda_k it would carry Lambda's
    rounding into the segments near the viewer as well."""
    def split(v):
        c = 134217729.0 * v
        hi = c - (c - v)
        return hi, v - hi

    p = a * D
    ah, al = split(a)
    dh, dl = split(D)
    e = ((ah * dh - p) + ah * dl + al * dh) + al * dl  # a dz = p + e exactly (Dekker)
    hi = np.zeros(len(a))
    lo = np.zeros(len(a))
    T = np.ones_like(D)
    for k in range(D.shape[1] - 1, -1, -1):
        T[:, k] = np.exp(-hi) * np.exp(-lo)
        s = hi + p[:, k]
        b = s - hi
        lo = lo + ((hi - (s - b)) + (p[:, k] - b)) + e[:, k]
        hi = s + lo
        lo = lo - (hi - s)
    return T


def ray_matrices(xyz, cells, alpha, q, rots, res_x, res_y, bounds, limit: float = 2.5, rows=None):
    """The per-segment quantities of the rays of the global rows `rows` (default: all) as [pixel, k] matrices, k the
    processing order (deepest first), pixel = local row * res_x + col.  A dict: C cell (-1: no segment), D dz, valid,
    a_raw, Q, active, clamped, E, S = (1 - E) / a, B = Q (dz E / a - (1 - E) / a^2) (by its series below a dz = 1/8),
    T, I_prev, F (module docstring), abs_da, sens_a, sens_q, and per pixel I and tau.  What image_gradients, tangent_reference.image_tangent and
    gn_reference.segment_terms are built from."""
    rows = np.arange(res_y) if rows is None else np.asarray(rows)
    alpha, q = np.asarray(alpha, np.float64), np.asarray(q, np.float64)
    pix, cell, _zh, dz, slope = segment_lists(xyz, cells, rots, res_x, res_y, bounds, with_slope=True)
    row_slot = np.full(res_y, -1)
    row_slot[rows] = np.arange(len(rows))
    lp = row_slot[pix // res_x] * res_x + pix % res_x
    sel = row_slot[pix // res_x] >= 0
    lp, cell, dz, slope = lp[sel], cell[sel], dz[sel], slope[sel]
    n_px = len(rows) * res_x
    starts = np.searchsorted(lp, np.arange(n_px))
    k = np.arange(len(lp)) - starts[lp]
    M = int(k.max()) + 1 if len(k) else 1
    C = np.full((n_px, M), -1)
    D = np.zeros((n_px, M))
    F = np.ones((n_px, M))
    C[lp, k], D[lp, k], F[lp, k] = cell, dz, np.maximum(1.0, slope)
    return matrices_of(C, D, F, alpha, q, limit, (len(rows), res_x))


def matrices_of(C, D, F, alpha, q, limit, shape):
    """ray_matrices' dict from C, D, F [pixel, k] (a row's segments deepest first, C = -1 where it has none) and the scalars
    alpha, q that C indexes: everything after the geometry.  ray_matrices indexes cells; tests/slab_reference.py the layers
    of a layered medium."""
    alpha, q = np.asarray(alpha, np.float64), np.asarray(q, np.float64)
    n_px = len(C)
    M = C.shape[1]
    valid = C >= 0
    a_raw = np.where(valid, alpha[np.maximum(C, 0)], 0.0)
    Q = np.where(valid, q[np.maximum(C, 0)], 0.0)
    a = np.minimum(a_raw, limit)
    active = valid & ~(a < EPS)
    x = np.where(active, a * D, 0.0)
    E = np.exp(-x)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        S = np.where(active, -np.expm1(-x) / np.where(active, a, 1.0), 0.0)
        ser = sum((-1.0) ** (m + 1) * (m + 1) / math.factorial(m + 2) * x ** m for m in range(14))
        direct = (x * E + np.expm1(-x)) / np.where(x > 0, x * x, 1.0)
    B = Q * D * D * np.where(x < 0.125, ser, direct)
    T = _transmittance(np.where(active, a, 0.0), D)
    a_eff = np.where(active, a, 0.0)
    I_prev = np.zeros_like(D)
    I = np.zeros(n_px)
    for j in range(M):
        I_prev[:, j] = I
        I = np.where(active[:, j], E[:, j] * I + Q[:, j] * S[:, j], I)
    tau = (np.where(valid, D * a_raw, 0.0)).sum(1)
    moves = active & ~(a_raw > limit)
    abs_da = np.where(moves, T * (np.abs(B) + D * E * np.abs(I_prev)), 0.0)
    # chord sensitivities of a segment's dI/dQ and dI/dalpha (module docstring): F |term| / dz
    F_dz = np.where(valid, F / np.where(valid, D, 1.0), 0.0)
    sens_q = np.where(active, T * S, 0.0) * F_dz
    sens_a = np.where(moves, np.abs(T * (B - D * E * I_prev)), 0.0) * F_dz
    return dict(C=C, D=D, F=F, F_dz=F_dz, valid=valid, a_raw=a_raw, a=a_eff, Q=Q, active=active, clamped=a_raw > limit, E=E, S=S,
                B=B, T=T, I_prev=I_prev, I=I, tau=tau, abs_da=abs_da, sens_a=sens_a, sens_q=sens_q, n_px=n_px,
                shape=tuple(shape))


def image_gradients(xyz, cells, alpha, q, rots, res_x, res_y, bounds, weights, limit: float = 2.5, rows=None, skip=None,
                    with_scale: bool = False):
    """The helper over whole images, vectorised over the pixels.  weights: [len(rows), res_x, 2] (g_tau, g_I) of the
    global rows `rows` (default: all); skip: optional bool [len(rows), res_x], True = the pixel contributes nothing
    (solid).  Returns (grad_alpha, grad_q, tau, I) with tau / I the fp64 images of those rows; with_scale: and
    gradients_of's dict."""
    m = ray_matrices(xyz, cells, alpha, q, rots, res_x, res_y, bounds, limit, rows)
    return gradients_of(m, len(np.asarray(alpha)), weights, skip, with_scale)


def gradients_of(m, n_cells: int, weights, skip=None, with_scale: bool = False):
    """image_gradients from ray_matrices' dict (one set of matrices serves many upstream images).

    with_scale: also a dict of per-cell bounds on what rounding can do to each gradient: scale_alpha / scale_q, the same
    sums with every contribution replaced by its absolute value (|g_tau| dz, |g_I| T s, |g_I| T (|B| + dz E I_{k-1})),
    and sens_alpha / sens_q, the chord sensitivity (module docstring)."""
    C, D, valid, active, E, T = m["C"], m["D"], m["valid"], m["active"], m["E"], m["T"]
    w = np.asarray(weights, np.float64).reshape(m["n_px"], 2).copy()
    if skip is not None:
        w[np.asarray(skip).reshape(-1)] = 0.0
    moves = active & ~m["clamped"]
    dI_dq = np.where(active, T * m["S"], 0.0)
    dI_da = np.where(moves, T * (m["B"] - D * E * m["I_prev"]), 0.0)
    g_tau, g_I = w[:, :1], w[:, 1:]
    ga = np.zeros(n_cells)
    gq = np.zeros(n_cells)
    np.add.at(ga, C[valid], (g_tau * D + g_I * dI_da)[valid])
    np.add.at(gq, C[valid], (np.broadcast_to(g_I, D.shape) * dI_dq)[valid])
    out = ga, gq, m["tau"].reshape(m["shape"]), m["I"].reshape(m["shape"])
    if not with_scale:
        return out
    terms = {"scale_alpha": np.abs(g_tau) * D + np.abs(g_I) * m["abs_da"], "scale_q": np.abs(g_I) * dI_dq,
             "sens_alpha": np.abs(g_tau) * m["F"] + np.abs(g_I) * m["sens_a"], "sens_q": np.abs(g_I) * m["sens_q"]}
    extra = {name: np.bincount(C[valid], weights=np.broadcast_to(t, D.shape)[valid], minlength=n_cells) for name, t in terms.items()}
    return out + (extra,)


def forward_of(m, skip=None, with_scale: bool = False):
    """The forward render (include/course5_hip.h: c5_render) from ray_matrices' dict: (tau, I), the fp64 images of the
    dict's rows; skip: optional bool [rows, res_x], True = a solid-marked pixel, NaN in both channels.

    with_scale: also a dict of the per-pixel terms of the bar a render is held to (tests/derivative_fuzz.py: the forward
    sweep), every one [rows, res_x] and 0 on a pixel without a segment:
      scale_tau  sum dz_k |alpha_k|, sens_tau  sum F_k |alpha_k|                     (the raw alpha: tau is not clamped)
      scale_I    sum T_k |Q_k| S_k, the emission with every contribution by its absolute value
      sens_I     sum F_k T_k E_k |Q_k - a_k I_{k-1}| over the active segments: dI / d dz_k = T_k E_k (Q_k - a_k I_{k-1}), the
                 chord derivative the motion tangent's header states (c5_render_motion_tangent)
      cancel     8 x 2^-53 x sum T_k (|Q_k| + a_k |I_{k-1}|) / a_k over the active segments: the rounding of the REFERENCE'S
                 OWN step C = Q - a I; I = (Q - C e) / a (line.cpp:220-224).  With u = 2^-53, M = |Q| + a |I| >= |C| and
                 N = Q - C e = Q (1 - e) + a I e, |N| <= M, the step's roundings reach the numerator as: a I and C, u M e
                 each; e = exp(-x) within one ulp of an argument that is itself rounded, (2 + x) u M e; the product C e,
                 u M e; the difference, u |N|; and the division adds u |N| / a.  Together u M (e (5 + x) + 2) / a, and
                 e^-x (5 + x) <= 5: 7 u M / a to first order, 8 with the second.  The step's error reaches the pixel through
                 T_k.  This is what makes the reference "its own cancellation noise" for a in [DBL_EPSILON, ~1e-8) (DESIGN
                 section 5): 2^-50 / a is 4e-8 at a = 2e-8 and 4 at DBL_EPSILON, against the 2^-23 = 1.2e-7 of the output's
                 rounding; for a >= 1e-6 it is below 1e-9.  A render on "integration" 0 repeats the reference's roundings;
                 the restatement (E and S from exp and expm1) has none of them: the term is the distance between the two.
      emission   sum |Q_k| S_k over the active segments: what an early-out at transmittance c can drop is at most
                 c x this ("integration" 1 with a non-zero "transmittance_cutoff": the segments behind the cut have T < c)."""
    valid, active, D, F, T, E, S, Q = m["valid"], m["active"], m["D"], m["F"], m["T"], m["E"], m["S"], m["Q"]
    # I as sum T_k Q_k S_k, not the recurrence's last value (m["I"]): T carries its exponent in double-double
    # (_transmittance), while the recurrence multiplies by exp(-a dz) of a ROUNDED a dz - a ray that ends behind an optical
    # depth of 370 with nothing emitted in front has all of its I at 370 x 2^-53 of relative error that way
    # (tests/test_forward_reference_cpu.py, seed 2000: 127 x 2^-52 x scale against the 80-digit reference)
    tau, I = m["tau"].reshape(m["shape"]).copy(), np.where(active, T * Q * S, 0.0).sum(1).reshape(m["shape"])
    if skip is not None:
        tau[np.asarray(skip)] = np.nan
        I[np.asarray(skip)] = np.nan
    if not with_scale:
        return tau, I
    a, a_raw, I_prev = m["a"], np.abs(m["a_raw"]), m["I_prev"]
    inv_a = np.where(active, 1.0 / np.where(active, a, 1.0), 0.0)
    terms = {"scale_tau": np.where(valid, D * a_raw, 0.0), "sens_tau": np.where(valid, F * a_raw, 0.0),
             "scale_I": np.where(active, T * np.abs(Q) * S, 0.0),
             "sens_I": np.where(active, F * T * E * np.abs(Q - a * I_prev), 0.0),
             "cancel": 8.0 * 2.0 ** -53 * np.where(active, T * (np.abs(Q) + a * np.abs(I_prev)) * inv_a, 0.0),
             "emission": np.where(active, np.abs(Q) * S, 0.0)}
    return tau, I, {name: t.sum(1).reshape(m["shape"]) for name, t in terms.items()}

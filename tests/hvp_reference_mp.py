"""80-digit references of the Hessian-vector render (include/course5_hip.h: c5_render_hvp), in mpmath, two of them:

hvp(seg, ...)       the header's formulas evaluated AS WRITTEN over derivative_reference_mp.Segments' rays - S_a and S_aa in
                    closed form, no series, no threshold at a dz = 1/8 - with the suffix sums from the viewer's end and the
                    absolute-sum scale of tests/hvp_reference.py (the whole ray's sum |a_dot dz| in the suffix's place).
hvp_by_difference   independent of those formulas: the central difference (grad(+h) - grad(-h)) / 2h at h = 1e-25 of the
                    adjoint, derivative_reference_mp.adjoint's own per-segment terms (g_tau dz + g_I dI_da, g_I dI_dq) over
                    rays rebuilt as Segments builds them, with the scalars alpha + h d_alpha, Q + h d_q at 80 digits.  That
                    module's Segments takes the scalars as doubles and its adjoint returns doubles, neither of which a step
                    of 1e-25 survives, so the rays and the per-cell sums are rebuilt here in mpf; the terms are its own.
                    Whether a cell is active and whether its alpha is clamped is decided by the unperturbed double (a
                    clamped alpha stays at the limit, an unclamped one moves freely: the one-sided convention of the
                    adjoint).  The truncation error is h^2 = 1e-50 of the third derivative, the rounding 1e-80 / h = 1e-55.
"""
from __future__ import annotations

import numpy as np
from mpmath import mp, mpf

from tests import derivative_reference_mp as dm


def hvp(seg: dm.Segments, n_cells: int, d_alpha, d_q, weights):
    """h_alpha / h_q per cell with their scales for the upstream weights (g_tau, g_I) [len(pixels), 2] of seg.pixels: a
    dict alpha, q, scale_alpha, scale_q of fp64 arrays (one rounding of the 80-digit sums)."""
    mp.dps = dm.DPS
    zero, one, two = mpf(0), mpf(1), mpf(2)
    acc = {}
    for ray, (_g_tau, g_I) in zip(seg.rays, weights):
        g_I = mpf(float(g_I))
        n = len(ray)
        a_dot = [mpf(float(d_alpha[t["c"]])) if (d_alpha is not None and t["moves"]) else zero for t in ray]
        q_dot = [mpf(float(d_q[t["c"]])) if (d_q is not None and t["active"]) else zero for t in ray]
        suffix = [zero] * n
        s = zero
        for k in range(n - 1, -1, -1):
            suffix[k] = s
            s += a_dot[k] * ray[k]["d"]
        whole = sum((abs(a_dot[k] * ray[k]["d"]) for k in range(n)), zero)
        I_dot = abs_I_dot = zero
        for k, t in enumerate(ray):
            if not t["active"]:
                continue
            a, d, E, Q, S, I_prev, T = t["a"], t["d"], t["E"], t["Q"], t["s"], t["I_prev"], t["T"]
            S_a = d * E / a - (one - E) / (a * a)
            S_aa = two * (one - E) / a ** 3 - two * d * E / (a * a) - d * d * E / a
            lam = g_I * T
            lam_dot = -lam * suffix[k]
            G = Q * S_a - d * E * I_prev
            v = acc.setdefault(t["c"], [zero, zero, zero, zero])
            v[1] += lam_dot * S + lam * S_a * a_dot[k]
            v[3] += abs(lam) * (whole * S + abs(S_a * a_dot[k]))
            if t["moves"]:
                v[0] += lam_dot * G + lam * (q_dot[k] * S_a + Q * S_aa * a_dot[k] + d * d * E * a_dot[k] * I_prev - d * E * I_dot)
                v[2] += abs(lam) * (whole * (abs(Q * S_a) + d * E * abs(I_prev)) + abs(q_dot[k] * S_a) + abs(Q * S_aa * a_dot[k])
                                    + d * d * E * abs(a_dot[k] * I_prev) + d * E * abs_I_dot)
            I_dot = E * I_dot - d * E * a_dot[k] * I_prev + q_dot[k] * S + Q * S_a * a_dot[k]
            abs_I_dot = E * abs_I_dot + abs(q_dot[k]) * S + abs(a_dot[k]) * (abs(Q * S_a) + d * E * abs(I_prev))
    out = np.zeros((4, n_cells))
    for c, v in acc.items():
        out[:, c] = [float(x) for x in v]
    return dict(zip(("alpha", "q", "scale_alpha", "scale_q"), out))


def _gradient(seg: dm.Segments, d_alpha, d_q, h, weights):
    """{cell: [grad_alpha, grad_q]} in mpf at the scalars (alpha + h d_alpha, Q + h d_q): the rays as Segments builds them,
    the terms as derivative_reference_mp.adjoint sums them (the tau channel left out: it is linear in alpha)."""
    zero, one = mpf(0), mpf(1)
    acc = {}
    for ray0, (_g_tau, g_I) in zip(seg.rays, weights):
        g_I = mpf(float(g_I))
        ray, I = [], zero
        for t0 in ray0:
            c, d = t0["c"], t0["d"]
            t = dict(c=c, d=d, active=t0["active"], moves=t0["moves"], E=one, s=zero, B=zero, I_prev=I)
            if t0["active"]:
                a = t0["a"] + (h * mpf(float(d_alpha[c])) if (d_alpha is not None and t0["moves"]) else zero)
                Q = t0["Q"] + (h * mpf(float(d_q[c])) if d_q is not None else zero)
                E = mp.exp(-a * d)
                s = (one - E) / a
                t.update(E=E, s=s, B=Q * (d * E / a - (one - E) / (a * a)))
                I = E * I + Q * s
            ray.append(t)
        T = one
        for t in reversed(ray):
            if t["active"]:
                v = acc.setdefault(t["c"], [zero, zero])
                v[1] += g_I * T * t["s"]
                if t["moves"]:
                    v[0] += g_I * T * (t["B"] - t["d"] * t["E"] * t["I_prev"])
            T = T * t["E"]
    return acc


def hvp_by_difference(seg: dm.Segments, n_cells: int, d_alpha, d_q, weights, step: str = "1e-25"):
    """(h_alpha, h_q) fp64 [n_cells]: the central difference of the adjoint at 80 digits (module docstring)."""
    mp.dps = dm.DPS
    h = mpf(step)
    up, down = _gradient(seg, d_alpha, d_q, h, weights), _gradient(seg, d_alpha, d_q, -h, weights)
    out = np.zeros((2, n_cells))
    for c, v in up.items():
        out[:, c] = [float((v[j] - down[c][j]) / (2 * h)) for j in range(2)]
    return out[0], out[1]

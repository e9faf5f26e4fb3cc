"""numpy restatement of the Hessian-vector render (include/course5_hip.h: c5_render_hvp) over adjoint_reference.ray_matrices'
dict: h = Hess(phi) v for phi = sum_p (g_tau tau + g_I I) and a direction v = (d_alpha, d_q) of the cells' scalars.

DERIVATION.  Notation of tests/adjoint_reference.py: the segments of a pixel k = 1..n in processing order (deepest first),
a_k = min(alpha_k, limit), E_k = exp(-a_k dz_k), S_k = (1 - E_k) / a_k, I_k = E_k I_{k-1} + Q_k S_k over the active segments,
T_k = prod_{j > k} E_j = exp(-sum_{j > k} a_j dz_j).  tau = sum dz_k alpha_k is linear in alpha: its second derivative is
zero and g_tau drops out.  The adjoint's first derivatives of phi are, with lambda_k = g_I T_k,
    d phi / d Q_k     = lambda_k S_k                                              (active)
    d phi / d alpha_k = lambda_k G_k,  G_k = Q_k S_a,k - dz_k E_k I_{k-1}          (active, alpha_k not clamped)
    S_a = d S / d a = dz E / a - (1 - E) / a^2.
Differentiate both once more along v.  a_dot_k = d_alpha[cell_k] where the segment is active and its alpha not clamped,
else 0 (a clamped alpha does not move: min(alpha, limit) is constant there - no row and no column, the adjoint's own
convention); Q_dot_k = d_q[cell_k].
    d/dv lambda_k = g_I T_k d/dv (-sum_{j > k} a_j dz_j) = -lambda_k sum_{j > k} a_dot_j dz_j      =: lambda_dot_k
    d/dv S_k = S_a,k a_dot_k,   d/dv S_a,k = S_aa,k a_dot_k,   S_aa = 2 (1 - E) / a^3 - 2 dz E / a^2 - dz^2 E / a
    d/dv E_k = -dz_k E_k a_dot_k
    d/dv I_k = I_dot_k = E_k I_dot_{k-1} - dz_k E_k a_dot_k I_{k-1} + Q_dot_k S_k + Q_k S_a,k a_dot_k      (the tangent's I_dot)
so, by the product rule, a segment adds to its cell
    h_q     += lambda_dot_k S_k + lambda_k S_a,k a_dot_k
    h_alpha += lambda_dot_k G_k + lambda_k (Q_dot_k S_a,k + Q_k S_aa,k a_dot_k + dz_k^2 E_k a_dot_k I_{k-1} - dz_k E_k I_dot_{k-1})
(h_alpha only where alpha is not clamped; an inactive segment adds nothing).  S_a and S_aa are taken by their series
below a dz = 1/8, as the kernels take them: S_a = dz^2 (-1/2 + x/3 - x^2/8 + ...), S_aa = dz^3 sum_m (-1)^m (m + 2)(m + 1) /
(m + 3)! x^m = dz^3 (1/3 - x/4 + x^2/10 - x^3/36 + ...).  The suffix sums sum_{j > k} a_dot_j dz_j are formed from the
viewer's end, not as total minus prefix; T is the dict's double-double one.

SCALE (with_scale): per element the same sum with every contribution replaced by its absolute value, I_dot by the tangent's
absolute recurrence |I_dot|_k = E |I_dot|_{k-1} + |Q_dot| S + |a_dot| (|Q S_a| + dz E |I_{k-1}|), and the suffix sum by the WHOLE
ray's sum_j |a_dot_j dz_j|: the kernels form Lambda_dot - Lambda_dot_k as total minus prefix, whose rounding is that of the
whole ray's sum wherever the segment sits.
SENS (with_scale): the chord sensitivity, in the manner of gradients_of: an error delta_j <= F_j dz_err of chord j changes
a contribution by its derivative in dz_j.  A term proportional to dz_k^p counts p F_k |term| / dz_k (S: 1, S_a: 2, S_aa: 3,
dz E I: 1); the suffix sum moves by sum_{j > k} F_j |a_dot_j|; I_{k-1} and I_dot_{k-1} by their own recurrences
sens_I_k = E sens_I_{k-1} + F E |Q - a I_{k-1}| (d I_k / d dz_k = E_k (Q_k - a_k I_{k-1}), the motion tangent's chord derivative)
and sens_Idot_k = E sens_Idot_{k-1} + F / dz (|Q_dot| S + |a_dot| (2 |Q S_a| + dz E |I_{k-1}|)) + dz E |a_dot| sens_I_{k-1}.
The dependence of T on the chords (a relative a_j delta_j) is left to the 1e-9 scale term, as gradients_of leaves it.
"""
from __future__ import annotations

import math

import numpy as np


def second_order_terms(m):
    """S_a / (per unit Q) and S_aa of every segment of ray_matrices' dict, [pixel, k]; 0 where inactive."""
    D, E, active = m["D"], m["E"], m["active"]
    x = np.where(active, m["a"] * D, 0.0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        xs = np.where(x > 0, x, 1.0)
        ser_a = sum((-1.0) ** (k + 1) * (k + 1) / math.factorial(k + 2) * x ** k for k in range(14))
        dir_a = (x * E + np.expm1(-x)) / (xs * xs)
        ser_aa = sum((-1.0) ** k * (k + 2) * (k + 1) / math.factorial(k + 3) * x ** k for k in range(14))
        dir_aa = (-2.0 * np.expm1(-x) - 2.0 * x * E - x * x * E) / (xs * xs * xs)
    S_a = np.where(active, D * D * np.where(x < 0.125, ser_a, dir_a), 0.0)
    S_aa = np.where(active, D * D * D * np.where(x < 0.125, ser_aa, dir_aa), 0.0)
    return S_a, S_aa


def hvp_of(m, n_cells: int, d_alpha, d_q, weights, skip=None, with_scale: bool = False):
    """(h_alpha, h_q) [n_cells] from ray_matrices' dict m for the direction d_alpha / d_q ([n_cells]; None: zero) and the
    upstream image weights [rows, res_x, 2] of the dict's rows (channel 0 has no effect); skip: optional bool [rows,
    res_x], True = the pixel contributes nothing (solid).  with_scale: and a dict scale_alpha / scale_q / sens_alpha /
    sens_q (module docstring)."""
    C, D, F, valid, active, E, S, T, Q, I_prev = (m[k] for k in ("C", "D", "F", "valid", "active", "E", "S", "T", "Q", "I_prev"))
    M = D.shape[1]
    w = np.asarray(weights, np.float64).reshape(m["n_px"], 2).copy()
    if skip is not None:
        w[np.asarray(skip).reshape(-1)] = 0.0
    g_I = w[:, 1:]
    moves = active & ~m["clamped"]
    Cz = np.maximum(C, 0)
    a_dot = np.where(moves, 0.0 if d_alpha is None else np.asarray(d_alpha, np.float64)[Cz], 0.0)
    q_dot = np.where(active, 0.0 if d_q is None else np.asarray(d_q, np.float64)[Cz], 0.0)
    S_a, S_aa = second_order_terms(m)
    S = np.where(active, S, 0.0)
    DE = np.where(active, D * E, 0.0)
    F_dz = m["F_dz"]

    # carried from the deepest segment: I_dot_{k-1}, its absolute recurrence and the chord sensitivities of I and I_dot
    Id_prev, absId_prev, sI_prev, sId_prev = (np.zeros_like(D) for _ in range(4))
    Id = np.zeros(m["n_px"])
    absId, sI, sId = Id.copy(), Id.copy(), Id.copy()
    for j in range(M):
        Id_prev[:, j], absId_prev[:, j], sI_prev[:, j], sId_prev[:, j] = Id, absId, sI, sId
        act = active[:, j]
        src = q_dot[:, j] * S[:, j] + a_dot[:, j] * (Q[:, j] * S_a[:, j] - DE[:, j] * I_prev[:, j])
        a_src = np.abs(q_dot[:, j]) * S[:, j] + np.abs(a_dot[:, j]) * (np.abs(Q[:, j] * S_a[:, j]) + DE[:, j] * np.abs(I_prev[:, j]))
        s_src = (F_dz[:, j] * (np.abs(q_dot[:, j]) * S[:, j] + np.abs(a_dot[:, j]) * (2.0 * np.abs(Q[:, j] * S_a[:, j]) + DE[:, j] * np.abs(I_prev[:, j])))
                 + DE[:, j] * np.abs(a_dot[:, j]) * sI)
        Id = np.where(act, E[:, j] * Id + src, Id)
        absId = np.where(act, E[:, j] * absId + a_src, absId)
        sId = np.where(act, E[:, j] * sId + s_src, sId)
        sI = np.where(act, E[:, j] * sI + F[:, j] * E[:, j] * np.abs(Q[:, j] - m["a"][:, j] * I_prev[:, j]), sI)
    # from the viewer's end: sum_{j > k} a_dot_j dz_j, its absolute value and its chord sensitivity
    suffix, abs_suffix, F_suffix = (np.zeros_like(D) for _ in range(3))
    acc = np.zeros(m["n_px"])
    a_acc, f_acc = acc.copy(), acc.copy()
    for k in range(M - 1, -1, -1):
        suffix[:, k], abs_suffix[:, k], F_suffix[:, k] = acc, a_acc, f_acc
        acc = acc + a_dot[:, k] * D[:, k]
        a_acc = a_acc + np.abs(a_dot[:, k] * D[:, k])
        f_acc = f_acc + F[:, k] * np.abs(a_dot[:, k])
    whole = np.broadcast_to(a_acc[:, None], D.shape)  # the whole ray's sum |a_dot dz|

    lam = np.where(active, g_I * T, 0.0)
    lam_dot = -lam * suffix
    G = Q * S_a - DE * I_prev
    tq = lam_dot * S + lam * S_a * a_dot
    ta = np.where(moves, lam_dot * G + lam * (q_dot * S_a + Q * S_aa * a_dot + D * DE * a_dot * I_prev - DE * Id_prev), 0.0)
    ha = np.bincount(C[valid], weights=ta[valid], minlength=n_cells).astype(np.float64)
    hq = np.bincount(C[valid], weights=tq[valid], minlength=n_cells).astype(np.float64)
    if not with_scale:
        return ha, hq
    al = np.abs(lam)
    absG = np.abs(Q * S_a) + DE * np.abs(I_prev)
    second = np.abs(q_dot * S_a) + np.abs(Q * S_aa * a_dot) + D * DE * np.abs(a_dot * I_prev)
    terms = {
        "scale_q": al * (whole * S + np.abs(S_a * a_dot)),
        "scale_alpha": np.where(moves, al * (whole * absG + second + DE * absId_prev), 0.0),
        "sens_q": al * (F_suffix * S + F_dz * (abs_suffix * S + 2.0 * np.abs(S_a * a_dot))),
        "sens_alpha": np.where(moves, al * (
            F_suffix * absG + DE * sId_prev + (abs_suffix * DE + D * DE * np.abs(a_dot)) * sI_prev
            + F_dz * (abs_suffix * (2.0 * np.abs(Q * S_a) + DE * np.abs(I_prev)) + 2.0 * np.abs(q_dot * S_a)
                      + 3.0 * np.abs(Q * S_aa * a_dot) + 2.0 * D * DE * np.abs(a_dot * I_prev) + DE * absId_prev)), 0.0),
    }
    extra = {name: np.bincount(C[valid], weights=t[valid], minlength=n_cells).astype(np.float64) for name, t in terms.items()}
    return ha, hq, extra

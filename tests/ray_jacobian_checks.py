"""What holds a ray Jacobian (capi.Context.ray_jacobian: row_ptr, col, dz, dI_dalpha, dI_dq) to the numpy restatement,
element by element; shared by tests/test_gpu_ray_jacobian.py and scripts of one's own.  No GPU in here.

THE BAR of one stored value (tests/derivative_fuzz.py's form, none of it fitted to what the GPU returns):
    tol = 1e-9 scale + dz_err sens + 2^-970
scale: the element's own absolute parts - dz itself; |dI/dQ| = T S; for dI/dalpha the two parts of its bracket added in
absolute value, T (|B| + dz E |I_{k-1}|) (adjoint_reference: abs_da).  dz_err: derivative_fuzz.dz_err, the unit of a
chord's error; segment j's chord is known to dz_err F_j, F_j = max(1, |gx| + |gy|) of the steeper of its two faces.

sens FOR A SINGLE ELEMENT.  A per-cell sum's sens (adjoint_reference) takes a contribution to be proportional to its own
chord.  A single element of the Jacobian also sees the OTHER segments of its ray: the ones in front of it through
T_k = exp(-sum_{j > k} a_j dz_j), the ones behind it through I_{k-1}.  With k the processing order (deepest first),
S = (1 - E) / a, B = Q dS/da and the recurrence I_j = E_j I_{j-1} + Q_j S_j, the partial derivatives are
    d(dI/dQ_k) / d dz_k      = T_k E_k                                         (dS/d dz = E)
    d(dI/dQ_k) / d dz_j, j>k = -a_j dI/dQ_k                                    (through T_k)
    d(dI/dQ_k) / d dz_j, j<k = 0
    d(dI/da_k) / d dz_k      = -T_k E_k (Q_k dz_k + I_{k-1} (1 - a_k dz_k))    (dB/d dz = -Q dz E; d(dz E)/d dz = E (1 - a dz))
    d(dI/da_k) / d dz_j, j>k = -a_j dI/da_k                                    (through T_k)
    d(dI/da_k) / d dz_j, j<k = -T_k dz_k E_k P_jk E_j (Q_j - a_j I_{j-1}),  P_jk = prod_{j<i<k} E_i
                                                                               (dI_j / d dz_j = E_j (Q_j - a_j I_{j-1}), carried to I_{k-1} by P_jk)
(an inactive segment j has a_j = 0 and E_j = 1 and its chord moves nothing of I).  Hence, each chord off by dz_err F_j:
    sens_q[k] = F_k T_k E_k + |dI/dQ_k| sum_{j>k} a_j F_j
    sens_a[k] = F_k T_k E_k (|Q_k| dz_k + |I_{k-1}| |1 - a_k dz_k|) + |dI/da_k| sum_{j>k} a_j F_j + T_k dz_k E_k G_{k-1},
    G_j = E_j G_{j-1} + F_j E_j |Q_j - a_j I_{j-1}|  (active j; G_0 = 0),     sens_dz[k] = F_k.
tests/test_gpu_ray_jacobian.py checks the derivation on the CPU: the restatement with every chord moved by e F_j (every
sign pattern tried: all up, all down, random) moves no element by more than e sens, up to the second order."""
import numpy as np

from tests import derivative_fuzz as fz


def element_terms(m, skip=None):
    """From adjoint_reference.ray_matrices' dict, flat in CSR order (by pixel, deepest segment first; skip: bool per pixel,
    True = solid-marked, an empty row): a dict pixel, cell, dz, da, dq, scale_a, scale_q, sens_dz, sens_a, sens_q, and
    x = a dz of the active segments (nan elsewhere), clamped, active."""
    C, D, F, valid, active, E, T, S, B, Q, I_prev = (m[k] for k in ("C", "D", "F", "valid", "active", "E", "T", "S", "B", "Q", "I_prev"))
    a = m["a"]
    moves = active & ~m["clamped"]
    dq = np.where(active, T * S, 0.0)
    da = np.where(moves, T * (B - D * E * I_prev), 0.0)
    aF = np.where(active, a * F, 0.0)
    tail = aF[:, ::-1].cumsum(1)[:, ::-1] - aF  # sum over j > k
    G_prev = np.zeros_like(D)
    G = np.zeros(len(D))
    for j in range(D.shape[1]):
        G_prev[:, j] = G
        G = np.where(active[:, j], E[:, j] * G + F[:, j] * E[:, j] * np.abs(Q[:, j] - a[:, j] * I_prev[:, j]), G)
    sens_q = np.where(active, F * T * E + dq * tail, 0.0)
    sens_a = np.where(moves, F * T * E * (np.abs(Q) * D + np.abs(I_prev) * np.abs(1.0 - a * D)) + np.abs(da) * tail + T * D * E * G_prev, 0.0)
    if skip is not None:
        valid = valid & ~np.asarray(skip).reshape(-1)[:, None]
    P = np.broadcast_to(np.arange(m["n_px"])[:, None], C.shape)
    out = dict(pixel=P, cell=C, dz=D, da=da, dq=dq, scale_a=m["abs_da"], scale_q=dq, sens_dz=F, sens_a=sens_a, sens_q=sens_q,
               x=np.where(active, a * D, np.nan), clamped=m["clamped"] & valid, active=active)
    return {k: v[valid] for k, v in out.items()}


def worst_ratios(jac, ref, dz_e, n_px, n_cells):
    """error / tolerance of every stored value of jac = (row_ptr, col, dz, da, dq) against element_terms' dict: the
    structure must be the reference's exactly; returns the worst ratio of (dz, dI_dalpha, dI_dq) and where."""
    row_ptr, col, dz, da, dq = jac
    assert row_ptr.shape == (n_px + 1,) and row_ptr[0] == 0 and len(col) == len(dz) == len(da) == len(dq) == row_ptr[-1]
    pix = np.repeat(np.arange(n_px), np.diff(row_ptr))
    assert len(pix) == len(ref["pixel"]), f"{len(pix)} elements, the reference has {len(ref['pixel'])}"
    og, orf = np.lexsort((col, pix)), np.lexsort((ref["cell"], ref["pixel"]))
    assert np.array_equal(pix[og], ref["pixel"][orf]) and np.array_equal(col[og], ref["cell"][orf])
    assert ((col >= 0) & (col < n_cells)).all()
    out = []
    for got, want, scale, sens in ((dz, "dz", "dz", "sens_dz"), (da, "da", "scale_a", "sens_a"), (dq, "dq", "scale_q", "sens_q")):
        r = fz.ratio(got[og], ref[want][orf], ref[scale][orf], ref[sens][orf], dz_e)
        i = int(np.argmax(r)) if len(r) else 0
        out.append((float(r.max()) if len(r) else 0.0, f"pixel {int(pix[og][i])} cell {int(col[og][i])}" if len(r) else "-"))
    # what the header says of the zeros: explicit, and exact
    assert (da[og][~ref["active"][orf] | ref["clamped"][orf]] == 0).all() and (dq[og][~ref["active"][orf]] == 0).all()
    return out

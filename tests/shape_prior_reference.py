"""numpy restatement of the shape prior (include/course5_hip.h: c5_shape_prior_*), and its 80-digit form.

The restatement is float64 in the header's order of operations - every product rounded before the sum that takes it, every
3-term inner product (a0 b0 + a1 b1) + a2 b2, a point's sum over its cells in ascending cell index from 0, lambda last - so
that, fed the library's own rest data (c5_shape_prior_rest_data), the Dirichlet operators are the library's bits.  Beside
every result it returns `scale`, the absolute sum of the terms the result is made of (the products |F| |B|, |F^-T| ... with
their signs dropped, summed where the result sums): the bars of the tests are K x 2^-52 x scale.

The mpmath part (80 digits, as tests/derivative_reference_mp.py) holds psi, P, dP and B from the definitions, and the
operators assembled from them without rounding: what the restatement is measured against.

K: 4 x the worst ratio |restatement - mpmath| / (2^-52 scale) that tests/test_shape_prior_reference_cpu.py measures over its
grids, both energies and all operators, rounded up to a power of two; the margin covers the device's log and division
(which need not round as numpy's do) and the value's summation tree.  The CPU test asserts the measured ratios stay under
K / 4, so K cannot drift from what it stands for; DESIGN.md 4.21 records the ratios.

Nothing here knows the device's cell order: everything is in the caller's."""
import math

import numpy as np

from course5_amd import capi
from course5_amd import meshgen as mg
from tests.prior_reference import tree_depth, tree_sum  # noqa: F401 (one tree for both priors' values)

DIRICHLET, NEO_HOOKEAN = capi.C5_SHAPE_DIRICHLET, capi.C5_SHAPE_NEO_HOOKEAN
EPS = 2.0 ** -52
K = 8  # (measured: worst ratio 1.84: see the module docstring and test_the_restatement_s_error_against_mpmath_gives_K)


# ---- small dense helpers over [n, 3, 3] arrays, in the header's order ---------------------------------------------------

def _edges(x, vert):
    """D[n, r, c] = x[vert[:, c + 1], r] - x[vert[:, 0], r]."""
    x = np.asarray(x, dtype=np.float64)
    p0 = x[vert[:, 0]]
    return np.stack([x[vert[:, c + 1]] - p0 for c in range(3)], axis=2)


def _cofactors(A):
    """(C, det, abs_C, abs_det): the cofactors and det = (A00 C00 + A01 C01) + A02 C02, with the absolute sums of their terms."""
    a = lambda r, c: A[:, r, c]  # noqa: E731
    pairs = {(0, 0): ((1, 1, 2, 2), (1, 2, 2, 1)), (0, 1): ((1, 2, 2, 0), (1, 0, 2, 2)), (0, 2): ((1, 0, 2, 1), (1, 1, 2, 0)),
             (1, 0): ((0, 2, 2, 1), (0, 1, 2, 2)), (1, 1): ((0, 0, 2, 2), (0, 2, 2, 0)), (1, 2): ((0, 1, 2, 0), (0, 0, 2, 1)),
             (2, 0): ((0, 1, 1, 2), (0, 2, 1, 1)), (2, 1): ((0, 2, 1, 0), (0, 0, 1, 2)), (2, 2): ((0, 0, 1, 1), (0, 1, 1, 0))}
    C, aC = np.zeros_like(A), np.zeros_like(A)
    for (r, c), (p, m) in pairs.items():
        t1, t2 = a(p[0], p[1]) * a(p[2], p[3]), a(m[0], m[1]) * a(m[2], m[3])
        C[:, r, c] = t1 - t2
        aC[:, r, c] = np.abs(t1) + np.abs(t2)
    det = (a(0, 0) * C[:, 0, 0] + a(0, 1) * C[:, 0, 1]) + a(0, 2) * C[:, 0, 2]
    adet = (np.abs(a(0, 0)) * aC[:, 0, 0] + np.abs(a(0, 1)) * aC[:, 0, 1]) + np.abs(a(0, 2)) * aC[:, 0, 2]
    return C, det, aC, adet


def _times_b(D, B):
    """F = D B: F[r][c] = (D[r][0] B[0][c] + D[r][1] B[1][c]) + D[r][2] B[2][c]."""
    F = np.zeros_like(D)
    for r in range(3):
        for c in range(3):
            F[:, r, c] = (D[:, r, 0] * B[:, 0, c] + D[:, r, 1] * B[:, 1, c]) + D[:, r, 2] * B[:, 2, c]
    return F


def _squares(A):
    s = A[:, 0, 0] * A[:, 0, 0]
    for k in range(1, 9):
        s = s + A[:, k // 3, k % 3] * A[:, k // 3, k % 3]
    return s


def _to_shares(P, B, V0):
    """sh[n, 4, 3]: G = V0 (P B^T), point i + 1 takes column i, point 0 minus their sum."""
    sh = np.zeros((len(P), 4, 3))
    for r in range(3):
        for i in range(3):
            sh[:, i + 1, r] = V0 * ((P[:, r, 0] * B[:, i, 0] + P[:, r, 1] * B[:, i, 1]) + P[:, r, 2] * B[:, i, 2])
        sh[:, 0, r] = -((sh[:, 1, r] + sh[:, 2, r]) + sh[:, 3, r])
    return sh


def _share_scale(aP, B, V0):
    """_to_shares with every term's sign dropped: the absolute sum a share is made of."""
    aB = np.abs(B)
    sc = np.zeros((len(aP), 4, 3))
    for r in range(3):
        for i in range(3):
            sc[:, i + 1, r] = V0 * ((aP[:, r, 0] * aB[:, i, 0] + aP[:, r, 1] * aB[:, i, 1]) + aP[:, r, 2] * aB[:, i, 2])
        sc[:, 0, r] = (sc[:, 1, r] + sc[:, 2, r]) + sc[:, 3, r]
    return sc


# ---- rest data -----------------------------------------------------------------------------------------------------------

def welded_cells(xyz, cells):
    rep, _ = capi.weld_points(xyz)
    return rep[np.asarray(cells, dtype=np.int64).reshape(-1, 4)].astype(np.int64)


def rest(X, vert, with_scale=False):
    """(B [n, 3, 3], V0 [n], n_degenerate) of the cells `vert` (representatives, the order the library uses: c5_shape_prior_
    rest_data's, or welded_cells where the device keeps the caller's vertex order) at the rest coordinates X."""
    D = _edges(X, vert)
    C, det, aC, adet = _cofactors(D)
    with np.errstate(divide="ignore", invalid="ignore"):
        B = np.transpose(C, (0, 2, 1)) / det[:, None, None]
        V0 = np.abs(det) / 6.0
        ok = (V0 > 0) & np.isfinite(V0) & np.isfinite(B).all(axis=(1, 2))
        # |B| (|C| / |C|_terms ...) : a cofactor's terms over the determinant, and the determinant's own terms
        scale = np.transpose(aC, (0, 2, 1)) / np.abs(det)[:, None, None] + np.abs(B) * (adet / np.abs(det))[:, None, None]
    B = np.where(ok[:, None, None], B, 0.0)
    V0 = np.where(ok, V0, 0.0)
    out = (B, V0, int((~ok).sum()))
    return out + (np.where(ok[:, None, None], scale, 0.0),) if with_scale else out


# ---- the cells' parts -------------------------------------------------------------------------------------------------------

class _Cells:
    """What the operators share at a point x: F, J, which cells are live (not degenerate), inverted, and the energy's state."""

    def __init__(self, B, V0, vert, x, energy, kappa):
        self.B, self.V0, self.vert, self.energy, self.kappa = B, V0, vert, energy, kappa
        self.live = V0 > 0
        n = len(V0)
        self.F = self.J = self.Fit = self.lnJ = None
        self.inverted = np.zeros(n, dtype=bool)
        if x is not None:
            self.F = _times_b(_edges(x, vert), B)
            C, self.J, _aC, _adet = _cofactors(self.F)
            with np.errstate(invalid="ignore"):
                self.inverted = self.live & ~((self.J > 0) & (self.J < np.inf))
            if energy == NEO_HOOKEAN:
                with np.errstate(divide="ignore", invalid="ignore"):
                    self.Fit = C / self.J[:, None, None]
                    self.lnJ = np.log(self.J)
        self.active = self.live & ~self.inverted if energy == NEO_HOOKEAN else self.live

    def stress(self):
        """(P, |terms of P|)."""
        F = self.F
        if self.energy == DIRICHLET:
            eye = np.eye(3)[None]
            return np.where(eye > 0, F - 1.0, F), np.abs(F) + eye
        c0 = self.kappa * self.lnJ - 1.0
        t = c0[:, None, None] * self.Fit
        return F + t, np.abs(F) + np.abs(t)

    def dstress(self, dF):
        """(dP, |terms of dP|)."""
        if self.energy == DIRICHLET:
            return dF.copy(), np.abs(dF)
        Fit = self.Fit
        c1 = 1.0 - self.kappa * self.lnJ
        tr = Fit[:, 0, 0] * dF[:, 0, 0]
        for k in range(1, 9):
            tr = tr + Fit[:, k // 3, k % 3] * dF[:, k // 3, k % 3]
        kt = self.kappa * tr
        T, aT = np.zeros_like(dF), np.zeros_like(dF)
        aFit, adF = np.abs(Fit), np.abs(dF)
        for a in range(3):
            for b in range(3):
                T[:, a, b] = (dF[:, 0, a] * Fit[:, 0, b] + dF[:, 1, a] * Fit[:, 1, b]) + dF[:, 2, a] * Fit[:, 2, b]
                aT[:, a, b] = (adF[:, 0, a] * aFit[:, 0, b] + adF[:, 1, a] * aFit[:, 1, b]) + adF[:, 2, a] * aFit[:, 2, b]
        atr = (aFit * adF).sum(axis=(1, 2))
        dP, adP = np.zeros_like(dF), np.zeros_like(dF)
        for r in range(3):
            for c in range(3):
                m = (Fit[:, r, 0] * T[:, 0, c] + Fit[:, r, 1] * T[:, 1, c]) + Fit[:, r, 2] * T[:, 2, c]
                am = (aFit[:, r, 0] * aT[:, 0, c] + aFit[:, r, 1] * aT[:, 1, c]) + aFit[:, r, 2] * aT[:, 2, c]
                dP[:, r, c] = (dF[:, r, c] + c1 * m) + kt * Fit[:, r, c]
                adP[:, r, c] = (adF[:, r, c] + np.abs(c1) * am) + self.kappa * atr * aFit[:, r, c]
        return dP, adP

    def psi(self):
        """(psi, |terms of psi|)."""
        if self.energy == DIRICHLET:
            P, aP = self.stress()
            return 0.5 * _squares(P), 0.5 * _squares(aP)
        n2 = _squares(self.F)
        lnJ = self.lnJ
        return (0.5 * (n2 - 3.0) - lnJ) + (0.5 * self.kappa) * (lnJ * lnJ), (0.5 * (n2 + 3.0) + np.abs(lnJ)) + (0.5 * self.kappa) * (lnJ * lnJ)

    def shares(self, P, aP):
        """The cells' [n, 4, 3] shares and their scales; zeros for the cells that contribute nothing."""
        with np.errstate(invalid="ignore", over="ignore"):
            sh, sc = _to_shares(P, self.B, self.V0), _share_scale(aP, self.B, self.V0)
        keep = self.active[:, None, None]
        return np.where(keep, sh, 0.0), np.where(keep, sc, 0.0)


def point_sums(shares, vert, n_pts, lam):
    """out[p] = lam * (the shares of p's (cell, vertex) incidences, added in ascending cell index from 0)."""
    flat_pt = vert.reshape(-1)
    order = np.argsort(flat_pt, kind="stable")  # (stable: within a point, ascending flat index 4 c + k, i.e. ascending cell)
    pts = flat_pt[order]
    start = np.searchsorted(pts, np.arange(n_pts))
    count = np.bincount(pts, minlength=n_pts)
    flat = shares.reshape(-1, 3)
    total = np.zeros((n_pts, 3))
    for j in range(int(count.max()) if len(count) else 0):
        has = count > j
        total[has] = total[has] + flat[order[start[has] + j]]
    return lam * total


def _apply(B, V0, vert, n_pts, x, energy, kappa, lam, what, v=None, with_scale=False):
    cells = _Cells(B, V0, vert, x if (what == "gradient" or energy == NEO_HOOKEAN) else None, energy, kappa)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if what == "gradient":
            sh, sc = cells.shares(*cells.stress())
        elif what == "product":
            sh, sc = cells.shares(*cells.dstress(_times_b(_edges(v, vert), B)))
        else:  # the diagonal: entry (k, r) of the product applied to the unit vector of (point k, coordinate r)
            sh, sc = np.zeros((len(V0), 4, 3)), np.zeros((len(V0), 4, 3))
            for k in range(4):
                for r in range(3):
                    D = np.zeros((len(V0), 3, 3))
                    for c in range(3):
                        D[:, r, c] = (1.0 if k == c + 1 else 0.0) - (1.0 if k == 0 else 0.0)
                    one, one_sc = cells.shares(*cells.dstress(_times_b(D, B)))
                    sh[:, k, r], sc[:, k, r] = one[:, k, r], one_sc[:, k, r]
    out = point_sums(sh, vert, n_pts, lam)
    return (out, point_sums(sc, vert, n_pts, lam)) if with_scale else out


def gradient(B, V0, vert, n_pts, x, energy, kappa, lam, with_scale=False):
    return _apply(B, V0, vert, n_pts, x, energy, kappa, lam, "gradient", with_scale=with_scale)


def product(B, V0, vert, n_pts, x, v, energy, kappa, lam, with_scale=False):
    return _apply(B, V0, vert, n_pts, x, energy, kappa, lam, "product", v=v, with_scale=with_scale)


def diagonal(B, V0, vert, n_pts, x, energy, kappa, lam, with_scale=False):
    return _apply(B, V0, vert, n_pts, x, energy, kappa, lam, "diagonal", with_scale=with_scale)


def quality(B, V0, vert, x):
    """(ratio [n_cells] = J (0 for a degenerate rest cell), n_inverted)."""
    cells = _Cells(B, V0, vert, x, DIRICHLET, 0.0)
    return np.where(cells.live, cells.J, 0.0), int(cells.inverted.sum())


def value(B, V0, vert, x, energy, kappa, lam, with_scale=False):
    """R(x): the cells' V0 psi summed without error (math.fsum) - the library's tree differs from it by its own roundings
    only; +inf under the Neo-Hookean energy where a cell is inverted."""
    cells = _Cells(B, V0, vert, x, energy, kappa)
    if energy == NEO_HOOKEAN and cells.inverted.any():
        return (math.inf, math.inf) if with_scale else math.inf
    with np.errstate(invalid="ignore", divide="ignore"):
        psi, apsi = cells.psi()
        terms, aterms = np.where(cells.active, V0 * psi, 0.0), np.where(cells.active, V0 * apsi, 0.0)
    out = lam * math.fsum(terms)
    return (out, lam * math.fsum(aterms)) if with_scale else out


# ---- the conditioned scale ---------------------------------------------------------------------------------------------------
#
# `scale` above counts the terms of P (or dP) and of P B^T.  It does not count the terms of F = Ds B itself: on a sliver
# |Ds| |B| reaches 10^3 while F ~ I, and the rounding of F, 2^-53 of |Ds| |B| per product and sum, is then hundreds of times
# 2^-52 |F|.  The conditioned scale adds, per cell, the first-order image of every such hidden rounding; the bars built on it
# are K_CONDITIONED x 2^-52 x (scale + these), and hold on graded grids where K's do not.  Rounding by rounding, with |.| taken
# entry by entry and E_. a bound, in units of 2^-52, on the absolute error of the float64 quantity:
#   Ds = x_i - x_0           one rounding of |Ds| each; carried into the next line's products
#   F = Ds B                 three products and two sums per entry, each within 2^-53 of the partial sums, which
#                            |Ds| |B| bounds:                                   E_F   = |Ds| |B|     (>= |F|)
#   dF = Dv B                likewise:                                          E_dF  = |Dv| |B|     (>= |dF|)
#   C = cofactors(F), J      a cofactor is a difference of two products, J three products of F and C: their own terms
#                            aC, aJ (what _cofactors returns) over |J|, and F's error through d F^-T = -F^-T dF^T F^-T:
#   F^-T = C / J                                                                E_Fit = aC / |J| + |F^-T| aJ / |J| + |F^-T| E_F^T |F^-T|
#   ln J                     d ln J = tr(F^-1 dF), and J's own terms:           E_ln  = aJ / |J| + sum |F^-T| E_F
#   Dirichlet   P = F - I:   dP = dF, so                                        E_P   = E_F,    E_dP = E_dF
#               psi          d psi = P : dF                                     E_psi = sum |P| E_F
#   Neo-Hookean P = F + (kappa ln J - 1) F^-T:                                  E_P   = E_F + kappa E_ln |F^-T| + |kappa ln J - 1| E_Fit
#               dP = dF + c1 F^-T dF^T F^-T + kappa tr(F^-1 dF) F^-T, c1 = 1 - kappa ln J, with A = E_dF in place of |dF|:
#                            from dF     A + |c1| |F^-T| A^T |F^-T| + kappa (sum |F^-T| A) |F^-T|
#                            from F^-T   |c1| (E_Fit A^T |F^-T| + |F^-T| A^T E_Fit) + kappa (sum E_Fit A) |F^-T| + kappa (sum |F^-T| A) E_Fit
#                            from ln J   kappa E_ln |F^-T| A^T |F^-T|             E_dP  = the sum of the three
#               psi          d psi = F : dF - (1 - kappa ln J) d ln J            E_psi = sum |F| E_F + (1 + kappa |ln J|) E_ln
#   J (quality)              d J = C : dF                                        E_J   = sum |C| E_F
# E_P and E_dP go through _share_scale (|.| |B|^T, V0, the three columns' sum for point 0) and point_sums like the terms they
# stand beside; E_psi is multiplied by V0 and summed; the diagonal is the product's on the unit vectors' Dv.  The rest data B and
# V0 are INPUTS here (the library's own, or rest()'s), given exactly to the 80-digit form too: their error is test_rest_data's.
#
# K_CONDITIONED: 4 x the worst ratio |restatement - mpmath| / (2^-52 x conditioned scale) that tests/test_prior_fuzz_cpu.py
# measures on the unstructured scenes 7000 - 7011 and the six strain regimes, rounded up to a power of two - the project's
# rule, as for K.  No GPU result enters it.

K_CONDITIONED = 4  # (measured: see test_prior_fuzz_cpu.py::test_the_conditioned_scale_gives_K_CONDITIONED and DESIGN.md 4.21)


def _abs3(A, Bm, Cm):
    """A B^T C for stacks of non-negative 3 x 3 matrices."""
    return A @ np.transpose(Bm, (0, 2, 1)) @ Cm


class _Conditioning:
    """E_F, E_Fit, E_ln of the cells at x (the derivation above); nan / inf where a cell is not active: masked by the callers."""

    def __init__(self, cells, x):
        self.cells = cells
        aB = np.abs(cells.B)
        self.aB = aB
        self.EF = None if x is None else np.abs(_edges(x, cells.vert)) @ aB
        if cells.energy == NEO_HOOKEAN:
            _C, J, aC, aJ = _cofactors(cells.F)
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                self.aFit = np.abs(cells.Fit)
                rel = (aJ / np.abs(J))[:, None, None]
                self.EFit = aC / np.abs(J)[:, None, None] + self.aFit * rel + _abs3(self.aFit, self.EF, self.aFit)
                self.Eln = (rel[:, 0, 0] + (self.aFit * self.EF).sum(axis=(1, 2)))[:, None, None]
                self.c1 = np.abs(1.0 - cells.kappa * cells.lnJ)[:, None, None]

    def spread(self, D):
        """E_dF = |D| |B| of edge differences D."""
        return np.abs(D) @ self.aB

    def stress(self):
        """E_P."""
        if self.cells.energy == DIRICHLET:
            return self.EF
        with np.errstate(invalid="ignore", over="ignore"):
            return self.EF + self.cells.kappa * self.Eln * self.aFit + self.c1 * self.EFit

    def dstress(self, A):
        """E_dP for E_dF = A."""
        if self.cells.energy == DIRICHLET:
            return A
        k, aFit, EFit = self.cells.kappa, self.aFit, self.EFit
        with np.errstate(invalid="ignore", over="ignore"):
            M = _abs3(aFit, A, aFit)
            tr = (aFit * A).sum(axis=(1, 2))[:, None, None]
            out = A + self.c1 * M + k * tr * aFit
            out = out + self.c1 * (_abs3(EFit, A, aFit) + _abs3(aFit, A, EFit)) + k * (EFit * A).sum(axis=(1, 2))[:, None, None] * aFit + k * tr * EFit
            return out + k * self.Eln * M

    def psi(self):
        """E_psi."""
        c = self.cells
        with np.errstate(invalid="ignore", over="ignore"):
            if c.energy == DIRICHLET:
                return (np.abs(c.stress()[0]) * self.EF).sum(axis=(1, 2))
            return (np.abs(c.F) * self.EF).sum(axis=(1, 2)) + (1.0 + c.kappa * np.abs(c.lnJ)) * self.Eln[:, 0, 0]


def _unit_edges(n, k, r):
    D = np.zeros((n, 3, 3))
    for c in range(3):
        D[:, r, c] = (1.0 if k == c + 1 else 0.0) - (1.0 if k == 0 else 0.0)
    return D


def conditioned(B, V0, vert, n_pts, x, energy, kappa, lam, what, v=None):
    """(result, conditioned scale) of `what` in "gradient", "product", "diagonal": `scale` plus the propagation derived above."""
    out, scale = _apply(B, V0, vert, n_pts, x, energy, kappa, lam, what, v=v, with_scale=True)
    need_x = what == "gradient" or energy == NEO_HOOKEAN
    cells = _Cells(B, V0, vert, x if need_x else None, energy, kappa)
    cond = _Conditioning(cells, x if need_x else None)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if what == "gradient":
            extra = _share_scale(cond.stress(), B, V0)
        elif what == "product":
            extra = _share_scale(cond.dstress(cond.spread(_edges(v, vert))), B, V0)
        else:
            extra = np.zeros((len(V0), 4, 3))
            for k in range(4):
                for r in range(3):
                    extra[:, k, r] = _share_scale(cond.dstress(cond.spread(_unit_edges(len(V0), k, r))), B, V0)[:, k, r]
    extra = np.where(cells.active[:, None, None], extra, 0.0)
    return out, scale + point_sums(extra, vert, n_pts, lam)


def value_terms(B, V0, vert, x, energy, kappa):
    """(terms, scales) per cell, before lambda: V0 psi as the header forms it (0 where a cell contributes nothing; Neo-Hookean:
    inverted cells are NOT turned into +inf here) and the conditioned absolute sum each term is made of."""
    cells = _Cells(B, V0, vert, x, energy, kappa)
    cond = _Conditioning(cells, x)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        psi, apsi = cells.psi()
        terms = np.where(cells.active, V0 * psi, 0.0)
        scales = np.where(cells.active, V0 * (apsi + cond.psi()), 0.0)
    return terms, scales


def conditioned_value(B, V0, vert, x, energy, kappa, lam):
    """(value, conditioned scale): value()'s result, and lam x the exact sum of the cells' conditioned scales."""
    out = value(B, V0, vert, x, energy, kappa, lam)
    return out, (math.inf if out == math.inf else lam * math.fsum(value_terms(B, V0, vert, x, energy, kappa)[1]))


def conditioned_quality(B, V0, vert, x):
    """(ratio, n_inverted, scale [n_cells]): quality()'s and per cell the determinant's terms plus sum |C| E_F."""
    ratio, n_inv = quality(B, V0, vert, x)
    cells = _Cells(B, V0, vert, x, DIRICHLET, 0.0)
    C, _J, _aC, aJ = _cofactors(cells.F)
    EF = _Conditioning(cells, x).EF
    return ratio, n_inv, np.where(cells.live, aJ + (np.abs(C) * EF).sum(axis=(1, 2)), 0.0)


# ---- the strain regimes and the sampled points of the fuzz sweeps (tests/test_prior_fuzz_cpu.py, tests/test_gpu_prior_fuzz.py)

STRAINS = ("shrunk", "grown", "squashed", "rotated", "translated", "displaced")
FUZZ_SEEDS = tuple(range(7000, 7012))  # tests/unstructured_scenes.py: any 12 consecutive seeds hold every class


def strained(X, vert, regime):
    """The point x of a regime: a uniform scale about the centre by 1e-3 and by 1e3 (J = 1e-9, 1e9), a squash along z to
    J = 1e-9, a rotation by 2.5 rad about z, a translation by 1e6, a displacement of 0.24 of the local cell size (a
    quarter would let a cell invert)."""
    X = np.asarray(X, dtype=np.float64)
    c = X.mean(axis=0)
    if regime in ("shrunk", "grown"):
        return c + (1e-3 if regime == "shrunk" else 1e3) * (X - c)
    if regime == "squashed":
        return c + (X - c) * np.array([1.0, 1.0, 1e-9])
    if regime == "rotated":
        R = np.array([[math.cos(2.5), -math.sin(2.5), 0.0], [math.sin(2.5), math.cos(2.5), 0.0], [0.0, 0.0, 1.0]])
        return c + (X - c) @ R.T
    if regime == "translated":
        return X + 1e6
    assert regime == "displaced"
    return displaced(X, vert, share=0.24)


def sampled_points(vert, n_pts, seed, most=48, most_cells=64):
    """At most `most` points, drawn per seed among those in 1 .. most_cells cells, ascending."""
    count = np.bincount(np.asarray(vert).reshape(-1), minlength=n_pts)
    ok = np.flatnonzero((count > 0) & (count <= most_cells))
    rng = np.random.default_rng([seed, 0x5A])
    return np.sort(rng.choice(ok, size=min(most, len(ok)), replace=False))


def directions(n_pts, seed):
    """The product's direction v, per seed."""
    return np.random.default_rng([seed, 0xD1]).normal(size=(n_pts, 3))


def mp_ratio(got, want_mp, scale):
    """max |got - want| / (2^-52 scale) over the entries; where the scale is 0, got must be 0."""
    mp = _mp()
    worst = 0.0
    for g, w, s in zip(np.asarray(got, dtype=np.float64).reshape(-1), want_mp, np.asarray(scale, dtype=np.float64).reshape(-1)):
        if s == 0:
            assert g == 0 and abs(w) < mp.mpf(10) ** -60
            continue
        worst = max(worst, float(abs(mp.mpf(float(g)) - w) / (mp.mpf(EPS) * mp.mpf(float(s)))))
    return worst


class MpSamples:
    """The 80-digit operators of one (rest data, x, v) at sampled points, both energies, computed once and shared:
    gradient[energy] and product[energy]: {p: [3] mpf}; diagonal[energy]: {p: [3] mpf} at every fourth sampled point;
    value[energy]: {p: mpf}, the sum over p's incident cells; J: {cell: mpf} of those cells."""

    def __init__(self, B, V0, vert, x, v, kappa, lam, points, energies=(DIRICHLET, NEO_HOOKEAN)):
        mp = _mp()
        self.points, self.cells_of = points, {int(p): np.flatnonzero((vert == p).any(axis=1)) for p in points}
        self.gradient, self.product, self.diagonal, self.value = ({e: {} for e in energies} for _ in range(4))
        xs = None
        for e in energies:
            for i, p in enumerate(points):
                p = int(p)
                self.gradient[e][p] = mp_at_point(B, V0, vert, p, x, e, kappa, lam)
                self.product[e][p] = mp_at_point(B, V0, vert, p, x, e, kappa, lam, v=v)
                if i % 4 == 0:
                    self.diagonal[e][p] = [mp_at_point(B, V0, vert, p, x, e, kappa, lam, unit=r)[r] for r in range(3)]
                cells = self.cells_of[p]
                pts, local = np.unique(vert[cells], return_inverse=True)
                xs = _mp_points(np.asarray(x)[pts])
                self.value[e][p] = mp_value(B[cells], V0[cells], local.reshape(-1, 4), xs, e, kappa, lam)
        self.J = {}
        for p in points[::4]:
            for c in self.cells_of[int(p)]:
                if V0[c] > 0 and int(c) not in self.J:
                    self.J[int(c)] = mp.det(_mp_F(_mp_matrix(B[c]), _mp_points(np.asarray(x)[vert[c]])))

    def ratios(self, energy, gradient=None, product=None, diagonal=None, value_terms=None, quality=None):
        """{quantity: worst |got - 80 digits| / (2^-52 scale)} of the (result, scale) pairs given: vectors [n_pts, 3] read at
        the sampled points; value_terms = (terms, scales) per cell, summed exactly over a sampled point's cells."""
        out = {}
        for name, pair, want in (("gradient", gradient, self.gradient), ("product", product, self.product), ("diagonal", diagonal, self.diagonal)):
            if pair is not None:
                out[name] = max(mp_ratio(pair[0][p], want[energy][p], pair[1][p]) for p in want[energy])
        if value_terms is not None:
            out["value"] = max(mp_ratio([math.fsum(value_terms[0][c])], [w], [math.fsum(value_terms[1][c])])
                               for p, w in self.value[energy].items() for c in (self.cells_of[p],))
        if quality is not None:
            cells = sorted(self.J)
            out["quality"] = mp_ratio(quality[0][cells], [self.J[c] for c in cells], quality[1][cells])
        return out


# ---- the value's tree -----------------------------------------------------------------------------------------------------------

def value_tree(B, V0, vert, x, energy, kappa, lam):
    """R(x) as the device sums it under "cell_order" 0: tree_sum of the cells' V0 psi in the caller's order, lambda last; +inf
    under the Neo-Hookean energy where a cell is inverted."""
    cells = _Cells(B, V0, vert, x, energy, kappa)
    if energy == NEO_HOOKEAN and cells.inverted.any():
        return math.inf
    return lam * tree_sum(value_terms(B, V0, vert, x, energy, kappa)[0])


def dense_hessian(B, V0, vert, n_pts, x, energy, kappa, lam):
    """[3 n_pts, 3 n_pts]: column j is the product applied to unit vector j."""
    H = np.zeros((3 * n_pts, 3 * n_pts))
    for j in range(3 * n_pts):
        e = np.zeros(3 * n_pts)
        e[j] = 1.0
        H[:, j] = product(B, V0, vert, n_pts, x, e.reshape(n_pts, 3), energy, kappa, lam).reshape(-1)
    return H


# ---- 80 digits ---------------------------------------------------------------------------------------------------------------

def _mp():
    import mpmath as mp  # (what tests/derivative_reference_mp.py uses)
    mp.mp.dps = 80
    return mp


def mp_B(X4):
    """B = Dm^-1 and V0 of one cell from its four rest points (exact inputs: the float64 coordinates)."""
    mp = _mp()
    D = mp.matrix(3, 3)
    for c in range(3):
        for r in range(3):
            D[r, c] = mp.mpf(float(X4[c + 1][r])) - mp.mpf(float(X4[0][r]))
    return D ** -1, abs(mp.det(D)) / 6


def _mp_F(B, x4):
    mp = _mp()
    D = mp.matrix(3, 3)
    for c in range(3):
        for r in range(3):
            D[r, c] = x4[c + 1][r] - x4[0][r]
    return D * B


def mp_psi(F, energy, kappa):
    mp = _mp()
    if energy == DIRICHLET:
        P = F - mp.eye(3)
        return sum(P[i, j] ** 2 for i in range(3) for j in range(3)) / 2
    lnJ = mp.log(mp.det(F))
    return (sum(F[i, j] ** 2 for i in range(3) for j in range(3)) - 3) / 2 - lnJ + mp.mpf(kappa) / 2 * lnJ ** 2


def mp_P(F, energy, kappa):
    mp = _mp()
    if energy == DIRICHLET:
        return F - mp.eye(3)
    Fit = (F ** -1).T
    return F + (mp.mpf(kappa) * mp.log(mp.det(F)) - 1) * Fit


def mp_dP(F, dF, energy, kappa):
    mp = _mp()
    if energy == DIRICHLET:
        return dF.copy()
    Fi = F ** -1
    Fit = Fi.T
    lnJ = mp.log(mp.det(F))
    tr = sum((Fi * dF)[i, i] for i in range(3))
    return dF + (1 - mp.mpf(kappa) * lnJ) * (Fit * dF.T * Fit) + mp.mpf(kappa) * tr * Fit


def _mp_matrix(A):
    mp = _mp()
    M = mp.matrix(3, 3)
    for i in range(3):
        for j in range(3):
            M[i, j] = mp.mpf(float(A[i][j]))
    return M


def _mp_points(x):
    mp = _mp()
    return [[mp.mpf(float(t)) for t in p] for p in np.asarray(x, dtype=np.float64)]


def mp_value(B, V0, vert, x, energy, kappa, lam, cells=None):
    """R(x) in 80 digits from the float64 rest data; x: a list of points of mpf coordinates (so that it can be
    differentiated).  cells: only these."""
    mp = _mp()
    total = mp.mpf(0)
    for c in (range(len(V0)) if cells is None else cells):
        if V0[c] > 0:
            F = _mp_F(_mp_matrix(B[c]), [x[p] for p in vert[c]])
            total += mp.mpf(float(V0[c])) * mp_psi(F, energy, kappa)
    return mp.mpf(lam) * total


def mp_at_point(B, V0, vert, p, x, energy, kappa, lam, v=None, unit=None):
    """Row p of mp_operator - [3] of mpf - from p's incident cells alone (mp_operator(cells=) on their points): the gradient,
    the product with v, or with unit = r the product with the unit vector of (p, r), whose entry r is the diagonal's."""
    cells = np.flatnonzero((vert == p).any(axis=1))
    pts, local = np.unique(vert[cells], return_inverse=True)
    local = local.reshape(-1, 4)
    at = int(np.searchsorted(pts, p))
    if unit is not None:
        v = np.zeros((len(pts), 3))
        v[at, unit] = 1.0
    else:
        v = None if v is None else np.asarray(v)[pts]
    return mp_operator(B[cells], V0[cells], local, len(pts), np.asarray(x)[pts], energy, kappa, lam, v=v)[at]


def mp_operator(B, V0, vert, n_pts, x, energy, kappa, lam, v=None, cells=None):
    """The gradient (v None) or the product with v, [n_pts][3] of mpf, assembled from mp_P / mp_dP without rounding.
    cells: only these (as mp_value's)."""
    mp = _mp()
    out = [[mp.mpf(0)] * 3 for _ in range(n_pts)]
    xs = x if isinstance(x, list) else _mp_points(x)
    vs = None if v is None else (v if isinstance(v, list) else _mp_points(v))
    for c in (range(len(V0)) if cells is None else cells):
        if not V0[c] > 0:
            continue
        Bc = _mp_matrix(B[c])
        F = _mp_F(Bc, [xs[p] for p in vert[c]])
        S = mp_P(F, energy, kappa) if vs is None else mp_dP(F, _mp_F(Bc, [vs[p] for p in vert[c]]), energy, kappa)
        G = mp.mpf(float(V0[c])) * (S * Bc.T)
        for r in range(3):
            for i in range(3):
                out[vert[c][i + 1]][r] = out[vert[c][i + 1]][r] + G[r, i]
                out[vert[c][0]][r] = out[vert[c][0]][r] - G[r, i]
    return [[mp.mpf(lam) * t for t in p] for p in out]


# ---- the grids of tests/test_gpu_shape_prior.py: the smallest at which each thing can break ------------------------------------

def one_tet():
    return np.array([[0.6, -0.2, -0.1], [1.3, -0.1, 0.0], [0.8, 0.4, 0.1], [0.9, 0.0, 0.5]]), np.array([[0, 1, 2, 3]], dtype=np.int32)


def with_a_flat_cell():
    """cube8 and one more cell whose four points lie in a plane: a rest cell of zero volume."""
    xyz, cells = mg.cube8()
    flat = np.array([[2.0, 0.0, 0.0], [3.0, 0.0, 0.0], [2.0, 1.0, 0.0], [3.0, 1.0, 0.0]])
    n = len(xyz)
    return np.vstack([xyz, flat]), np.vstack([cells, [[n, n + 1, n + 2, n + 3]]]).astype(np.int32)


STAR_SEED = 46  # tests/unstructured_scenes.py: a "star" base kept whole - its centre is in hundreds of cells


def grids():
    """{name: (xyz, cells)}.  kuhn9's cells are in a random order: the caller's ids are not the device's (Morton order
    starts at 4 096 cells)."""
    from tests import unstructured_scenes as us
    out = {"one_tet": one_tet(), "cube8": mg.cube8(), "kuhn4": mg.kuhn_box(4, jitter=0.1)}
    xyz, cells = mg.kuhn_box(9, jitter=0.1)
    out["kuhn9"] = (xyz, cells[np.random.default_rng(5).permutation(len(cells))])
    out["soup"] = mg.per_cell_point_copies(*mg.kuhn_box(2))
    out["interface"] = mg.refined_interface(n=2)[:2]
    out["star"] = us.scene(STAR_SEED)[:2]
    out["flat"] = with_a_flat_cell()
    return {k: (np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(c, dtype=np.int32)) for k, (x, c) in out.items()}


def local_size(xyz, vert):
    """Per point: the smallest altitude of any cell it is in (inf for a point of no cell, cells without volume left out) -
    the cell size a displacement is measured against: moving every point by less than a quarter of it inverts nothing."""
    x = np.asarray(xyz, dtype=np.float64)
    p = x[vert]  # [n, 4, 3]
    vol = np.abs(np.einsum("ni,ni->n", np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), p[:, 3] - p[:, 0])) / 6.0
    faces = ((1, 2, 3), (0, 2, 3), (0, 1, 3), (0, 1, 2))
    area = np.stack([0.5 * np.linalg.norm(np.cross(p[:, b] - p[:, a], p[:, c] - p[:, a]), axis=1) for a, b, c in faces], axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        alt = np.where(vol[:, None] > 0, 3.0 * vol[:, None] / area, np.inf).min(axis=1)
    h = np.full(len(x), np.inf)
    np.minimum.at(h, vert.reshape(-1), np.repeat(alt, 4))
    return h


def displaced(xyz, vert, share=0.07, phase=0.0):
    """The rest shape plus a smooth displacement of `share` (5 - 10 %) of the local cell size: a unit-bounded field of
    sines of the coordinates, scaled per point by local_size.  `vert` names weld representatives: only they move (the
    library does not read the others' coordinates)."""
    x = np.asarray(xyz, dtype=np.float64)
    h = local_size(x, vert)
    h = np.where(np.isfinite(h), h, 0.0)
    field = np.stack([np.sin(5.0 * x[:, 1] + 3.0 * x[:, 2] + phase), np.sin(4.0 * x[:, 2] - 2.0 * x[:, 0] + 1.0 + phase),
                      np.cos(3.0 * x[:, 0] + 6.0 * x[:, 1] + phase)], axis=1) / math.sqrt(3.0)
    return x + share * h[:, None] * field

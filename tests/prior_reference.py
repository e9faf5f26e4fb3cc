"""numpy restatement of the cell-field smoothness prior (include/course5_hip.h: c5_prior_*).

Three parts.  adjacency(): the interior faces, from sorted face keys over c5_weld_points' representatives (the table
c5_upload_grid builds; tests/test_prior_reference_cpu.py checks it against c5_face_adjacency).  weights(): the two
weightings in np.longdouble, straight from the definition - A the area of the face, x the mean of a cell's four points -
with the factor |e1| |e2| / (2 A) that bounds the cross product's cancellation in the library's fp64.  The four
operators in float64, in the header's order of operations: a cell's sum over f = 0..3 from 0, every term by plain
multiplies, lambda on the finished sum - so that, fed the library's own weights, the quadratic operators are the library's
bits.  The penalties' three functions are checked against 80-digit mpmath in the CPU test.

Nothing here knows the device's cell order: everything is in the caller's."""
import math

import numpy as np

from course5_amd import capi
from course5_amd import meshgen as mg

FACES = ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3))
QUADRATIC, PSEUDO_HUBER = capi.C5_PRIOR_QUADRATIC, capi.C5_PRIOR_PSEUDO_HUBER
UNIT, TPFA = capi.C5_PRIOR_UNIT, capi.C5_PRIOR_TPFA
EPS = 2.0 ** -52


def welded_cells(xyz, cells):
    rep, _ = capi.weld_points(xyz)
    return rep[np.asarray(cells, dtype=np.int64).reshape(-1, 4)].astype(np.int64)


def adjacency(xyz, cells):
    """adj [n_cells, 4]: the cell across face f, or -1.  Raises ValueError where a face is in more than two cells."""
    wc = welded_cells(xyz, cells)
    n = len(wc)
    keys = np.sort(np.stack([wc[:, list(f)] for f in FACES], axis=1).reshape(4 * n, 3), axis=1)
    order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
    sk = keys[order]
    new = np.ones(4 * n, dtype=bool)
    new[1:] = (sk[1:] != sk[:-1]).any(axis=1)
    start = np.flatnonzero(new)
    length = np.diff(np.append(start, 4 * n))
    if (length > 2).any():
        raise ValueError("a face is shared by more than two cells")
    adj = np.full(4 * n, -1, dtype=np.int64)
    first = start[length == 2]
    a, b = order[first], order[first + 1]
    adj[a], adj[b] = b // 4, a // 4
    return adj.reshape(n, 4)


def n_interior_faces(adj) -> int:
    return int((adj >= 0).sum()) // 2


def weights(xyz, cells, adj, weighting):
    """(w, factor): w np.longdouble [n_cells, 4] - 0 without a neighbour, 1 (UNIT) or A / |x_n - x_c| (TPFA; 0 where that
    is not finite and positive) - and factor float64 [n_cells, 4] = |e1| |e2| / (2 A) of the edges the library's cross
    product is formed from (from the face's lowest welded point id to the two others; 0 without a neighbour)."""
    n = len(adj)
    has = adj >= 0
    if weighting == UNIT:
        return has.astype(np.longdouble), np.zeros((n, 4))
    wc = welded_cells(xyz, cells)
    P = np.asarray(xyz, dtype=np.longdouble)
    cen = P[wc].sum(axis=1) / np.longdouble(4)
    w = np.zeros((n, 4), dtype=np.longdouble)
    factor = np.zeros((n, 4))
    for f, fv in enumerate(FACES):
        ids = np.sort(wc[:, list(fv)], axis=1)
        e1, e2 = P[ids[:, 1]] - P[ids[:, 0]], P[ids[:, 2]] - P[ids[:, 0]]
        cr = np.cross(e1, e2)
        area = np.sqrt((cr * cr).sum(axis=1)) / np.longdouble(2)
        g = cen[np.where(has[:, f], adj[:, f], 0)] - cen
        dist = np.sqrt((g * g).sum(axis=1))
        with np.errstate(divide="ignore", invalid="ignore"):
            t = area / dist
            fac = np.sqrt((e1 * e1).sum(axis=1)) * np.sqrt((e2 * e2).sum(axis=1)) / (2 * area)
        ok = has[:, f] & np.isfinite(t) & (t > 0)
        w[:, f] = np.where(ok, t, 0)
        factor[:, f] = np.where(has[:, f], fac.astype(np.float64), 0.0)
    return w, factor


# ---- the penalties, in the header's order of operations (float64 arrays in, float64 out)

TAIL = 2.0 ** 256  # |u| from which the header takes the pseudo-Huber penalty's linear tail in closed form


def _quiet(f):
    """The header's forms pass through inf on their way to a finite result (u u, d d): numpy need not warn of it."""
    def wrapped(*args):
        with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
            return f(*args)
    wrapped.__name__, wrapped.__doc__ = f.__name__, f.__doc__
    return wrapped


@_quiet
def psi(penalty, d, delta):
    if penalty == QUADRATIC:
        return 0.5 * (d * d)
    d = np.asarray(d, dtype=np.float64)
    u = d / delta
    dd, s1 = d * d, 1.0 + np.sqrt(1.0 + u * u)
    below = np.where(dd < np.inf, dd / s1, np.abs(d) * (np.abs(d) / s1))
    return np.where(np.abs(u) >= TAIL, delta * (np.abs(d) - delta), below)[()]


def psi_naive(d, delta):
    """delta^2 (sqrt(1 + t) - 1): the form the header rules out (the CPU test's negative control)."""
    u = d / delta
    return (delta * delta) * (np.sqrt(1.0 + u * u) - 1.0)


@_quiet
def slope(penalty, d, delta):
    if penalty == QUADRATIC:
        return d
    d = np.asarray(d, dtype=np.float64)
    u = d / delta
    return np.where(np.abs(u) >= TAIL, np.copysign(delta, d), d / np.sqrt(1.0 + u * u))[()]


@_quiet
def curvature(penalty, d, delta):
    if penalty == QUADRATIC:
        return np.ones_like(d)
    d = np.asarray(d, dtype=np.float64)
    u = d / delta
    q = 1.0 + u * u
    au = np.abs(u)
    return np.where(au >= TAIL, ((1.0 / au) / au) / au, 1.0 / (q * np.sqrt(q)))[()]


# ---- the pseudo-Huber penalty over the format's range (tests/test_prior_fuzz_cpu.py, tests/test_gpu_prior_fuzz.py)

HUBER_BAR = 24 * EPS  # tests/test_gpu_prior.py derives it
TINY = 2.0 ** -1022   # the smallest normal number: below it a result is held to HUBER_BAR x TINY absolutely


def huber_at_80_digits(d, delta):
    """(psi, psi', psi'') of the float64 d and delta from the definitions; psi = delta^2 (sqrt(1 + t) - 1) as d^2 / (1 +
    sqrt(1 + t)), the same number, since 80 digits do not hold 1 + 1e-600 either."""
    import mpmath as mp
    mp.mp.dps = 80
    md, mdelta = mp.mpf(float(d)), mp.mpf(float(delta))
    t = (md / mdelta) ** 2
    return md ** 2 / (1 + mp.sqrt(1 + t)), md / mp.sqrt(1 + t), (1 + t) ** mp.mpf(-1.5)


def huber_sweep():
    """[(delta, d)]: |d| / delta by decades from 1e-300 to 1e300 for delta in 1e-150, 1, 1e150, both signs in turn, where d
    is a finite non-zero float64."""
    out = []
    for delta in (1e-150, 1.0, 1e150):
        for k in range(-300, 301):
            d = (10.0 ** k) * delta  # (Python floats: inf beyond the format, 0 or a subnormal below it)
            if math.isfinite(d) and d != 0:
                out.append((delta, float(d) if k % 2 else -float(d)))
    return out


def huber_within_the_bar(got, want):
    """|got - want| <= HUBER_BAR max(|want|, TINY) where want is inside the format; beyond it nothing is asked but no NaN."""
    import mpmath as mp
    if abs(want) >= mp.mpf(2) ** 1024:
        return not math.isnan(got)
    return math.isfinite(got) and abs(mp.mpf(float(got)) - want) <= mp.mpf(HUBER_BAR) * max(abs(want), mp.mpf(TINY))


# ---- the operators

def _faces(adj, x):
    """Per face f: (has a neighbour, the neighbour's index or 0, d = x_c - x_n)."""
    for f in range(4):
        has = adj[:, f] >= 0
        nb = np.where(has, adj[:, f], 0)
        yield f, has, nb, (x - x[nb] if x is not None else np.zeros(len(adj)))


def _sum(adj, x, term):
    """(sum, scale): (((0 + t0) + t1) + t2) + t3 over the faces with a neighbour, and the sum of |t_f|."""
    total, scale = np.zeros(len(adj)), np.zeros(len(adj))
    for f, has, nb, d in _faces(adj, x):
        t = np.where(has, term(f, nb, d), 0.0)
        total = total + t
        scale = scale + np.abs(t)
    return total, scale


def gradient(w, adj, x, lam, penalty=QUADRATIC, delta=1.0, with_scale=False):
    w = np.asarray(w, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    total, scale = _sum(adj, x, lambda f, nb, d: w[:, f] * slope(penalty, d, delta))
    return (lam * total, lam * scale) if with_scale else lam * total


def product(w, adj, x, p, lam, penalty=QUADRATIC, delta=1.0, with_scale=False):
    w = np.asarray(w, dtype=np.float64)
    p = np.asarray(p, dtype=np.float64)
    x = None if x is None else np.asarray(x, dtype=np.float64)
    total, scale = _sum(adj, x, lambda f, nb, d: (w[:, f] * curvature(penalty, d, delta)) * (p - p[nb]))
    return (lam * total, lam * scale) if with_scale else lam * total


def diagonal(w, adj, x, lam, penalty=QUADRATIC, delta=1.0, with_scale=False):
    w = np.asarray(w, dtype=np.float64)
    x = None if x is None else np.asarray(x, dtype=np.float64)
    total, scale = _sum(adj, x, lambda f, nb, d: w[:, f] * curvature(penalty, d, delta))
    return (lam * total, lam * scale) if with_scale else lam * total


def value(w, adj, x, lam, penalty=QUADRATIC, delta=1.0) -> float:
    """R(x): the cells' halves as the header forms them, summed without error (math.fsum) - the library's tree differs
    from it by its own roundings only."""
    w = np.asarray(w, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    total, _ = _sum(adj, x, lambda f, nb, d: w[:, f] * psi(penalty, d, delta))
    return lam * math.fsum(0.5 * total)


# ---- the value's tree

def block_sums(v):
    """[m, 256] lane values -> [m]: per wavefront of 64 lanes v[l] += v[l + off] for off = 32, 16, ..., 1, then the block's
    four wavefronts added in order from 0 - the header's fixed tree, in float64."""
    w = np.array(v, dtype=np.float64).reshape(-1, 4, 64)
    off = 32
    while off:
        w[:, :, :off] = w[:, :, :off] + w[:, :, off:2 * off]
        off //= 2
    t = np.zeros(len(w))
    for k in range(4):
        t = t + w[:, k, 0]
    return t


def tree_sum(lane_values):
    """The device's sum of one value per cell, cells in the device's order (the caller's under "cell_order" 0): 256 cells
    per block (the last padded with zeros) through block_sums, 256 strided sums over the blocks' partials, each from 0
    (lane j takes partials j, j + 256, ...), and block_sums once more.  TREE_DEPTH(n) additions on the longest path."""
    v = np.asarray(lane_values, dtype=np.float64)
    n_blocks = max(1, -(-len(v) // 256))
    padded = np.zeros(n_blocks * 256)
    padded[:len(v)] = v
    partials = block_sums(padded.reshape(n_blocks, 256))
    s = np.zeros(256)
    for j0 in range(0, n_blocks, 256):
        chunk = partials[j0:j0 + 256]
        s[:len(chunk)] = s[:len(chunk)] + chunk
    return float(block_sums(s[None])[0])


def tree_depth(n_cells):
    """Additions on the longest path from a cell's term to the total: 6 in the wavefront and 4 over the block's wavefronts
    (from 0), ceil(n_blocks / 256) strided over the partials (from 0), and 6 + 4 again."""
    n_blocks = max(1, -(-n_cells // 256))
    return 10 + -(-n_blocks // 256) + 10


def value_terms(w, adj, x, penalty=QUADRATIC, delta=1.0):
    """The cells' halves h_c = 0.5 (((0 + w_0 psi_0) + w_1 psi_1) + ...) as the header forms them, before lambda."""
    w = np.asarray(w, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    total, _ = _sum(adj, x, lambda f, nb, d: w[:, f] * psi(penalty, d, delta))
    return 0.5 * total


def value_tree(w, adj, x, lam, penalty=QUADRATIC, delta=1.0) -> float:
    """R(x) as the device sums it under "cell_order" 0: tree_sum of the cells' halves in the caller's order, lambda last."""
    return lam * tree_sum(value_terms(w, adj, x, penalty, delta))


def dense_laplacian(w, adj, coefficient=None):
    """L [n, n] = sum over interior faces, each once, of k (e_c - e_n)(e_c - e_n)^T with k = w (x coefficient[c, f] where
    given: the pseudo-Huber curvature), assembled entry by entry."""
    n = len(adj)
    L = np.zeros((n, n))
    for c in range(n):
        for f in range(4):
            m = adj[c, f]
            if m < 0 or m < c:
                continue
            k = float(w[c, f]) * (1.0 if coefficient is None else float(coefficient[c, f]))
            L[c, c] += k
            L[m, m] += k
            L[c, m] -= k
            L[m, c] -= k
    return L


# ---- the grids of tests/test_gpu_prior.py: the smallest at which each thing can break

def one_tet():
    return np.array([[0.6, -0.2, -0.1], [1.3, -0.1, 0.0], [0.8, 0.4, 0.1], [0.9, 0.0, 0.5]]), np.array([[0, 1, 2, 3]], dtype=np.int32)


def three_on_a_face():
    """Three tetrahedra on one face: not a manifold, c5_upload_grid keeps no adjacency."""
    xyz = np.array([[0.6, -0.2, 0.0], [1.3, -0.2, 0.0], [0.9, 0.4, 0.0], [0.9, 0.0, 0.5], [0.9, 0.0, -0.5], [1.0, 0.1, 0.3]])
    return xyz, np.array([[0, 1, 2, 3], [0, 1, 2, 4], [0, 1, 2, 5]], dtype=np.int32)


def grids():
    """{name: (xyz, cells)}.  kuhn9's cells are in a random order: the caller's ids are not the device's (Morton order
    starts at 4 096 cells)."""
    out = {"one_tet": one_tet(), "cube8": mg.cube8(), "kuhn4": mg.kuhn_box(4, jitter=0.1)}
    xyz, cells = mg.kuhn_box(9, jitter=0.1)
    out["kuhn9"] = (xyz, cells[np.random.default_rng(5).permutation(len(cells))])
    out["soup"] = mg.per_cell_point_copies(*mg.kuhn_box(2))
    out["interface"] = mg.refined_interface(n=2)[:2]
    return out

"""Random UNSTRUCTURED scenes for the fuzz sweeps (tests/derivative_fuzz.py: derivative_scene(seed, mesh=scene)): graded,
high-valence, relabelled conforming tetrahedral meshes - what tests/fuzz_scenes.py's lattices never are.  numpy and meshgen
only.  scene(seed) returns fuzz_scenes.scene's 7-tuple (xyz, cells, alpha, q, rots, res, limit), deterministic per seed
from default_rng([seed, tag]) streams; tests/test_unstructured_scenes_cpu.py pins digests.

The classes a sweep must see go by the seed, so that any 12 consecutive seeds hold every one of them:
  base     seed % 3: "kuhn" (kuhn_box(2..4), jittered), "star" (an icosahedron subdivided 1..3 times, pushed to a sphere,
           every surface triangle joined to the centre: one point in every one of the 80 / 320 / 1 280 cells), "fan" (n in
           {3, 5, 17, 64, 200} cells about one hub edge, the ring with radial jitter: an edge in n cells, at 200 wedges of 1.8
           degrees);
  size     seed % 4 == 3: a target of 4 500 - 9 000 cells (the Morton pass, tight block spheres), else 300 - 2 500;
  removal  (seed // 3) % 3: "whole"; "cavity" (the cells about a point and a tunnel from it along an axis: rays leave the
           grid and enter it again); "random" (a share keep_p ~ U[0.6, 0.95) of the cells stays).
Operations until the target is reached, each keeping the mesh conforming and every cell positively oriented, and
keeping the volume:
  bisect   (7 in 10) toward a drawn focus - a point inside the bounding box, or (every other scene) one side plane of it: a
           boundary layer.  Of the cells not yet refused the one with the largest longest-edge / (distance of the centroid
           to the focus + floor) x U[0.5, 1) has its longest edge cut at the midpoint - one time in seven a random edge of
           it instead: slivers.  EVERY cell holding both end points is cut, at the one new point.  floor = 10^U[-3, -1.3);
  insert   (3 in 20) a point inside a random cell, barycentric weights >= 0.04: 1 -> 4;
  flip     (3 in 20) a random face of a random cell with a cell behind it: 2 -> 3, if the three new cells have one
           orientation and the new edge is in no other cell.
An operation that would leave a cell below VOLUME_FLOOR x (the base's volume) is refused (and, for bisect, the cell set
aside).  VOLUME_FLOOR = 1e-13 (the bases' cells are 1e-4 .. 2e-2 of it).  It is set against the references alone, by the
share of seeds on which the port oracle and adjoint_reference.segment_lists agree on segment and covered-pixel counts
(derivative_fuzz.qualify): at 1e-13, the first value tried, 57 of the seeds 7000-7059 are used and the other three (7008,
7029, 7053) are left out because the grid reaches the image's border, none for a disagreement - with cells down to 1e-11
of the largest of their scene and edges down to 1 / 7 000 of the longest.  meshgen.validate's 1e-6 of the mean volume would
refuse most of these scenes.  No GPU result went into the value.
Then the removal, and the relabelling: unused points dropped, point ids and the order of the cells permuted, the four
vertices of every cell permuted, orient_positive.  Placement, view, alpha / Q and the limit are drawn as
fuzz_scenes.scene draws them; images are 24-90 x 18-70.

describe(seed): what the scene holds (base, operations, valences, ratios, removal, cells, volumes).
"""
import functools
import hashlib

import numpy as np

from course5_amd import meshgen as mg

BASES = ("kuhn", "star", "fan")
REMOVALS = ("whole", "cavity", "random")
FAN_SIZES = (3, 5, 17, 64, 200)
VOLUME_FLOOR = 1e-13
LARGE = 4096
_EDGES = np.array([(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)])


def _icosphere(level, radius=0.5):
    t = (1.0 + 5.0 ** 0.5) / 2.0
    pts = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
           (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    tri = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
           (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    pts = [np.array(p, np.float64) for p in pts]
    for _ in range(level):
        mid, out = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                mid[key] = len(pts)
                pts.append(0.5 * (pts[a] + pts[b]))
            return mid[key]

        for a, b, c in tri:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        tri = out
    pts = np.array(pts)
    return radius * pts / np.sqrt((pts ** 2).sum(1))[:, None], np.array(tri, np.int64)


def _base(seed, rng):
    kind = BASES[seed % 3]
    if kind == "kuhn":
        xyz, cells = mg.kuhn_box(int(rng.integers(2, 5)), lo=(0.0, 0.0, 0.0), jitter=float(rng.uniform(0.0, 0.15)), seed=seed)
        what = kind
    elif kind == "star":
        level = int(rng.integers(1, 4))
        pts, tri = _icosphere(level)
        xyz = np.vstack([pts, np.zeros((1, 3))])
        cells = np.hstack([np.full((len(tri), 1), len(pts)), tri])
        what = f"star of {len(tri)}"
    else:
        n = int(FAN_SIZES[int(rng.integers(len(FAN_SIZES)))])
        phi = 2.0 * np.pi * np.arange(n) / n
        r = 0.5 * (1.0 + rng.uniform(-0.3, 0.3, n))
        ring = np.stack([r * np.cos(phi), r * np.sin(phi), np.zeros(n)], 1)
        xyz = np.vstack([[0.0, 0.0, -0.5], [0.0, 0.0, 0.5], ring])
        i = np.arange(n)
        cells = np.stack([np.zeros(n, np.int64), np.ones(n, np.int64), 2 + i, 2 + (i + 1) % n], 1)
        what = f"fan of {n}"
    return what, xyz, mg.orient_positive(xyz, np.asarray(cells, np.int64))


class _Mesh:
    """Points and cells in arrays with room to grow, and per cell what the operations ask for again and again."""

    def __init__(self, xyz, cells, room):
        self.n_pts, self.n = len(xyz), len(cells)
        self.x = np.zeros((len(xyz) + room, 3))
        self.x[:self.n_pts] = xyz
        self.c = np.zeros((len(cells) + room, 4), np.int64)
        self.c[:self.n] = cells
        self.vol, self.size, self.cen = np.zeros(len(self.c)), np.zeros(len(self.c)), np.zeros((len(self.c), 3))
        self.refused = np.zeros(len(self.c), bool)
        self.refresh(np.arange(self.n))

    def room_for(self, pts, cells):
        if self.n_pts + pts > len(self.x):
            self.x = np.vstack([self.x, np.zeros_like(self.x)])
        if self.n + cells > len(self.c):
            k = max(len(self.c), cells)
            self.c = np.vstack([self.c, np.zeros((k, 4), np.int64)])
            self.vol, self.size = np.concatenate([self.vol, np.zeros(k)]), np.concatenate([self.size, np.zeros(k)])
            self.cen, self.refused = np.vstack([self.cen, np.zeros((k, 3))]), np.concatenate([self.refused, np.zeros(k, bool)])

    def refresh(self, rows):
        p = self.x[self.c[rows]]
        self.vol[rows] = np.einsum("ij,ij->i", p[:, 1] - p[:, 0], np.cross(p[:, 2] - p[:, 0], p[:, 3] - p[:, 0])) / 6.0
        e = p[:, _EDGES[:, 0]] - p[:, _EDGES[:, 1]]
        self.size[rows] = np.sqrt((e ** 2).sum(-1)).max(1)
        self.cen[rows] = p.mean(1)
        self.refused[rows] = False

    def holding(self, *points):
        c = self.c[:self.n]
        m = (c == points[0]).any(1)
        for p in points[1:]:
            m &= (c == p).any(1)
        return np.flatnonzero(m)


def _bisect(m, rng, focus, floor, min_vol):
    kind, at = focus
    d = np.abs(m.cen[:m.n, at[0]] - at[1]) if kind == "plane" else np.sqrt(((m.cen[:m.n] - at) ** 2).sum(1))
    score = np.where(m.refused[:m.n], -1.0, m.size[:m.n] / (d + floor) * rng.uniform(0.5, 1.0, m.n))
    cell = int(np.argmax(score))
    random_edge = rng.integers(7) == 0
    k = int(rng.integers(6))
    if score[cell] < 0:
        return False
    if not random_edge:
        e = m.x[m.c[cell][_EDGES[:, 0]]] - m.x[m.c[cell][_EDGES[:, 1]]]
        k = int(np.argmax((e ** 2).sum(1)))
    a, b = (int(v) for v in m.c[cell][_EDGES[k]])
    rows = m.holding(a, b)
    if (0.5 * m.vol[rows]).min() < min_vol:
        m.refused[cell] = True
        return False
    m.room_for(1, len(rows))
    new = m.n_pts
    m.x[new] = 0.5 * (m.x[a] + m.x[b])
    m.n_pts += 1
    second = m.c[rows].copy()
    second[second == a] = new  # (new, b, ., .)
    first = m.c[rows]
    first[first == b] = new    # (a, new, ., .): a vertex moved along its own edge keeps the orientation
    m.c[rows] = first
    tail = np.arange(m.n, m.n + len(rows))
    m.c[tail] = second
    m.n += len(rows)
    m.refresh(np.concatenate([rows, tail]))
    return True


def _insert(m, rng, min_vol):
    cell = int(rng.integers(m.n))
    w = 0.04 + 0.84 * rng.dirichlet(np.ones(4))
    if (w * m.vol[cell]).min() < min_vol:
        return False
    m.room_for(1, 3)
    new = m.n_pts
    m.x[new] = w @ m.x[m.c[cell]]
    m.n_pts += 1
    four = np.repeat(m.c[cell][None], 4, 0)
    four[np.arange(4), np.arange(4)] = new  # (a point inside in place of one vertex keeps the orientation)
    rows = np.concatenate([[cell], np.arange(m.n, m.n + 3)])
    m.c[rows] = four
    m.n += 3
    m.refresh(rows)
    return True


def _flip(m, rng, min_vol):
    cell = int(rng.integers(m.n))
    k = int(rng.integers(4))
    d = int(m.c[cell][k])
    a, b, c = (int(v) for v in np.delete(m.c[cell], k))
    pair = m.holding(a, b, c)
    if len(pair) != 2:
        return False  # (a boundary face)
    other = int(pair[pair != cell][0])
    e = int(m.c[other][~np.isin(m.c[other], (a, b, c))][0])
    if len(m.holding(d, e)):
        return False
    three = np.array([(d, e, a, b), (d, e, b, c), (d, e, c, a)], np.int64)
    vol = mg.signed_volumes(m.x, three)
    if not ((vol > 0).all() or (vol < 0).all()) or np.abs(vol).min() < min_vol:
        return False
    m.room_for(0, 1)
    rows = np.array([cell, other, m.n])
    m.c[rows] = mg.orient_positive(m.x, three)
    m.n += 1
    m.refresh(rows)
    return True


def _remove(kind, xyz, cells, rng):
    """The mask of the cells that stay."""
    cen = xyz[cells].mean(1)
    if kind == "whole":
        return np.ones(len(cells), bool)
    if kind == "random":
        return rng.uniform(size=len(cells)) < rng.uniform(0.6, 0.95)
    lo, hi = xyz.min(0), xyz.max(0)
    p = lo + rng.uniform(0.3, 0.7, 3) * (hi - lo)
    r, rt = rng.uniform(0.12, 0.25) * (hi - lo).max(), rng.uniform(0.05, 0.12) * (hi - lo).max()
    axis = int(rng.integers(3))
    side = rng.integers(2) == 0
    off = cen - p
    lateral = np.sqrt((np.delete(off, axis, 1) ** 2).sum(1))
    tunnel = (lateral < rt) & ((off[:, axis] > 0) == side)
    keep = ~((np.sqrt((off ** 2).sum(1)) < r) | tunnel)
    return keep if keep.any() else np.ones(len(cells), bool)


def valences(cells):
    """(the largest number of cells at a point, the largest number of cells round an edge)."""
    cells = np.asarray(cells, np.int64).reshape(-1, 4)
    e = np.sort(cells[:, _EDGES].reshape(-1, 2), 1)
    _u, n_edge = np.unique(e[:, 0] * (int(cells.max()) + 1) + e[:, 1], return_counts=True)
    return int(np.bincount(cells.reshape(-1)).max()), int(n_edge.max())


@functools.lru_cache(maxsize=4)
def _build(seed):
    rng = np.random.default_rng([seed, 0xBA5E])
    what, xyz, cells = _base(seed, rng)
    large = seed % 4 == 3
    target = int(rng.integers(4500, 9001)) if large else int(rng.integers(300, 2501))
    target = max(target, len(cells) + 200)  # (a star of 1 280 or a fan of 200 under a small target: still operated on)
    m = _Mesh(xyz, cells, target)
    base_volume = float(m.vol[:m.n].sum())
    min_vol = VOLUME_FLOOR * base_volume
    # -- operations
    rng = np.random.default_rng([seed, 0x0B5])
    lo, hi = xyz.min(0), xyz.max(0)
    if rng.integers(2) == 0:
        axis = int(rng.integers(3))
        focus = ("plane", (axis, float((lo, hi)[int(rng.integers(2))][axis])))
    else:
        focus = ("point", lo + rng.uniform(0.1, 0.9, 3) * (hi - lo))
    floor = float(10.0 ** rng.uniform(-3.0, -1.3))
    ops = {"bisect": 0, "insert": 0, "flip": 0, "refused": 0}
    for _ in range(40 * target):
        if m.n >= target:
            break
        u = rng.uniform()
        name = "bisect" if u < 0.7 else "insert" if u < 0.85 else "flip"
        done = (_bisect(m, rng, focus, floor, min_vol) if name == "bisect" else _insert(m, rng, min_vol) if name == "insert"
                else _flip(m, rng, min_vol))
        ops[name if done else "refused"] += 1
    xyz, cells = m.x[:m.n_pts].copy(), m.c[:m.n].copy()
    # -- removal
    rng = np.random.default_rng([seed, 0x2E3])
    removal = REMOVALS[(seed // 3) % 3]
    keep = _remove(removal, xyz, cells, rng)
    removed_volume = float(m.vol[:m.n][~keep].sum())
    cells = cells[keep]
    # -- relabelling
    rng = np.random.default_rng([seed, 0x1D5])
    used = np.unique(cells)
    new_id = np.full(len(xyz), -1, np.int64)
    new_id[used] = rng.permutation(len(used))
    moved = np.empty((len(used), 3))
    moved[new_id[used]] = xyz[used]
    xyz = moved
    cells = new_id[cells][rng.permutation(len(cells))]
    cells = np.take_along_axis(cells, np.argsort(rng.uniform(size=cells.shape), 1), 1)
    # -- placement, view, scalars: as fuzz_scenes.scene
    rng = np.random.default_rng([seed, 0x5CE])
    scale = rng.uniform(0.3, 0.9, 3)
    xyz = (xyz - xyz.mean(0)) * scale + np.array([1.0, 0.0, 0.0]) + rng.uniform(-0.15, 0.15, 3)
    cells = mg.orient_positive(xyz, cells).astype(np.int32)
    alpha = rng.uniform(0, 5, len(cells))
    alpha[rng.uniform(size=len(cells)) < 0.1] = 0.0
    q = rng.uniform(0, 2, len(cells))
    rots = mg.view_rotations(rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-1, 1))
    res = (int(rng.integers(24, 91)), int(rng.integers(18, 71)))
    limit = float(rng.uniform(0.5, 6))
    # -- what it holds
    vol = mg.signed_volumes(xyz, cells)
    e = xyz[cells[:, _EDGES[:, 0]]] - xyz[cells[:, _EDGES[:, 1]]]
    length = np.sqrt((e ** 2).sum(-1))
    point_valence, edge_valence = valences(cells)
    info = {"base": BASES[seed % 3], "base_detail": what, "operations": ops, "focus": focus[0], "removal": removal,
            "cells": len(cells), "points": len(xyz), "point_valence": point_valence, "edge_valence": edge_valence,
            "edge_ratio": float(length.max() / length.min()), "volume_ratio": float(vol.max() / vol.min()),
            "base_volume": base_volume * float(np.prod(scale)), "removed_volume": removed_volume * float(np.prod(scale))}
    for a in (xyz, cells, alpha, q, rots):
        a.setflags(write=False)
    return (xyz, cells, alpha, q, rots, res, limit), info


def scene(seed):
    xyz, cells, alpha, q, rots, res, limit = _build(int(seed))[0]
    return xyz.copy(), cells.copy(), alpha.copy(), q.copy(), rots.copy(), res, limit


def describe(seed):
    return dict(_build(int(seed))[1])


def describe_line(seed):
    d = describe(seed)
    o = d["operations"]
    return (f"{d['base_detail']}, {d['cells']} cells, {o['bisect']} bisections toward a {d['focus']}, {o['insert']} insertions, "
            f"{o['flip']} flips ({o['refused']} refused), removal {d['removal']}, a point in {d['point_valence']} cells, an edge in "
            f"{d['edge_valence']}, edge ratio {d['edge_ratio']:.3g}, volume ratio {d['volume_ratio']:.3g}")


def digest(seed):
    """sha256 over the bytes of scene(seed)'s arrays and scalars, as fuzz_scenes.digest."""
    xyz, cells, alpha, q, rots, res, limit = scene(seed)
    h = hashlib.sha256()
    for a, dt in ((xyz, np.float64), (cells, np.int64), (alpha, np.float64), (q, np.float64), (rots, np.float64),
                  (res, np.int64), ([limit], np.float64)):
        a = np.ascontiguousarray(np.asarray(a, dtype=dt))
        h.update(str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()

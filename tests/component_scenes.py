"""Random scenes of SEVERAL COMPONENTS for the fuzz sweeps (tests/derivative_fuzz.py: derivative_scene(seed, mesh=scene)): two or
three Kuhn lattices that share no point id and no face, placed apart, touching, nested or interpenetrating - what decides
between the walk and bin_sort_resolve (csrc/walk_common.hpp: next_entry; a ray that meets a boundary entry inside a stretch
of cells it has walked is `skipped`, the host answers C5_RETRY and renders the grid from sorted lists from then on).  numpy,
meshgen and the numpy restatement adjoint_reference.segment_lists only.  scene(seed) returns fuzz_scenes.scene's 7-tuple (xyz, cells, alpha, q, rots, res, limit), deterministic per
seed from default_rng([seed, tag]) streams; tests/test_component_scenes_cpu.py pins digests.

The class goes by seed % 8 (CLASSES), so that any 8 consecutive seeds hold every one of them.  Part A is kuhn_box(n) on the
unit cube of a LOCAL frame, its interior points jittered (its sides stay planar); B is another one, scaled per axis, turned
and placed against A's side `side` (x = 1 or x = 0 of the local frame):
  apart     B's facing side parallel to A's at a gap of 2^U[-30, -2) of the local diagonal (gaps below the entry-key slack
            s included), shifted sideways so that the two sides overlap in part;
  abutting  the same at a gap of exactly 0: the facing points have the SAME local x, and the maps that follow act on it alone,
            so the two sides are coplanar to the bit before the view.  B's lattice does not match A's (another n, or a
            sideways shift and size that are no multiple of A's cell);
  nested    A has n in {3, 4} and loses its central cube (n = 3) or its central 2 x 2 x 2 cubes (n = 4) through keep=; B is a
            cube turned by up to 0.3 rad about a random axis, small enough to touch none of the (jittered) cavity walls;
  deep      B turned by up to 0.5 rad and pushed into A through the side by 5 - 50 % of its extent along x;
  enclosed  B a cube of 0.2 - 0.5 of A's size (0.2 - 0.3 in a scene of three), turned by up to 0.5 rad, wholly inside A;
  flush     B inside A, one of its sides IN A's side plane (the same local x), turned about x by up to 0.5 rad;
  window    the local frame is the VIEW's (the view is drawn first; local x is the view's z, and the scene is turned back
            into object space with the inverse of the view): unjittered facing sides at right angles to the rays, B's behind
            A's by t x s along z, t = WINDOW_T[(seed // 8) % 6] - either side of the two slacks up to which next_entry takes
            an entry that lies inside the stretch just walked, and beyond which it flags it;
  three     three parts: B against x = 1 and C against x = 0 of A, each pair of a class drawn from apart, abutting, deep,
            enclosed and flush (nested has one cavity in the middle of A and window one frame for the whole scene: they stay
            scenes of two).
Parts are kuhn_box(2..4), redrawn until the scene holds 100 - 800 cells.  Elsewhere than in `window` the local axes are permuted
and the scene is scaled per axis by U[0.3, 0.9) about its centroid and put at (1, 0, 0) + U[-0.15, 0.15)^3 as fuzz_scenes.scene
does; every scene is then shrunk about (1, 0, 0), if need be, into a ball of radius 0.8 - every view turns the grid about
axes through that point, the image spans [-0.2, 2.2] x [-0.9, 0.9] and a pixel of the smallest image is 0.083 x 0.078, so the
grid stays a pixel inside the border under any view (derivative_fuzz.qualify).  All of these maps act on each coordinate alone:
points with one local x keep one x.  alpha / Q, the view and the limit are drawn as fuzz_scenes.scene draws them; images are
30-100 x 24-80.

slack(xyz) restates the frame's entry-key slack (csrc/grid.hip: measure_grid; csrc/frame.hip: entry_key_slack):
2^-24 x the diagonal of the bounding box + 2^-40 x (the largest |coordinate| + 2).

describe(seed): the class, the parts, the placement, and from adjoint_reference.segment_lists alone the rays on which two
segments overlap by more than 1e-13 x the diagonal, the largest overlap in units of s, the rays with a gap between two
parts, the exact ties of z_hi within a pixel; `overlapping`: some ray overlaps by more than 2 s.
"""
import functools
import hashlib

import numpy as np

from course5_amd import meshgen as mg
from tests import adjoint_reference as ar

CLASSES = ("apart", "abutting", "nested", "deep", "enclosed", "flush", "window", "three")
THREE_CLASSES = ("apart", "abutting", "deep", "enclosed", "flush")
WINDOW_T = (0.25, 0.75, 1.25, 1.75, 3.0, 16.0)
MIN_CELLS, MAX_CELLS = 100, 800
RADIUS = 0.8
MIN_RAYS = 8      # rays that must show a class's overlap
MAX_ATTEMPTS = 32
ROUNDING = 1e-13  # x the diagonal: what two evaluations of one plane may differ by, with room


def slack(xyz):
    """The frame's entry-key slack s of a grid with these points (object space)."""
    xyz = np.asarray(xyz, np.float64)
    d = xyz.max(0) - xyz.min(0)
    return 2.0 ** -24 * float(np.sqrt((d * d).sum())) + 2.0 ** -40 * (float(np.abs(xyz).max()) + 2.0)


def unrotate(p, rots):
    """The inverse of adjoint_reference.rotate: view space -> object space."""
    p = np.array(p, np.float64).reshape(-1, 3)
    for axis, angle, x0 in np.asarray(rots, np.float64).reshape(-1, 3)[::-1]:
        co, si = np.cos(-angle), np.sin(-angle)
        if int(axis) == 0:
            y, z = p[:, 1].copy(), p[:, 2].copy()
            p[:, 1], p[:, 2] = y * co - z * si, y * si + z * co
        else:
            x, z = p[:, 0] - x0, p[:, 2].copy()
            p[:, 0], p[:, 2] = x * co - z * si + x0, x * si + z * co
    return p


def _rotation(axis, angle):
    """Rodrigues: the matrix turning by `angle` about the unit vector `axis`."""
    k = np.asarray(axis, np.float64)
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def _turned(u, size, R):
    """The unit-cube points u scaled per axis about the cube's centre and turned by R: centred at 0."""
    return ((u - 0.5) * size) @ R.T


def _against(x_extent_lo, x_extent_hi, side, at):
    """The shift along x that puts a centred part's near side (its far side for side 0) at local x = at."""
    return at - x_extent_lo if side == 1 else at - x_extent_hi


def _place(kind, rng, side, u, in_three, overlap=0.0):
    """Part B's points in A's local frame (A: the unit cube) for the unit-cube lattice points u, and what was drawn."""
    wall = float(side)  # local x of A's side
    out = 1.0 if side == 1 else -1.0
    if kind in ("apart", "abutting", "window"):
        size = rng.uniform(0.4, 0.9, 3)
        centre = rng.uniform(0.2, 0.8, 2)
        gap = 0.0
        if kind == "apart":
            gap = 2.0 ** rng.uniform(-30.0, -2.0) * 3.0  # (the local diagonal of two boxes side by side is about 3)
        if kind == "window":
            gap = -overlap
        near = wall + out * gap
        # the facing points are those with u_x == 0: near + 0 * size is `near` itself, to the bit
        p = np.empty_like(u)
        p[:, 0] = near + out * (u[:, 0] * size[0])
        p[:, 1:] = centre + (u[:, 1:] - 0.5) * size[1:]
        return p, dict(size=size.tolist(), lateral=centre.tolist(), gap=gap)
    if kind == "flush":
        size = rng.uniform(0.25, 0.5, 3)
        angle = float(rng.uniform(-0.5, 0.5))
        co, si = np.cos(angle), np.sin(angle)
        half = 0.5 * (abs(co) + abs(si)) * max(size[1], size[2]) + 0.03
        centre = rng.uniform(half, 1.0 - half, 2)
        v = (u[:, 1:] - 0.5) * size[1:]
        p = np.empty_like(u)
        p[:, 0] = wall - out * (u[:, 0] * size[0])  # (u_x == 0: in A's side plane, to the bit)
        p[:, 1] = centre[0] + v[:, 0] * co - v[:, 1] * si
        p[:, 2] = centre[1] + v[:, 0] * si + v[:, 1] * co
        return p, dict(size=size.tolist(), lateral=centre.tolist(), angle=angle)
    axis = rng.normal(size=3)
    axis /= np.sqrt((axis * axis).sum())
    if kind == "deep":
        size = rng.uniform(0.4, 0.8, 3)
        angle = float(rng.uniform(0.05, 0.5)) * (1.0 if rng.integers(2) else -1.0)
        q = _turned(u, size, _rotation(axis, angle))
        lo, hi = q[:, 0].min(), q[:, 0].max()
        depth = float(rng.uniform(0.05, 0.5))
        shift = _against(lo, hi, side, wall - out * depth * (hi - lo))
        q[:, 0] += shift
        lateral = rng.uniform(0.25, 0.75, 2)
        q[:, 1:] += lateral
        return q, dict(size=size.tolist(), angle=angle, depth=depth, lateral=lateral.tolist())
    if kind == "enclosed":
        b = float(rng.uniform(0.2, 0.3 if in_three else 0.5))
        angle = float(rng.uniform(-0.5, 0.5))
        q = _turned(u, np.full(3, b), _rotation(axis, angle))
        half = np.abs(q).max(0) + 0.02
        lo, hi = half.copy(), 1.0 - half
        if in_three:  # B in the half of A behind its side
            lo[0], hi[0] = (0.5 + half[0], 1.0 - half[0]) if side == 1 else (half[0], 0.5 - half[0])
        assert (hi >= lo).all()
        centre = lo + rng.uniform(0.0, 1.0, 3) * (hi - lo)
        return q + centre, dict(size=b, angle=angle, centre=centre.tolist())
    raise ValueError(kind)


def _nested(rng, n_a, jitter_a, u):
    """B inside the cavity of A (_cavity): a cube whose half diagonal fits between the jittered walls."""
    h = 1.0 / n_a
    c = h if n_a == 3 else 2.0 * h
    b = 2.0 * (0.5 * c - jitter_a * h) * 0.9 / np.sqrt(3.0)
    axis = rng.normal(size=3)
    axis /= np.sqrt((axis * axis).sum())
    angle = float(rng.uniform(-0.3, 0.3))
    room = (0.5 * c - jitter_a * h) * 0.1
    centre = 0.5 + rng.uniform(-room, room, 3) / np.sqrt(3.0)
    return _turned(u, np.full(3, b), _rotation(axis, angle)) + centre, dict(size=float(b), angle=angle, centre=centre.tolist())


def _cavity(n_a):
    lo, hi = (1.0 / 3.0, 2.0 / 3.0) if n_a == 3 else (0.25, 0.75)
    return lambda cen: ~((cen > lo) & (cen < hi)).all(1)


def _part(n, jitter, seed, keep=None):
    xyz, cells = mg.kuhn_box(n, lo=(0.0, 0.0, 0.0), size=1.0, jitter=jitter, seed=seed, keep=keep)
    return xyz, np.asarray(cells, np.int64)


def _fit(p):
    """Shrunk about (1, 0, 0), if need be, into the ball of radius RADIUS."""
    c = np.array([1.0, 0.0, 0.0])
    r = float(np.sqrt(((p - c) ** 2).sum(1)).max())
    return p if r <= RADIUS else (p - c) * (RADIUS / (r * (1.0 + 1e-12))) + c


@functools.lru_cache(maxsize=128)
def _build(seed):
    kind = CLASSES[seed % 8]
    # -- the parts
    rng = np.random.default_rng([seed, 0xC0B])
    pairs = [kind]
    if kind == "three":
        pairs = [THREE_CLASSES[int(rng.integers(len(THREE_CLASSES)))] for _ in range(2)]
    while True:
        n = [int(rng.integers(3 if kind == "nested" else 2, 5))] + [int(rng.integers(2, 5)) for _ in pairs]
        jitter = [0.0 if kind == "window" else float(rng.uniform(0.0, 0.15)) for _ in n]
        a_xyz, a_cells = _part(n[0], jitter[0], seed, _cavity(n[0]) if kind == "nested" else None)
        total = len(a_cells) + sum(6 * k ** 3 for k in n[1:])
        if MIN_CELLS <= total <= MAX_CELLS:
            break
    first_side = int(rng.integers(2))
    t = WINDOW_T[(seed // 8) % len(WINDOW_T)] if kind == "window" else None
    perm = rng.permutation(3)
    if kind == "window":  # the local frame is the view's, local x its z
        perm = np.array([1, 2, 0])
    ax = int(np.flatnonzero(perm == 0)[0])  # where local x went
    def assemble(attempt, overlap_local):
        prng = np.random.default_rng([seed, 0x91A, attempt])
        pts, cls, part, placed = [a_xyz], [a_cells], [np.zeros(len(a_cells), np.int64)], []
        for j, pair in enumerate(pairs):
            side = first_side if j == 0 else 1 - first_side
            u, c = _part(n[j + 1], jitter[j + 1], seed + 7919 * (j + 1))
            if pair == "nested":
                p, what = _nested(prng, n[0], jitter[0], u)
            else:
                p, what = _place(pair, prng, side, u, kind == "three", overlap_local)
            what.update({"class": pair, "side": side})
            placed.append(what)
            cls.append(c + sum(len(x) for x in pts))
            part.append(np.full(len(c), j + 1, np.int64))
            pts.append(p)
        scale, offset = prng.uniform(0.3, 0.9, 3), prng.uniform(-0.15, 0.15, 3)
        local = np.vstack(pts)[:, perm]
        world = _fit((local - local.mean(0)) * scale + np.array([1.0, 0.0, 0.0]) + offset)
        shrink = float((world[:, ax].max() - world[:, ax].min()) / (local[:, ax].max() - local[:, ax].min()))
        if kind == "window":
            world = unrotate(world, rots)
        return world, np.vstack(cls), np.concatenate(part), placed, shrink

    # The view and the placement, with the scale and the offset, are drawn again (streams [seed, 0x71E / 0x91A, attempt]) until the reference's own lists show what the class is for
    # (_accept): a handful of rays in the overlap, and no two segments of a pixel with one z_hi (coplanar sides of two parts
    # evaluate to the same double on about one ray in a hundred; the reference's order of the two is then its sort's).
    for attempt in range(MAX_ATTEMPTS):
        # the view, image and limit (window places B in view space: drawn first, for every class)
        vrng = np.random.default_rng([seed, 0x71E, attempt])
        rots = mg.view_rotations(vrng.uniform(-1, 1), vrng.uniform(-1, 1), vrng.uniform(-1, 1))
        res = (int(vrng.integers(30, 101)), int(vrng.integers(24, 81)))
        limit = float(vrng.uniform(0.5, 6))
        xyz, cells, part, placed, shrink = assemble(attempt, 0.0)
        if kind == "window":
            # t x s along the view's z is t x s / (world extent / local extent) of the local frame; s from the grid as placed without the
            # overlap (the overlap changes the diagonal by 1e-7 of itself)
            xyz, cells, part, placed, shrink = assemble(attempt, t * slack(xyz) / shrink)
        diagonal = float(np.sqrt(((xyz.max(0) - xyz.min(0)) ** 2).sum()))
        stats = ray_statistics(ar.segment_lists(xyz, cells, rots, res[0], res[1], mg.REFERENCE_BOUNDS), part, slack(xyz), diagonal)
        if _accept(kind, t, stats):
            break
    else:
        raise RuntimeError(f"seed {seed} ({kind}): no placement in {MAX_ATTEMPTS} draws")
    cells = mg.orient_positive(xyz, cells).astype(np.int32)
    # -- scalars: as fuzz_scenes.scene
    rng = np.random.default_rng([seed, 0x5CA])
    alpha = rng.uniform(0, 5, len(cells))
    alpha[rng.uniform(size=len(cells)) < 0.1] = 0.0
    q = rng.uniform(0, 2, len(cells))
    info = {"class": kind, "pairs": list(pairs), "parts": [dict(n=k, jitter=j, cells=int((part == i).sum())) for i, (k, j) in
                                                          enumerate(zip(n, jitter))],
            "placement": placed, "attempts": attempt + 1, "t": t, "cells": len(cells), "points": len(xyz), "slack": slack(xyz),
            "diagonal": diagonal}
    info.update(stats)
    for a in (xyz, cells, alpha, q, rots, part):
        a.setflags(write=False)
    return (xyz, cells, alpha, q, rots, res, limit), info, part


def scene(seed):
    xyz, cells, alpha, q, rots, res, limit = _build(int(seed))[0]
    return xyz.copy(), cells.copy(), alpha.copy(), q.copy(), rots.copy(), res, limit


def part_of_cell(seed):
    """The part (0 = A) every cell belongs to."""
    return _build(int(seed))[2].copy()


def ray_statistics(segments, part, s, diagonal):
    """From adjoint_reference.segment_lists' (pixel, cell, z_hi, dz), sorted by pixel and ascending z_hi: per pair of
    consecutive segments of a pixel, how far the earlier one's z_hi lies above the later one's lower end (no more than either
    chord).  -> dict(overlap_rays, max_overlap_in_s, overlaps_in_s (the largest per overlapping ray), gap_rays, ties,
    overlapping)."""
    pix, cell, zh, dz = (np.asarray(a) for a in segments[:4])
    same = pix[1:] == pix[:-1]
    over = np.minimum(np.minimum(zh[:-1] - (zh[1:] - dz[1:]), dz[:-1]), dz[1:])
    over = np.where(same, over, -np.inf)
    hit = over > ROUNDING * diagonal
    per_ray = np.zeros(int(pix.max()) + 1 if len(pix) else 0)
    np.maximum.at(per_ray, pix[1:][hit], over[hit])
    rays = per_ray[per_ray > 0] / s
    other = part[cell[1:]] != part[cell[:-1]]
    gap = same & other & ((zh[1:] - dz[1:]) - zh[:-1] > ROUNDING * diagonal)
    return dict(overlap_rays=int(len(rays)), max_overlap_in_s=float(rays.max()) if len(rays) else 0.0, overlaps_in_s=rays,
                gap_rays=int(len(np.unique(pix[1:][gap]))), ties=int((same & (zh[1:] == zh[:-1])).sum()),
                overlapping=bool(len(rays) and rays.max() > 2.0))


def _accept(kind, t, stats):
    """What a placement must show in the reference's lists to be the scene of its seed (the class predicates that tests/
    test_component_scenes_cpu.py asserts of every scene)."""
    over = stats["overlaps_in_s"]
    if stats["ties"]:
        return False
    if kind in ("deep", "enclosed", "flush"):
        return int((over > 4.0).sum()) >= MIN_RAYS
    if kind == "window":
        return int((np.abs(over - t) <= 0.1 * t).sum()) >= MIN_RAYS and not (over > 2.0 * t).any()
    return True


def describe(seed):
    return dict(_build(int(seed))[1])


def describe_line(seed):
    d = describe(seed)
    what = d["class"] + (f" (t = {d['t']})" if d["t"] is not None else "") + (f" ({' + '.join(d['pairs'])})" if d["class"] == "three" else "")
    return (f"{what}, parts of {' + '.join(str(p['cells']) for p in d['parts'])} cells, {d['overlap_rays']} rays overlap (at most "
            f"{d['max_overlap_in_s']:.3g} s), {d['gap_rays']} rays with a gap between parts, {d['ties']} ties"
            f"{', OVERLAPPING' if d['overlapping'] else ''}")


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

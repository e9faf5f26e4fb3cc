"""The random scenes of the fuzz sweeps (tests/fuzz_parity.py, tests/derivative_fuzz.py): numpy and meshgen only, so
that CPU tests can draw them too.  tests/test_derivative_references_cpu.py pins a digest of scene(seed): the scenes of a
seed must not change.

Scenes: jittered Kuhn boxes with random cells removed (holes, non-convex, disconnected parts); every fifth scene
a coarse box against a 2x-refined one (hanging nodes all over the interface, crumpled or planar, ids shared or
not) with a few more cells cut at an edge midpoint, moved by an affine map that leaves the hanging nodes on their
faces only to rounding;
random anisotropic scaling / placement inside the domain, random views, scalars including zeros
and values above the clamp, random image sizes.
"""
import numpy as np

from course5_amd import meshgen as mg

# (lds_stage, integration, tile); the first one is the product default
# lds_stage 3 here: LDS-DMA staging with 21 slots ("stage_slots" 21)
VARIANTS = ((2, 0, 3), (1, 0, 0), (2, 1, 3), (0, 0, 1), (2, 0, 1), (0, 1, 0), (1, 1, 1), (3, 0, 3), (1, 0, 2), (3, 1, 1), (2, 0, 0), (2, 0, 2), (1, 1, 3), (0, 0, 3))


def scene(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 8))
    dense = seed % 5 == 4  # cells smaller than a pixel: every lane of a wavefront in a cell of its own
    if dense:
        n = int(rng.integers(10, 19))
    keep_p = rng.uniform(0.55, 1.0)
    if seed % 5 == 3:  # conforming in space, not in connectivity (SURVEY f-4)
        xyz, cells, _ = mg.refined_interface(int(rng.integers(2, 6)), int(rng.integers(1, 4)), int(rng.integers(1, 5)),
                                             lo=(0.0, 0.0, 0.0), size=1.0, jitter=float(rng.uniform(0, 0.15)),
                                             warp=float(rng.choice([0.0, 0.05, 0.12])), seed=seed, weld=bool(rng.integers(0, 2)))
        for _ in range(int(rng.integers(0, 4))):
            e = rng.choice(4, 2, replace=False)
            xyz, cells = mg.split_cell_at_edge_midpoint(xyz, cells, int(rng.integers(0, len(cells))), (int(e[0]), int(e[1])))
    else:
        xyz, cells = mg.kuhn_box(n, jitter=float(rng.uniform(0, 0.15)), seed=seed,
                                 keep=(lambda cen: rng.uniform(size=len(cen)) < keep_p) if keep_p < 0.98 else None)
    # anisotropic scale + shift, staying inside x in [-0.2, 2.2], y in [-0.9, 0.9] after any rotation about (1,0,0)
    c = xyz.mean(axis=0)
    scale = rng.uniform(0.3, 0.9, 3)
    xyz = (xyz - c) * scale + np.array([1.0, 0.0, 0.0]) + rng.uniform(-0.15, 0.15, 3)
    cells = mg.orient_positive(xyz, cells)
    alpha = rng.uniform(0, 5, len(cells))
    alpha[rng.uniform(size=len(cells)) < 0.1] = 0.0
    q = rng.uniform(0, 2, len(cells))
    rots = mg.view_rotations(rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-1, 1))
    res = (int(rng.integers(30, 500)), int(rng.integers(30, 400)))
    if dense:
        res = (int(rng.integers(24, 90)), int(rng.integers(18, 70)))
    limit = float(rng.uniform(0.5, 6))
    return xyz, cells, alpha, q, rots, res, limit


def digest(seed):
    """sha256 over the bytes of scene(seed)'s arrays and scalars (what the CPU test pins)."""
    import hashlib
    xyz, cells, alpha, q, rots, res, limit = scene(seed)
    h = hashlib.sha256()
    for a, dt in ((xyz, np.float64), (cells, np.int64), (alpha, np.float64), (q, np.float64), (rots, np.float64),
                  (res, np.int64), ([limit], np.float64)):
        a = np.ascontiguousarray(np.asarray(a, dtype=dt))
        h.update(str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()

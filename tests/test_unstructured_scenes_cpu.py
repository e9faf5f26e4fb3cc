"""tests/unstructured_scenes.py without a GPU: the scenes pinned by digest; every mesh of the first 60 seeds conforming,
positively oriented and of the base's volume less the removed cells'; the share of them the references agree on
(derivative_fuzz.qualify with the port oracle); the classes the family exists for, counted over the used seeds; and the
numpy restatements held to the 80-digit reference on a graded, a star and a fan scene (tests/
test_derivative_references_cpu.py's machinery and bars, the same pixel subsampling) - on sliver chords at edge ratios the
lattice scenes never had.
"""
import numpy as np
import pytest

from course5_amd import meshgen as mg
from tests import adjoint_reference as ar
from tests import derivative_fuzz as df
from tests import test_derivative_references_cpu as refs
from tests import unstructured_scenes as us

FIRST, N_SEEDS = 7000, 60
TILE = 8
MAX_STAGED = 21  # the most cells a walk step stages ("stage_slots" 21)

DIGESTS = {
    7000: "cabd272239bf1db1a844865454e2dea9b0701f3ee25ea2190c79a0c97b64f3a7",
    7001: "5f8d01c37b0e4eb693d6ea38289cef1b50b574128987be1ebdba8217d003d262",
    7002: "b41b2da931986525571596dffe6f941e3e695a3c246cb4177106f73c6a3a8174",
    7003: "f2c23535410dd008e96e696f2cf139d17e34f2d190e0638362e63cc96d8a177e",
    7004: "33e7b957da2629e868e0fbddba9d1722090eb4c2104e3cec7a5645115205c1c4",
    7005: "e7a1111b5769a5f07f55cb6ed869d02dac54392d1968b60512b807edf8a6f5d3",
    7006: "bfa0b9916eb2ab0191dcae4db9e340781973eb879b6d581ee560fb9a51ae27ba",
    7007: "02ffd888369e15faba5791b1c39bafb9a6ffc827ce4fa9a13ed756aa956c0d6e",
    7008: "f0c8b199855c7a30b0b7f6ca1cb9a1da5525aaa5d7aef87676b924fec531472c",
    7009: "fa23335c9aa33db9fb43b5a403c38ddc25c833532a17557f278b55532cfe00d7",
}


@pytest.mark.parametrize("seed", sorted(DIGESTS))
def test_the_unstructured_scenes_have_not_changed(seed):
    assert us.digest(seed) == DIGESTS[seed]


def test_the_classes_go_by_the_seed():
    for seed in range(FIRST, FIRST + 12):
        d = us.describe(seed)
        assert d["base"] == us.BASES[seed % 3] and d["removal"] == us.REMOVALS[(seed // 3) % 3]
        if d["removal"] == "whole":  # (what a removal leaves of a large scene is the draw's)
            assert (d["cells"] >= us.LARGE) == (seed % 4 == 3)
        rx, ry = us.scene(seed)[5]
        assert 24 <= rx <= 90 and 18 <= ry <= 70


def _frame_classes(s):
    """From the reference's segments of the whole frame: (pixels with a gap between consecutive segments, the most distinct
    cells the rays of one 8x8 tile are in at one step along them, whether the rays of some tile with a covered pixel are in
    no more than 2 cells in all - at these image sizes a tile on the silhouette, where a coarse cell ends)."""
    pix, cell, zh, dz = s.segments[:4]
    rx, ry = s.res
    same = pix[1:] == pix[:-1]
    reentering = len(np.unique(pix[1:][same & ((zh[1:] - dz[1:]) - zh[:-1] > 1e-6)]))
    first = np.flatnonzero(np.concatenate([[True], ~same]))
    rank = np.arange(len(pix)) - np.repeat(first, np.diff(np.concatenate([first, [len(pix)]])))
    tiles_x = -(-rx // TILE)
    tile = (pix // rx // TILE) * tiles_x + pix % rx // TILE
    n_cells = int(cell.max()) + 1
    at_depth = np.unique((tile * (int(rank.max()) + 1) + rank) * n_cells + cell) // n_cells  # one entry per (tile, step, cell)
    widest = int(np.unique(at_depth, return_counts=True)[1].max())
    in_tile = np.unique(tile * n_cells + cell) // n_cells
    narrow = bool((np.unique(in_tile, return_counts=True)[1] <= 2).any())
    return reentering, widest, narrow


class _Family:
    """The first 60 scenes, each built and qualified once."""

    def __init__(self, oracle):
        self.oracle, self.rows = oracle, None

    def all(self):
        if self.rows is None:
            self.rows = []
            for seed in range(FIRST, FIRST + N_SEEDS):
                s = df.derivative_scene(seed, us.scene)
                why = df.qualify(s, self.oracle)
                d = us.describe(seed)
                d.update(seed=seed, why=why)
                if why is None:
                    d["reentering"], d["widest"], d["narrow"] = _frame_classes(s)
                self.rows.append(d)
                print(f"seed {seed}: {us.describe_line(seed)}; {s.res[0]}x{s.res[1]}, {len(s.segments[0])} segments"
                      + (f"; rays re-enter at {d['reentering']} pixels, at most {d['widest']} cells of a tile at one step"
                         f"{', a tile in <= 2 cells' if d['narrow'] else ''}" if why is None else f" - not used: {why}"))
        return self.rows


@pytest.fixture(scope="module")
def family(oracle_port):
    return _Family(oracle_port)


def test_every_mesh_is_conforming_positive_and_of_the_right_volume():
    for seed in range(FIRST, FIRST + N_SEEDS):
        xyz, cells = us.scene(seed)[:2]
        d = us.describe(seed)
        c = np.sort(np.asarray(cells, np.int64), 1)
        assert len(np.unique(c, axis=0)) == len(c), (seed, "duplicate cells")
        assert (c[:, 1:] != c[:, :-1]).all(), (seed, "a cell names a point twice")
        faces = np.concatenate([c[:, [0, 1, 2]], c[:, [0, 1, 3]], c[:, [0, 2, 3]], c[:, [1, 2, 3]]])  # (rows stay sorted)
        _f, count = np.unique(faces, axis=0, return_counts=True)
        assert count.max() <= 2, (seed, "a face in more than two cells")
        vol = mg.signed_volumes(xyz, cells)
        assert (vol > 0).all(), (seed, "orientation")
        assert np.array_equal(np.unique(cells), np.arange(len(xyz))), (seed, "unused points")
        want = d["base_volume"] - d["removed_volume"]
        assert abs(vol.sum() - want) <= 1e-12 * want, (seed, vol.sum(), want)
        # two cells on one face lie on opposite sides of it (with the counts above: no overlap across a shared face)
        order = np.lexsort(faces.T[::-1])
        fs = faces[order]
        twin = np.flatnonzero((fs[1:] == fs[:-1]).all(1))
        owner = (order % len(c))
        a, b = owner[twin], owner[twin + 1]
        p = xyz[fs[twin]]
        normal = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        side = lambda k: np.einsum("ij,ij->i", normal, xyz[np.asarray(cells, np.int64)[k]].mean(1) - p[:, 0])  # noqa: E731
        assert (side(a) * side(b) < 0).all(), (seed, "two cells on the same side of a shared face")


def test_the_references_agree_on_nine_scenes_in_ten(family):
    used = [d for d in family.all() if d["why"] is None]
    print(f"{len(used)} of {N_SEEDS} seeds used; not used: " + "; ".join(f"{d['seed']} ({d['why']})" for d in family.all() if d["why"]))
    assert len(used) >= 0.9 * N_SEEDS


def test_the_used_scenes_cover_every_class(family):
    used = [d for d in family.all() if d["why"] is None]
    counts = {f"base {b}": sum(d["base"] == b for d in used) for b in us.BASES}
    counts.update({f"removal {r}": sum(d["removal"] == r for d in used) for r in us.REMOVALS})
    counts["a point in >= 64 cells"] = sum(d["point_valence"] >= 64 for d in used)
    counts["an edge in >= 32 cells"] = sum(d["edge_valence"] >= 32 for d in used)
    counts["edge ratio >= 200"] = sum(d["edge_ratio"] >= 200 for d in used)
    counts[f">= {us.LARGE} cells"] = sum(d["cells"] >= us.LARGE for d in used)
    counts["re-entering rays"] = sum(d["reentering"] > 0 for d in used)
    counts["a wide and a narrow tile in one frame"] = sum(d["widest"] > MAX_STAGED and d["narrow"] for d in used)
    print(counts)
    print("largest: a point in", max(d["point_valence"] for d in used), "cells, an edge in", max(d["edge_valence"] for d in used),
          f"edge ratio {max(d['edge_ratio'] for d in used):.3g}, volume ratio {max(d['volume_ratio'] for d in used):.3g}, "
          f"{max(d['cells'] for d in used)} cells")
    assert all(v >= 3 for v in counts.values()), counts


# ---- the restatements against 80 digits on the new family ---------------------------------------------------------------

# graded (a Kuhn box refined toward a side plane: a boundary layer), a star, a fan of 64
SEEDS = {"graded": 7035, "star": 7009, "fan": 7052}
GEOMETRY_SEED = 7049  # a fan of 200: wedges of 1.8 degrees


@pytest.mark.parametrize("kind", sorted(SEEDS))
def test_restatements_against_80_digits(kind, oracle_port):
    seed = SEEDS[kind]
    d = us.describe(seed)
    assert d["base"] == {"graded": "kuhn"}.get(kind, kind) and (kind != "graded" or (d["focus"] == "plane" and d["edge_ratio"] >= 200))
    seen = refs._against_80_digits(seed, oracle_port, us.scene)
    print(us.describe_line(seed))
    for r, what, _ in seen["worst"]:
        assert r <= 64, (what, r)


def test_geometry_restatements_against_80_digits(oracle_port):
    d = us.describe(GEOMETRY_SEED)
    assert d["base"] == "fan" and d["edge_valence"] >= 200
    assert refs.N_PIXELS == 90
    refs._geometry_against_80_digits(GEOMETRY_SEED, oracle_port, us.scene, False)
    print(us.describe_line(GEOMETRY_SEED))


# ---- the forward sweep's block on the GPU (tests/test_gpu_unstructured_fuzz.py) lies beyond the 60 seeds above --------------

def test_the_forward_block_is_qualified_and_shows_every_call_form(oracle_port):
    """Seeds 7096 - 7107, what tests/test_gpu_unstructured_fuzz.py says of them: at most one in ten is left out by qualify, the
    used ones hold every base and a scene of 4 096 cells or more, and the used scenes whose transition is not "points"
    (those upload a grid shrunk to a pixel or less: their frames as uploaded are blank at these image sizes) show all six
    forward call kinds between them."""
    from tests import test_gpu_unstructured_fuzz as gpu
    first = gpu.SWEEPS["forward"][0]
    assert first == 7096
    used, kinds = [], set()
    for seed in range(first, first + gpu.BLOCKS * gpu.PER_BLOCK):
        s = df.forward_scene(seed, us.scene)
        if df.qualify(s, oracle_port) is not None:
            continue
        used.append(us.describe(seed))
        lds, order, tile = s.variant
        whole = s.soup or order == 1 or s.depth_split == 1 or not (lds >= 2 and tile == 3)  # (check_forward's base_kind)
        kind = "front_to_back" if order == 1 and not s.soup else "split" if not whole and s.depth_split >= 2 else s.form
        small = ar.segment_lists(s.small, s.cells, s.rots, s.res[0], s.res[1], mg.REFERENCE_BOUNDS)
        print(f"seed {seed}: {kind}, transition {s.transition}, the grid shrunk by 1/16 covers {len(np.unique(small[0]))} pixels")
        if s.transition != "points":
            kinds.add(kind)
    assert len(used) >= 0.9 * gpu.BLOCKS * gpu.PER_BLOCK
    assert {d["base"] for d in used} == set(us.BASES) and any(d["cells"] >= us.LARGE for d in used)
    assert kinds == {"render", "render_device", "host_async", "frame_rows", "split", "front_to_back"}

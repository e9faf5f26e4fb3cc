"""The five fuzz sweeps of tests/derivative_fuzz.py - forward, scalar derivatives, geometry, second order / exact sums,
vertex exact - on the UNSTRUCTURED scenes of tests/unstructured_scenes.py: graded over three orders of magnitude in edge
length, points in hundreds of cells and edges in up to 200, point ids, cell order and cell vertices permuted, cavities and
tunnels, 4 500 - 9 000 cells in one scene of four.  Every mesh the other sweep files draw is a lattice.

Each sweep draws 12 seeds of its own from 7000 on (derivative_scene(seed, mesh=unstructured_scenes.scene); everything but the
mesh, view, image size and limit is drawn as for the lattice scenes) in 4 blocks of 3 and runs its check_* function and its
bars UNCHANGED (the module docstring of tests/derivative_fuzz.py derives them).  Any 12 consecutive seeds hold every base
four times and three scenes of the large class; which of them the references agree on (qualify) is pinned on the CPU by
tests/test_unstructured_scenes_cpu.py: seeds 7000 - 7059 with their classes, and the forward sweep's block 7096 - 7107 in a
test of its own (used seeds, bases, a large scene, the call forms it shows).

Named regression cases (sweep, seed -> what the scene showed) are listed in REGRESSIONS.
"""
import time

import pytest

from tests import derivative_fuzz as df
from tests import unstructured_scenes as us

pytestmark = pytest.mark.gpu
BLOCKS, PER_BLOCK = 4, 3
MESH = us.scene

# (sweep, seed) -> what it showed
REGRESSIONS = {
}


def _forward(oracle, tally):
    return lambda s, w: df.check_forward(s, w, oracle, tally)


# sweep -> (first seed, call kinds, draw, tally, check(oracle, tally)).  The forward sweep's block is chosen on the CPU, from
# the draws alone: at these image sizes the grid shrunk by 1/16 that a "points" transition uploads covers a pixel or none, so
# only the other scenes show their call form on a frame that is not blank, and of the blocks of 12 from 7000 to 7108 this is
# the one where those show all six (render, render_device, host_async, frame_rows, split, front_to_back).
SWEEPS = {
    "forward": (7096, df.FORWARD_KINDS, df.forward_scene, df.ForwardTally, _forward),
    "scalar": (7012, df.KINDS, df.derivative_scene, None, lambda oracle, tally: df.check_scene),
    "geometry": (7024, df.GEOMETRY_KINDS, df.geometry_scene, None, lambda oracle, tally: df.check_geometry),
    "second_order": (7036, df.SECOND_KINDS, df.second_order_scene, df.BitTally,
                     lambda oracle, tally: (lambda s, w: df.check_second_order(s, w, tally))),
    "vertex_exact": (7048, df.VERTEX_EXACT_KINDS, df.geometry_scene, df.BitTally,
                     lambda oracle, tally: (lambda s, w: df.check_vertex_exact(s, w, tally))),
}


class _Sweep:
    """The four blocks of three seeds of one sweep, each run once whichever test asks first."""

    def __init__(self, name, oracle):
        self.first, kinds, draw, tally, check = SWEEPS[name]
        self.name, self.oracle, self.worst, self.blocks = name, oracle, df.Worst(kinds), {}
        self.tally = tally() if tally else None
        self.draw = lambda seed: draw(seed, MESH)
        self.check = check(oracle, self.tally)
        self.used_seeds = []

    def run(self, seeds):
        used = skipped = 0
        mismatches = []
        for seed in seeds:
            t0 = time.time()
            u, s, m = df.run([seed], self.oracle, self.worst, draw=self.draw, check=self.check)
            print(f"{self.name} seed {seed} ({'used' if u else 'skipped'}, {time.time() - t0:.1f} s): {us.describe_line(seed)}")
            used, skipped, mismatches = used + u, skipped + s, mismatches + m
            if u:
                self.used_seeds.append(seed)
        return used, skipped, mismatches

    def block(self, i):
        if i not in self.blocks:
            first = self.first + PER_BLOCK * i
            self.blocks[i] = self.run(range(first, first + PER_BLOCK))
        return self.blocks[i]

    def report(self):
        for line in self.worst.lines() + (self.tally.lines() if self.tally else []):
            print(line)


@pytest.fixture(scope="module")
def sweeps(oracle_port):
    made = {}

    def get(name):
        if name not in made:
            made[name] = _Sweep(name, oracle_port)
        return made[name]

    return get


@pytest.mark.parametrize("block", range(BLOCKS))
@pytest.mark.parametrize("name", sorted(SWEEPS))
def test_unstructured_scenes_match_the_restatements_element_by_element(sweeps, name, block):
    sweep = sweeps(name)
    used, skipped, mismatches = sweep.block(block)
    print(f"{name} block {block}: {used} scenes used, {skipped} skipped, {sweep.worst.elements} elements compared so far")
    sweep.report()
    assert not mismatches, "\n".join(f"seed {seed}: {text}" for seed, text in mismatches)


@pytest.mark.parametrize("name", sorted(SWEEPS))
def test_at_most_a_tenth_skipped_and_every_class_used(sweeps, name):
    sweep = sweeps(name)
    used = sum(sweep.block(i)[0] for i in range(BLOCKS))
    skipped = sum(sweep.block(i)[1] for i in range(BLOCKS))
    print(f"{name}: {used} scenes used, {skipped} skipped, {sweep.worst.elements} elements compared")
    sweep.report()
    assert used + skipped == BLOCKS * PER_BLOCK and skipped <= 0.1 * (used + skipped)
    assert len(sweep.used_seeds) == used
    about = [us.describe(seed) for seed in sweep.used_seeds]
    assert {d["base"] for d in about} == set(us.BASES)
    assert any(d["cells"] >= us.LARGE for d in about)


def test_named_regression_scenes(oracle_port):
    for name, seed in sorted(REGRESSIONS):
        sweep = _Sweep(name, oracle_port)
        used, _skipped, mismatches = sweep.run([seed])
        sweep.report()
        assert used == 1 and not mismatches, "\n".join(f"{name} seed {seed}: {text}" for _seed, text in mismatches)

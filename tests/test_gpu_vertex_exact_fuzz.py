"""Bounded randomised sweep of the batched vertex adjoint (c5_render_vertex_adjoint_batch*) and of the exact vertex adjoint
sums ("vertex_exact", c5_render_vertex_exact_*, c5_vertex_exact_finish) on the GPU against the numpy restatement
(tests/vertex_adjoint_reference.py), ELEMENT BY ELEMENT, on the 40 scenes of tests/test_gpu_geometry_fuzz.py in 8 blocks of
5 - welded soups, "vertex_merge" 0 / 1, either cell order, update_points, cyclic row tiles and solids together.
tests/derivative_fuzz.py (geometry_scene, check_vertex_exact) holds the scenes and the bars
    vertex_adjoint_batch   1e-9 scale_raw + dz_err sens_raw + 2^-970 per component against gradients_of, at both widths;
                           every slice against the single call at check_geometry's rerun bar
    vertex_exact           the same reference bar for the single call
    vertex_exact_duality   <g, J v> = <J^T g, v> with the vertex tangent at 2^-22 sum |g| |out|
and the bit identities of the exact mode: call to call, the other cell order and merge, every slice of the batch at both
widths against the exact single call, the staged bounds / sums / finish over row parts against the single whole-image
call, welded non-representatives +0.0.  On soups ("algorithm" 1) the identities that compare two calls are counted and
printed, not asserted.  Every scene opens its own contexts; the used and skipped seeds are the scalar sweep's.

Named regression cases (seeds whose scene showed something) are listed in REGRESSIONS.
"""
import time

import pytest

from tests import derivative_fuzz as df

pytestmark = pytest.mark.gpu
BLOCKS, PER_BLOCK = 8, 5

# seed -> what it showed
REGRESSIONS = {}


class _Sweep:
    """The eight blocks of five seeds, each run once whichever test asks first."""

    def __init__(self, oracle):
        self.oracle, self.worst, self.tally, self.blocks = oracle, df.Worst(df.VERTEX_EXACT_KINDS), df.BitTally(), {}

    def block(self, i):
        if i not in self.blocks:
            t0 = time.time()
            first = 3000 + PER_BLOCK * i
            self.blocks[i] = df.run(range(first, first + PER_BLOCK), self.oracle, self.worst, draw=df.geometry_scene,
                                    check=lambda s, w: df.check_vertex_exact(s, w, self.tally))
            print(f"block {i}: {time.time() - t0:.1f} s")
        return self.blocks[i]

    def lines(self):
        return self.worst.lines() + self.tally.lines()


@pytest.fixture(scope="module")
def sweep(oracle_port):
    return _Sweep(oracle_port)


@pytest.mark.parametrize("block", range(BLOCKS))
def test_random_scenes_match_the_restatement_element_by_element(sweep, block):
    used, skipped, mismatches = sweep.block(block)
    print(f"block {block}: {used} scenes used, {skipped} skipped, {sweep.worst.elements} elements compared so far")
    for line in sweep.lines():
        print(line)
    assert not mismatches, "\n".join(f"seed {seed}: {text}" for seed, text in mismatches)


def test_at_most_a_tenth_of_the_seeds_was_skipped(sweep):
    used = sum(sweep.block(i)[0] for i in range(BLOCKS))
    skipped = sum(sweep.block(i)[1] for i in range(BLOCKS))
    print(f"{used} scenes used, {skipped} skipped, {sweep.worst.elements} elements compared")
    for line in sweep.lines():
        print(line)
    assert used + skipped == BLOCKS * PER_BLOCK and skipped <= 0.1 * (used + skipped)


@pytest.mark.parametrize("seed", sorted(REGRESSIONS))
def test_named_regression_scenes(oracle_port, seed):
    worst = df.Worst(df.VERTEX_EXACT_KINDS)
    used, _skipped, mismatches = df.run([seed], oracle_port, worst, draw=df.geometry_scene, check=df.check_vertex_exact)
    for line in worst.lines():
        print(line)
    assert used == 1 and not mismatches, "\n".join(text for _seed, text in mismatches)

"""Bounded randomised sweep of the Hessian-vector render (c5_render_hvp*) and of the exact-sum modes ("adjoint_exact",
"exact_sums", the C5_EXACT_* bounds / sums pair) on the GPU against the numpy restatements (tests/hvp_reference.py,
adjoint_reference.py, gn_reference.py), ELEMENT BY ELEMENT, on the 40 scenes of tests/test_gpu_derivative_fuzz.py in 8
blocks of 5 - tests/derivative_fuzz.py (second_order_scene, check_second_order) holds what is drawn on top of those scenes
and the bars
    hvp, exact_hvp                     1e-9 scale + dz_err sens + 2^-970          (hvp_of's scale and sens)
    exact_adjoint, exact_gn_diagonal   the same with gradients_of's and diagonal_scale's
    exact_gn_product                   (1e-9 + 2^-22) scale_h + dz_err sens + 2^-970
    hvp_symmetry                       |<u, H v> - <v, H u>| <= 1e-9 (sum |u (H v)| + sum |v (H u)|)
and the bit identities of the exact modes: call to call, a context on another walk option, the product as the exact adjoint
of weight x fp32(J v), and a second split of the rows whose exponents, integer words and finished doubles are the whole
image's.  On soups ("algorithm" 1) the identities that compare two calls are counted and printed, not asserted.  The
restatements are held to 80 digits in tests/test_hvp_cpu.py and tests/test_derivative_references_cpu.py.  Every scene
opens its own contexts; the used and skipped seeds are the scalar sweep's (qualify is the same).

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
        self.oracle, self.worst, self.tally, self.blocks = oracle, df.Worst(df.SECOND_KINDS), df.BitTally(), {}

    def block(self, i):
        if i not in self.blocks:
            t0 = time.time()
            first = 3000 + PER_BLOCK * i
            self.blocks[i] = df.run(range(first, first + PER_BLOCK), self.oracle, self.worst, draw=df.second_order_scene,
                                    check=lambda s, w: df.check_second_order(s, w, self.tally))
            print(f"block {i}: {time.time() - t0:.1f} s")
        return self.blocks[i]

    def lines(self):
        return self.worst.lines() + self.tally.lines()


@pytest.fixture(scope="module")
def sweep(oracle_port):
    return _Sweep(oracle_port)


@pytest.mark.parametrize("block", range(BLOCKS))
def test_random_scenes_match_the_restatements_element_by_element(sweep, block):
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
    worst = df.Worst(df.SECOND_KINDS)
    used, _skipped, mismatches = df.run([seed], oracle_port, worst, draw=df.second_order_scene, check=df.check_second_order)
    for line in worst.lines():
        print(line)
    assert used == 1 and not mismatches, "\n".join(text for _seed, text in mismatches)

"""Bounded randomised sweep of the derivative renders on the GPU: render_tangent, render_tangent_batch (both batch widths),
render_adjoint, render_adjoint_batch, render_gn_product and render_gn_diagonal (one scene in four through their _device
forms) against the numpy restatements, ELEMENT BY ELEMENT, on 4 x 10 scenes of tests/derivative_fuzz.py - which holds the
generator (image sizes off the 8x8 tile, views about three axes, every alpha limit, alpha at, next to and above the limit,
in [DBL_EPSILON, 1e-6) and below, a dz on both sides of 1/8, Q = 0, row ranges, cyclic row tiles, soups, solids), the rule
for which scenes count and the derivation of the bar
    tol = r_out |ref| + 1e-9 scale + dz_err sens + 2^-970        (r_out = 2^-23 for fp32 outputs; 2^-22 scale_h for H v)
term by term (sens = sum_k F_k |contribution_k| / dz_k with the slope factor F of the segment's steeper face, twice that
for the diagonal; the floor of an fp32 output is 2^-103).  The restatements themselves are held to an 80-digit reference (tests/test_derivative_references_cpu.py).
Every scene opens its own context.

Besides the bar: every slice of a tangent batch and the product's J v are the single tangents bit for bit; the GPU's own
segment and covered-pixel counts are the reference's; a plain render after the derivative calls is the one before them bit
for bit; at most 10 % of the seeds may be skipped.

Named regression cases (seeds whose scene showed something) are listed in REGRESSIONS.
"""
import pytest

from tests import derivative_fuzz as df

pytestmark = pytest.mark.gpu

# seed -> what it showed
REGRESSIONS = {
    # grad_q of cell 18845 off by 42.8 x the bar (4e-8 of its scale), and every other "underflow" scene likewise: with
    # alpha = 1e9 one chord is worth 1e7 of Lambda, and T = exp(-(Lambda - Lambda_k)) carried Lambda's rounding into the
    # cells in front of it.  Fixed in deriv_ray.hpp: lambda_add caps a segment's share of Lambda at 1024.
    3009: "Lambda - Lambda_k cancels behind a cell of optical depth 1e7",
    # I_dot = 3.6e-86 in fp64 is 0 in the fp32 image: the absolute floor of an fp32 output is fp32's own,
    # FLT_MIN / 2^-23 = 2^-103, not the 2^-970 of a double (a mistake of the bar, not of the kernel)
    3033: "an fp32 output below FLT_MIN",
    # cells that one ray crosses in a sliver (dz 1e-5 .. 4e-7) ending on a face with |dz/dx| + |dz/dy| of 19 to 23: the
    # GPU's chord is off by up to 11 x a dz_err that took the planes' terms to be of the size of the coordinates
    # (diag_q[108] 5.5 x, grad[13922] 1.08 x, diag_q[13851] 1.03 x that bar).  dz_err now carries the faces' slopes per
    # segment, and the diagonal's sensitivity the factor 2 of a square (tests/adjoint_reference.py, gn_reference.py).
    10166: "a sliver chord on a steep face, squared in the diagonal",
    10114: "a sliver chord on a steep face",
    10269: "a sliver chord on a steep face",
}


class _Sweep:
    """The four blocks of ten seeds, each run once whichever test asks first."""

    def __init__(self, oracle):
        self.oracle, self.worst, self.blocks = oracle, df.Worst(), {}

    def block(self, i):
        if i not in self.blocks:
            self.blocks[i] = df.run(range(3000 + 10 * i, 3010 + 10 * i), self.oracle, self.worst)
        return self.blocks[i]


@pytest.fixture(scope="module")
def sweep(oracle_port):
    return _Sweep(oracle_port)


@pytest.mark.parametrize("block", range(4))
def test_random_scenes_match_the_restatements_element_by_element(sweep, block):
    used, skipped, mismatches = sweep.block(block)
    print(f"block {block}: {used} scenes used, {skipped} skipped, {sweep.worst.elements} elements compared so far")
    for line in sweep.worst.lines():
        print(line)
    assert not mismatches, "\n".join(f"seed {seed}: {text}" for seed, text in mismatches)


def test_at_most_a_tenth_of_the_seeds_was_skipped(sweep):
    used = sum(sweep.block(i)[0] for i in range(4))
    skipped = sum(sweep.block(i)[1] for i in range(4))
    print(f"{used} scenes used, {skipped} skipped, {sweep.worst.elements} elements compared")
    for line in sweep.worst.lines():
        print(line)
    assert used + skipped == 40 and skipped <= 0.1 * (used + skipped)


@pytest.mark.parametrize("seed", sorted(REGRESSIONS))
def test_named_regression_scenes(oracle_port, seed):
    worst = df.Worst()
    used, _skipped, mismatches = df.run([seed], oracle_port, worst)
    for line in worst.lines():
        print(line)
    assert used == 1 and not mismatches, "\n".join(text for _seed, text in mismatches)

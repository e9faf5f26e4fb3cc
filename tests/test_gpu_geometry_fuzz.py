"""Bounded randomised sweep of the renders that differentiate in the geometry, and of the ray matrix, on the GPU:
render_motion_tangent, render_vertex_tangent, render_vertex_adjoint (one scene in four through their _device forms; one in
four on a grid moved into place by update_points) and ray_matrix against the numpy restatements (tests/motion_reference.py,
vertex_tangent_reference.py, vertex_adjoint_reference.py, adjoint_reference.segment_lists), ELEMENT BY ELEMENT, on the 40
scenes of tests/test_gpu_derivative_fuzz.py in 8 blocks of 5 - tests/derivative_fuzz.py (geometry_scene, check_geometry)
holds what is drawn on top of those scenes and the bars
    tangents        2^-23 |ref| + 1e-9 scale + dz_err sens + 2^-103     (the motion tangent's sens with its kappa terms)
    vertex adjoint  1e-9 scale_raw + dz_err sens_raw + 2^-970           (per component of every point)
    ray matrix      structure exact, dz and z_exit within dz_err x max(1, slope)
and the identities held on the GPU's own results.  The restatements are held to an 80-digit reference of the geometry
(tests/test_derivative_references_cpu.py) and their bars calibrated on the CPU (tests/test_motion_cpu.py,
test_vertex_tangent_cpu.py, test_vertex_adjoint_cpu.py).  Every scene opens its own contexts; the used and skipped seeds are
the scalar sweep's (qualify is the same).

Named regression cases (seeds whose scene showed something) are listed in REGRESSIONS.
"""
import time

import pytest

from tests import derivative_fuzz as df

pytestmark = pytest.mark.gpu
BLOCKS, PER_BLOCK = 8, 5

# seed -> what it showed
REGRESSIONS = {
    # 2 241 chords of the ray matrix up to 1.52 x their bar (468 up to 1.51 x in 3020), every one by its face's slope times
    # a shift of the PIXEL: the library sums the pixel coordinates up as the reference does (plane.cpp:304-314), the
    # restatements formed them as x_min + i step - tens of ulps apart after 300 columns.  A mistake of the restatements, not
    # of the kernels: adjoint_reference.pixel_coordinates now sums them up too (worst chord since: 0.08 of the bar).
    3032: "the restatements' pixel coordinates were x_min + i step, not the reference's running sums",
    3020: "the same on a soup: on \"algorithm\" 1 the library's chords are now segment_lists' to the bit",
}


class _Sweep:
    """The eight blocks of five seeds, each run once whichever test asks first."""

    def __init__(self, oracle):
        self.oracle, self.worst, self.blocks = oracle, df.Worst(df.GEOMETRY_KINDS), {}

    def block(self, i):
        if i not in self.blocks:
            t0 = time.time()
            first = 3000 + PER_BLOCK * i
            self.blocks[i] = df.run(range(first, first + PER_BLOCK), self.oracle, self.worst, draw=df.geometry_scene, check=df.check_geometry)
            print(f"block {i}: {time.time() - t0:.1f} s")
        return self.blocks[i]


@pytest.fixture(scope="module")
def sweep(oracle_port):
    return _Sweep(oracle_port)


@pytest.mark.parametrize("block", range(BLOCKS))
def test_random_scenes_match_the_restatements_element_by_element(sweep, block):
    used, skipped, mismatches = sweep.block(block)
    print(f"block {block}: {used} scenes used, {skipped} skipped, {sweep.worst.elements} elements compared so far")
    for line in sweep.worst.lines():
        print(line)
    assert not mismatches, "\n".join(f"seed {seed}: {text}" for seed, text in mismatches)


def test_at_most_a_tenth_of_the_seeds_was_skipped(sweep):
    used = sum(sweep.block(i)[0] for i in range(BLOCKS))
    skipped = sum(sweep.block(i)[1] for i in range(BLOCKS))
    print(f"{used} scenes used, {skipped} skipped, {sweep.worst.elements} elements compared")
    for line in sweep.worst.lines():
        print(line)
    assert used + skipped == BLOCKS * PER_BLOCK and skipped <= 0.1 * (used + skipped)


@pytest.mark.parametrize("seed", sorted(REGRESSIONS))
def test_named_regression_scenes(oracle_port, seed):
    worst = df.Worst(df.GEOMETRY_KINDS)
    used, _skipped, mismatches = df.run([seed], oracle_port, worst, draw=df.geometry_scene, check=df.check_geometry)
    for line in worst.lines():
        print(line)
    assert used == 1 and not mismatches, "\n".join(text for _seed, text in mismatches)

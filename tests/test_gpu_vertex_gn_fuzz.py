"""Bounded randomised sweep of the vertex Gauss-Newton product (c5_render_vertex_gn_product) under "vertex_exact" 1 on the
first 12 scenes of the geometry sweep (tests/derivative_fuzz.py: geometry_scene, seeds 3000 .. 3011, in 3 blocks of 4) -
threshold and underflow alphas, welded soups on "algorithm" 1 with garbage in the rows that are never read, either cell
order, solids, a late alpha limit, the scene's own fields (1 to 13, more than one chunk at either width) and weights (zeros
in a patch and in a tenth of the values, or none).  Per scene, bit for bit:
    h       against render_vertex_adjoint_batch(np.float32(w) * render_vertex_tangent(v)), the composition
    jv_out  against render_vertex_tangent
No scene is skipped: one that the vertex tangent or the vertex adjoint itself refuses is named in the output and counted,
and the count must be zero.  At least 10 of the scenes must have a product that is not all zeros (11 have: the weights of
seed 3008 are zero on every pixel its grid covers)."""
import time

import numpy as np
import pytest

from course5_amd import capi
from tests import derivative_fuzz as df

pytestmark = pytest.mark.gpu
BLOCKS, PER_BLOCK, FIRST = 3, 4, 3000


def _bits(a, kind):
    return np.ascontiguousarray(a).view(kind)


def _check(s):
    """(mismatches, why the parts themselves cannot render the scene or None, whether the product has a non-zero value)
    for one scene."""
    fields = s.v_fields if s.v_garbage is None else s.v_garbage
    bad = []
    with df._open(s, s.xyz, s.walk_option) as ctx:
        if not s.late_limit:
            ctx.set_alpha_limit(s.limit)
        ctx.render()
        if s.late_limit:
            ctx.set_alpha_limit(s.limit)
        if s.solid:
            ctx.set_solid(0, df._solid_of(s))
        ctx.set_option("vertex_exact", 1)
        try:
            jv = ctx.render_vertex_tangent(fields)
            g = jv if s.w is None else np.float32(s.w) * jv
            want = ctx.render_vertex_adjoint_batch(g)
        except capi.C5Error as e:
            return bad, f"the vertex tangent and adjoint refuse it ({e})", False
        for width in (4, 8):
            ctx.set_option("batch_width", width)
            h, jv_out = ctx.render_vertex_gn_product(fields, s.w, want_jv=True)
            if not np.array_equal(_bits(jv_out, np.uint32), _bits(jv, np.uint32)):
                bad.append(f"width {width}: jv_out differs from the tangent render in {int((_bits(jv_out, np.uint32) != _bits(jv, np.uint32)).sum())} values")
            if not np.array_equal(_bits(h, np.uint64), _bits(want, np.uint64)):
                bad.append(f"width {width}: h differs from the composition in {int((_bits(h, np.uint64) != _bits(want, np.uint64)).sum())} of {h.size} values")
        welded = s.rep != np.arange(len(s.xyz))
        if _bits(h[:, welded], np.uint64).any():
            bad.append("welded non-representatives are not +0.0 to the bit")
    return bad, None, bool(want.any())


class _Sweep:
    def __init__(self):
        self.blocks = {}

    def block(self, i):
        if i not in self.blocks:
            t0 = time.time()
            mismatches, unrenderable, soups, nonzero = [], [], 0, 0
            for seed in range(FIRST + PER_BLOCK * i, FIRST + PER_BLOCK * (i + 1)):
                s = df.geometry_scene(seed)
                soups += s.soup
                bad, why, some = _check(s)
                nonzero += some
                print(f"seed {seed}: {df.describe_geometry(s)}" + (f" - NOT RENDERED: {why}" if why else "")
                      + ("" if some or why else " - the weights are zero on every covered pixel: a product of zeros"))
                mismatches += [(seed, text) for text in bad]
                if why:
                    unrenderable.append((seed, why))
            print(f"block {i}: {time.time() - t0:.1f} s")
            self.blocks[i] = mismatches, unrenderable, soups, nonzero
        return self.blocks[i]


@pytest.fixture(scope="module")
def sweep():
    return _Sweep()


@pytest.mark.parametrize("block", range(BLOCKS))
def test_random_scenes_are_the_composition_bit_for_bit(sweep, block):
    mismatches, unrenderable, _soups, _nonzero = sweep.block(block)
    assert not unrenderable, "\n".join(f"seed {seed}: {why}" for seed, why in unrenderable)
    assert not mismatches, "\n".join(f"seed {seed}: {text}" for seed, text in mismatches)


def test_every_scene_was_rendered_and_soups_were_among_them(sweep):
    done = [sweep.block(i) for i in range(BLOCKS)]
    assert sum(len(unrenderable) for _m, unrenderable, _s, _n in done) == 0
    assert sum(soups for _m, _u, soups, _n in done) >= 1  # ("algorithm" 1 with welded points)
    # (seed 3008's weights are zero on every pixel its grid covers: its product is zeros on both sides)
    assert sum(nonzero for _m, _u, _s, nonzero in done) >= 10

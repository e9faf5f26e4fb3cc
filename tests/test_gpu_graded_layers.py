"""Graded layer stacks on the GPU against the slab reference with unequal layers (tests/slab_reference.py: planes=,
graded_scenes; pinned on the CPU by tests/test_slab_reference_cpu.py): a 4 x 4 lateral lattice in 12 layers whose
thicknesses run from half the box down to 2^-20 and 2^-26 of it - a boundary layer.  The walk's set-up has constants that
go with the size of the whole grid: the entry-key slack is 2^-24 of the bounding box's diagonal, times up to 2^15 on steep
faces (csrc/walk_common.hpp: entry_key_exponent), and its comments say such keys can swap with a neighbour closer than
their slack.  On the lattices of every other test no neighbour is; here the next face is 2^-20 or 2^-26 away.

Stacks (slab_reference.STACKS; the box and the scalars are tests/test_gpu_degenerate_rays.py's, the image 65 x 49):
  geometric      thicknesses 2^-12, 2^-14 .. 2^-20 of the box from each side toward the middle (a ratio of 1/4), the two
                 outermost layers the rest
  thin           the same with the middle pair at 2^-26: below the uniform slack
  gap, gap-thin  those two without the cells of one layer of the middle pair: every ray through the core leaves the grid and
                 re-enters it through next_entry across a gap of 2^-20 / 2^-26; the reference is the whole stack with that layer
                 at alpha = Q = 0
  layered-outer  the thin layers outside: the boundary faces are followed by neighbours 2^-20 behind them
  layered-outer-thin  ... 2^-26 behind them: inside the uniform slack.  (No face of any stack gets more than the uniform
                 slack: that takes a slope of about 1 300, slab_reference.STACKS; the documented swap of steep keys is untested.)
each under two generic views - view_rotations(0.37, -0.61), and (0.498, 0.13), which puts the layer planes at |gx| + |gy| =
159 (no lattice alignment: that is tests/test_gpu_degenerate_rays.py's ground).

Per scene the default variant (three frames), ("integration", 1), ("depth_split", 3) and a row range cut off the 8-row tile:
EVERY pixel at test_gpu_degenerate_rays.forward_ratio's bar, its statistics (walk_overflow, entry_overflow, odd_pixels 0;
steps > 0: the frame came from the walk, not from a fall-back to bin_sort_resolve after a false interpenetration); and every
one of those frames FIRST through render_device + synchronize(), whose status must be C5_OK (render() itself renders
again on C5_RETRY and would hide one) and whose frame must be render()'s to the bit.  render_tangent per pixel,
render_adjoint, render_gn_product and render_hvp summed per layer, and ray_matrix per pixel and layer, as that file holds them - its functions, its bars, no new term.
The image is moved by 2^-10 (slab_reference.GRADED_BOUNDS; tests/test_slab_reference_cpu.py asserts that no pixel centre is on
the image of a vertex or an edge).  The last section runs the same stacks on the unmoved image, where pixel (24, 32) is the
image of the lattice vertex (1, 0, 0): frames and derivative renders are held like the others', four ray matrices are strict
expected failures at that pixel (VERTEX_RAY says what each lists) and a second test holds everything else of all twelve.
profiles/unstructured_fuzz.md has the measured figures.
"""
import functools

import numpy as np
import pytest

from course5_amd import capi
from tests import slab_reference as sr
from tests import test_gpu_degenerate_rays as dr

pytestmark = pytest.mark.gpu
SCENES = sr.graded_scenes()
ROW_RANGE = (13, 30)  # (begin, count): both ends off the 8-row tile


@functools.lru_cache(maxsize=None)
def reference(name):
    return dr.reference_of(ALL[name]())


def _frame(ctx, ref, rows, cutoff, kind, what, tally, bad):
    """The frame first through render_device + synchronize(), the form that hands the frame's status out - on the fresh
    context and after every change of an option or of the rows, before any render() of that state: render() renders again
    by itself on C5_RETRY (c5_render: up to three times) and would hide one - then dr.hold_frame.  The
    status must be C5_OK - no entry refused by the overflow pool, no ray that took components of the grid for
    interpenetrating - and the frame the one render() gave, to the bit."""
    import torch
    out = torch.full((len(rows), ref.s.res[0], 2), float("nan"), dtype=torch.float32, device="cuda")
    ctx.render_device(out.data_ptr())  # BEFORE render(): a retry render() had absorbed (the pool grown, the grid sent to
    status = ctx.synchronize()         # bin_sort_resolve for good) would leave this frame nothing to report
    if status != capi.C5_OK:
        bad.append(f"{what}: render_device answered status {status}" + (" (C5_RETRY)" if status == capi.C5_RETRY else ""))
    img = dr.hold_frame(ctx, ref, rows, cutoff, kind, what, tally, bad)
    if status == capi.C5_OK and not np.array_equal(dr._bits(out.cpu().numpy()), dr._bits(img)):
        bad.append(f"{what}: render_device's frame is not render()'s to the bit")
    return img


ALIGNED = sr.graded_scenes(aligned=True)
ALL = dict(SCENES, **ALIGNED)


@pytest.mark.parametrize("name", sorted(ALL))
def test_every_pixel_of_the_graded_stacks(name):
    ref = reference(name)
    s = ref.s
    all_rows = np.arange(s.res[1])
    tally, bad = dr.Tally(name), []
    with dr.open_context(s) as ctx:
        first = [_frame(ctx, ref, all_rows, 0.0, "default", f"frame {k}", tally, bad) for k in range(3)]
        if not (np.array_equal(dr._bits(first[0]), dr._bits(first[1])) and np.array_equal(dr._bits(first[0]), dr._bits(first[2]))):
            bad.append("three frames in a row are not equal to the bit")
        ctx.set_option("integration", 1)
        _frame(ctx, ref, all_rows, dr.DEFAULT_CUTOFF, "integration 1", "front to back", tally, bad)
        ctx.set_option("integration", 0)
        ctx.set_option("depth_split", 3)
        _frame(ctx, ref, all_rows, 0.0, "depth_split", "3 slabs", tally, bad)
        ctx.set_option("depth_split", 1)
        whole = _frame(ctx, ref, all_rows, 0.0, "rows", "whole rays", tally, bad)
        begin, count = ROW_RANGE
        ctx.set_row_range(begin, count)
        rows = np.arange(begin, begin + count)
        part = _frame(ctx, ref, rows, 0.0, "rows", f"rows {begin} .. {begin + count - 1}", tally, bad)
        if not np.array_equal(dr._bits(part), dr._bits(whole[rows])):
            bad.append(f"the row range differs from the whole frame's rows in {int((dr._bits(part) != dr._bits(whole[rows])).sum())} values")
    tally.report()
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", sorted(ALL))
def test_derivative_renders_summed_over_the_layers(name):
    dr.derivative_renders_against_the_slab(reference(name))


@pytest.mark.parametrize("name", sorted(SCENES))
def test_ray_matrix_holds_the_slab_chords(name):
    dr.ray_matrix_against_the_slab(reference(name), depth_order=True)


# ---- the same stacks with a pixel centre on a lattice vertex ----------------------------------------------------------------
# On BOUNDS itself pixel (24, 32) is the image of the lattice vertex (1, 0, 0), the pivot of both views: the ray runs up the
# common edge of the cells about it, through layers 2^-20 and 2^-26 thick (tests/test_gpu_degenerate_rays.py's ground; the
# frames and derivative renders of these scenes are held above like the others').  Four of the twelve ray matrices miss
# there, each a strict expected failure; every other property of theirs is held by the test after it.

_STEP = ("  The step takes every exit as the next chord's start (carry_next = w_exit), also the exit of a sliver whose chord "
         "came out negative and was dropped; keeping the larger depth is a change to the step of every walk (DESIGN section 5)")
_OVERLAP = ("pixel (24, 32), layer 6 (2^-20 thick): the row lists cell 398 (362 without layer 5) with a chord of 2.4012884e-6 that "
            "starts 6.79e-13 BELOW the exit listed before it, and the chords of the layer add up to exactly that much more than "
            "the layer's 2.4013078e-6: 6.2 x dz_err (F + lat).  The cells about the vertex are slivers with an edge 2^-20 long; "
            "a face through that edge projects to 2.4e-7 of area, its slope is known to 1e-10, its depth 0.25 away to 1e-11 and not "
            "to dz_err F." + _STEP)
VERTEX_RAY = {
    "geometric/generic/aligned": _OVERLAP,
    "gap/generic/aligned": _OVERLAP,
    "thin/steep/aligned": ("pixel (24, 32): z_exit decreases by 1.35e-17 between cells 681 and 686 (layers 5 and 6, chords 2.6e-12 and "
                           "6.3e-18), the order of depths of scene G's expected failure; the chords are inside the bar." + _STEP),
    "gap-thin/steep/aligned": ("pixel (24, 32), layer 6 (2^-26 thick, behind the gap): the row lists cell 627, which the ray only "
                               "touches, with a chord of 3.8e-12 ahead of cell 695, whose chord is the layer's 2.3716091e-6 to 6e-17: "
                               "1.31 x dz_err (F + lat).  The entry is right: face_plane gives every face in the layer's two planes "
                               "(slope 159) at that pixel to 1e-16 of the exact plane through its rounded points "
                               "(tests/test_slab_reference_cpu.py restates it).  The sliver face of cell 627 with an edge 2^-26 long "
                               "(projected area 1.5e-9, slope 2.3) comes out 3.0e-12 BELOW the plane the ray entered at: the cell "
                               "before 627 leaves through such a face, its negative chord is dropped - so it is not listed, and the "
                               "overlap is with the entry's depth, not with a listed exit - and 627's chord starts there." + _STEP),
}
# the scene whose dropped chord comes first after a re-entry: its overlap is with the entry's depth, which no row lists.  The chords
# of that pixel are held through the exits instead (below)
AFTER_AN_ENTRY = {"gap-thin/steep/aligned": (sr.ALIGNED_PIXEL[0] * sr.GRADED_RES[0] + sr.ALIGNED_PIXEL[1],)}


@pytest.mark.parametrize("name", [pytest.param(n, marks=pytest.mark.xfail(strict=True, reason=VERTEX_RAY[n])) if n in VERTEX_RAY else n
                                  for n in sorted(ALIGNED)])
def test_ray_matrix_of_the_aligned_stacks(name):
    dr.ray_matrix_against_the_slab(reference(name), depth_order=True)


@pytest.mark.parametrize("name", sorted(ALIGNED))
def test_ray_matrix_of_the_aligned_stacks_but_for_the_vertex_ray(name):
    """Everything test_ray_matrix_of_the_aligned_stacks asks, of all twelve scenes, except that (a) where a listed chord
    starts below the exit listed before it the overlap is taken off the chord first - which alone brings the chords of
    geometric / generic and gap / generic inside the bar: the excess IS the overlap - and z_exit may step down, and (b) at the
    vertex pixel of gap-thin / steep, where the dropped chord comes first after a re-entry and overlaps the entry's depth,
    the chords are held through the exits: from the last exit listed in one layer to the last exit listed in the next
    listed layer the ray covers the slab chords of the layers in between (the absent one included), within the sum of
    their bars - what the chords would add up to if every start were the exit before it or the entry.  An overlap or a step down beyond the rounding of a depth
    (2^-50 x the largest |z|: a chord start is a difference of two doubles) is allowed at the vertex pixel alone."""
    ref = reference(name)
    s = ref.s
    row_ptr, col, dz, z, overlap = dr.ray_matrix_against_the_slab(ref, depth_order=False, less_overlap=True,
                                                                  leave_out=AFTER_AN_ENTRY.get(name, ()))
    pix = dr.rmc.rows_of(row_ptr)
    m, n = ref.m, s.n_layers
    for p in AFTER_AN_ENTRY.get(name, ()):
        v = m["valid"][p]
        want, bar = np.zeros(n), np.zeros(n)
        want[m["C"][p][v]], bar[m["C"][p][v]] = m["D"][p][v], ref.e * (m["F"][p][v] + m["lat"][p][v])
        row = slice(row_ptr[p], row_ptr[p + 1])
        layer, exits = s.layer_of_cell[col[row]], z[row]
        last = np.flatnonzero(np.concatenate([layer[1:] != layer[:-1], [True]]))  # the last listed cell of every layer of the row
        assert (np.diff(layer[last]) > 0).all() and len(last) >= 6  # (deepest first: this view walks the layers upward)
        for a, b in zip(last[:-1], last[1:]):
            between = slice(layer[a] + 1, layer[b] + 1)
            r = abs((exits[b] - exits[a]) - want[between].sum()) / bar[between].sum()
            print(f"scene {name}, pixel {p}: exits of layers {layer[a]} -> {layer[b]}: {exits[b] - exits[a]:.17g} against {want[between].sum():.17g}, "
                  f"error / bar {r:.3g}")
            assert r <= 1.0, (int(layer[a]), int(layer[b]), r)
    vertex = sr.ALIGNED_PIXEL[0] * s.res[0] + sr.ALIGNED_PIXEL[1]
    rounding = 2.0 ** -50 * float(np.abs(z).max())
    down = np.concatenate([[0.0], np.where(pix[1:] == pix[:-1], np.maximum(-np.diff(z), 0.0), 0.0)])
    big = (overlap > rounding) | (down > rounding)
    i = np.flatnonzero((pix == vertex) & ((overlap > 0) | (down > 0)))
    print(f"scene {name}: {int((overlap > 0).sum())} chords start below the exit before them, by up to {overlap.max():.3g} "
          f"({int(big.sum())} beyond the rounding {rounding:.3g}); z_exit steps down at {int((down > 0).sum())} places by up to {down.max():.3g}; "
          f"at the vertex pixel cells {col[i].tolist()} layers {s.layer_of_cell[col[i]].tolist()} dz {dz[i].tolist()} "
          f"overlap {overlap[i].tolist()} down {down[i].tolist()}")
    assert set(pix[big].tolist()) <= {vertex}

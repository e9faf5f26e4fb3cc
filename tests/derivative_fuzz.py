"""Randomised sweep of the derivative renders (tangent, adjoint, their batches, the Gauss-Newton product and diagonal)
against the numpy restatements, element by element.

    python tests/derivative_fuzz.py [n_scenes] [seed0]
    python tests/derivative_fuzz.py geometry [n_scenes] [seed0]      (the geometry sweep, below)
    python tests/derivative_fuzz.py forward [n_scenes] [seed0]       (the forward sweep, at the end of this text)
    python tests/derivative_fuzz.py second [n_scenes] [seed0]        (the second-order and exact-sum sweep, below)
    python tests/derivative_fuzz.py vertex_exact [n_scenes] [seed0]  (the vertex sweep, below)
    python tests/derivative_fuzz.py chords [unstructured] SEED PIXEL   (the GPU's chords along one ray against the
                                                            reference's; unstructured: tests/unstructured_scenes.py's scene)

reports every mismatch and the worst error / tolerance per call kind; exit status 1 on any mismatch or when more than
10 % of the seeds had to be skipped.  tests/test_gpu_derivative_fuzz.py runs 40 seeds of it under pytest;
tests/test_derivative_references_cpu.py holds the restatements to an 80-digit reference on the same scenes.

derivative_scene(seed) takes grid, view, image size and alpha limit from fuzz_scenes.scene(seed) (images of 20-500
pixels a side, almost never a multiple of the 8x8 tile; limits U[0.5, 6); views about three axes) - or, with
mesh=unstructured_scenes.scene, from the graded, high-valence, relabelled meshes of tests/unstructured_scenes.py, which
tests/test_gpu_unstructured_fuzz.py sends through all five sweeps; geometry_scene, forward_scene and second_order_scene pass
the argument on - and adds
  * alpha by class, every class in every scene with >= 10 cells (ALPHA_CLASSES): 0; (0, DBL_EPSILON); [DBL_EPSILON, 1e-6)
    log-uniform; == limit; the two doubles next to the limit; (limit, 2 limit]; the rest U[0, limit).  "threshold" scenes
    (one in four) scale the rest so that the median a dz of the segments sits at 1/8, the switch between series and closed
    form in segment_terms (the limit is raised to the scaled maximum where it would clamp them), and give up to six
    cells alpha = 0.125 / dz of one of their own chords or one of its two neighbouring doubles.  "underflow" scenes (one
    in eight) have limit 1e9 and alpha up to 200 / (mean chord): T and E run through the subnormals to 0.
    Q = U[0, 2) with 10 % zeros;
  * K in 2..11 normal directions, d_alpha or d_q NULL in a third of the scenes; K normal upstream images with a patch
    of exact zeros; Gauss-Newton weights U[0, 2) with a patch and a tenth of exact zeros (NULL in a fifth of the scenes);
  * the frame layout: whole image, a random row range, or cyclic row tiles over every rank of a world of 2..5 (adjoints
    summed, tangents put back in their rows), a third each;
  * one in five as a soup on "algorithm" 1; one in five with a solid over part of the grid (its mask from the NaNs of a
    forward render); one in four through the _device calls; in half of them the alpha limit is set only AFTER a first
    forward render.

A scene is used iff the port oracle renders it, adjoint_reference.segment_lists gives the oracle's segment and
covered-pixel counts and the grid stays a pixel inside the image border (qualify).  No element of a used scene is left
out of a comparison; GPU stats that disagree with those counts are a mismatch, not a skip.

The bar, per element (a pixel's channel, a cell's gradient), with scale and sens from the reference:
    tol = r_out |ref| + r64 scale + dz_err sens + 2^-970                                                   (tolerance)
  r_out  2^-23 for fp32 outputs (one rounding to fp32 is 2^-24, doubled), 0 for fp64 ones.  The product's h carries its
         fp32 intermediate as 2^-22 scale_h instead: one fp32 rounding of J v and one of its product with the weight,
         2 x 2^-24, doubled; scale_h the absolute sums of the adjoint with the upstream image |w| |J v|.
  r64    1e-9: the project's bar between two fp64 derivative results, on the element's own absolute-sum
         scale instead of the array's maximum.
  dz_err 16 x 2^-52 x max(1, max |coordinate in view space|), per segment times F = max(1, |gx| + |gy|) of the steeper of
         its two faces z = c + gx x + gy y: the GPU's chord is a difference of two plane evaluations at absolute pixel
         coordinates, three products and three sums each, whose terms have the size of (|gx| + |gy|) x the coordinates
         (csrc/walk_common.hpp says the same of its entry keys: "rounding eps * kappa * |x|"); the reference gets the
         chord from differences about a vertex.  sens = sum_k F_k |contribution_k| / dz_k, twice that for the
         diagonal, whose terms go with dz^2 (tests/adjoint_reference.py, gn_reference.py).  Matters for sliver chords
         only.  F and the 2 were missing at first: over 300 scenes three cells that a single weighted ray crosses in a
         sliver ending on a steep face showed it - seed 10166 diag_q[108] (dz 9.6e-6, |gx| + |gy| = 18.7) at 5.5 x that
         bar, 10114 grad[13922] (9.7e-7, 21.1) at 1.08 x, 10269 diag_q[13851] (3.5e-7, 23.2) at 1.03 x.  The GPU's chords
         there, read back with `chords` (gpu_chords), are off by -11.05, -1.26 and +1.08 of the unscaled dz_err, 0.59,
         0.06 and 0.05 of F x dz_err; the other 108 segments of those rays by at most 0.96 of F x dz_err, following their
         faces' slopes (profiles/derivative_fuzz.md has the table).
  2^-970 DBL_MIN / DBL_EPSILON: below it (underflow scenes) a double keeps no relative accuracy.  For an fp32 output the
         same with fp32's numbers, FLT_MIN / 2^-23 = 2^-103: seed 3033's I_dot = 3.6e-86 is 0 in the image.
None of these is fitted to what the GPU returns.

THE GEOMETRY SWEEP (geometry_scene, check_geometry; tests/test_gpu_geometry_fuzz.py runs 40 seeds of it): the renders that
differentiate in the grid's points - render_motion_tangent, render_vertex_tangent, render_vertex_adjoint with
update_points - and ray_matrix, on the same scenes.  geometry_scene(seed) is derivative_scene(seed), unchanged (qualify
too: the used and skipped seeds are the scalar sweep's), plus, from a stream of its own (default_rng([seed, 0x6E0])):
  * affine fields: rotation_motion of every angle of the view, two normal ones, Z_SCALE, Z_TRANSLATION, a pure x / y
    translation, and the first normal one times 2^20 and times 2^-20;
  * per-point fields: K in 1..11 normal ones, one that is non-zero at a single point, one that is M^T (A p_v + b) of the
    first affine field; all of them constant over a weld group (capi.weld_points: a group moves as one), and where points
    are welded - soups, hanging-node interfaces whose ids are not shared - a second copy with 1e6 x normal garbage in the
    rows of the non-representatives;
  * upstream images of the vertex adjoint: g[0], and in a third of the scenes each an image with only the tau channel and
    one with only the I channel (the patch of exact zeros exercises the walk's `wanted`);
  * options: "vertex_merge" 0 / 1, "cell_order" 0 / 1 (before the upload), in a quarter of the scenes one of
    ("depth_split", 2) and ("integration", 1) - the header promises whole rays in the reference's order whatever these say;
    such a scene is held to the same bars, and whether its tangents are bit-equal to a default context's is printed;
  * in a quarter of the scenes the context is uploaded with the points displaced by a normal field of 1e-3 x the shortest
    cell edge (constant over a weld group), one call of each kind and three plain renders (the third reuses the per-view
    data) run on that grid, then update_points(xyz): the next plain render must be a fresh upload's bit for bit, and
    everything after it is held to the reference of xyz.
Layout, soup, solid, device forms and the late limit are derivative_scene's.  Per used scene, every element compared:
  motion_tangent, vertex_tangent   2^-23 |ref| + 1e-9 scale + dz_err sens + 2^-103 against motion_reference.motion_of (every
      affine field; its sens with the kappa terms) and vertex_tangent_reference.tangent_of (the first per-point field, the
      single-point one and one drawn; the others are held to the single calls by the batches); every slice of a batch at
      both widths bit-equal to the single call; row parts put back in their rows;
  vertex_adjoint   1e-9 scale_raw + dz_err sens_raw + 2^-970 per component against vertex_adjoint_reference.gradients_of
      (sens_raw: its docstring; calibrated in tests/test_vertex_adjoint_cpu.py), row parts and ranks summed, the
      reference's per-copy gradients, scales and sensitivities summed onto the representatives and the other rows
      exactly 0; a second call on tests/test_gpu_vertex_adjoint.py's run-to-run bar (rtol 1e-12, atol 1e-15 x max, per part);
  ray_matrix   structure exact against s.segments (without the solid-marked pixels), dz and z_exit within dz_err x
      max(1, slope) (tests/ray_matrix_checks.py); a part's matrix is bit for bit rows of the whole frame's;
  identities on the GPU's own results: <g, J v> = <J^T g, v> between the vertex tangent and the vertex adjoint for two
      fields at 2^-22 sum |g| |out|; Z_TRANSLATION exactly 0; the 2^+-20 multiples are the field's image with every
      finite, normal fp32 value scaled exactly (bits after ldexp; only values subnormal on either side are left out); the
      single-point field is exactly 0 at every pixel whose ray crosses no cell holding the point; garbage rows change no
      bit; stats() before and after the calls; a plain render after the calls bit-equal to the one before them.
What the first run of it found is in profiles/geometry_fuzz.md: the restatements' pixel coordinates
(adjoint_reference.pixel_coordinates).

THE FORWARD SWEEP (forward_scene, check_forward; tests/test_gpu_forward_fuzz.py runs 40 seeds of it): the render itself,
frame by frame, against adjoint_reference.forward_of - the kernel every performance change rewrites.  forward_scene(seed) is
derivative_scene(seed), unchanged (qualify too), plus, from a stream of its own (default_rng([seed, 0xF0])):
  * class eps_to_1e-6 as drawn in one scene of four, redrawn as U[0, limit) elsewhere: where it stands, the bar of I is the
    reference's own cancellation noise (`cancel`, below) at 5 - 74 % of the covered pixels and a render is held to no more
    than that; redrawn, most scenes have no such pixel (tests/test_forward_reference_cpu.py asserts: at least half);
  * the exp regime, a third each: as drawn; "short", alpha and limit times f so that exp_rule = min(largest alpha, limit) x
    longest cell edge = 0.124; "just_over", 0.126 (to_rule).  Below 0.125 the library takes every exp of a frame by a
    10-term series without range reduction (csrc/frame.hip: small_exp_only; csrc/walk_common.hpp: exp_small_nonpositive)
    if the frame also runs on "lds_stage" 2, "tile" 3 and at most 14 staged cells.  predicted_kernel says which walk that
    rule selects; it is printed per state and counted - there is no read-out of the kernel that ran;
  * the kernel variant: the product default (2, 0, 3) in half of the scenes with "stage_slots" 14 or 0 (by the frame
    before) and "depth_split" 0, 1 or forced 2..7 with tilted planes, a third each; else one of fuzz_scenes.VARIANTS (21
    slots where the variant says so); "transmittance_cutoff" 0 in half of the "integration" 1 scenes;
  * the call form: render(); render_device + synchronize; three outstanding render_host_async frames into pinned images,
    each waited for; render_frame_rows_async into full pinned frames where the layout is sharded;
  * one transition of the state exp_rule reads, with the reference made again for every state; two frames after it and
    two after going back:
      scalars  from the short regime (the scene is brought there first if it is not) by update_scalars or
               update_scalars_device (by the seed's parity, the way back by the other) to alpha x g with the largest a dz
               of a segment at 1.75 (every other such scene: the median at 4), the limit raised first; and back;
      limit    alpha scaled to a limit of 0.124 / L with class above_limit stretched to 14 x the limit (the top on the
               cell with the longest chord of the view); set_alpha_limit to the top alpha (the rule at 1.74), and back;
      points   the context is uploaded with the grid shrunk by 1/16 about its centroid and alpha for 0.124 there; the shrunk
               grid must qualify itself (else the scene makes the limit transition and says so); update_points to the
               drawn size (1.98: the longest edge is made again), and shrunk again.
Layout, soup, solid and the late limit are derivative_scene's.  Three frames in a row of every part of the layout (the
second may change the staged cells and the slab count from the first's statistics, the third reuses the per-view data),
EVERY frame compared, every pixel of it:
    tol_tau = 2^-23 |tau| + 1e-9 scale_tau + dz_err sens_tau + 2^-103
    tol_I   = 2^-23 |I|   + 1e-9 scale_I   + dz_err sens_I + cancel (+ cutoff) + 2^-103                       (forward_ratio)
  with forward_of's terms: scale_tau = sum dz |alpha| and sens_tau = sum F |alpha| (the raw alpha), scale_I = sum T |Q| S,
  sens_I = sum F T E |Q - a I_prev| (dI / d dz, the motion tangent's chord derivative), cancel = 8 x 2^-53 sum T (|Q| + a |I_prev|)
  / a, the rounding of the reference's own step C = Q - a I; I = (Q - C e) / a (derived in forward_of's docstring: the
  oracle's fp32 image is at 0.49 of the bar with it and at 2e7 without), and cutoff = c sum |Q| S on "integration" 1 with a
  "transmittance_cutoff" c (what the early-out may drop).  2^-23, 1e-9, dz_err and F are the ones above.  A pixel without a
  segment is exactly 0 in both channels, the NaN pixels are exactly the port oracle's solid-marked ones, stats() report
  the reference's segments and covered pixels of the part's rows (with a solid: the oracle's marked pixels; the reference's
  own counts then depend on the order its threads bin in, line.cpp:29-67) and walk_overflow 0.  None of it is fitted to
  what the GPU returns.  Reported, not asserted: how many fp32 values of the frames on "integration" 0 with whole rays
  are not the port oracle's bit for bit.  What the first runs found is in profiles/forward_fuzz.md.

THE SECOND-ORDER AND EXACT-SUM SWEEP (second_order_scene, check_second_order; tests/test_gpu_second_order_fuzz.py runs 40
seeds of it): render_hvp and the exact modes ("adjoint_exact" 1, "exact_sums" 1, the C5_EXACT_* bounds / sums pair).
second_order_scene(seed) is derivative_scene(seed), unchanged (qualify too), plus, from a stream of its own
(default_rng([seed, 0x2E0])):
  * the walk option of a comparison context (COMPARE_OPTIONS): none, ("depth_split", 2), ("integration", 1), ("cell_order", 0),
    or ("lds_stage", 0) with ("tile", 0);
  * a second split of the rows of the WHOLE image, whatever the scene's layout: cyclic tiles with the scene's tile_rows and
    world, or two row ranges [0, cut), [cut, ry) with cut no multiple of the 8-row tile (off_tile_cut).
Layout, soup, solid, device forms and the late limit are derivative_scene's, applied as check_scene applies them (the first
render and the stats check included).  Per part of the layout, sums over the parts compared:
  hvp   render_hvp for direction 0 (with the scene's NULL d_alpha / d_q) and g[0], and with fit=("alpha",) / ("q",) (the other
      block None), every element of h_alpha and h_q at 1e-9 scale + dz_err sens + 2^-970 against hvp_reference.hvp_of; clamped
      and inactive cells exactly 0 in h_alpha; stats() and a plain render after the calls as before them;
  hvp_symmetry   with direction 1: |<u, H v> - <v, H u>| <= 1e-9 (sum |u (H v)| + sum |v (H u)|), tests/test_gpu_hvp.py's bar;
  exact_adjoint, exact_gn_diagonal, exact_gn_product, exact_hvp   the adjoint of g[0], the diagonal, the product and the
      Hessian-vector product of direction 0 on the same context with both options on, each on the bar of its atomic form
      above (the product's r64 + 2^-22 on scale_h), NOT on a relation to the atomic result;
  bit identities of the exact mode (BitTally): a second call; the comparison context; the product against the exact adjoint
      of weight x fp32(J v) and its J v against the tangent; the second split - the bounds per part combined
      (sharding.combine_exact) are the whole image's exponents, the words per part against them add up to the whole image's
      integers, and finished (capi.exact_sums_finish) they are the single whole-image call's doubles, for C5_EXACT_ADJOINT,
      _GN_DIAGONAL and _HVP.  A part's words must not all be zero where it owns a cell's largest contribution (its own exponent
      is the combined one, so that contribution is >= 2^(e-1) on the cell's grid) or, for the two kinds with a tau term
      (g_tau dz, w_tau dz^2), where it holds a covered, not solid-marked pixel whose image is not zero - a pixel with a zero
      image, and a part 300 decades below another in every cell it shares, may rightly add nothing;
  afterwards   the four atomic results within rtol 1e-12, atol 1e-15 x max of the ones before the exact calls
      (tests/test_gpu_exact_fit.py's run-to-run bar), stats() and a plain render as before.
On soups ("algorithm" 1: lists with equal depths may change their order from call to call) the identities that compare
two calls - second call, comparison context, second split - are counted and printed, not asserted
(tests/test_gpu_exact_adjoint.py's rule); the bars, the product identity and `afterwards` hold everywhere.

THE VERTEX SWEEP (check_vertex_exact; tests/test_gpu_vertex_exact_fuzz.py runs 40 seeds of it): render_vertex_adjoint_batch and
"vertex_exact" on geometry_scene(seed), unchanged - welded soups, "vertex_merge" 0 / 1, either cell order, the walk option,
update_points (a moved scene is uploaded displaced, one call and a frame run there, then update_points), cyclic tiles, solids
and device forms together.  The batch is s.vg followed by g[1:K]: up to 13 images, more than one pass at either width.
  vertex_adjoint_batch   at "batch_width" 4 and 8 over the parts of the layout, summed: the slices of s.vg at 1e-9 scale_raw +
      dz_err sens_raw + 2^-970 against vertex_adjoint_reference.gradients_of on the representatives, welded non-representatives
      exactly 0, every slice against the single call at check_geometry's rerun bar;
  vertex_exact   the single call of vg[0] on the same reference bar; on the whole image a second call, a context with the OTHER
      cell_order and the OTHER vertex_merge, and every slice of the batch at both widths against the exact single call of
      that image: equal bits; the staged path (render_vertex_exact_bounds per part, sharding.combine_vertex_exact, _sums,
      combine, vertex_exact_finish) over the layout's cyclic tiles, else over two ranges cut off the 8-row tile
      (default_rng([seed, 0x7E0])): the single whole-image call's bits; welded non-representatives +0.0 to the bit;
  vertex_exact_duality   <g, J v> = <J^T g, v> with render_vertex_tangent of field v_compare[0] at 2^-22 sum |g| |out|.
The soup rule is the one above.

On the scenes of several components of tests/component_scenes.py (tests/test_gpu_component_fuzz.py) both sweeps read one
optional attribute, s.shards (shard_identities): the row split of the exact sums once more over CONTEXTS OF THEIR OWN, one
per part - asserted with "algorithm" 1 on each, counted with the parts left to find an overlap from their own rays; and the
second-order sweep's comparison context, which renders nothing but the layout's parts, is then opened on "algorithm" 1.  No
other scene carries the attribute.

Both sweeps take their restatements over the rows of the layout that hold a covered pixel and over the covered pixels alone
(covered_rows, covered_only; second_order_restatements and vertex_restatements run without a GPU): a pixel without a segment
adds nothing to any cell or point.  The GPU calls run over every row and pixel.  profiles/second_order_fuzz.md has the runs.
"""
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import numpy as np

from course5_amd import meshgen as mg, sharding
from tests import adjoint_reference as ar, gn_reference as gr, tangent_reference as tr
from tests import motion_reference as mr, ray_matrix_checks as rmc, vertex_adjoint_reference as vr, vertex_tangent_reference as vt
from tests import exact_sum_reference as er, hvp_reference as hr
from tests.fuzz_scenes import scene

B = mg.REFERENCE_BOUNDS
EPS = float(np.finfo(np.float64).eps)
R_OUT = 2.0 ** -23
R_H = 2.0 ** -22
R64 = 1e-9
ABS_FLOOR = 2.0 ** -970
ABS_FLOOR_32 = 2.0 ** -103
ALPHA_CLASSES = ("zero", "below_eps", "eps_to_1e-6", "at_limit", "ulp_above_limit", "ulp_below_limit", "above_limit", "rest")
_CLASS_P = (0.05, 0.04, 0.08, 0.05, 0.03, 0.03, 0.10, 0.62)
KINDS = ("tangent", "tangent_batch", "adjoint", "adjoint_batch", "gn_product", "gn_diagonal")
GEOMETRY_KINDS = ("motion_tangent", "vertex_tangent", "vertex_adjoint", "vertex_adjoint_rerun", "ray_matrix", "duality")
WALK_OPTIONS = (("depth_split", 2), ("integration", 1))
FORWARD_KINDS = ("render", "render_device", "host_async", "frame_rows", "split", "front_to_back", "after_update_scalars",
                 "after_set_limit", "after_update_points")
DEFAULT_VARIANT = (2, 0, 3)
SECOND_KINDS = ("hvp", "hvp_symmetry", "exact_adjoint", "exact_gn_diagonal", "exact_gn_product", "exact_hvp")
VERTEX_EXACT_KINDS = ("vertex_adjoint_batch", "vertex_exact", "vertex_exact_duality")
COMPARE_OPTIONS = ((), (("depth_split", 2),), (("integration", 1),), (("cell_order", 0),), (("lds_stage", 0), ("tile", 0)))


def alpha_class(alpha, limit):
    """The class index (ALPHA_CLASSES) of every alpha."""
    a = np.asarray(alpha)
    c = np.full(a.shape, 7)
    c[a == 0] = 0
    c[(a > 0) & (a < EPS)] = 1
    c[(a >= EPS) & (a < 1e-6)] = 2
    c[a > limit] = 6
    c[a == limit] = 3
    c[a == np.nextafter(limit, np.inf)] = 4
    c[a == np.nextafter(limit, -np.inf)] = 5
    return c


def derivative_scene(seed, mesh=scene):
    """mesh: the draw of grid, view, image size and limit - fuzz_scenes.scene, or tests/unstructured_scenes.py's."""
    xyz, cells, _alpha, _q, rots, res, limit = mesh(seed)
    rng = np.random.default_rng([seed, 0xD5])
    s = types.SimpleNamespace(seed=seed, rots=rots, res=res)
    s.soup = bool(rng.integers(5) == 0)
    if s.soup:
        xyz, cells = mg.per_cell_point_copies(xyz, cells)
    s.xyz, s.cells = xyz, cells
    n = len(cells)
    rx, ry = res
    # (alpha is drawn from the chords at the pixel coordinates x_min + i step, as it was before adjoint_reference.
    # pixel_coordinates went over to the reference's running sums: the scenes of a seed do not change)
    pix, cell, _zh, dz, _slope = ar.segment_lists(xyz, cells, rots, rx, ry, B, with_slope=True, running=False)
    s.segments = ar.segment_lists(xyz, cells, rots, rx, ry, B, with_slope=True)
    s.mode = ("threshold", "threshold", "underflow", "plain", "plain", "plain", "plain", "plain")[int(rng.integers(8))]
    # -- alpha
    u = rng.uniform(0.0, 1.0, n)
    amp = limit
    if s.mode == "threshold" and len(dz):
        amp = 0.125 / max(float(np.median(u[cell] * dz)), 1e-300)
        limit = max(limit, amp)
    elif s.mode == "underflow":
        limit = 1e9
        amp = 200.0 / float(dz.mean()) if len(dz) else 1e4
    s.limit = limit
    alpha = u * amp
    cls = rng.choice(8, n, p=_CLASS_P)
    first = rng.permutation(n)
    if n >= 10:
        cls[first[:8]] = np.arange(8)
    k = [int((cls == c).sum()) for c in range(8)]
    alpha[cls == 0] = 0.0
    alpha[cls == 1] = np.minimum(10.0 ** rng.uniform(-300.0, np.log10(EPS), k[1]), np.nextafter(EPS, 0.0))
    alpha[cls == 2] = np.clip(10.0 ** rng.uniform(np.log10(EPS), -6.0, k[2]), EPS, np.nextafter(1e-6, 0.0))
    alpha[cls == 3] = limit
    alpha[cls == 4] = np.nextafter(limit, np.inf)
    alpha[cls == 5] = np.nextafter(limit, -np.inf)
    alpha[cls == 6] = limit * (2.0 - rng.uniform(0.0, 1.0, k[6]))
    s.threshold_cells = []
    if s.mode == "threshold" and len(dz):
        free = np.setdiff1d(np.flatnonzero(cls == 7), first[:8])
        for j, c in enumerate(rng.permutation(free)):
            chords = dz[cell == c]
            if len(chords) == 0:
                continue
            a0 = 0.125 / float(rng.choice(chords))
            if not a0 < limit:
                continue
            alpha[c] = (a0, np.nextafter(a0, np.inf), np.nextafter(a0, 0.0))[len(s.threshold_cells) % 3]
            s.threshold_cells.append(int(c))
            if len(s.threshold_cells) == 6:
                break
    s.alpha = alpha
    s.q = rng.uniform(0.0, 2.0, n)
    s.q[rng.uniform(size=n) < 0.1] = 0.0
    # -- directions, upstream images, weights
    s.k = int(rng.integers(2, 12))
    null = int(rng.integers(6))
    s.d_alpha = None if null == 0 else rng.normal(size=(s.k, n))
    s.d_q = None if null == 1 else rng.normal(size=(s.k, n))

    def patch():
        r = np.sort(rng.integers(0, ry + 1, 2))
        c = np.sort(rng.integers(0, rx + 1, 2))
        return slice(r[0], max(r[1], r[0] + 1)), slice(c[0], max(c[1], c[0] + 1))

    s.g = rng.normal(size=(s.k, ry, rx, 2)).astype(np.float32)
    r, c = patch()
    s.g[:, r, c] = 0.0
    s.w = rng.uniform(0.0, 2.0, (ry, rx, 2)).astype(np.float32)
    r, c = patch()
    s.w[r, c] = 0.0
    s.w[rng.uniform(size=s.w.shape) < 0.1] = 0.0
    if rng.integers(5) == 0:
        s.w = None
    # -- frame layout
    s.layout = ("whole", "range", "cyclic")[int(rng.integers(3))]
    begin = int(rng.integers(0, ry))
    s.row_range = (begin, int(rng.integers(1, ry - begin + 1)))
    s.tile_rows, s.world = int(rng.choice([1, 3, 8, 16])), int(rng.integers(2, 6))
    s.solid = bool(rng.integers(5) == 0)
    s.solid_at = rng.uniform(0.3, 0.7, 3), float(rng.uniform(0.2, 0.5))
    s.device = bool(rng.integers(4) == 0)
    s.late_limit = bool(rng.integers(2) == 0)
    return s


def qualify(s, oracle):
    """None if the scene is used, else why it is not (docstring: which scenes count)."""
    rx, ry = s.res
    v = oracle.rotate_points(s.xyz, s.rots)
    px, py = (B[0] - B[1]) / (rx - 1), (B[2] - B[3]) / (ry - 1)
    if v[:, 0].min() < B[1] + px or v[:, 0].max() > B[0] - px or v[:, 1].min() < B[3] + py or v[:, 1].max() > B[2] - py:
        return "the grid reaches the image's border"
    try:
        ref = oracle.render(s.xyz, s.cells, s.alpha, s.q, s.rots, rx, ry, B, alpha_limit=s.limit, threads=8)
    except RuntimeError as e:
        return f"the oracle rejects the scene ({e})"
    pix = s.segments[0]
    s.n_segments, s.n_covered = len(pix), len(np.unique(pix))
    if (s.n_segments, s.n_covered) != (ref["segments"], ref["covered"]):
        return (f"segment_lists gives {s.n_segments} segments on {s.n_covered} pixels, the oracle "
                f"{ref['segments']} on {ref['covered']}")
    return None


def dz_err(s):
    return 16.0 * 2.0 ** -52 * max(1.0, float(np.abs(ar.rotate(s.xyz, s.rots)).max()))


def ratio(got, ref, scale, sens, dz_e, r_out=0.0, r_scale=R64, extra=0.0):
    """error / tolerance per element (docstring: the bar); a value that is not finite counts as infinitely wrong.  extra:
    further absolute terms of the bar (the forward sweep's cancel and cutoff)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    tol = r_out * np.abs(ref) + r_scale * scale + dz_e * sens + extra + (ABS_FLOOR_32 if r_out else ABS_FLOOR)
    r = np.abs(got - ref) / tol
    return np.where(np.isfinite(got), r, np.inf)


class Worst:
    """The worst error / tolerance per call kind, with the seed and element that showed it, and the elements compared."""

    def __init__(self, kinds=KINDS):
        self.by_kind = {k: (0.0, None) for k in kinds}
        self.elements = 0

    def add(self, kind, r, seed, what=""):
        r = np.asarray(r)
        self.elements += r.size
        if r.size and r.max() > self.by_kind[kind][0]:
            i = np.unravel_index(int(np.argmax(r)), r.shape)
            self.by_kind[kind] = (float(r.max()), f"seed {seed} {what} element {tuple(int(v) for v in i)}")
        return float(r.max()) if r.size else 0.0

    def lines(self):
        return [f"worst error / tol, {k}: {v:.3g} ({w})" for k, (v, w) in self.by_kind.items()]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class _Calls:
    """The derivative calls of one context in their host forms (numpy in, numpy out)."""

    def __init__(self, ctx):
        self.ctx = ctx

    def tangent(self, da, dq):
        return self.ctx.render_tangent(da, dq)

    def tangent_batch(self, da, dq):
        return self.ctx.render_tangent_batch(da, dq)

    def adjoint(self, g):
        return self.ctx.render_adjoint(g)

    def adjoint_batch(self, g):
        return self.ctx.render_adjoint_batch(g)

    def gn_product(self, da, dq, w):
        return self.ctx.render_gn_product(da, dq, w, want_jv=True)

    def gn_diagonal(self, w):
        return self.ctx.render_gn_diagonal(w)

    def hvp(self, da, dq, g, fit=("alpha", "q")):
        return self.ctx.render_hvp(da, dq, g, fit=fit)


class _DeviceCalls(_Calls):
    """The same through the _device forms: torch tensors on the GPU, the status from synchronize() (C5_RETRY: again)."""

    def _run(self, call):
        from course5_amd import capi
        for _ in range(3):
            call()
            if self.ctx.synchronize() == capi.C5_OK:
                return
        raise RuntimeError("C5_RETRY three times in a row")

    def _t(self, a, dtype=None):
        import torch
        return None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")

    def _empty(self, shape, dtype):
        import torch
        return torch.full(shape, float("nan"), dtype=dtype, device="cuda")

    def _image_shape(self):
        return (self.ctx.local_rows, self.ctx.res_x, 2)

    def tangent(self, da, dq):
        import torch
        out = self._empty(self._image_shape(), torch.float32)
        a, q = self._t(da), self._t(dq)
        self._run(lambda: self.ctx.render_tangent_device(a, q, out))
        return out.cpu().numpy()

    def tangent_batch(self, da, dq):
        import torch
        k = len(da if da is not None else dq)
        out = self._empty((k,) + self._image_shape(), torch.float32)
        a, q = self._t(da), self._t(dq)
        self._run(lambda: self.ctx.render_tangent_batch_device(a, q, out))
        return out.cpu().numpy()

    def adjoint(self, g):
        import torch
        n = self.ctx.n_cells
        ga, gq, gt = self._empty((n,), torch.float64), self._empty((n,), torch.float64), self._t(g, torch.float32)
        self._run(lambda: self.ctx.render_adjoint_device(gt, ga, gq))
        return ga.cpu().numpy(), gq.cpu().numpy()

    def adjoint_batch(self, g):
        import torch
        n, k = self.ctx.n_cells, len(g)
        ga, gq, gt = self._empty((k, n), torch.float64), self._empty((k, n), torch.float64), self._t(g, torch.float32)
        self._run(lambda: self.ctx.render_adjoint_batch_device(gt, ga, gq))
        return ga.cpu().numpy(), gq.cpu().numpy()

    def gn_product(self, da, dq, w):
        import torch
        n, k = self.ctx.n_cells, len(da if da is not None else dq)
        ha, hq = self._empty((k, n), torch.float64), self._empty((k, n), torch.float64)
        jv = self._empty((k,) + self._image_shape(), torch.float32)
        a, q, wt = self._t(da), self._t(dq), self._t(w, torch.float32)
        self._run(lambda: self.ctx.render_gn_product_device(a, q, wt, ha, hq, jv))
        return ha.cpu().numpy(), hq.cpu().numpy(), jv.cpu().numpy()

    def gn_diagonal(self, w):
        import torch
        n = self.ctx.n_cells
        da, dq, wt = self._empty((n,), torch.float64), self._empty((n,), torch.float64), self._t(w, torch.float32)
        self._run(lambda: self.ctx.render_gn_diagonal_device(wt, da, dq))
        return da.cpu().numpy(), dq.cpu().numpy()

    def hvp(self, da, dq, g, fit=("alpha", "q")):
        import torch
        n = self.ctx.n_cells
        ha = self._empty((n,), torch.float64) if "alpha" in fit else None
        hq = self._empty((n,), torch.float64) if "q" in fit else None
        a, q, gt = self._t(da), self._t(dq), self._t(g, torch.float32)
        self._run(lambda: self.ctx.render_hvp_device(a, q, gt, ha, hq))
        return None if ha is None else ha.cpu().numpy(), None if hq is None else hq.cpu().numpy()


def check_scene(s, worst):
    """Every derivative call on one used scene (qualify first) in a context of its own.  Returns the mismatches, strings."""
    from course5_amd import capi
    bad = []
    rx, ry = s.res
    n = len(s.cells)
    K = s.k
    with capi.Context(0) as ctx:
        if s.soup:
            ctx.set_option("algorithm", 1)
        ctx.upload_grid(s.xyz, s.cells, s.alpha, s.q)
        ctx.set_image(rx, ry, B)
        ctx.set_view(s.rots)
        if not s.late_limit:
            ctx.set_alpha_limit(s.limit)
        ctx.render()
        st = ctx.stats()
        if (st["segments"], st["covered_pixels"]) != (s.n_segments, s.n_covered):
            bad.append(f"stats: {st['segments']} segments on {st['covered_pixels']} pixels, the reference has "
                       f"{s.n_segments} on {s.n_covered}")
        if s.late_limit:
            ctx.set_alpha_limit(s.limit)  # (after a frame: the cell records carry the clamp and must be rebuilt)
        skip = None
        if s.solid:
            v = ar.rotate(s.xyz, s.rots)
            frac, size = s.solid_at
            ext = v.max(0) - v.min(0)
            sx, sc = mg.kuhn_box(2, lo=tuple(v.min(0) + frac * ext - 0.5 * size * ext.max()), size=size * float(ext.max()))
            ctx.set_solid(0, sx[sc].reshape(-1, 12))
            skip = np.isnan(ctx.render()[..., 0])
        if s.layout == "range":
            b, c = s.row_range
            rows_ref = np.arange(b, b + c)
            parts = [(lambda: ctx.set_row_range(b, c), np.arange(c))]
        elif s.layout == "cyclic":
            rows_ref = np.arange(ry)
            parts = [((lambda r=r: ctx.set_row_tiles(s.tile_rows, r, s.world)), sharding.local_rows(ry, s.tile_rows, r, s.world))
                     for r in range(s.world)]
        else:
            rows_ref = np.arange(ry)
            parts = [(lambda: None, np.arange(ry))]
        nr = len(rows_ref)
        g_ref = s.g[:, rows_ref]
        w_ref = None if s.w is None else s.w[rows_ref]
        calls = _DeviceCalls(ctx) if s.device else _Calls(ctx)
        tan = np.full((K, nr, rx, 2), np.nan, np.float32)
        sums = {name: 0.0 for name in ("ga1", "gq1", "ga", "gq", "ha", "hq", "diag_a", "diag_q")}
        for place, where in parts:
            if len(where) == 0:  # (a rank without rows: small images in tall tiles)
                continue
            place()
            before = ctx.render()
            da, dq = s.d_alpha, s.d_q
            singles = np.stack([calls.tangent(None if da is None else da[j], None if dq is None else dq[j]) for j in range(K)])
            for width in (4, 8):
                ctx.set_option("batch_width", width)
                batch = calls.tangent_batch(da, dq)
                if not np.array_equal(_bits(batch), _bits(singles)):
                    bad.append(f"tangent batch (width {width}) differs from the single calls in "
                               f"{int((_bits(batch) != _bits(singles)).sum())} values")
            tan[:, where] = singles
            g_part = np.ascontiguousarray(g_ref[:, where])
            w_part = None if w_ref is None else np.ascontiguousarray(w_ref[where])
            out = dict(zip(("ga1", "gq1"), calls.adjoint(g_part[0])))
            out.update(zip(("ga", "gq"), calls.adjoint_batch(g_part)))
            ha, hq, jv = calls.gn_product(da, dq, w_part)
            if not np.array_equal(_bits(jv), _bits(singles)):
                bad.append(f"the product's J v differs from the tangent batch in {int((_bits(jv) != _bits(singles)).sum())} values")
            out.update(ha=ha, hq=hq)
            out.update(zip(("diag_a", "diag_q"), calls.gn_diagonal(w_part)))
            for name, v in out.items():
                sums[name] = sums[name] + v
            if not np.array_equal(_bits(ctx.render()), _bits(before)):
                bad.append("a plain render after the derivative calls differs from the one before them")
    # -- against the restatement, element by element
    e = dz_err(s)
    m = ar.ray_matrices(s.xyz, s.cells, s.alpha, s.q, s.rots, rx, ry, B, s.limit, rows_ref)
    skip_ref = None if skip is None else skip[rows_ref]
    found = []
    for j in range(K):
        td, Id, _tau, _I, x = tr.tangent_of(m, n, None if s.d_alpha is None else s.d_alpha[j],
                                            None if s.d_q is None else s.d_q[j], skip_ref, with_scale=True)
        r = np.stack([ratio(tan[j, ..., 0], td, x["scale_tau"], x["sens_tau"], e, R_OUT),
                      ratio(tan[j, ..., 1], Id, x["scale_I"], x["sens_I"], e, R_OUT)], axis=-1)
        found.append(("tangent" if j == 0 else "tangent_batch", f"direction {j}", r))
        ga, gq, _tau, _I, x = ar.gradients_of(m, n, g_ref[j], skip_ref, with_scale=True)
        r = np.stack([ratio(sums["ga"][j], ga, x["scale_alpha"], x["sens_alpha"], e),
                      ratio(sums["gq"][j], gq, x["scale_q"], x["sens_q"], e)])
        found.append(("adjoint_batch", f"image {j} (alpha, q)", r))
        if j == 0:
            r = np.stack([ratio(sums["ga1"], ga, x["scale_alpha"], x["sens_alpha"], e),
                          ratio(sums["gq1"], gq, x["scale_q"], x["sens_q"], e)])
            found.append(("adjoint", "(alpha, q)", r))
    terms = gr.terms_of(m, skip_ref, with_scale=True)
    for j in range(K):
        ha, hq, _jv, x = gr.product_header(terms, nr * rx, n, None if s.d_alpha is None else s.d_alpha[j],
                                           None if s.d_q is None else s.d_q[j], w_ref)
        r = np.stack([ratio(sums["ha"][j], ha, x["scale_alpha"], x["sens_alpha"], e, r_scale=R64 + R_H),
                      ratio(sums["hq"][j], hq, x["scale_q"], x["sens_q"], e, r_scale=R64 + R_H)])
        found.append(("gn_product", f"direction {j} (alpha, q)", r))
    da, dq = gr.diagonal(terms, nr * rx, n, w_ref)
    x = gr.diagonal_scale(terms, nr * rx, n, w_ref)
    r = np.stack([ratio(sums["diag_a"], da, x["scale_alpha"], x["sens_alpha"], e),
                  ratio(sums["diag_q"], dq, x["scale_q"], x["sens_q"], e)])
    found.append(("gn_diagonal", "(alpha, q)", r))
    for kind, what, r in found:
        top = worst.add(kind, r, s.seed, what)
        if not top <= 1.0:
            i = np.unravel_index(int(np.argmax(r)), r.shape)
            bad.append(f"{kind} {what}: {int((~(r <= 1.0)).sum())} elements beyond the bar, worst error / tol {top:.3g} at {tuple(int(v) for v in i)}")
    return bad


# ---- the geometry sweep: motion tangent, vertex tangent, vertex adjoint, ray matrix -----------------------------------

def geometry_scene(seed, mesh=scene):
    """derivative_scene(seed), unchanged, with what the geometry calls need drawn from a stream of its own (module
    docstring: the geometry sweep)."""
    from course5_amd import capi
    s = derivative_scene(seed, mesh)
    rng = np.random.default_rng([seed, 0x6E0])
    n_pts = len(s.xyz)
    cells = np.asarray(s.cells).reshape(-1, 4)
    s.rep, s.merged = capi.weld_points(s.xyz)
    s.rep = s.rep.astype(np.int64)
    others = s.rep != np.arange(n_pts)
    # -- affine fields
    rot = [capi.rotation_motion(s.rots, i) for i in range(len(s.rots))]
    a1, a2 = rng.normal(size=(2, 12))
    shift = np.zeros(12)
    shift[9:11] = rng.normal(size=2)
    s.motion = np.array(rot + [a1, a2, mr.Z_SCALE, mr.Z_TRANSLATION, shift, a1 * 2.0 ** 20, a1 * 2.0 ** -20])
    base = len(rot)
    s.motion_at = {"base": base, "z_translation": base + 3, "up": base + 5, "down": base + 6}
    # -- per-point fields: normal ones, one that moves a single point, one that is an affine field at the points
    kv = int(rng.integers(1, 12))
    normal = rng.normal(size=(kv, n_pts, 3))
    single = np.zeros((n_pts, 3))
    s.single_point = int(s.rep[cells.reshape(-1)[int(rng.integers(cells.size))]])
    single[s.single_point] = rng.normal(size=3)
    pv = ar.rotate(s.xyz, s.rots)
    affine = (pv @ a1[:9].reshape(3, 3).T + a1[9:]) @ vr.view_matrix(s.rots)  # d_xyz[v] = M^T (A p_v + b)
    s.v_fields = np.concatenate([normal, single[None], affine[None]])[:, s.rep]  # (a weld group moves as one)
    s.v_garbage = None
    if others.any():  # the rows of welded non-representatives are never read
        s.v_garbage = s.v_fields.copy()
        s.v_garbage[:, others] = 1e6 * rng.normal(size=(len(s.v_fields), int(others.sum()), 3))
    drawn = [j for j in range(len(s.v_fields)) if j not in (0, kv)]
    s.v_single = kv
    s.v_compare = [0, kv, int(rng.choice(drawn))]  # held to the restatement; the rest by the batches' bit equality
    # -- upstream images of the vertex adjoint
    s.vg = [s.g[0]]
    which = int(rng.integers(3))
    if which < 2:  # only the tau channel, only the I channel
        img = s.g[1].copy()
        img[..., 1 - which] = 0.0
        s.vg.append(img)
    # -- options, and a grid that is moved into place
    s.vertex_merge, s.cell_order = int(rng.integers(2)), int(rng.integers(2))
    s.walk_option = WALK_OPTIONS[int(rng.integers(2))] if rng.integers(4) == 0 else None
    s.moved = bool(rng.integers(4) == 0)
    e = s.xyz[cells[:, [0, 0, 0, 1, 1, 2]]] - s.xyz[cells[:, [1, 2, 3, 2, 3, 3]]]
    s.displaced = s.xyz + (1e-3 * np.sqrt((e ** 2).sum(-1)).min() * rng.normal(size=(n_pts, 3)))[s.rep]
    return s


class _GeoCalls:
    """The geometry calls of one context in their host forms; fields [K, 12], d [K, n_pts, 3], g [rows, res_x, 2]."""

    def __init__(self, ctx):
        self.ctx = ctx

    def motion(self, fields):
        return self.ctx.render_motion_tangent(fields)

    def vertex_tangent(self, d):
        return self.ctx.render_vertex_tangent(d)

    def vertex_adjoint(self, g):
        return self.ctx.render_vertex_adjoint(g)

    def vertex_adjoint_batch(self, g):
        return self.ctx.render_vertex_adjoint_batch(g)


class _GeoDeviceCalls(_DeviceCalls):
    def motion(self, fields):
        import torch
        out = self._empty((len(fields),) + self._image_shape(), torch.float32)
        self._run(lambda: self.ctx.render_motion_tangent_device(fields, out))
        return out.cpu().numpy()

    def vertex_tangent(self, d):
        import torch
        out = self._empty((len(d),) + self._image_shape(), torch.float32)
        dt = self._t(d, torch.float64)
        self._run(lambda: self.ctx.render_vertex_tangent_device(dt, out))
        return out.cpu().numpy()

    def vertex_adjoint(self, g):
        import torch
        out, gt = self._empty((self.ctx.n_pts, 3), torch.float64), self._t(g, torch.float32)
        self._run(lambda: self.ctx.render_vertex_adjoint_device(gt, out))
        return out.cpu().numpy()

    def vertex_adjoint_batch(self, g):
        import torch
        out, gt = self._empty((len(g), self.ctx.n_pts, 3), torch.float64), self._t(g, torch.float32)
        self._run(lambda: self.ctx.render_vertex_adjoint_batch_device(gt, out))
        return out.cpu().numpy()


def _open(s, xyz, walk_option=None, cell_order=None, vertex_merge=None, algorithm=None):
    """A context of the scene's own, as check_scene opens it, with the geometry sweep's options (cell_order, vertex_merge:
    in place of the scene's).  algorithm: set where the scene is no soup (a shard's context: shard_identities)."""
    from course5_amd import capi
    ctx = capi.Context(0)
    if s.soup:
        ctx.set_option("algorithm", 1)
    elif algorithm is not None:
        ctx.set_option("algorithm", algorithm)
    ctx.set_option("cell_order", s.cell_order if cell_order is None else cell_order)  # (read by the upload)
    ctx.set_option("vertex_merge", s.vertex_merge if vertex_merge is None else vertex_merge)
    if walk_option:
        ctx.set_option(*walk_option)
    ctx.upload_grid(xyz, s.cells, s.alpha, s.q)
    ctx.set_image(s.res[0], s.res[1], B)
    ctx.set_view(s.rots)
    return ctx


def _solid_of(s):
    v = ar.rotate(s.xyz, s.rots)
    frac, size = s.solid_at
    ext = v.max(0) - v.min(0)
    sx, sc = mg.kuhn_box(2, lo=tuple(v.min(0) + frac * ext - 0.5 * size * ext.max()), size=size * float(ext.max()))
    return sx[sc].reshape(-1, 12)


def _scaled_bits_differ(base, scaled, power):
    """How many fp32 values of `scaled` are not ldexp(base, power) bit for bit, leaving out only values that are subnormal
    (or beyond the finite range) on either side."""
    want = np.ldexp(base.astype(np.float64), power)
    tiny, huge = float(np.finfo(np.float32).tiny), float(np.finfo(np.float32).max)
    use = np.ones(base.shape, bool)
    for v in (np.abs(base.astype(np.float64)), np.abs(want), np.abs(scaled.astype(np.float64))):
        use &= ((v == 0) | (v >= tiny)) & (v <= huge)
    return int((_bits(want.astype(np.float32))[use] != _bits(scaled)[use]).sum()), int(use.sum())


def covered_only(m, geo):
    """ray_matrices' and segment_faces' dicts cut down to the pixels that have a segment (most of a frame has none and
    the restatements' time goes with the pixels): (covered [n_px] bool, m, geo), the results then [n_covered]."""
    cov = m["valid"].any(1)

    def cut(d):
        return {k: v[cov] if isinstance(v, np.ndarray) and v.shape[:1] == (m["n_px"],) else v for k, v in d.items()}

    mc = cut(m)
    mc["n_px"] = int(cov.sum())
    mc["shape"] = (mc["n_px"],)
    return cov, mc, cut(geo)


def check_geometry(s, worst, log=print):
    """Every geometry call on one used scene (geometry_scene, qualify first).  Returns the mismatches, strings."""
    from contextlib import ExitStack
    bad = []
    rx, ry = s.res
    n_pts = len(s.xyz)
    cells = np.asarray(s.cells).reshape(-1, 4)
    with ExitStack() as stack:
        ctx = stack.enter_context(_open(s, s.displaced if s.moved else s.xyz, s.walk_option))
        # a fresh upload of the points the moved grid ends at; a context without the walk option
        fresh = stack.enter_context(_open(s, s.xyz, s.walk_option)) if s.moved else None
        plain = stack.enter_context(_open(s, s.xyz)) if s.walk_option else None
        others_ctx = [c for c in (fresh, plain) if c is not None]
        if not s.late_limit:
            ctx.set_alpha_limit(s.limit)
        ctx.render()
        if not s.moved:
            st = ctx.stats()
            if (st["segments"], st["covered_pixels"]) != (s.n_segments, s.n_covered):
                bad.append(f"stats: {st['segments']} segments on {st['covered_pixels']} pixels, the reference has "
                           f"{s.n_segments} on {s.n_covered}")
        if s.late_limit:
            ctx.set_alpha_limit(s.limit)
        for c in others_ctx:
            c.set_alpha_limit(s.limit)
        calls = _GeoDeviceCalls(ctx) if s.device else _GeoCalls(ctx)
        if s.moved:  # one call of each kind on the displaced grid: their per-point and per-cell data are built for it
            calls.motion(s.motion[:1]), calls.vertex_tangent(s.v_fields[:1]), calls.vertex_adjoint(s.vg[0])
            for _ in range(3):  # (three frames of one view: the third reuses the per-view data of the displaced grid)
                ctx.render()
            ctx.update_points(s.xyz)
            if not np.array_equal(_bits(ctx.render()), _bits(fresh.render())):
                bad.append("the first plain render after update_points differs from a fresh upload's")
            st = ctx.stats()
            if (st["segments"], st["covered_pixels"]) != (s.n_segments, s.n_covered):
                bad.append(f"stats after update_points: {st['segments']} segments on {st['covered_pixels']} pixels, the "
                           f"reference has {s.n_segments} on {s.n_covered}")
        skip = None
        if s.solid:
            for c in [ctx] + others_ctx:
                c.set_solid(0, _solid_of(s))
            skip = np.isnan(ctx.render()[..., 0])
        whole = ctx.ray_matrix(with_depth=True)
        if s.layout == "range":
            b, c = s.row_range
            rows_ref = np.arange(b, b + c)
            parts = [(lambda x: x.set_row_range(b, c), np.arange(c))]
        elif s.layout == "cyclic":
            rows_ref = np.arange(ry)
            parts = [((lambda x, r=r: x.set_row_tiles(s.tile_rows, r, s.world)), sharding.local_rows(ry, s.tile_rows, r, s.world))
                     for r in range(s.world)]
        else:
            rows_ref = np.arange(ry)
            parts = [(lambda x: None, np.arange(ry))]
        nr = len(rows_ref)
        km, kv = len(s.motion), len(s.v_fields)
        mot = np.full((km, nr, rx, 2), np.nan, np.float32)
        vtan = np.full((kv, nr, rx, 2), np.nan, np.float32)
        grads = [np.zeros((n_pts, 3)) for _ in s.vg]
        rerun = [np.zeros((n_pts, 3)) for _ in s.vg]
        n_parts = 0
        for place, where in parts:
            if len(where) == 0:
                continue
            n_parts += 1
            place(ctx)
            before = ctx.render()
            st = ctx.stats()
            if fresh is not None:
                place(fresh)
                if not np.array_equal(_bits(before), _bits(fresh.render())):
                    bad.append("a plain render after update_points differs from a fresh upload's")
            # -- motion tangent and vertex tangent: singles, and the batches at both widths
            m1 = np.concatenate([calls.motion(s.motion[j:j + 1]) for j in range(km)])
            v1 = np.concatenate([calls.vertex_tangent(s.v_fields[j:j + 1]) for j in range(kv)])
            for width in (4, 8):
                ctx.set_option("batch_width", width)
                for name, single, batch in (("motion", m1, calls.motion(s.motion)), ("vertex", v1, calls.vertex_tangent(s.v_fields))):
                    if not np.array_equal(_bits(batch), _bits(single)):
                        bad.append(f"{name} tangent batch (width {width}) differs from the single calls in "
                                   f"{int((_bits(batch) != _bits(single)).sum())} values")
            if s.v_garbage is not None and not np.array_equal(_bits(calls.vertex_tangent(s.v_garbage)), _bits(v1)):
                bad.append("garbage in the rows of welded non-representatives changes the vertex tangent")
            mot[:, where], vtan[:, where] = m1, v1
            # -- vertex adjoint, twice
            for i, g in enumerate(s.vg):
                g_part = np.ascontiguousarray(g[rows_ref][where])
                grads[i] += calls.vertex_adjoint(g_part)
                rerun[i] += calls.vertex_adjoint(g_part)
            # -- ray matrix: a part is bit for bit rows of the whole frame's
            part = ctx.ray_matrix(with_depth=True)
            px = (rows_ref[where][:, None] * rx + np.arange(rx)).reshape(-1)
            if not rmc.bit_equal_rows(part, whole, px):
                bad.append("the ray matrix of a part is not the whole frame's rows bit for bit")
            if plain is not None and n_parts == 1:
                place(plain)
                pm, pv = plain.render_motion_tangent(s.motion), plain.render_vertex_tangent(s.v_fields)
                log(f"seed {s.seed} {s.walk_option}: against a context with default walk options the motion tangent differs "
                    f"in {int((_bits(pm) != _bits(m1)).sum())} values, the vertex tangent in {int((_bits(pv) != _bits(v1)).sum())}")
            after = ctx.stats()
            if (after["segments"], after["covered_pixels"]) != (st["segments"], st["covered_pixels"]):
                bad.append("stats() changed over the geometry calls")
            if not np.array_equal(_bits(ctx.render()), _bits(before)):
                bad.append("a plain render after the geometry calls differs from the one before them")
    # -- identities on the GPU's own results
    at = s.motion_at
    if mot[at["z_translation"]].any():
        bad.append(f"a z-translation gives {int((mot[at['z_translation']] != 0).sum())} non-zero values")
    for key, power in (("up", 20), ("down", -20)):
        n_bad, n_used = _scaled_bits_differ(mot[at["base"]], mot[at[key]], power)
        if n_bad:
            bad.append(f"the field times 2^{power}: {n_bad} of {n_used} values are not the field's scaled exactly")
    pix, cell = s.segments[:2]
    hit = np.zeros(rx * ry, bool)
    hit[pix[(s.rep[cells] == s.single_point).any(1)[cell]]] = True
    off = ~hit.reshape(ry, rx)[rows_ref]
    if vtan[s.v_single][off].any():
        bad.append(f"the single-point field moves {int(vtan[s.v_single][off].any(-1).sum())} pixels whose rays miss the point's cells")
    welded = s.rep != np.arange(n_pts)
    for i, g in enumerate(grads):
        if g[welded].any():
            bad.append(f"vertex adjoint {i}: welded non-representatives hold non-zero gradients")
    g64 = s.vg[0][rows_ref].astype(np.float64)
    for j in (s.v_compare[0], s.v_compare[-1]):
        out = vtan[j].astype(np.float64)
        lhs, rhs = float((g64 * out).sum()), float((grads[0] * s.v_fields[j]).sum())
        bar = 2.0 ** -22 * float((np.abs(g64) * np.abs(out)).sum()) + ABS_FLOOR_32
        r = worst.add("duality", np.array([abs(lhs - rhs) / bar]), s.seed, f"field {j}")
        if not r <= 1.0:
            bad.append(f"duality, field {j}: <g, J v> = {lhs:.9g}, <J^T g, v> = {rhs:.9g}, difference / bar {r:.3g}")
    # -- ray matrix against the reference's lists
    e = dz_err(s)
    keep = np.ones(len(pix), bool) if skip is None else ~skip.reshape(-1)[pix]
    try:
        r = rmc.check_against_reference(whole, tuple(a[keep] for a in s.segments), e, rx * ry, len(cells), int(keep.sum()),
                                        f"seed {s.seed} ray matrix", log=lambda t: None)
        worst.add("ray_matrix", np.array(r), s.seed, "(dz, z_exit)")
    except AssertionError as err:
        worst.add("ray_matrix", np.array([np.inf]), s.seed)
        bad.append(f"ray matrix: {err or 'structure differs from the reference'}")
    # -- against the restatements, element by element
    m = ar.ray_matrices(s.xyz, s.cells, s.alpha, s.q, s.rots, rx, ry, B, s.limit, rows_ref)
    geo = vr.segment_faces(s.xyz, s.cells, s.rots, rx, ry, B, rows_ref)
    skip_ref = None if skip is None else skip[rows_ref]
    cov, mc, gc = covered_only(m, geo)
    skip_cov = None if skip_ref is None else skip_ref.reshape(-1)[cov]
    found = []

    def images(got, ref, what, kind):
        def full(v):  # (a pixel without a segment: 0, bounds included)
            out = np.zeros(len(cov))
            out[cov] = v
            return out.reshape(nr, rx)
        td, Id, x = ref
        found.append((kind, what, np.stack([ratio(got[..., 0], full(td), full(x["scale_tau"]), full(x["sens_tau"]), e, R_OUT),
                                            ratio(got[..., 1], full(Id), full(x["scale_I"]), full(x["sens_I"]), e, R_OUT)], axis=-1)))

    for j in range(km):
        images(mot[j], mr.motion_of(mc, gc, s.motion[j], skip_cov, with_scale=True), f"field {j}", "motion_tangent")
    for j in s.v_compare:
        images(vtan[j], vt.tangent_of(mc, gc, s.cells, s.rots, s.v_fields[j], skip_cov, with_scale=True), f"field {j}", "vertex_tangent")
    for i, g in enumerate(s.vg):
        ref = vr.gradients_of(m, geo, s.cells, n_pts, s.rots, g[rows_ref], skip_ref)
        on_rep = {k: np.zeros((n_pts, 3)) for k in ("raw", "scale_raw", "sens_raw")}
        for k, v in on_rep.items():
            np.add.at(v, s.rep, ref[k])  # the group's sum on its representative
        found.append(("vertex_adjoint", f"image {i}", ratio(grads[i], on_rep["raw"], on_rep["scale_raw"], on_rep["sens_raw"], e)))
        # two runs: tests/test_gpu_vertex_adjoint.py::_assert_same_run's bar, per part
        tol = n_parts * (1e-12 * np.abs(grads[i]) + 1e-15 * np.abs(grads[i]).max()) + ABS_FLOOR
        found.append(("vertex_adjoint_rerun", f"image {i}", np.abs(rerun[i] - grads[i]) / tol))
    for kind, what, r in found:
        top = worst.add(kind, r, s.seed, what)
        if not top <= 1.0:
            i = np.unravel_index(int(np.argmax(r)), r.shape)
            bad.append(f"{kind} {what}: {int((~(r <= 1.0)).sum())} elements beyond the bar, worst error / tol {top:.3g} at {tuple(int(v) for v in i)}")
    return bad


def describe_geometry(s):
    return (describe(s) + f"; {len(s.motion)} affine and {len(s.v_fields)} per-point fields, {len(s.vg)} upstream images, "
            f"vertex_merge {s.vertex_merge}, cell_order {s.cell_order}" + (f", {s.walk_option[0]} {s.walk_option[1]}" if s.walk_option else "")
            + (", moved" if s.moved else "") + (f", {s.merged} welded points" if s.merged else ""))


def gpu_chords(s, pixel):
    """The GPU's own chords along the ray of one pixel (row * res_x + col) of the whole frame: grad_alpha for an upstream
    image that is (g_tau, g_I) = (1, 0) there is dz per cell.  Returns (cells, the reference's dz, the GPU's, F) in
    processing order - how the chord errors in the bar's derivation were read (`derivative_fuzz.py chords SEED PIXEL`)."""
    from course5_amd import capi
    rx, ry = s.res
    pix, cell, _zh, dz, slope = s.segments
    sel = pix == pixel
    with capi.Context(0) as ctx:
        if s.soup:
            ctx.set_option("algorithm", 1)
        ctx.upload_grid(s.xyz, s.cells, s.alpha, s.q)
        ctx.set_image(rx, ry, B)
        ctx.set_view(s.rots)
        ctx.set_alpha_limit(s.limit)
        g = np.zeros((ry, rx, 2), np.float32)
        g[pixel // rx, pixel % rx, 0] = 1.0
        ga, _gq = ctx.render_adjoint(g)
    return cell[sel], dz[sel], ga[cell[sel]], np.maximum(1.0, slope[sel])


# ---- the forward sweep: the render itself, frame by frame --------------------------------------------------------------

def longest_edge(xyz, cells):
    """The longest edge of any cell (what the library multiplies the largest effective alpha with: csrc/grid.hip)."""
    c = np.asarray(cells).reshape(-1, 4)
    e = xyz[c[:, [0, 0, 0, 1, 1, 2]]] - xyz[c[:, [1, 2, 3, 2, 3, 3]]]
    return float(np.sqrt((e ** 2).sum(-1)).max())


def exp_rule(alpha, limit, L):
    """min(largest alpha, limit) x longest edge: below 0.125 the library takes every exp of the frame by the short series
    (csrc/frame.hip: small_exp_only; its own edge carries a margin of 1e-9, so 0.124 and 0.126 decide it)."""
    return min(float(np.max(alpha)), float(limit)) * L


def to_rule(alpha, limit, cls, L, target):
    """alpha and limit times f so that exp_rule gives `target`; the classes that are defined by the limit (at it, the two
    doubles next to it) made again from the new one.  Returns (alpha, limit)."""
    f = target / exp_rule(alpha, limit, L)
    alpha, limit = alpha * f, float(limit * f)
    alpha[cls == 3] = limit
    alpha[cls == 4] = np.nextafter(limit, np.inf)
    alpha[cls == 5] = np.nextafter(limit, -np.inf)
    return alpha, limit


def forward_scene(seed, mesh=scene):
    """derivative_scene(seed), unchanged, with what the forward sweep adds drawn from a stream of its own (module
    docstring: the forward sweep)."""
    from tests.fuzz_scenes import VARIANTS
    s = derivative_scene(seed, mesh)
    rng = np.random.default_rng([seed, 0xF0])
    n = len(s.cells)
    s.L = longest_edge(s.xyz, s.cells)
    s.cls = alpha_class(s.alpha, s.limit)
    # -- class eps_to_1e-6: as drawn in one scene of four (there the bar of I is the reference's own cancellation noise)
    s.keep_eps = bool(rng.integers(4) == 0)
    redrawn = rng.uniform(0.0, 1.0, n) * s.limit
    if not s.keep_eps:
        s.alpha = np.where(s.cls == 2, redrawn, s.alpha)
    # -- the exp regime
    s.regime = ("as_drawn", "short", "just_over")[int(rng.integers(3))]
    if s.regime != "as_drawn":
        s.alpha, s.limit = to_rule(s.alpha.copy(), s.limit, s.cls, s.L, 0.124 if s.regime == "short" else 0.126)
    # -- the kernel variant
    s.depth_split, s.tilt, s.stage_slots = 0, (0.0, 0.0), 14
    if rng.integers(2) == 0:
        s.variant = DEFAULT_VARIANT
        s.stage_slots = (14, 0)[int(rng.integers(2))]
        k = int(rng.integers(3))
        if k == 1:
            s.depth_split = 1
        elif k == 2:
            s.depth_split = int(rng.integers(2, 8))
            s.tilt = tuple(float(v) for v in rng.uniform(-1.5, 1.5, 2))
    else:
        s.variant = VARIANTS[int(rng.integers(len(VARIANTS)))]
        if s.variant[0] == 3:
            s.stage_slots = 21
    s.cutoff = 0.0 if s.variant[1] == 1 and rng.integers(2) == 0 else None  # (None: the default, 1e-12)
    # -- the call form and the transition
    s.form = ("render", "render_device", "host_async")[int(rng.integers(3))]
    if s.form == "host_async" and s.layout != "whole":
        s.form = "frame_rows"
    s.transition = ("scalars", "limit", "points")[int(rng.integers(3))]
    s.subtle = bool(rng.integers(2) == 0)  # (scalars: the largest a dz to 1.75; else the median to 4)
    s.device_update = bool(seed % 2)
    s.stretch = rng.uniform(0.0, 1.0, n)
    c = s.xyz.mean(0)
    s.small = c + (s.xyz - c) / 16.0
    return s


def predicted_kernel(s, alpha, limit, L):
    """The walk the launch plan selects for this state (csrc/walk_plan.hpp: walk_plan, checked against the rules written
    out again in tests/cpp/walk_plan_check.cpp; csrc/walk_kernels.hip: launch_walk_t switches on it).  Predicted, not
    read back: the library has no read-out of the kernel that ran."""
    if s.soup:
        return "bin_sort_resolve"
    lds, order, tile = s.variant
    short = exp_rule(alpha, limit, L) * (1.0 + 1e-9) < 0.125
    if lds < 2:
        return f"walk_composite{'_lds' if lds else ''}<{tile}, {order}>"
    if tile != 3:
        return f"walk_composite_lds<{tile}, {order}, dma, {21 if s.stage_slots == 21 else 14}>"
    slots = {0: "14 or 21 by the frame before", 14: "14", 21: "21"}[s.stage_slots]
    series = "SMALLEXP unless 21 slots" if short and s.stage_slots == 0 else "SMALLEXP" if short and s.stage_slots == 14 else "general exp"
    split = "" if order else {0: ", SPLIT by the frame before", 1: ""}.get(s.depth_split, f", SPLIT {s.depth_split}")
    return f"walk_composite_lds<3, {order}, dma, {slots}, {series}{split}>"


def describe_forward(s):
    return (describe(s) + f"; {s.regime}, variant {s.variant}, stage_slots {s.stage_slots}, depth_split {s.depth_split}"
            + (", cutoff 0" if s.cutoff == 0.0 else "") + f", {s.form}, transition {s.transition}"
            + (", eps class as drawn" if s.keep_eps else ""))


class ForwardTally:
    """What the forward sweep reports beside Worst: the fp32 values compared bit for bit with the port oracle's image
    ("integration" 0, whole rays) and how many differ; per scene the share of covered pixels whose bar of I is dominated
    by `cancel`; the kernels the rule predicted."""

    def __init__(self):
        self.bit_values = self.bit_differ = self.frames = 0
        self.cancel_share = {}
        self.kernels = {}

    def lines(self):
        none = sum(1 for v in self.cancel_share.values() if v == 0.0)
        out = [f"{self.frames} frames compared; {self.bit_differ} of {self.bit_values} fp32 values (\"integration\" 0, whole rays) "
               f"are not the port oracle's bit for bit",
               f"covered pixels whose bar of I is dominated by cancel: none in {none} of {len(self.cancel_share)} scenes"]
        out += [f"predicted {k}: {v} states" for k, v in sorted(self.kernels.items())]
        return out


def cancel_share(I, x, cov):
    """The share of the covered pixels at which cancel exceeds 2^-23 |I| (forward_of's arrays of one frame; cov: the
    pixels with a segment)."""
    n = int(np.isfinite(I[cov]).sum())
    return float((x["cancel"][cov] > R_OUT * np.abs(I[cov])).sum()) / max(n, 1)


def forward_reference(s, xyz, alpha, limit, rows_ref, oracle, solid=None):
    """One state's reference: forward_of's images and bounds of the rows rows_ref, the port oracle's fp32 image of those
    rows, and the set of solid-marked pixels - the ORACLE'S, not the GPU's."""
    rx, ry = s.res
    kw = {} if solid is None else dict(solid_tets=solid, solid_colour=np.full(len(solid), np.nan))
    o = oracle.render(xyz, s.cells, alpha, s.q, s.rots, rx, ry, B, alpha_limit=limit, threads=8, **kw)
    img = o["image"][rows_ref]
    skip = np.isnan(img[..., 0]) if solid is not None else None
    m = ar.ray_matrices(xyz, s.cells, alpha, s.q, s.rots, rx, ry, B, limit, rows_ref)
    tau, I, x = ar.forward_of(m, skip, with_scale=True)
    seg_rows = m["valid"].sum(1).reshape(m["shape"]).sum(1)
    cov = m["valid"].any(1).reshape(m["shape"])
    return types.SimpleNamespace(tau=tau, I=I, x=x, skip=skip, covered=cov, oracle=img, seg_rows=seg_rows,
                                 cov_rows=cov.sum(1), alpha=alpha, limit=limit, xyz=xyz)


def forward_ratio(img, ref, dz_e, cutoff):
    """error / tolerance of one frame [rows, res_x, 2] against forward_reference's state (module docstring: the forward
    sweep's bar), and the mismatches that are not a matter of tolerance (strings)."""
    bad = []
    img = np.asarray(img)
    nan = np.isnan(img)
    skip = np.zeros(img.shape[:2], bool) if ref.skip is None else ref.skip
    for ch, name in ((0, "tau"), (1, "I")):
        if not np.array_equal(nan[..., ch], skip):
            bad.append(f"{name}: the NaN pixels are not the oracle's solid-marked ones ({int((nan[..., ch] != skip).sum())} differ)")
    empty = ~ref.covered & ~skip
    if (img[empty] != 0).any():
        bad.append(f"{int((img[empty] != 0).any(-1).sum())} pixels without a segment are not exactly 0")
    x = ref.x
    use = ~skip
    got = np.where(use[..., None], img, 0.0)
    extra_I = x["cancel"] + cutoff * x["emission"]
    r = np.stack([ratio(got[..., 0], np.where(use, ref.tau, 0.0), x["scale_tau"], x["sens_tau"], dz_e, R_OUT),
                  ratio(got[..., 1], np.where(use, ref.I, 0.0), x["scale_I"], x["sens_I"], dz_e, R_OUT, extra=extra_I)], axis=-1)
    r[~use] = 0.0
    return r, bad


def _apply_variant(ctx, s):
    lds, order, tile = s.variant
    if s.soup:
        ctx.set_option("algorithm", 1)
    ctx.set_option("lds_stage", min(lds, 2))
    ctx.set_option("stage_slots", s.stage_slots)
    ctx.set_option("integration", order)
    ctx.set_option("tile", tile)
    ctx.set_option("depth_split", s.depth_split)
    ctx.set_option("split_tilt_x", s.tilt[0])
    ctx.set_option("split_tilt_y", s.tilt[1])
    if s.cutoff is not None:
        ctx.set_option("transmittance_cutoff", s.cutoff)


def forward_frames(ctx, s, form, n_frames, parts, rows_ref, check_stats):
    """n_frames frames in a row of every part of the layout through one call form.  Returns n_frames images of the rows
    rows_ref, float32 [len(rows_ref), res_x, 2], the rows of the parts put back in place.  check_stats(part rows, frame):
    called after every frame whose statistics can be read (the last of a burst of outstanding ones)."""
    from course5_amd import capi
    rx, ry = s.res
    out = [np.full((len(rows_ref), rx, 2), np.float32(7e7), np.float32) for _ in range(n_frames)]
    for place, where in parts:
        if len(where) == 0:  # (a rank without rows: small images in tall tiles)
            continue
        place(ctx)
        if form == "render":
            for k in range(n_frames):
                out[k][where] = ctx.render()
                check_stats(where, k)
        elif form == "render_device":
            import torch
            for k in range(n_frames):
                t = torch.full((len(where), rx, 2), float("nan"), dtype=torch.float32, device="cuda")
                for _ in range(3):
                    ctx.render_device(t.data_ptr())
                    if ctx.synchronize() == capi.C5_OK:
                        break
                else:
                    raise RuntimeError("C5_RETRY three times in a row")
                out[k][where] = t.cpu().numpy()
                check_stats(where, k)
        else:  # outstanding frames into pinned host memory, each waited for
            full = form == "frame_rows"
            bufs = [ctx.host_image(full=full) for _ in range(n_frames)]
            try:
                for _ in range(3):
                    for b in bufs:
                        b[...] = np.float32(7e7)
                        (ctx.render_frame_rows_async if full else ctx.render_host_async)(b)
                    if all([ctx.render_host_wait() == capi.C5_OK for _b in bufs]):
                        break
                else:
                    raise RuntimeError("C5_RETRY three times in a row")
                check_stats(where, n_frames - 1)
                for k, b in enumerate(bufs):
                    out[k][where] = b[rows_ref[where]] if full else b
            finally:
                for b in bufs:
                    ctx.free_host_image(b)
    return out


def check_forward(s, worst, oracle, tally=None, log=print):
    """The forward render of one used scene (forward_scene, qualify first) in a context of its own, frame by frame: three
    frames of the scene's configuration, one transition, two frames after it and two after going back.  Returns the
    mismatches, strings."""
    from course5_amd import capi
    tally = tally if tally is not None else ForwardTally()
    bad = []
    rx, ry = s.res
    lds, order, tile = s.variant
    e = dz_err(s)  # (the drawn grid's: the shrunk one's coordinates are no larger)
    cutoff = (1e-12 if s.cutoff is None else s.cutoff) if order == 1 and not s.soup else 0.0
    whole_rays = s.soup or order == 1 or s.depth_split == 1 or not (lds >= 2 and tile == 3)
    base_kind = "front_to_back" if order == 1 and not s.soup else "split" if not whole_rays and s.depth_split >= 2 else s.form
    # -- the states: (xyz, alpha, limit) the context starts in, goes to, and comes back to
    transition = s.transition
    counts = (s.n_segments, s.n_covered)
    if transition == "points":
        small = types.SimpleNamespace(**vars(s))
        small.xyz = s.small
        small.alpha, small.limit = to_rule(s.alpha.copy(), s.limit, s.cls, s.L / 16.0, 0.124)
        small.segments = ar.segment_lists(small.xyz, s.cells, s.rots, rx, ry, B, with_slope=True)
        why = qualify(small, oracle)
        if why is None:
            start = (small.xyz, small.alpha, small.limit)
            there = (s.xyz, small.alpha, small.limit)
            counts = (small.n_segments, small.n_covered)
        else:
            log(f"seed {s.seed}: the shrunk grid does not qualify ({why}): the limit transition instead")
            transition = "limit"
    if transition == "scalars":
        start = (s.xyz, s.alpha, s.limit)
        a_short, l_short = (s.alpha, s.limit) if s.regime == "short" else to_rule(s.alpha.copy(), s.limit, s.cls, s.L, 0.124)
        cell, dz = s.segments[1], s.segments[3]
        x = a_short[cell] * dz  # (the limit is raised to the largest alpha: nothing is clamped)
        g = 1.75 / float(x.max()) if s.subtle else 4.0 / max(float(np.median(x[x > 0])) if (x > 0).any() else 1.0, 1e-300)
        a_big = a_short * g
        there, back = (s.xyz, a_big, max(l_short, float(a_big.max()))), (start if s.regime == "short" else (s.xyz, a_short, l_short))
    elif transition == "limit":
        start = (s.xyz, s.alpha, s.limit)
        l_small = 0.124 / s.L
        a = s.alpha * (l_small / s.limit)
        a[s.cls == 3], a[s.cls == 4], a[s.cls == 5] = l_small, np.nextafter(l_small, np.inf), np.nextafter(l_small, -np.inf)
        a[s.cls == 6] = l_small * (1.0 + 13.0 * s.stretch[s.cls == 6])
        chord = np.zeros(len(a))  # (the top alpha to the cell with the longest chord of this view, of its class if it has one)
        np.maximum.at(chord, s.segments[1], s.segments[3])
        a[int(np.argmax(np.where(s.cls == 6, chord, -1.0) if (s.cls == 6).any() else chord))] = 14.0 * l_small
        there, back = (s.xyz, a, float(a.max())), (s.xyz, a, l_small)
    elif transition == "points":
        back = start

    solid = _solid_of(s) if s.solid else None
    if s.layout == "range":
        b, c = s.row_range
        rows_ref = np.arange(b, b + c)
        parts = [(lambda x: x.set_row_range(b, c), np.arange(c))]
    elif s.layout == "cyclic":
        rows_ref = np.arange(ry)
        parts = [((lambda x, r=r: x.set_row_tiles(s.tile_rows, r, s.world)), sharding.local_rows(ry, s.tile_rows, r, s.world))
                 for r in range(s.world)]
    else:
        rows_ref = np.arange(ry)
        parts = [(lambda x: None, np.arange(ry))]

    def hold(images, ref, kind, what):
        name = predicted_kernel(s, ref.alpha, ref.limit, longest_edge(ref.xyz, s.cells))
        tally.kernels[name] = tally.kernels.get(name, 0) + 1
        log(f"seed {s.seed} {what}: rule {exp_rule(ref.alpha, ref.limit, longest_edge(ref.xyz, s.cells)):.4g}, predicted {name}")
        for k, img in enumerate(images):
            r, wrong = forward_ratio(img, ref, e, cutoff)
            bad.extend(f"{kind} {what} frame {k}: {t}" for t in wrong)
            top = worst.add(kind, r, s.seed, f"{what} frame {k}")
            tally.frames += 1
            if not top <= 1.0:
                i = np.unravel_index(int(np.argmax(r)), r.shape)
                bad.append(f"{kind} {what} frame {k}: {int((~(r <= 1.0)).sum())} values beyond the bar, worst error / tol {top:.3g} "
                           f"at (row, col, channel) {tuple(int(v) for v in i)}")
            if whole_rays and (order == 0 or s.soup):
                use = ~np.isnan(ref.oracle)
                tally.bit_values += int(use.sum())
                tally.bit_differ += int((_bits(img)[use] != _bits(ref.oracle)[use]).sum())

    with capi.Context(0) as ctx:
        _apply_variant(ctx, s)
        ctx.upload_grid(start[0], s.cells, start[1], s.q)
        ctx.set_image(rx, ry, B)
        ctx.set_view(s.rots)
        if not s.late_limit:
            ctx.set_alpha_limit(start[2])
        ctx.render()
        st = ctx.stats()
        if (st["segments"], st["covered_pixels"]) != counts:
            bad.append(f"stats: {st['segments']} segments on {st['covered_pixels']} pixels, the reference has {counts[0]} on {counts[1]}")
        if s.late_limit:
            ctx.set_alpha_limit(start[2])
        if solid is not None:
            ctx.set_solid(0, solid)

        def frames(ref, n_frames, kind, what):
            def check_stats(where, k):
                st = ctx.stats()
                want = (int(ref.seg_rows[where].sum()), int(ref.cov_rows[where].sum()))
                # (with a solid the reference's own counts depend on the order its threads bin in: line.cpp:29-67 drops the
                # hits of a pixel that is marked already; the marked pixels themselves are exact)
                if solid is None and (st["segments"], st["covered_pixels"]) != want:
                    bad.append(f"{kind} {what} frame {k}: stats report {st['segments']} segments on {st['covered_pixels']} pixels, "
                               f"the reference has {want[0]} on {want[1]}")
                if solid is not None and st["solid_pixels"] != int(ref.skip[where].sum()):
                    bad.append(f"{kind} {what} frame {k}: stats report {st['solid_pixels']} solid pixels, the oracle marks {int(ref.skip[where].sum())}")
                if st["walk_overflow"] != 0:
                    bad.append(f"{kind} {what} frame {k}: walk_overflow {st['walk_overflow']}")
            hold(forward_frames(ctx, s, s.form, n_frames, parts, rows_ref, check_stats), ref, kind, what)

        ref0 = forward_reference(s, *start, rows_ref, oracle, solid)
        tally.cancel_share[s.seed] = cancel_share(ref0.I, ref0.x, ref0.covered)
        log(f"seed {s.seed}: cancel dominates the bar of I at {100 * tally.cancel_share[s.seed]:.1f} % of the covered pixels")
        frames(ref0, 3, base_kind, "as uploaded")

        def scalars(alpha, device):
            if device:
                import torch
                ctx.update_scalars_device(torch.tensor(alpha, dtype=torch.float64, device="cuda"),
                                          torch.tensor(s.q, dtype=torch.float64, device="cuda"))
            else:
                ctx.update_scalars(alpha, s.q)

        ref_there = forward_reference(s, *there, rows_ref, oracle, solid)
        ref_back = ref0 if back is start else forward_reference(s, *back, rows_ref, oracle, solid)
        if transition == "scalars":
            kind = "after_update_scalars"
            if back is not start:
                scalars(back[1], not s.device_update)
                ctx.set_alpha_limit(back[2])
                frames(ref_back, 2, kind, "brought to the short regime")
            ctx.set_alpha_limit(there[2])  # (raised first where it would clamp)
            scalars(there[1], s.device_update)
            frames(ref_there, 2, kind, "after update_scalars" + ("_device" if s.device_update else ""))
            scalars(back[1], not s.device_update)
            ctx.set_alpha_limit(back[2])
            frames(ref_back, 2, kind, "back in the short regime by update_scalars" + ("" if s.device_update else "_device"))
        elif transition == "limit":
            kind = "after_set_limit"
            scalars(back[1], s.device_update)
            ctx.set_alpha_limit(back[2])
            frames(ref_back, 2, kind, "at the small limit")
            ctx.set_alpha_limit(there[2])
            frames(ref_there, 2, kind, "after set_alpha_limit to the top alpha")
            ctx.set_alpha_limit(back[2])
            frames(ref_back, 2, kind, "back at the small limit")
        else:
            kind = "after_update_points"
            ctx.update_points(there[0])
            frames(ref_there, 2, kind, "after update_points to the drawn size")
            ctx.update_points(back[0])
            frames(ref_back, 2, kind, "shrunk again")
    return bad


def forward_main():
    import torch  # noqa: F401  (HIP runtime load order)
    from oracle.pyoracle import Oracle
    n_scenes = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 3000
    worst, tally, oracle = Worst(FORWARD_KINDS), ForwardTally(), Oracle("port")
    t0 = time.time()
    log = lambda t: print(t, flush=True)  # noqa: E731
    used, skipped, mismatches = run(range(seed0, seed0 + n_scenes), oracle, worst, log=log, draw=forward_scene,
                                    check=lambda s, w: check_forward(s, w, oracle, tally, log))
    print(f"{n_scenes} seeds from {seed0}: {used} used, {skipped} skipped, {len(mismatches)} mismatches, "
          f"{worst.elements} elements compared, {time.time() - t0:.0f} s")
    for line in worst.lines() + tally.lines():
        print(line)
    too_many = skipped > 0.1 * n_scenes
    if too_many:
        print("more than 10 % of the seeds were skipped")
    return 1 if mismatches or too_many else 0


# ---- the second-order and exact-sum sweep, and the vertex sweep ----------------------------------------------------------

def off_tile_cut(rng, ry):
    """A row in 1..ry-1 that is no multiple of the walk's 8-row tile: rows [0, cut) and [cut, ry) cut a tile in two."""
    cut = int(rng.integers(1, ry))
    return cut - 1 if cut % 8 == 0 else cut


def second_order_scene(seed, mesh=scene):
    """derivative_scene(seed), unchanged, with the walk option of the comparison context and the second split of the rows
    drawn from a stream of its own (module docstring: the second-order sweep)."""
    s = derivative_scene(seed, mesh)
    rng = np.random.default_rng([seed, 0x2E0])
    s.compare_options = COMPARE_OPTIONS[int(rng.integers(len(COMPARE_OPTIONS)))]
    s.second_split = ("cyclic", "ranges")[int(rng.integers(2))]
    s.second_cut = off_tile_cut(rng, s.res[1])
    return s


def second_split(s):
    """[(place(ctx), the global rows the context then owns)] of the second split: together rows 0..ry-1, each once."""
    ry = s.res[1]
    if s.second_split == "cyclic":
        return [((lambda c, r=r: c.set_row_tiles(s.tile_rows, r, s.world)), sharding.local_rows(ry, s.tile_rows, r, s.world))
                for r in range(s.world)]
    return [((lambda c, b=b, n=n: c.set_row_range(b, n)), np.arange(b, b + n)) for b, n in ((0, s.second_cut), (s.second_cut, ry - s.second_cut))]


def layout_of(s):
    """(the global rows the scene's layout renders, [(place(ctx), the local rows of that part among them)])."""
    ry = s.res[1]
    if s.layout == "range":
        b, c = s.row_range
        return np.arange(b, b + c), [(lambda x: x.set_row_range(b, c), np.arange(c))]
    if s.layout == "cyclic":
        return np.arange(ry), [((lambda x, r=r: x.set_row_tiles(s.tile_rows, r, s.world)), sharding.local_rows(ry, s.tile_rows, r, s.world))
                               for r in range(s.world)]
    return np.arange(ry), [(lambda x: None, np.arange(ry))]


def covered_rows(s):
    """The rows of the scene's layout that hold a covered pixel (s.segments): the restatements are taken over these alone -
    a row without a segment adds nothing to any cell or point, and their time goes with the pixels."""
    rows = layout_of(s)[0]
    return rows[np.isin(rows, np.unique(s.segments[0] // s.res[0]))]


class BitTally:
    """The bit identities: asserted, except on soups ("algorithm" 1: lists with equal depths may change their order from
    call to call - tests/test_gpu_exact_adjoint.py), where they are counted and printed."""

    def __init__(self):
        self.counts = {}

    def hold(self, bad, s, name, same, text=None):
        if s.soup:
            c = self.counts.setdefault(name, [0, 0])
            c[0] += 1
            c[1] += 0 if same else 1
        elif not same:
            bad.append(text or f"{name}: the bits differ")

    def lines(self):
        return [f"on soups, {name}: {c[1]} of {c[0]} comparisons differ in bits (counted, not asserted)" for name, c in sorted(self.counts.items())]


def _bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same64(a, b):
    return len(a) == len(b) and all(np.array_equal(_bits64(x), _bits64(y)) for x, y in zip(a, b))


def _directions(s, j):
    return None if s.d_alpha is None else s.d_alpha[j], None if s.d_q is None else s.d_q[j]


def second_order_restatements(s, skip=None):
    """The reference half of check_second_order, no GPU: {name: ((alpha block, q block), hvp_of's / gradients_of's / ... dict
    of scales and sensitivities)} for the Hessian-vector product of direction 0 with g[0], the adjoint of g[0], the
    Gauss-Newton diagonal and the product of direction 0, over the rows of the scene's layout and their covered pixels
    only (covered_only: a pixel without a segment adds nothing to any cell).  skip: the solid-marked pixels, bool [ry, rx]."""
    rx, ry = s.res
    n = len(s.cells)
    rows_ref = covered_rows(s)
    m = ar.ray_matrices(s.xyz, s.cells, s.alpha, s.q, s.rots, rx, ry, B, s.limit, rows_ref)
    cov, mc, _ = covered_only(m, {})
    cut = lambda img: None if img is None else np.asarray(img)[rows_ref].reshape((len(cov),) + np.shape(img)[2:])[cov]  # noqa: E731
    skip_cov = cut(skip)
    da, dq = _directions(s, 0)
    g, w = cut(s.g[0]), cut(s.w)
    out = {}
    ha, hq, x = hr.hvp_of(mc, n, da, dq, g, skip_cov, with_scale=True)
    out["hvp"] = ((ha, hq), x)
    ga, gq, _tau, _I, x = ar.gradients_of(mc, n, g, skip_cov, with_scale=True)
    out["adjoint"] = ((ga, gq), x)
    terms = gr.terms_of(mc, skip_cov, with_scale=True)
    out["diagonal"] = (gr.diagonal(terms, mc["n_px"], n, w), gr.diagonal_scale(terms, mc["n_px"], n, w))
    ha, hq, _jv, x = gr.product_header(terms, mc["n_px"], n, da, dq, w)
    out["product"] = ((ha, hq), x)
    return out


def _open_scalar(s, options=(), exact=False, algorithm=None):
    """A context of the scene's own as check_scene opens it, `options` set before the upload; the alpha limit is left to
    the caller.  exact: on "adjoint_exact" 1 and "exact_sums" 1.  algorithm: set where the scene is no soup (a shard's
    context: shard_identities)."""
    from course5_amd import capi
    ctx = capi.Context(0)
    if s.soup:
        ctx.set_option("algorithm", 1)
    elif algorithm is not None:
        ctx.set_option("algorithm", algorithm)
    for k, v in options:
        ctx.set_option(k, v)
    ctx.upload_grid(s.xyz, s.cells, s.alpha, s.q)
    ctx.set_image(s.res[0], s.res[1], B)
    ctx.set_view(s.rots)
    if exact:
        _set_exact(ctx, 1)
    return ctx


def _set_exact(ctx, on):
    ctx.set_option("adjoint_exact", on)
    ctx.set_option("exact_sums", on)


def _four(calls, s, g, w):
    """The adjoint of g, the Gauss-Newton diagonal, the product and the Hessian-vector product of direction 0 (atomic or
    exact by the context's options): ({name: (alpha block, q block)}, the product's J v)."""
    da, dq = _directions(s, 0)
    ha, hq, jv = calls.gn_product(None if da is None else da[None], None if dq is None else dq[None], w)
    return {"adjoint": calls.adjoint(g), "diagonal": calls.gn_diagonal(w), "product": (ha[0], hq[0]), "hvp": calls.hvp(da, dq, g)}, jv[0]


def _counts(ctx):
    return {k: v for k, v in ctx.stats().items() if not k.startswith("ms_")}


def _exact_kinds(s, image_rows=None):
    """(name, kind, the image of the rows, the directions) of the three kinds of the bounds / sums pair."""
    from course5_amd import capi
    rows = slice(None) if image_rows is None else image_rows
    da, dq = _directions(s, 0)
    dirs = {k: v for k, v in (("d_alpha", da), ("d_q", dq)) if v is not None}
    w = None if s.w is None else np.ascontiguousarray(s.w[rows])
    g = np.ascontiguousarray(s.g[0][rows])
    return (("adjoint", capi.C5_EXACT_ADJOINT, g, {}), ("diagonal", capi.C5_EXACT_GN_DIAGONAL, w, {}), ("hvp", capi.C5_EXACT_HVP, g, dirs))


def shard_identities(s, bad, what, run):
    """The optional scene attribute s.shards (absent on every scene but those of tests/test_gpu_component_fuzz.py: grids of
    several components, where a context that renders a part of the rows cannot see an overlap that only other rows' rays
    cross, stays on the walk and takes its chords otherwise than the whole-image context, which fell back to sorted
    lists): a dict {"counts": {}}.  run(algorithm) -> {name: whether a row split over CONTEXTS OF THEIR OWN, one per part,
    opened with that "algorithm", gives the whole-image context's bits}.  With "algorithm" 1 that is asserted - what a
    caller who shards such a grid must set (fit.RowShards' docstring); with the parts left on their own judgement (None)
    it is counted into s.shards["counts"][what + name] = [comparisons, differing] and printed by the caller."""
    shards = getattr(s, "shards", None)
    if shards is None or s.soup:
        return
    for name, same in run(1).items():
        if not same:
            bad.append(f"{what}{name}: a row split over contexts of their own on \"algorithm\" 1 does not give the whole-image context's bits")
    for name, same in run(None).items():
        c = shards["counts"].setdefault(what + name, [0, 0])
        c[0] += 1
        c[1] += 0 if same else 1


def _second_split_identity(s, skip, tally, bad):
    """(e) of the module docstring: bounds per part, combined; sums per part against the combined exponents, combined;
    finished - the exponents, the integer words and the finished doubles are the whole image's."""
    from course5_amd import capi
    rx, ry = s.res
    pix = s.segments[0]
    covered = np.zeros(rx * ry, bool)
    covered[pix] = True
    covered = covered.reshape(ry, rx) & (True if skip is None else ~skip)
    live = {"adjoint": covered & (s.g[0][..., 0] != 0), "diagonal": covered & (True if s.w is None else s.w[..., 0] != 0)}
    finish = lambda e, w: (capi.exact_sums_finish(e[0], w[0], rx, ry), capi.exact_sums_finish(e[1], w[1], rx, ry))  # noqa: E731
    with _open_scalar(s, exact=True) as ctx:
        ctx.set_alpha_limit(s.limit)
        if s.solid:
            ctx.set_solid(0, _solid_of(s))
        calls = _Calls(ctx)
        single = _four(calls, s, s.g[0], s.w)[0]
        whole = {}
        for name, what, image, dirs in _exact_kinds(s):
            exps = ctx.render_exact_bounds(what, image=image, **dirs)
            words = ctx.render_exact_sums(what, *exps, image=image, **dirs)
            whole[name] = (exps, words)
            tally.hold(bad, s, "bounds, sums, finish against the single call",
                       _same64(finish(exps, words), single[name]), f"exact {name}: bounds, sums and finish do not give the single call's bits")
        parts = [(place, rows) for place, rows in second_split(s) if len(rows)]
        bounds = []
        for place, rows in parts:
            place(ctx)
            bounds.append({name: ctx.render_exact_bounds(what, image=image, **dirs) for name, what, image, dirs in _exact_kinds(s, rows)})
        combined = {name: sharding.combine_exact([b[name] + (None, None) for b in bounds])[:2] for name in whole}
        for name in whole:
            tally.hold(bad, s, "second split, exponents", all(np.array_equal(a, b) for a, b in zip(combined[name], whole[name][0])),
                       f"exact {name}: the combined exponents of the second split ({s.second_split}) are not the whole image's")
        words = []
        for place, rows in parts:
            place(ctx)
            words.append({name: ctx.render_exact_sums(what, *combined[name], image=image, **dirs) for name, what, image, dirs in _exact_kinds(s, rows)})
        for name in whole:
            total = sharding.combine_exact([combined[name] + w[name] for w in words])
            tally.hold(bad, s, "second split, words", np.array_equal(total[2], whole[name][1][0]) and np.array_equal(total[3], whole[name][1][1]),
                       f"exact {name}: the integer words of the second split ({s.second_split}) do not add up to the whole image's")
            tally.hold(bad, s, "second split, finished", _same64(finish(total[:2], total[2:]), single[name]),
                       f"exact {name}: the second split ({s.second_split}) finished is not the single whole-image call's bits")
            for (place, rows), b, w in zip(parts, bounds, words):
                # a part must hold non-zero words where it owns a cell's largest contribution (its own exponent is the
                # combined one: that contribution is at least 2^(e-1) on the cell's grid), and, for the two kinds with a
                # tau term g_tau dz / w_tau dz^2, where it holds a covered pixel whose image is not zero
                owns = any(((e == c) & (e != er.NONE)).any() for e, c in zip(b[name], combined[name]))
                if (owns or (name in live and live[name][rows].any())) and not (w[name][0].any() or w[name][1].any()):
                    bad.append(f"exact {name}: a part of the second split ({s.second_split}) with covered rows has all-zero words")

        def own_contexts(algorithm):
            from contextlib import ExitStack
            with ExitStack() as stack:
                each = []
                for place, rows in parts:
                    c = stack.enter_context(_open_scalar(s, exact=True, algorithm=algorithm))
                    c.set_alpha_limit(s.limit)
                    if s.solid:
                        c.set_solid(0, _solid_of(s))
                    place(c)
                    each.append((c, rows))
                same = {}
                for i, (name, what, _image, _dirs) in enumerate(_exact_kinds(s)):
                    kinds = [_exact_kinds(s, rows)[i] for _c, rows in each]
                    exps = sharding.combine_exact([c.render_exact_bounds(what, image=k[2], **k[3]) + (None, None)
                                                   for (c, _rows), k in zip(each, kinds)])[:2]
                    total = sharding.combine_exact([exps + c.render_exact_sums(what, *exps, image=k[2], **k[3])
                                                    for (c, _rows), k in zip(each, kinds)])
                    same[name] = _same64(finish(total[:2], total[2:]), single[name])
                return same

        shard_identities(s, bad, "exact ", own_contexts)


def check_second_order(s, worst, tally=None):
    """The Hessian-vector render and the exact-sum modes on one used scene (second_order_scene, qualify first; module
    docstring: the second-order sweep).  Returns the mismatches, strings."""
    from contextlib import ExitStack
    bad = []
    tally = tally or BitTally()
    n = len(s.cells)
    with ExitStack() as stack:
        ctx = stack.enter_context(_open_scalar(s))
        if not s.late_limit:
            ctx.set_alpha_limit(s.limit)
        ctx.render()
        st = ctx.stats()
        if (st["segments"], st["covered_pixels"]) != (s.n_segments, s.n_covered):
            bad.append(f"stats: {st['segments']} segments on {st['covered_pixels']} pixels, the reference has "
                       f"{s.n_segments} on {s.n_covered}")
        if s.late_limit:
            ctx.set_alpha_limit(s.limit)  # (after a frame: the cell records carry the clamp and must be rebuilt)
        # (the comparison context renders nothing but the layout's parts: on a scene with s.shards it is a shard's context)
        sharded = getattr(s, "shards", None) is not None and s.layout != "whole"
        cmp_ctx = stack.enter_context(_open_scalar(s, s.compare_options, exact=True, algorithm=1 if sharded else None))
        cmp_ctx.set_alpha_limit(s.limit)
        skip = None
        if s.solid:
            ctx.set_solid(0, _solid_of(s))
            cmp_ctx.set_solid(0, _solid_of(s))
            skip = np.isnan(ctx.render()[..., 0])
        rows_ref, parts = layout_of(s)
        g_ref = s.g[:, rows_ref]
        w_ref = None if s.w is None else s.w[rows_ref]
        calls = _DeviceCalls(ctx) if s.device else _Calls(ctx)
        da, dq = _directions(s, 0)
        ua, uq = _directions(s, 1)
        names = ("adjoint", "diagonal", "product", "hvp")
        sums = {k: [np.zeros(n), np.zeros(n)] for k in ("hvp", "hvp_u", "only_alpha", "only_q") + tuple("exact_" + k for k in names)}

        def add(name, pair):
            for acc, v in zip(sums[name], pair):
                if v is not None:
                    acc += v

        for place, where in parts:
            if len(where) == 0:  # (a rank without rows: small images in tall tiles)
                continue
            place(ctx), place(cmp_ctx)
            before, counts = ctx.render(), _counts(ctx)
            g = np.ascontiguousarray(g_ref[0, where])
            w = None if w_ref is None else np.ascontiguousarray(w_ref[where])
            # -- atomic mode: the Hessian-vector render
            add("hvp", calls.hvp(da, dq, g))
            add("hvp_u", calls.hvp(ua, uq, g))
            only_a, none_q = calls.hvp(da, dq, g, fit=("alpha",))
            none_a, only_q = calls.hvp(da, dq, g, fit=("q",))
            if none_q is not None or none_a is not None:
                bad.append("render_hvp returns a block that fit does not name")
            add("only_alpha", (only_a, None)), add("only_q", (None, only_q))
            atomic = _four(calls, s, g, w)[0]
            if _counts(ctx) != counts:
                bad.append("stats() changed over the Hessian-vector calls")
            if not np.array_equal(_bits(ctx.render()), _bits(before)):
                bad.append("a plain render after the Hessian-vector calls differs from the one before them")
            # -- exact modes, on the same context and inputs
            _set_exact(ctx, 1)
            exact, jv = _four(calls, s, g, w)
            again = _four(calls, s, g, w)[0]
            tangent = calls.tangent(da, dq)
            weighted = tangent if w is None else (w * tangent).astype(np.float32)
            as_adjoint = calls.adjoint(np.ascontiguousarray(weighted))
            other = _four(_Calls(cmp_ctx), s, g, w)[0]
            _set_exact(ctx, 0)
            for name in names:
                add("exact_" + name, exact[name])
                tally.hold(bad, s, "call to call", _same64(again[name], exact[name]), f"exact {name}: a second call gives other bits")
                tally.hold(bad, s, "comparison context", _same64(other[name], exact[name]),
                           f"exact {name}: a context on {s.compare_options or 'the default options'} gives other bits")
            if not _same64(as_adjoint, exact["product"]):
                bad.append("the exact product is not the exact adjoint of weight x fp32(J v) bit for bit")
            if not np.array_equal(_bits(jv), _bits(tangent)):
                bad.append(f"the exact product's J v differs from the tangent in {int((_bits(jv) != _bits(tangent)).sum())} values")
            # -- afterwards: the atomic mode on its run-to-run bar (tests/test_gpu_exact_fit.py), the frame as it was
            after = _four(calls, s, g, w)[0]
            for name in names:
                for a, b in zip(after[name], atomic[name]):
                    if not (np.abs(a - b) <= 1e-12 * np.abs(b) + 1e-15 * np.abs(b).max() + ABS_FLOOR).all():
                        bad.append(f"atomic {name} after the exact calls: beyond rtol 1e-12, atol 1e-15 x max of the call before them")
            if _counts(ctx) != counts:
                bad.append("stats() changed over the exact calls")
            if not np.array_equal(_bits(ctx.render()), _bits(before)):
                bad.append("a plain render after the exact calls differs from the one before them")
    _second_split_identity(s, skip, tally, bad)
    # -- identities on the library's own results
    frozen = (s.alpha > s.limit) | (np.minimum(s.alpha, s.limit) < EPS)
    for name in ("hvp", "hvp_u", "only_alpha", "exact_hvp"):
        if sums[name][0][frozen].any():
            bad.append(f"{name}: {int((sums[name][0][frozen] != 0).sum())} clamped or inactive cells have a non-zero h_alpha")
    zero = np.zeros(n)
    u, v = [zero if t is None else t for t in (ua, uq)], [zero if t is None else t for t in (da, dq)]
    hv, hu = sums["hvp"], sums["hvp_u"]
    lhs, rhs = float(u[0] @ hv[0] + u[1] @ hv[1]), float(v[0] @ hu[0] + v[1] @ hu[1])
    bar = 1e-9 * float(sum(np.abs(a * b).sum() for a, b in ((u[0], hv[0]), (u[1], hv[1]), (v[0], hu[0]), (v[1], hu[1]))))
    r = worst.add("hvp_symmetry", np.array([0.0 if lhs == rhs else abs(lhs - rhs) / bar if bar else np.inf]), s.seed, "directions 0, 1")
    if not r <= 1.0:
        bad.append(f"symmetry: <u, H v> = {lhs:.15g}, <v, H u> = {rhs:.15g}, difference / bar {r:.3g}")
    # -- against the restatements, element by element
    e = dz_err(s)
    ref = second_order_restatements(s, skip)

    def pair(got, name, r_scale=R64):
        want, x = ref[name]
        return np.stack([ratio(got[0], want[0], x["scale_alpha"], x["sens_alpha"], e, r_scale=r_scale),
                         ratio(got[1], want[1], x["scale_q"], x["sens_q"], e, r_scale=r_scale)])

    found = [("hvp", "(alpha, q)", pair(sums["hvp"], "hvp")),
             ("hvp", "one output at a time (alpha, q)", pair((sums["only_alpha"][0], sums["only_q"][1]), "hvp")),
             ("exact_adjoint", "(alpha, q)", pair(sums["exact_adjoint"], "adjoint")),
             ("exact_gn_diagonal", "(alpha, q)", pair(sums["exact_diagonal"], "diagonal")),
             ("exact_gn_product", "(alpha, q)", pair(sums["exact_product"], "product", R64 + R_H)),
             ("exact_hvp", "(alpha, q)", pair(sums["exact_hvp"], "hvp"))]
    for kind, what, r in found:
        top = worst.add(kind, r, s.seed, what)
        if not top <= 1.0:
            i = np.unravel_index(int(np.argmax(r)), r.shape)
            bad.append(f"{kind} {what}: {int((~(r <= 1.0)).sum())} elements beyond the bar, worst error / tol {top:.3g} at {tuple(int(v) for v in i)}")
    return bad


def describe_second_order(s):
    return (describe(s) + f"; comparison context on {dict(s.compare_options) or 'the default options'}, second split {s.second_split}"
            + (f" at row {s.second_cut}" if s.second_split == "ranges" else f" ({s.tile_rows} rows, world {s.world})"))


def vertex_batch(s):
    """The upstream images of the vertex sweep's batch: s.vg, then g[1:K] - up to 13, more than one pass at either width."""
    return np.stack(list(s.vg) + list(s.g[1:s.k]))


def vertex_restatements(s, skip=None):
    """The reference half of check_vertex_exact, no GPU: per image of s.vg the dict {raw, scale_raw, sens_raw} [n_pts, 3] of
    vertex_adjoint_reference.gradients_of over the rows of the scene's layout (covered pixels only), a weld group's sums
    on its representative."""
    rx, ry = s.res
    n_pts = len(s.xyz)
    rows_ref = covered_rows(s)
    m = ar.ray_matrices(s.xyz, s.cells, s.alpha, s.q, s.rots, rx, ry, B, s.limit, rows_ref)
    geo = vr.segment_faces(s.xyz, s.cells, s.rots, rx, ry, B, rows_ref)
    cov, mc, gc = covered_only(m, geo)
    skip_cov = None if skip is None else skip[rows_ref].reshape(-1)[cov]
    out = []
    for g in s.vg:
        ref = vr.gradients_of(mc, gc, s.cells, n_pts, s.rots, g[rows_ref].reshape(-1, 2)[cov], skip_cov)
        on_rep = {k: np.zeros((n_pts, 3)) for k in ("raw", "scale_raw", "sens_raw")}
        for k, v in on_rep.items():
            np.add.at(v, s.rep, ref[k])  # the group's sum on its representative
        out.append(on_rep)
    return out


def check_vertex_exact(s, worst, tally=None):
    """The batched vertex adjoint and the exact vertex adjoint sums on one used scene (geometry_scene, qualify first; module
    docstring: the vertex sweep).  Returns the mismatches, strings."""
    from contextlib import ExitStack
    bad = []
    tally = tally or BitTally()
    ry = s.res[1]
    n_pts = len(s.xyz)
    batch = vertex_batch(s)
    nb = len(batch)
    welded = s.rep != np.arange(n_pts)
    with ExitStack() as stack:
        ctx = stack.enter_context(_open(s, s.displaced if s.moved else s.xyz, s.walk_option))
        flipped = stack.enter_context(_open(s, s.xyz, s.walk_option, cell_order=1 - s.cell_order, vertex_merge=1 - s.vertex_merge))
        if not s.late_limit:
            ctx.set_alpha_limit(s.limit)
        ctx.render()
        if s.late_limit:
            ctx.set_alpha_limit(s.limit)
        flipped.set_alpha_limit(s.limit)
        calls = _GeoDeviceCalls(ctx) if s.device else _GeoCalls(ctx)
        if s.moved:  # one call on the displaced grid (its per-point and per-cell data are built for it), then into place
            calls.vertex_adjoint(s.vg[0])
            ctx.render()
            ctx.update_points(s.xyz)
            ctx.render()
        st = ctx.stats()
        if (st["segments"], st["covered_pixels"]) != (s.n_segments, s.n_covered):
            bad.append(f"stats: {st['segments']} segments on {st['covered_pixels']} pixels, the reference has {s.n_segments} on {s.n_covered}")
        skip = None
        if s.solid:
            for c in (ctx, flipped):
                c.set_solid(0, _solid_of(s))
            skip = np.isnan(ctx.render()[..., 0])
        rows_ref, parts = layout_of(s)
        # -- "vertex_exact" 1 on the whole image: the single calls, the other cell order and merge, the batches, duality
        ctx.set_option("vertex_exact", 1)
        flipped.set_option("vertex_exact", 1)
        singles = np.stack([calls.vertex_adjoint(g) for g in batch])
        tally.hold(bad, s, "call to call", np.array_equal(_bits64(calls.vertex_adjoint(batch[0])), _bits64(singles[0])),
                   "vertex_exact: a second call gives other bits")
        tally.hold(bad, s, "other cell_order and vertex_merge", np.array_equal(_bits64(flipped.render_vertex_adjoint(batch[0])), _bits64(singles[0])),
                   f"vertex_exact: cell_order {1 - s.cell_order}, vertex_merge {1 - s.vertex_merge} give other bits than {s.cell_order}, {s.vertex_merge}")
        for width in (4, 8):
            ctx.set_option("batch_width", width)
            got = calls.vertex_adjoint_batch(batch)
            tally.hold(bad, s, "batch against single calls", np.array_equal(_bits64(got), _bits64(singles)),
                       f"vertex_exact: the batch of {nb} (width {width}) differs from the single calls in {int((_bits64(got) != _bits64(singles)).sum())} values")
        if _bits64(singles[:, welded]).any():
            bad.append("vertex_exact: welded non-representatives are not +0.0 to the bit")
        j = s.v_compare[0]
        out = ctx.render_vertex_tangent(s.v_fields[j:j + 1])[0].astype(np.float64)
        g64 = batch[0].astype(np.float64)
        lhs, rhs = float((g64 * out).sum()), float((singles[0] * s.v_fields[j]).sum())
        bar = 2.0 ** -22 * float((np.abs(g64) * np.abs(out)).sum()) + ABS_FLOOR_32
        r = worst.add("vertex_exact_duality", np.array([abs(lhs - rhs) / bar]), s.seed, f"field {j}")
        if not r <= 1.0:
            bad.append(f"vertex_exact duality, field {j}: <g, J v> = {lhs:.9g}, <J^T g, v> = {rhs:.9g}, difference / bar {r:.3g}")
        # -- the staged path: over the layout's parts where it has any, else over two ranges cut off the 8-row tile
        if s.layout == "cyclic":
            staged = [(place, rows_ref[where]) for place, where in parts if len(where)]
        else:
            cut = off_tile_cut(np.random.default_rng([s.seed, 0x7E0]), ry)
            staged = [((lambda x, b=b, c=c: x.set_row_range(b, c)), np.arange(b, b + c)) for b, c in ((0, cut), (cut, ry - cut))]
        bounds = []
        for place, rows in staged:
            place(ctx)
            bounds.append(ctx.render_vertex_exact_bounds(np.ascontiguousarray(batch[0][rows])))
        exps, _ = sharding.combine_vertex_exact([(b, None) for b in bounds])
        words = []
        for place, rows in staged:
            place(ctx)
            words.append(ctx.render_vertex_exact_sums(np.ascontiguousarray(batch[0][rows]), exps))
        _, total = sharding.combine_vertex_exact([(exps, w) for w in words])
        tally.hold(bad, s, "staged path", np.array_equal(_bits64(ctx.vertex_exact_finish(exps, total)), _bits64(singles[0])),
                   f"vertex_exact: bounds, sums and finish over {len(staged)} parts do not give the single whole-image call's bits")

        def own_contexts(algorithm):
            with ExitStack() as shard_stack:
                each = []
                for place, rows in staged:
                    c = shard_stack.enter_context(_open(s, s.xyz, s.walk_option, algorithm=algorithm))
                    c.set_alpha_limit(s.limit)
                    if s.solid:
                        c.set_solid(0, _solid_of(s))
                    place(c)
                    each.append((c, np.ascontiguousarray(batch[0][rows])))
                exps, _ = sharding.combine_vertex_exact([(c.render_vertex_exact_bounds(g), None) for c, g in each])
                _, total = sharding.combine_vertex_exact([(exps, c.render_vertex_exact_sums(g, exps)) for c, g in each])
                return {"staged path": np.array_equal(_bits64(each[0][0].vertex_exact_finish(exps, total)), _bits64(singles[0]))}

        shard_identities(s, bad, "vertex_exact ", own_contexts)
        if s.layout != "cyclic":
            ctx.set_row_range(0, ry)
        ctx.set_option("vertex_exact", 0)
        # -- over the parts of the layout: the exact single call, and the atomic mode's batches and single calls
        exact = np.zeros((n_pts, 3))
        atomic = {width: np.zeros((nb, n_pts, 3)) for width in (4, 8)}
        alone = np.zeros((nb, n_pts, 3))
        n_parts = 0
        for place, where in parts:
            if len(where) == 0:
                continue
            n_parts += 1
            place(ctx)
            before, counts = ctx.render(), _counts(ctx)
            part = np.ascontiguousarray(batch[:, rows_ref[where]])
            ctx.set_option("vertex_exact", 1)
            exact += calls.vertex_adjoint(part[0])
            ctx.set_option("vertex_exact", 0)
            for width in (4, 8):
                ctx.set_option("batch_width", width)
                atomic[width] += calls.vertex_adjoint_batch(part)
            for i in range(nb):
                alone[i] += calls.vertex_adjoint(part[i])
            if _counts(ctx) != counts:
                bad.append("stats() changed over the vertex adjoint calls")
            if not np.array_equal(_bits(ctx.render()), _bits(before)):
                bad.append("a plain render after the vertex adjoint calls differs from the one before them")
    for name, a in (("the batches", atomic[4]), ("the batches", atomic[8]), ("the single calls", alone), ("vertex_exact", exact)):
        if a[..., welded, :].any():
            bad.append(f"{name}: welded non-representatives hold non-zero gradients")
    # -- against the restatement, element by element, and the batches against the single calls
    e = dz_err(s)
    found = []
    for i, ref in enumerate(vertex_restatements(s, skip)):
        for width in (4, 8):
            found.append(("vertex_adjoint_batch", f"width {width}, image {i}", ratio(atomic[width][i], ref["raw"], ref["scale_raw"], ref["sens_raw"], e)))
        if i == 0:
            found.append(("vertex_exact", "image 0", ratio(exact, ref["raw"], ref["scale_raw"], ref["sens_raw"], e)))
    for width in (4, 8):  # check_geometry's rerun bar (tests/test_gpu_vertex_adjoint.py::_assert_same_run), per part
        tol = n_parts * (1e-12 * np.abs(alone) + 1e-15 * np.abs(alone).max(axis=(1, 2), keepdims=True)) + ABS_FLOOR
        found.append(("vertex_adjoint_batch", f"width {width} against the single calls", np.abs(atomic[width] - alone) / tol))
    for kind, what, r in found:
        top = worst.add(kind, r, s.seed, what)
        if not top <= 1.0:
            i = np.unravel_index(int(np.argmax(r)), r.shape)
            bad.append(f"{kind} {what}: {int((~(r <= 1.0)).sum())} elements beyond the bar, worst error / tol {top:.3g} at {tuple(int(v) for v in i)}")
    return bad


def sweep_main(kinds, draw, check):
    """`second` and `vertex_exact`: n seeds from seed0 in blocks of 25, the worst ratios and the soups' counts at the end."""
    import torch  # noqa: F401  (HIP runtime load order)
    from oracle.pyoracle import Oracle
    n_scenes = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 3000
    worst, tally, oracle = Worst(kinds), BitTally(), Oracle("port")
    t0 = time.time()
    used = skipped = 0
    mismatches = []
    for k in range(0, n_scenes, 25):
        u, sk, mm = run(range(seed0 + k, seed0 + min(k + 25, n_scenes)), oracle, worst, log=lambda t: print(t, flush=True),
                        draw=draw, check=lambda s, w: check(s, w, tally))
        used, skipped, mismatches = used + u, skipped + sk, mismatches + mm
        print(f"... {min(k + 25, n_scenes)} of {n_scenes} seeds, {len(mismatches)} mismatches so far", flush=True)
    print(f"{n_scenes} seeds from {seed0}: {used} used, {skipped} skipped, {len(mismatches)} mismatches, "
          f"{worst.elements} elements compared, {time.time() - t0:.0f} s")
    for line in worst.lines() + tally.lines():
        print(line)
    too_many = skipped > 0.1 * n_scenes
    if too_many:
        print("more than 10 % of the seeds were skipped")
    return 1 if mismatches or too_many else 0


def describe(s):
    return (f"{len(s.cells)} cells, {s.res[0]}x{s.res[1]}, limit {s.limit:.4g}, {s.mode}, {s.layout}, K {s.k}"
            + (", soup" if s.soup else "") + (", solid" if s.solid else "") + (", device" if s.device else "")
            + (", late limit" if s.late_limit else "") + (", no d_alpha" if s.d_alpha is None else "")
            + (", no d_q" if s.d_q is None else "") + (", no weight" if s.w is None else ""))


def run(seeds, oracle, worst, log=print, draw=None, check=None):
    """check_scene over seeds (draw / check: geometry_scene and check_geometry for the geometry sweep).  Returns (used,
    skipped, mismatches [(seed, text)])."""
    draw, check = draw or derivative_scene, check or check_scene
    used = skipped = 0
    mismatches = []
    for seed in seeds:
        s = draw(seed)
        why = qualify(s, oracle)
        if why is not None:
            skipped += 1
            log(f"seed {seed}: {why} - skipped")
            continue
        used += 1
        for text in check(s, worst):
            mismatches.append((seed, text))
            about = (describe_geometry(s) if hasattr(s, "motion") else describe_forward(s) if hasattr(s, "regime")
                     else describe_second_order(s) if hasattr(s, "compare_options") else describe(s))
            log(f"seed {seed} ({about}): {text}")
    return used, skipped, mismatches


def main():
    import torch  # noqa: F401  (HIP runtime load order)
    from oracle.pyoracle import Oracle
    if len(sys.argv) > 3 and sys.argv[1] == "chords":
        mesh = scene
        if sys.argv[2] == "unstructured":  # (the family of tests/unstructured_scenes.py)
            from tests import unstructured_scenes
            mesh = unstructured_scenes.scene
            del sys.argv[2]
        s = derivative_scene(int(sys.argv[2]), mesh)
        for c, d, got, f in zip(*gpu_chords(s, int(sys.argv[3]))):
            print(f"cell {c}: dz {d:.6g}, GPU - reference {got - d:+.3g} = {(got - d) / dz_err(s):+.2f} dz_err, F {f:.1f}")
        return 0
    if len(sys.argv) > 1 and sys.argv[1] == "forward":
        del sys.argv[1]
        return forward_main()
    if len(sys.argv) > 1 and sys.argv[1] in ("second", "vertex_exact"):
        second = sys.argv[1] == "second"
        del sys.argv[1]
        return sweep_main(*((SECOND_KINDS, second_order_scene, check_second_order) if second
                            else (VERTEX_EXACT_KINDS, geometry_scene, check_vertex_exact)))
    geometry = len(sys.argv) > 1 and sys.argv[1] == "geometry"
    if geometry:
        del sys.argv[1]
    n_scenes = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    worst = Worst(GEOMETRY_KINDS if geometry else KINDS)
    draw, check = (geometry_scene, check_geometry) if geometry else (None, None)
    t0 = time.time()
    used = skipped = 0
    mismatches = []
    oracle = Oracle("port")
    for k in range(0, n_scenes, 25):
        u, sk, mm = run(range(seed0 + k, seed0 + min(k + 25, n_scenes)), oracle, worst, log=lambda t: print(t, flush=True),
                        draw=draw, check=check)
        used, skipped, mismatches = used + u, skipped + sk, mismatches + mm
        print(f"... {min(k + 25, n_scenes)} of {n_scenes} seeds, {len(mismatches)} mismatches so far", flush=True)
    print(f"{n_scenes} seeds from {seed0}: {used} used, {skipped} skipped, {len(mismatches)} mismatches, "
          f"{worst.elements} elements compared, {time.time() - t0:.0f} s")
    for line in worst.lines():
        print(line)
    too_many = skipped > 0.1 * n_scenes
    if too_many:
        print("more than 10 % of the seeds were skipped")
    return 1 if mismatches or too_many else 0


if __name__ == "__main__":
    sys.exit(main())

"""The FORWARD render on the GPU, frame by frame and ELEMENT BY ELEMENT, against the numpy restatement
(tests/adjoint_reference.py: forward_of, itself held to 80 digits by tests/test_forward_reference_cpu.py) at the bar
    tau  2^-23 |tau| + 1e-9 scale_tau + dz_err sens_tau + 2^-103
    I    2^-23 |I|   + 1e-9 scale_I   + dz_err sens_I + cancel (+ cutoff) + 2^-103
(tests/derivative_fuzz.py: the forward sweep; forward_scene, check_forward), on the 40 scenes of
tests/test_gpu_derivative_fuzz.py in 4 blocks of 10: three frames in a row of the scene's kernel variant, call form and row
layout, then one transition of the state the walk's choice of exp depends on (update_scalars / update_scalars_device,
set_alpha_limit, update_points) with two frames after it and two after going back.  A third of the scenes sits just below
and a third just above min(largest alpha, limit) x longest edge = 1/8, where the library switches every exp of the frame to
a 10-term series without range reduction (csrc/walk_common.hpp: exp_small_nonpositive; csrc/frame.hip: small_exp_only).

Then four named tests that do not depend on the draw: a jittered Kuhn-3 box at 61x47 (off the 8x8 tile) at 0.124 and at
0.126 of that rule, and the three ways the state behind it changes - each frame held to the same bar.

Named regression cases (seeds whose scene showed something) are listed in REGRESSIONS.
"""
import time
import types

import numpy as np
import pytest

from course5_amd import capi, meshgen as mg
from tests import adjoint_reference as ar
from tests import derivative_fuzz as df

pytestmark = pytest.mark.gpu
BLOCKS, PER_BLOCK = 4, 10
B = mg.REFERENCE_BOUNDS

# seed -> what it showed
REGRESSIONS = {
}


class _Sweep:
    """The four blocks of ten seeds, each run once whichever test asks first."""

    def __init__(self, oracle):
        self.oracle, self.worst, self.tally, self.blocks = oracle, df.Worst(df.FORWARD_KINDS), df.ForwardTally(), {}

    def block(self, i):
        if i not in self.blocks:
            t0 = time.time()
            first = 3000 + PER_BLOCK * i
            self.blocks[i] = df.run(range(first, first + PER_BLOCK), self.oracle, self.worst, draw=df.forward_scene,
                                    check=lambda s, w: df.check_forward(s, w, self.oracle, self.tally))
            print(f"block {i}: {time.time() - t0:.1f} s")
        return self.blocks[i]

    def report(self):
        for line in self.worst.lines() + self.tally.lines():
            print(line)


@pytest.fixture(scope="module")
def sweep(oracle_port):
    return _Sweep(oracle_port)


@pytest.mark.parametrize("block", range(BLOCKS))
def test_random_scenes_match_the_restatement_element_by_element(sweep, block):
    used, skipped, mismatches = sweep.block(block)
    print(f"block {block}: {used} scenes used, {skipped} skipped, {sweep.worst.elements} elements compared so far")
    sweep.report()
    assert not mismatches, "\n".join(f"seed {seed}: {text}" for seed, text in mismatches)


def test_at_most_a_tenth_of_the_seeds_was_skipped(sweep):
    used = sum(sweep.block(i)[0] for i in range(BLOCKS))
    skipped = sum(sweep.block(i)[1] for i in range(BLOCKS))
    print(f"{used} scenes used, {skipped} skipped, {sweep.worst.elements} elements compared")
    sweep.report()
    assert used + skipped == BLOCKS * PER_BLOCK and skipped <= 0.1 * (used + skipped)


def test_cancel_dominates_no_pixel_in_half_of_the_scenes(sweep):
    """In at least half of the used scenes the bar of I is nowhere the reference's own cancellation noise: there a render is
    held to the fp32 rounding of its value (the same condition on the CPU: tests/test_forward_reference_cpu.py)."""
    used = sum(sweep.block(i)[0] for i in range(BLOCKS))
    share = sweep.tally.cancel_share
    assert len(share) == used
    assert 2 * sum(1 for v in share.values() if v == 0.0) >= used, share


def test_named_regression_scenes(oracle_port):
    worst, tally = df.Worst(df.FORWARD_KINDS), df.ForwardTally()
    used, _skipped, mismatches = df.run(sorted(REGRESSIONS), oracle_port, worst, draw=df.forward_scene,
                                        check=lambda s, w: df.check_forward(s, w, oracle_port, tally))
    for line in worst.lines() + tally.lines():
        print(line)
    assert used == len(REGRESSIONS) and not mismatches, "\n".join(f"seed {seed}: {text}" for seed, text in mismatches)


# ---- the named tests: a Kuhn-3 box either side of the rule, and the rule's state changed under a live context ----------

RES = (61, 47)


class _Box:
    """The scene of the named tests and its references, each computed once."""

    def __init__(self, oracle):
        self.oracle = oracle
        self.xyz, self.cells = mg.kuhn_box(3, jitter=0.1)
        n = len(self.cells)
        self.s = types.SimpleNamespace(seed="kuhn3", cells=self.cells, rots=mg.view_rotations(0.31, -0.17, 0.4), res=RES)
        rng = np.random.default_rng(61)
        self.u = rng.uniform(0.2, 1.0, n)
        self.s.q = rng.uniform(0.0, 2.0, n)
        self.s.q[::9] = 0.0
        self.L = df.longest_edge(self.xyz, self.cells)
        assert 0.4 < self.L < 0.8
        self.s.xyz = self.xyz
        self.e = df.dz_err(self.s)
        # the cell with the longest chord of this view carries the largest alpha: the exp arguments come as close to the
        # rule's min(largest alpha, limit) x longest edge as the view lets them
        _pix, cell, _zh, dz = ar.segment_lists(self.xyz, self.cells, self.s.rots, RES[0], RES[1], B)
        chord = np.zeros(n)
        np.maximum.at(chord, cell, dz)
        self.longest = int(np.argmax(chord))
        self.u[self.longest] = 1.0
        self.refs = {}

    def alpha(self, rule, L=None):
        """U[0.2, 1) x a_max with a cell at a_max and a few at 0, a_max x L = rule."""
        a = self.u * (rule / (L or self.L))
        a[5::31] = 0.0
        a[self.longest] = rule / (L or self.L)
        return a

    def ref(self, key, xyz, alpha, limit):
        if key not in self.refs:
            self.refs[key] = df.forward_reference(self.s, xyz, alpha, limit, np.arange(RES[1]), self.oracle)
        return self.refs[key]

    def open(self, xyz, alpha, limit=None, **options):
        ctx = capi.Context(0)
        for name, value in options.items():
            ctx.set_option(name, value)
        ctx.upload_grid(xyz, self.cells, alpha, self.s.q)
        ctx.set_image(RES[0], RES[1], B)
        ctx.set_view(self.s.rots)
        if limit is not None:
            ctx.set_alpha_limit(limit)
        return ctx

    def hold(self, ctx, ref, n_frames, what, cutoff=0.0):
        """n_frames frames of the context's state, each inside the bar of `ref` with the reference's counts."""
        top = 0.0
        for k in range(n_frames):
            img = ctx.render()
            st = ctx.stats()
            r, wrong = df.forward_ratio(img, ref, self.e, cutoff)
            assert not wrong, (what, k, wrong)
            i = np.unravel_index(int(np.argmax(r)), r.shape)
            print(f"{what} frame {k}: worst error / tol {r.max():.3g} at (row, col, channel) {tuple(int(v) for v in i)}; "
                  f"{int((df._bits(img) != df._bits(ref.oracle)).sum())} of {img.size} values differ from the port oracle's bits")
            assert r.max() <= 1.0, (what, k, float(r.max()), i)
            assert (st["segments"], st["covered_pixels"]) == (int(ref.seg_rows.sum()), int(ref.cov_rows.sum())), (what, k)
            assert st["walk_overflow"] == 0
            top = max(top, float(r.max()))
        return top


@pytest.fixture(scope="module")
def box(oracle_port):
    return _Box(oracle_port)


# "stage_slots" 0 (the default) lets the frame before decide between 14 and 21 staged cells, and this scene's 48 segments per
# cell make that 21, which has no instantiation with the short series: a library that ALWAYS took the short series passed
# every named test on the default options alone (profiles/forward_fuzz.md).  So each configuration comes a second time
# with "stage_slots" 14, where the rule alone decides.
CONFIGS = {"default": {}, "depth_split_2": {"depth_split": 2}, "depth_split_4": {"depth_split": 4}, "front_to_back": {"integration": 1}}
CONFIGS.update({f"{k}_14_slots": dict(v, stage_slots=14) for k, v in list(CONFIGS.items())})
SLOTS = pytest.mark.parametrize("slots", [0, 14], ids=["slots_by_the_frame_before", "14_slots"])


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_the_short_series_kernel_against_the_reference(box, config):
    """a_max x L = 0.124, default options (and rays cut in 2 and 4 slabs; front to back): by the rule the frames are walked by
    walk_composite_lds<3, ORDER, true, 14, SMALLEXP> (and its SPLIT sibling), the kernels the benchmark times."""
    alpha = box.alpha(0.124)
    assert df.exp_rule(alpha, 2.5, box.L) * (1 + 1e-9) < 0.125
    ref = box.ref("short", box.xyz, alpha, 2.5)
    with box.open(box.xyz, alpha, **CONFIGS[config]) as ctx:
        box.hold(ctx, ref, 3, f"0.124 {config}", cutoff=1e-12 if config.startswith("front_to_back") else 0.0)


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_the_general_kernel_just_over_the_rule(box, config):
    """The same scene at 0.126: the general exp at the same arguments, held to the same reference's bar."""
    alpha = box.alpha(0.126)
    assert df.exp_rule(alpha, 2.5, box.L) > 0.125
    ref = box.ref("just_over", box.xyz, alpha, 2.5)
    with box.open(box.xyz, alpha, **CONFIGS[config]) as ctx:
        box.hold(ctx, ref, 3, f"0.126 {config}", cutoff=1e-12 if config.startswith("front_to_back") else 0.0)


@SLOTS
@pytest.mark.parametrize("device", [False, True], ids=["update_scalars", "update_scalars_device"])
def test_the_kernel_choice_follows_the_scalars(box, device, slots):
    """0.124 -> median a dz of 4 -> 0.124 in one context: a largest alpha left over from the scalars before would walk the
    second state with the short series (x^11 / 11! of error: 0.1 at x = 4) or the third with the general one."""
    short = box.alpha(0.124)
    ref_short = box.ref("short", box.xyz, short, 2.5)
    m = ar.ray_matrices(box.xyz, box.cells, short, box.s.q, box.s.rots, RES[0], RES[1], B, 2.5)
    x = (m["a"] * m["D"])[m["active"]]
    big = short * (4.0 / float(np.median(x)))
    limit = max(2.5, float(big.max()))
    ref_big = box.ref("thick", box.xyz, big, limit)

    def update(ctx, alpha):
        if device:
            import torch
            ctx.update_scalars_device(torch.tensor(alpha, dtype=torch.float64, device="cuda"),
                                      torch.tensor(box.s.q, dtype=torch.float64, device="cuda"))
        else:
            ctx.update_scalars(alpha, box.s.q)

    with box.open(box.xyz, short, stage_slots=slots) as ctx:
        box.hold(ctx, ref_short, 2, "0.124")
        ctx.set_alpha_limit(limit)  # (raised first: nothing of the thick state is clamped)
        update(ctx, big)
        box.hold(ctx, ref_big, 2, "median a dz 4")
        update(ctx, short)
        ctx.set_alpha_limit(2.5)
        box.hold(ctx, ref_short, 2, "0.124 again")


@SLOTS
@pytest.mark.parametrize("wide", [False, True], ids=["as_the_sweep", "wide"])
@pytest.mark.parametrize("through", ["set_alpha_limit", "update_points"])
def test_the_kernel_choice_follows_the_limit_and_the_points(box, through, wide, slots):
    """The sweep's two other transitions, in one context each.  set_alpha_limit: alpha up to 14 x a small limit,
    min(top, limit) x L = 0.124; the limit to the top alpha (1.74), and back.  update_points: the grid shrunk by 1/16 about
    its centroid with alpha for 0.124 there; to the drawn size (1.98, the longest edge made again), and shrunk again.
    No chord of this view is longer than 0.52 L, so the exp arguments of those second states end at 0.90 and 1.02, where the
    short series is still good to x^11 / 11! = 3e-8: the states' images differ by far more than the bar and a call that was
    ignored shows, a short series kept by mistake does not.  "wide" is the same with 56 x the small limit (the rule at 6.9,
    arguments to 3.6) and a grid shrunk by 1/64 (7.9, arguments to 4.1): there the series is off by percents."""
    factor = 4.0 if wide else 1.0
    if through == "set_alpha_limit":
        small = 0.124 / box.L
        alpha = box.alpha(0.124)
        alpha[3::7] = small * (1.0 + (14.0 * factor - 1.0) * box.u[3::7])
        alpha[box.longest] = 14.0 * factor * small
        top = float(alpha.max())
        assert top == 14.0 * factor * small and abs(df.exp_rule(alpha, small, box.L) - 0.124) < 1e-12
        ref_a = box.ref(f"small limit {wide}", box.xyz, alpha, small)
        ref_b = box.ref(f"limit at the top {wide}", box.xyz, alpha, top)
        with box.open(box.xyz, alpha, small, stage_slots=slots) as ctx:
            box.hold(ctx, ref_a, 2, "limit 0.124 / L")
            ctx.set_alpha_limit(top)
            box.hold(ctx, ref_b, 2, "limit at the top alpha")
            ctx.set_alpha_limit(small)
            box.hold(ctx, ref_a, 2, "limit 0.124 / L again")
    else:
        shrink = 16.0 * factor
        small_xyz = box.xyz.mean(0) + (box.xyz - box.xyz.mean(0)) / shrink
        alpha = box.alpha(0.124, box.L / shrink)
        limit = 2.0 * float(alpha.max())
        assert abs(df.exp_rule(alpha, limit, df.longest_edge(small_xyz, box.cells)) - 0.124) < 1e-9
        ref_a, ref_b = box.ref(f"shrunk {wide}", small_xyz, alpha, limit), box.ref(f"drawn size {wide}", box.xyz, alpha, limit)
        assert wide or ref_a.cov_rows.sum() > 0
        with box.open(small_xyz, alpha, limit, stage_slots=slots) as ctx:
            box.hold(ctx, ref_a, 2, f"shrunk by 1/{shrink:.0f}")
            ctx.update_points(box.xyz)
            box.hold(ctx, ref_b, 2, "at the drawn size")
            ctx.update_points(small_xyz)
            box.hold(ctx, ref_a, 2, "shrunk again")

"""The restatement of the FORWARD render and its bar (tests/adjoint_reference.py: forward_of; tests/derivative_fuzz.py: the
forward sweep), pinned on the CPU before anything on a GPU is held to them:
  * forward_of against the 80-digit reference (tests/derivative_reference_mp.py: forward) on the ten scenes and at the bar
    of tests/test_derivative_references_cpu.py, 64 x 2^-52 x scale; its bounds (scales, sensitivities, cancel) are the
    reference's;
  * the port oracle's own fp32 image - the reference's arithmetic, roundings and all - is inside the bar at every pixel of
    seeds 3000 to 3039: the bar does not ask more of a render than the reference itself delivers, cancel included;
  * the bar has teeth: the 10-term Taylor series without range reduction (csrc/walk_common.hpp: exp_small_nonpositive) in
    place of exp, on scenes whose largest a dz is 1.75 - what a stale longest edge, largest alpha or limit would let the
    library select - is beyond 4 x the bar in every scene, where the suite's older bar (tests/parity.py) sees next to none;
  * what forward_scene draws over the pytest seeds: every regime, call form and transition, the short series predicted for
    the product default, and the condition on the cancel share (in half of the scenes it dominates no pixel's bar).
"""
import math
import types

import numpy as np
import pytest

from course5_amd import meshgen as mg
from tests import adjoint_reference as ar
from tests import derivative_fuzz as df
from tests import derivative_reference_mp as dm
from tests.test_derivative_references_cpu import RTOL, SEEDS, _worst

B = mg.REFERENCE_BOUNDS
SWEEP_SEEDS = range(3000, 3040)
TEETH_SEEDS = range(3000, 3010)


@pytest.mark.parametrize("seed", SEEDS)
def test_forward_of_against_80_digits(seed, oracle_port):
    s = df.derivative_scene(seed)
    assert df.qualify(s, oracle_port) is None
    rx, ry = s.res
    pix, cell, _zh, dz, slope = s.segments
    covered = np.unique(pix)
    pixels = covered if len(pix) <= 40_000 else np.sort(np.random.default_rng(seed).choice(covered, 500, replace=False))
    seg = dm.Segments(pix, cell, dz, s.alpha, s.q, s.limit, pixels, slope=slope)
    want = dm.forward(seg)
    m = ar.ray_matrices(s.xyz, s.cells, s.alpha, s.q, s.rots, rx, ry, B, s.limit)
    tau, I, x = ar.forward_of(m, with_scale=True)
    flat = lambda a: np.asarray(a).reshape(-1)[pixels]  # noqa: E731
    record = []
    _worst(flat(tau), want[0], want[2], "tau", seed, record)
    _worst(flat(I), want[1], want[3], "I", seed, record)
    print(f"seed {seed} ({df.describe(s)}; {seg.n_segments} segments on {len(pixels)} pixels at 80 digits): "
          + ", ".join(f"{what} {r:.3g}" for r, what, _ in record) + "  [x 2^-52 x scale]")
    for r, what, _ in record:
        assert r <= 64, (what, r)
    for name, row in (("scale_tau", 2), ("scale_I", 3), ("sens_tau", 4), ("sens_I", 5), ("cancel", 6)):
        np.testing.assert_allclose(flat(x[name]), want[row], rtol=RTOL.get(name[:4], 1e-9), atol=2.0 ** -970, err_msg=name)
    # a pixel without a segment: 0, bounds included
    empty = np.ones(rx * ry, bool)
    empty[covered] = False
    assert not tau.reshape(-1)[empty].any() and not I.reshape(-1)[empty].any()
    assert all(not v.reshape(-1)[empty].any() for v in x.values())


class _Oracle:
    """The port oracle's image against forward_of per seed, each computed once."""

    def __init__(self, oracle):
        self.oracle, self.done = oracle, {}

    def seed(self, seed):
        if seed not in self.done:
            s = df.derivative_scene(seed)
            why = df.qualify(s, self.oracle)
            if why is not None:
                self.done[seed] = None
            else:
                ref = df.forward_reference(s, s.xyz, s.alpha, s.limit, np.arange(s.res[1]), self.oracle)
                r, wrong = df.forward_ratio(ref.oracle, ref, df.dz_err(s), 0.0)
                x = dict(ref.x, cancel=np.zeros_like(ref.x["cancel"]))
                r0, _ = df.forward_ratio(ref.oracle, types.SimpleNamespace(**dict(vars(ref), x=x)), df.dz_err(s), 0.0)
                self.done[seed] = (float(r[..., 0].max()), float(r[..., 1].max()), float(r0[..., 1].max()), wrong)
        return self.done[seed]


@pytest.fixture(scope="module")
def oracle_images(oracle_port):
    return _Oracle(oracle_port)


@pytest.mark.parametrize("block", range(4))
def test_the_reference_alone_stays_inside_the_bar(oracle_images, block):
    for seed in SWEEP_SEEDS[10 * block:10 * block + 10]:
        got = oracle_images.seed(seed)
        if got is None:
            continue
        tau, I, _without, wrong = got
        assert not wrong, (seed, wrong)
        assert tau <= 1.0 and I <= 1.0, (seed, tau, I)


def test_the_cancel_term_is_needed_and_the_seeds_are_used(oracle_images):
    got = [oracle_images.seed(seed) for seed in SWEEP_SEEDS]
    used = [g for g in got if g is not None]
    print(f"{len(used)} used, {len(got) - len(used)} skipped; worst error / tol of the oracle's fp32 image: tau "
          f"{max(g[0] for g in used):.3g}, I {max(g[1] for g in used):.3g}; I without cancel {max(g[2] for g in used):.3g}")
    assert len(got) - len(used) <= 0.1 * len(got)
    assert max(g[2] for g in used) > 1.0  # (without the term the reference itself fails the bar)


def _series_exp(x):
    """sum_{k <= 10} (-x)^k / k! by Horner's rule, as csrc/walk_common.hpp: exp_small_nonpositive forms it."""
    r = -x
    p = np.full_like(x, 1.0 / math.factorial(10))
    for k in range(9, -1, -1):
        p = p * r + 1.0 / math.factorial(k)
    return p


@pytest.mark.parametrize("seed", TEETH_SEEDS)
def test_the_bar_catches_the_short_series_out_of_its_range(seed, oracle_port):
    s = df.derivative_scene(seed)
    assert df.qualify(s, oracle_port) is None
    rx, ry = s.res
    rng = np.random.default_rng([seed, 0x7EE7])
    cell, dz = s.segments[1], s.segments[3]
    u = rng.uniform(0.2, 1.0, len(s.cells))
    alpha = u * (1.75 / float((u[cell] * dz).max()))
    limit = 2.0 * float(alpha.max())
    m = ar.ray_matrices(s.xyz, s.cells, alpha, s.q, s.rots, rx, ry, B, limit)
    tau, I, x = ar.forward_of(m, with_scale=True)
    assert abs(float((m["a"] * m["D"]).max()) - 1.75) < 1e-12
    # the reference's recurrence (line.cpp:220-224) with the series in place of exp
    E = _series_exp(m["a"] * m["D"])
    got = np.zeros(m["n_px"])
    for j in range(m["D"].shape[1]):
        on, a, Q = m["active"][:, j], np.where(m["active"][:, j], m["a"][:, j], 1.0), m["Q"][:, j]
        C = Q - a * got
        got = np.where(on, (Q - C * E[:, j]) / a, got)
    got = got.reshape(m["shape"]).astype(np.float32)
    cov = m["valid"].any(1).reshape(m["shape"])
    r = df.ratio(got, I, x["scale_I"], x["sens_I"], df.dz_err(s), df.R_OUT, extra=x["cancel"])
    a64 = got.astype(np.float64)
    old = np.abs(a64 - I) > 1e-5 * np.maximum(np.abs(a64), np.abs(I)) + 1e-6 * np.abs(I).max()  # (tests/parity.py)
    beyond = int((r[cov] > 1.0).sum())
    print(f"seed {seed}: {int(cov.sum())} covered pixels, {beyond} beyond the bar (worst error / tol {r[cov].max():.3g}), "
          f"{int(old[cov].sum())} beyond the 1e-5 bar: it would have caught {100.0 * old[cov].sum() / max(beyond, 1):.2f} % of them")
    assert r[cov].max() > 4.0


class _Draws:
    def __init__(self):
        self.scenes = None

    def get(self, oracle):
        if self.scenes is None:
            self.scenes = []
            for seed in SWEEP_SEEDS:
                s = df.forward_scene(seed)
                if df.qualify(s, oracle) is None:
                    m = ar.ray_matrices(s.xyz, s.cells, s.alpha, s.q, s.rots, s.res[0], s.res[1], B, s.limit)
                    _tau, I, x = ar.forward_of(m, with_scale=True)
                    s.share = df.cancel_share(I, x, m["valid"].any(1).reshape(m["shape"]))
                    self.scenes.append(s)
        return self.scenes


@pytest.fixture(scope="module")
def draws():
    return _Draws()


def test_cancel_dominates_no_pixel_in_half_of_the_scenes(draws, oracle_port):
    """The condition on the sweep's draw of class eps_to_1e-6: in at least half of the used scenes no covered pixel's cancel
    exceeds 2^-23 |I| - there the render is held to the fp32 rounding of I and not to the reference's own noise."""
    scenes = draws.get(oracle_port)
    for s in scenes:
        print(f"seed {s.seed}: cancel dominates at {100 * s.share:.1f} % of the covered pixels" + (" (class as drawn)" if s.keep_eps else ""))
    none = sum(1 for s in scenes if s.share == 0.0)
    print(f"none in {none} of {len(scenes)} scenes")
    assert 2 * none >= len(scenes)


def test_what_the_sweep_draws_over_the_pytest_seeds(draws, oracle_port):
    scenes = draws.get(oracle_port)
    assert {s.regime for s in scenes} == {"as_drawn", "short", "just_over"}
    assert {s.transition for s in scenes} == {"scalars", "limit", "points"}
    assert {s.form for s in scenes} == {"render", "render_device", "host_async", "frame_rows"}
    kernels = {}
    for s in scenes:
        if s.regime != "as_drawn":
            assert abs(df.exp_rule(s.alpha, s.limit, s.L) - {"short": 0.124, "just_over": 0.126}[s.regime]) < 1e-12
        k = df.predicted_kernel(s, s.alpha, s.limit, s.L)
        kernels[k] = kernels.get(k, 0) + 1
    for k, v in sorted(kernels.items()):
        print(f"{v:3d} x {k}")
    # the short series, whole rays and cut in slabs, is predicted for scenes as uploaded (the transitions add more)
    assert any("SMALLEXP" in k and "SPLIT" not in k for k in kernels)
    assert any("SMALLEXP" in k and "SPLIT" in k for k in kernels)

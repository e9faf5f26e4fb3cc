"""The exact adjoint sums on the GPU ("adjoint_exact", c5_render_adjoint_exact_bounds / _sums, c5_exact_sums_finish):
accuracy against the numpy helper and the atomic mode, equal bits from call to call and under the walk's options,
additivity of the integer words over row ranges and row tiles, the integers themselves against the Python restatement
(tests/exact_sum_reference.py), the guards, "algorithm" 1, and no trace left on the atomic mode.

The scene is the smallest at which this can go wrong: 384 cells, a few dozen of them share a wavefront, and a 29 x 21
image that is off the 8 x 8 tile.  Every test opens its own contexts."""
import math
from fractions import Fraction

import numpy as np
import pytest

from course5_amd import capi, sharding
from course5_amd import meshgen as mg
from tests import adjoint_reference as ar
from tests import exact_sum_reference as er

pytestmark = pytest.mark.gpu
B = mg.REFERENCE_BOUNDS
RX, RY = 29, 21
M = er.word_bits(RX, RY)
ROW_SPLITS = (((0, 5), (5, 16)), ((0, 13), (13, 8)))  # (begin, count): cuts off the 8-row tiles


def _scalars(n, seed):
    """test_gpu_adjoint._scalars: alpha ~ U[0, 4) (the 2.5 clamp) with exact zeros, nothing in [eps, 1e-6); Q ~ U[0, 1)."""
    rng = np.random.default_rng(seed)
    alpha = rng.uniform(0.0, 4.0, n)
    alpha[rng.random(n) < 0.05] = 0.0
    alpha[(alpha > 0) & (alpha < 1e-6)] = 1e-6
    return alpha, rng.uniform(0.0, 1.0, n)


class _Scene:
    def __init__(self, xyz, cells, seed=3, options=()):
        self.xyz, self.cells, self.options = xyz, cells, tuple(options)
        self.rots = mg.view_rotations(0.13, 0.21)
        self.alpha, self.q = _scalars(len(cells), seed)
        self.w = np.random.default_rng(seed + 1).normal(size=(RY, RX, 2)).astype(np.float32)
        self.want = ar.image_gradients(xyz, cells, self.alpha, self.q, self.rots, RX, RY, B, self.w.astype(np.float64))[:2]

    def ctx(self, options=(), exact=True):
        ctx = capi.Context(0)
        for k, v in self.options + tuple(options):
            ctx.set_option(k, v)
        ctx.upload_grid(self.xyz, self.cells, self.alpha, self.q)
        ctx.set_image(RX, RY, B)
        ctx.set_view(self.rots)
        if exact:
            ctx.set_option("adjoint_exact", 1)
        return ctx


@pytest.fixture(scope="module")
def scene():
    xyz, cells = mg.kuhn_box(4, jitter=0.1)
    assert len(cells) == 384
    return _Scene(xyz, cells)


@pytest.fixture(scope="module")
def soup():
    xyz, cells = mg.per_cell_point_copies(*mg.kuhn_box(3, jitter=0.1))
    return _Scene(xyz, cells, seed=7, options=(("algorithm", 1),))


def _same_bits(a, b):
    return all(np.array_equal(np.asarray(x, np.float64).view(np.int64), np.asarray(y, np.float64).view(np.int64)) for x, y in zip(a, b))


def _assert_close(got, want, what):
    for g, w, name in zip(got, want, ("grad_alpha", "grad_q")):
        err = np.abs(g - w).max()
        assert err <= 1e-6 * np.abs(w).max(), f"{what}: {name} max abs error {err:.3g} vs max {np.abs(w).max():.3g}"


def _finish(parts):
    ea, eq, sa, sq = parts
    return capi.exact_sums_finish(ea, sa, RX, RY), capi.exact_sums_finish(eq, sq, RX, RY)


def _split(s, layouts, whole):
    """The exponents by max and the words by integer add over the parts of each layout (place(ctx) -> the local rows):
    exactly the whole image's, and finished the single call's bits."""
    whole_exps, whole_words, single = whole
    for places in layouts:
        ctxs = [s.ctx() for _ in places]
        try:
            rows = [place(c) for place, c in zip(places, ctxs)]
            assert sorted(np.concatenate(rows).tolist()) == list(range(RY))
            bounds = [c.render_adjoint_exact_bounds(s.w[r]) for c, r in zip(ctxs, rows)]
            ea, eq, _, _ = sharding.combine_exact([b + (None, None) for b in bounds])
            assert np.array_equal(ea, whole_exps[0]) and np.array_equal(eq, whole_exps[1])
            words = [c.render_adjoint_exact_sums(s.w[r], ea, eq) for c, r in zip(ctxs, rows)]
            combined = sharding.combine_exact([(ea, eq) + w for w in words])
            assert np.array_equal(combined[2], whole_words[0]) and np.array_equal(combined[3], whole_words[1])
            assert any(w[0].any() for w in words[1:]) and words[0][0].any()  # (no part is empty)
            assert _same_bits(_finish(combined), single)
        finally:
            for c in ctxs:
                c.close()


def _whole(s):
    with s.ctx() as ctx:
        exps = ctx.render_adjoint_exact_bounds(s.w)
        words = ctx.render_adjoint_exact_sums(s.w, *exps)
        single = ctx.render_adjoint(s.w)
    assert _same_bits(_finish(exps + words), single)  # (the single call IS the composition)
    return exps, words, single


def _row_layouts():
    ranges = [[(lambda c, b=b, n=n: (c.set_row_range(b, n), np.arange(b, b + n))[1]) for b, n in split] for split in ROW_SPLITS]
    tiles = [[(lambda c, r=r: (c.set_row_tiles(4, r, 2), sharding.local_rows(RY, 4, r, 2))[1]) for r in range(2)]]
    return ranges + tiles


# ---- 1. accuracy ---------------------------------------------------------------------------------------------------
def test_exact_sums_against_the_helper_and_the_atomic_mode(scene):
    with scene.ctx(exact=False) as ctx:
        atomic = ctx.render_adjoint(scene.w)
        ctx.set_option("adjoint_exact", 1)
        exact = ctx.render_adjoint(scene.w)
    _assert_close(exact, scene.want, "exact")
    _assert_close(atomic, scene.want, "atomic")
    for g, g0 in zip(exact, atomic):
        np.testing.assert_allclose(g, g0, rtol=1e-12, atol=1e-15 * np.abs(g0).max())


@pytest.mark.parametrize("seed", range(3000, 3010))
def test_fuzz_scenes_pass_the_per_element_adjoint_bar(oracle_port, seed):
    from tests import derivative_fuzz as df
    s = df.derivative_scene(seed)
    why = df.qualify(s, oracle_port)
    if why is not None:
        print(f"seed {seed}: {why} - not used")
        return
    rx, ry = s.res
    with capi.Context(0) as ctx:
        if s.soup:
            ctx.set_option("algorithm", 1)
        ctx.set_option("adjoint_exact", 1)
        ctx.upload_grid(s.xyz, s.cells, s.alpha, s.q)
        ctx.set_image(rx, ry, B)
        ctx.set_view(s.rots)
        ctx.set_alpha_limit(s.limit)
        got = ctx.render_adjoint(s.g[0])
        again = ctx.render_adjoint(s.g[0])
    assert _same_bits(got, again) or s.soup  # ("algorithm" 1: lists with equal depths may change their order)
    m = ar.ray_matrices(s.xyz, s.cells, s.alpha, s.q, s.rots, rx, ry, B, s.limit, np.arange(ry))
    ga, gq, _tau, _I, x = ar.gradients_of(m, len(s.cells), s.g[0], None, with_scale=True)
    e = df.dz_err(s)
    r = np.stack([df.ratio(got[0], ga, x["scale_alpha"], x["sens_alpha"], e), df.ratio(got[1], gq, x["scale_q"], x["sens_q"], e)])
    print(f"seed {seed} ({df.describe(s)}): worst error / tol {r.max():.3g}")
    assert r.max() <= 1.0, f"{int((~(r <= 1.0)).sum())} elements beyond the bar, worst {r.max():.3g} at {np.unravel_index(int(np.argmax(r)), r.shape)}"


# ---- 2. bits -------------------------------------------------------------------------------------------------------
def test_equal_bits_from_call_to_call_and_whatever_the_walk_options(scene):
    with scene.ctx() as ctx:
        first = ctx.render_adjoint(scene.w)
        assert _same_bits(ctx.render_adjoint(scene.w), first)
    assert np.abs(first[0]).max() > 0 and np.abs(first[1]).max() > 0
    for opts in ((("lds_stage", 0), ("tile", 0)), (("depth_split", 2),), (("integration", 1),), (("cell_order", 0),)):
        with scene.ctx(opts) as ctx:
            assert _same_bits(ctx.render_adjoint(scene.w), first), opts


def test_device_form_batch_and_autograd_give_the_host_form_s_bits(scene):
    import torch
    from course5_amd import autograd
    n = len(scene.cells)
    w3 = np.stack([scene.w, scene.w[::-1].copy(), 0.5 * scene.w])
    with scene.ctx() as ctx:
        singles = [ctx.render_adjoint(w) for w in w3]
        g = torch.tensor(scene.w, device="cuda")
        ga = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
        gq = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
        ctx.render_adjoint_device(g, ga, gq)
        assert ctx.synchronize() == capi.C5_OK
        assert _same_bits((ga.cpu().numpy(), gq.cpu().numpy()), singles[0])
        for width in (4, 8):
            ctx.set_option("batch_width", width)
            ba, bq = ctx.render_adjoint_batch(w3)
            for j in range(3):
                assert _same_bits((ba[j], bq[j]), singles[j]), (width, j)
        g3 = torch.tensor(w3, device="cuda")
        ba_d = torch.full((3, n), float("nan"), dtype=torch.float64, device="cuda")
        bq_d = torch.full((3, n), float("nan"), dtype=torch.float64, device="cuda")
        ctx.render_adjoint_batch_device(g3, ba_d, bq_d)
        assert ctx.synchronize() == capi.C5_OK
        assert np.array_equal(ba_d.cpu().numpy().view(np.int64), ba.view(np.int64))
        assert np.array_equal(bq_d.cpu().numpy().view(np.int64), bq.view(np.int64))
        # torch.autograd.grad through autograd.render, twice
        grads = []
        for _ in range(2):
            a = torch.tensor(scene.alpha, requires_grad=True)
            qq = torch.tensor(scene.q, requires_grad=True)
            img = autograd.render(ctx, a, qq)
            grads.append(tuple(t.detach().cpu().numpy() for t in torch.autograd.grad((img * g).sum(), (a, qq))))
        assert _same_bits(grads[0], grads[1])
        assert _same_bits(grads[0], singles[0])


# ---- 3. additivity in the integers ------------------------------------------------------------------------------------
def test_words_of_row_ranges_and_row_tiles_add_up_to_the_whole_image_s_exactly(scene):
    _split(scene, _row_layouts(), _whole(scene))


# ---- 4. the integers themselves ---------------------------------------------------------------------------------------
def test_tau_weights_give_the_restatement_s_integers_exactly(scene):
    """With an upstream image (g_tau, 0) every grad_alpha contribution is fl(g_tau dz), dz the ray matrix's chord (the
    same ray_step; alpha and Q are finite and below the limit's reach, so that fma(0, dI/dalpha, ga) leaves ga as it is):
    exponents, words and finished doubles are built here in Python integers and must be the device's."""
    w = scene.w.copy()
    w[..., 1] = 0.0
    n = len(scene.cells)
    with scene.ctx() as ctx:
        row_ptr, col, dz = ctx.ray_matrix()
        ea, eq = ctx.render_adjoint_exact_bounds(w)
        sa, sq = ctx.render_adjoint_exact_sums(w, ea, eq)
        ga, gq = ctx.render_adjoint(w)
    g_tau = np.repeat(w[..., 0].reshape(-1).astype(np.float64), np.diff(row_ptr))
    x = g_tau * dz  # (one fp64 multiply per segment, as the kernel's)
    per_cell = [[] for _ in range(n)]
    for c, v in zip(col, x):
        per_cell[c].append(float(v))
    assert len(col) > 3 * n and max(len(p) for p in per_cell) > 2  # (cells with several contributions, from several wavefronts)
    want_e = np.array([er.exponent_over(p) for p in per_cell], np.int64)
    assert np.array_equal(ea, want_e), np.flatnonzero(ea != want_e)
    want_words = [er.words(p, int(e), M) for p, e in zip(per_cell, want_e)]
    assert sa.tolist() == [list(t) for t in want_words]
    want_ga = np.array([er.finish(int(e), s1, s0, M) for e, (s1, s0) in zip(want_e, want_words)])
    assert _same_bits((ga,), (want_ga,))
    for p, v in zip(per_cell, ga):  # (and the bound of the format: n 2^(e-2m), and the one rounding)
        exact = sum(Fraction(t) for t in p)
        assert abs(Fraction(float(v)) - exact) <= len(p) * Fraction(2) ** (er.exponent_over(p) - 2 * M) + Fraction(math.ulp(v)) / 2
    assert (eq == er.NONE).all() and not sq.any()
    assert np.array_equal(gq.view(np.int64), np.zeros(n, np.int64))  # +0.0


# ---- 5. guards -----------------------------------------------------------------------------------------------------
def test_exponents_that_are_too_small_are_refused_not_wrapped(scene):
    with scene.ctx() as ctx:
        ea, eq = ctx.render_adjoint_exact_bounds(scene.w)
        assert (ea != er.NOT_FINITE).all() and (ea != er.NONE).any()
        with pytest.raises(capi.C5Error) as err:
            ctx.render_adjoint_exact_sums(scene.w, np.where(ea == er.NONE, ea, ea - 2).astype(np.int32),
                                          np.where(eq == er.NONE, eq, eq - 2).astype(np.int32))
        assert err.value.code == capi.C5_ERR_INVALID and "exponent" in err.value.message
        words = ctx.render_adjoint_exact_sums(scene.w, ea, eq)  # the next ordinary call works
        assert _same_bits(_finish((ea, eq) + words), ctx.render_adjoint(scene.w))
        # larger exponents than needed are fine: a coarser grid, the same value to the format's bound
        up = np.where(ea == er.NONE, ea, ea + 3).astype(np.int32)
        coarse = ctx.render_adjoint_exact_sums(scene.w, up, eq)
        fine, rough = capi.exact_sums_finish(ea, words[0], RX, RY), capi.exact_sums_finish(up, coarse[0], RX, RY)
        assert np.abs(fine - rough).max() <= RX * RY * 2.0 ** (float(ea.max()) + 3 - 2 * M) + 2.0 ** -52 * np.abs(fine).max()


def test_a_nan_pixel_gives_nan_in_exactly_the_cells_on_its_ray(scene):
    row, column = 10, 14
    w = scene.w.copy()
    w[row, column] = np.nan
    w0 = scene.w.copy()
    w0[row, column] = 0.0  # (a pixel with zero weights is not walked)
    with scene.ctx() as ctx:
        row_ptr, col, _dz = ctx.ray_matrix()
        ga, gq = ctx.render_adjoint(w)
        ga0, gq0 = ctx.render_adjoint(w0)
        ea, eq = ctx.render_adjoint_exact_bounds(w)
    p = row * RX + column
    on_ray = np.zeros(len(scene.cells), bool)
    on_ray[col[row_ptr[p]:row_ptr[p + 1]]] = True
    assert 3 <= on_ray.sum() < len(scene.cells) // 4
    assert np.array_equal(np.isnan(ga), on_ray) and np.array_equal(ea == er.NOT_FINITE, on_ray)
    active = on_ray & ~(np.minimum(scene.alpha, 2.5) < np.finfo(np.float64).eps)  # (an inactive cell has no dI/dQ: 0, not NaN)
    assert np.array_equal(np.isnan(gq), active) and np.array_equal(eq == er.NOT_FINITE, active)
    assert _same_bits((ga[~on_ray], gq[~active]), (ga0[~on_ray], gq0[~active]))  # other cells are untouched


# ---- 6. "algorithm" 1 ------------------------------------------------------------------------------------------------
def test_the_soup_on_bin_sort_resolve(soup):
    whole = _whole(soup)
    _assert_close(whole[2], soup.want, "soup, algorithm 1")
    with soup.ctx() as ctx:
        assert _same_bits(ctx.render_adjoint(soup.w), whole[2]) and _same_bits(ctx.render_adjoint(soup.w), whole[2])
    _split(soup, _row_layouts(), whole)


# ---- 7. no trace left ------------------------------------------------------------------------------------------------
def test_the_atomic_mode_and_the_frame_are_as_they_were_after_an_exact_call(scene):
    def counts(ctx):
        return {k: v for k, v in ctx.stats().items() if not k.startswith("ms_")}

    with scene.ctx(exact=False) as ctx, scene.ctx(exact=False) as never:
        for _ in range(3):  # (three frames: the view cache is in use by the third)
            frame, frame_never = ctx.render(), never.render()
        before, stats = ctx.render_adjoint(scene.w), counts(ctx)
        ctx.set_option("adjoint_exact", 1)
        exact = ctx.render_adjoint(scene.w)
        ctx.render_adjoint_exact_bounds(scene.w)
        ctx.set_option("adjoint_exact", 0)
        after = ctx.render_adjoint(scene.w)
        assert counts(ctx) == stats
        for _ in range(3):
            again = ctx.render()
            assert np.array_equal(again.view(np.uint32), frame.view(np.uint32))
            assert np.array_equal(again.view(np.uint32), frame_never.view(np.uint32))
        assert counts(ctx) == stats == counts(never)
    _assert_close(after, scene.want, "atomic, after an exact call")
    for g, g0 in zip(after, before):
        np.testing.assert_allclose(g, g0, rtol=1e-12, atol=1e-15 * np.abs(g0).max())
    assert not _same_bits(exact, (np.zeros_like(exact[0]), np.zeros_like(exact[1])))

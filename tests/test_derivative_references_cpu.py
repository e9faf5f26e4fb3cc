"""The numpy restatements of the derivative renders (tests/adjoint_reference.py, tangent_reference.py, gn_reference.py)
against the 80-digit reference (tests/derivative_reference_mp.py), element by element, on scenes of the derivative fuzz
(tests/derivative_fuzz.py) - and the fuzz scenes themselves pinned by digest.

The restatements switch to the same series at the same a dz = 1/8 as the kernels; the mpmath reference evaluates the
formulas as written, with no series and no threshold.  Bar: |numpy - mpmath| <= 64 x 2^-52 x scale, scale the element's
absolute-sum scale (DBL_MIN where it is smaller: _worst).  Reference against reference: one rounding per segment accumulates in a ray's running sums, up to
~300 segments per ray.
"""
import numpy as np
import pytest

from course5_amd import meshgen as mg
from tests import adjoint_reference as ar
from tests import derivative_fuzz as df
from tests import derivative_reference_mp as dm
from tests import fuzz_scenes
from tests import gn_reference as gr
from tests import motion_reference as mr
from tests import tangent_reference as tr
from tests import vertex_adjoint_reference as vr
from tests import vertex_tangent_reference as vt

B = mg.REFERENCE_BOUNDS
RTOL = {"scal": 1e-9, "sens": 1e-6}
# threshold: 2027, 2014, 2016; underflow: 2009, 2000; plain: 2019, 2020, 2004; a soup: 2011; sampled (92 129 segments): 2002
SEEDS = (2027, 2014, 2016, 2009, 2000, 2019, 2020, 2004, 2011, 2002)

# sha256 of scene(seed)'s arrays (fuzz_scenes.digest), computed with the generator as it stood in tests/fuzz_parity.py
# before it moved to tests/fuzz_scenes.py
DIGESTS = {
    0: "e7b673784e62a6f78ea25064587cccfde9255116a94f25a74d5e34843657e78a",
    3: "4e1c1a3667b615cdd2137517ae17c9c257536b0cc8acab68451f3088e1326aa0",
    4: "3c6b865e0fa1a24180f03ac72323408bcfafcc23be0e867ea9620feba5f3d10d",
    1003: "8be6e2fcdb8b79f1064a683d019df9b9feda4f4e05a65be8ca52c974aed340ba",
    1014: "7efb089c1acef062762578ebd1176be3ec2ddb9c907f91dd3bbf93ed93ff0e34",
    2033: "419446453c12ecef84c9b9ae333086b32d118768b8e5fe8e040d0d010bbae4eb",
    2059: "d0f51bdafc3161b80ff5829bdddd9cb66f20de2b04ed614ac8514a84c92afe8a",
}


@pytest.mark.parametrize("seed", sorted(DIGESTS))
def test_the_fuzz_scenes_have_not_changed(seed):
    assert fuzz_scenes.digest(seed) == DIGESTS[seed]


def test_fuzz_parity_draws_its_scenes_from_fuzz_scenes():
    import ast
    import os
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "fuzz_parity.py")).read()
    tree = ast.parse(src)
    assert not any(isinstance(n, ast.FunctionDef) and n.name == "scene" for n in tree.body)
    assert any(isinstance(n, ast.ImportFrom) and n.module == "tests.fuzz_scenes" and {"scene", "VARIANTS"} <= {a.name for a in n.names}
               for n in tree.body)


def _worst(got, want, scale, what, seed, record):
    got, want, scale = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(scale, np.float64)
    # (2^-52 x scale is the spacing of the doubles at scale, and that spacing stops shrinking at DBL_MIN = 2^-1022: below
    # it - T and E on their way to 0 in the "underflow" scenes - the bar is 64 of the subnormal spacing 2^-1074)
    r = np.abs(got - want) / (2.0 ** -52 * np.maximum(scale, 2.0 ** -1022))
    record.append((float(r.max()) if r.size else 0.0, what, seed))
    return r


class _Scenes:
    """The scenes' results, each computed once whichever test asks first."""

    def __init__(self, oracle):
        self.oracle, self.done = oracle, {}

    def scene(self, seed):
        if seed not in self.done:
            self.done[seed] = _against_80_digits(seed, self.oracle)
        return self.done[seed]


@pytest.fixture(scope="module")
def scenes(oracle_port):
    return _Scenes(oracle_port)


def _against_80_digits(seed, oracle_port, mesh=fuzz_scenes.scene):
    """One scene: the worst ratios per output, and what the scene covered.  mesh: derivative_scene's (tests/
    test_unstructured_scenes_cpu.py sends three scenes of its family through here)."""
    seen = {"classes": np.zeros(8, np.int64), "series": 0, "closed": 0, "modes": set(), "worst": [], "elements": 0}
    s = df.derivative_scene(seed, mesh)
    assert df.qualify(s, oracle_port) is None
    rx, ry = s.res
    n = len(s.cells)
    pix, cell, _zh, dz = s.segments[:4]
    cls = np.bincount(df.alpha_class(s.alpha, s.limit)[cell], minlength=8)  # (per segment: what the rays see)
    assert n < 10 or (cls > 0).all(), dict(zip(df.ALPHA_CLASSES, cls))
    x = np.minimum(s.alpha, s.limit)[cell] * dz
    active = ~(np.minimum(s.alpha, s.limit)[cell] < df.EPS)
    seen["classes"] += cls
    seen["series"] += int((active & (x < 0.125)).sum())
    seen["closed"] += int((active & (x >= 0.125)).sum())
    seen["modes"].add(s.mode)
    covered = np.unique(pix)
    if len(pix) <= 40_000:
        pixels = covered
    else:
        pixels = np.sort(np.random.default_rng(seed).choice(covered, 500, replace=False))
    assert len(pixels) >= min(500, len(covered))
    seg = dm.Segments(pix, cell, dz, s.alpha, s.q, s.limit, pixels, slope=s.segments[4])
    chosen = np.zeros(rx * ry, bool)
    chosen[pixels] = True
    m = ar.ray_matrices(s.xyz, s.cells, s.alpha, s.q, s.rots, rx, ry, B, s.limit)
    record = []
    da = None if s.d_alpha is None else s.d_alpha[0]
    dq = None if s.d_q is None else s.d_q[0]
    # tangent, per pixel
    td, Id, _tau, _I, ex = tr.tangent_of(m, n, da, dq, with_scale=True)
    want = dm.tangent(seg, da, dq)
    flat = lambda a: np.asarray(a).reshape(-1)[pixels]  # noqa: E731
    rs = [_worst(flat(td), want[0], want[2], "tau_dot", seed, record), _worst(flat(Id), want[1], want[3], "I_dot", seed, record)]
    # ... and the restatement's own scales and sensitivities are the reference's: the scales are sums of positive terms
    # (1e-9), a sensitivity's terms |contribution| / dz may cancel inside (1e-6: it enters the bar with a factor of 16)
    for name, row in (("scale_tau", 2), ("scale_I", 3), ("sens_tau", 4), ("sens_I", 5)):
        np.testing.assert_allclose(flat(ex[name]), want[row], rtol=RTOL[name[:4]], atol=2.0 ** -970, err_msg=name)
    # adjoint, per cell: upstream image 0 on the chosen pixels, zero elsewhere
    g = np.where(chosen[:, None], s.g[0].reshape(-1, 2).astype(np.float64), 0.0)
    ga, gq, _tau, _I, ex = ar.gradients_of(m, n, g, with_scale=True)
    want = dm.adjoint(seg, n, g[pixels])
    rs += [_worst(ga, want["alpha"], want["scale_alpha"], "grad_alpha", seed, record),
           _worst(gq, want["q"], want["scale_q"], "grad_q", seed, record)]
    for name in ("scale_alpha", "scale_q", "sens_alpha", "sens_q"):
        np.testing.assert_allclose(ex[name], want[name], rtol=RTOL[name[:4]], atol=2.0 ** -970, err_msg=name)
    # Gauss-Newton diagonal and product (the fp32 intermediate of the header), weights on the chosen pixels
    w = np.ones((rx * ry, 2), np.float32) if s.w is None else s.w.reshape(-1, 2)
    w = np.where(chosen[:, None], w, np.float32(0.0)).astype(np.float32)
    terms = gr.terms_of(m, with_scale=True)
    d_a, d_q = gr.diagonal(terms, rx * ry, n, w)
    ex = gr.diagonal_scale(terms, rx * ry, n, w)
    want = dm.gn_diagonal(seg, n, w[pixels].astype(np.float64))
    rs += [_worst(d_a, want["alpha"], want["scale_alpha"], "diag_alpha", seed, record),
           _worst(d_q, want["q"], want["scale_q"], "diag_q", seed, record)]
    for name in ("scale_alpha", "scale_q", "sens_alpha", "sens_q"):
        np.testing.assert_allclose(ex[name], want[name], rtol=RTOL[name[:4]], atol=2.0 ** -970, err_msg="diagonal " + name)
    ha, hq, jv32, ex = gr.product_header(terms, rx * ry, n, da, dq, w)
    want, want_jv = dm.gn_product(seg, n, da, dq, w[pixels])
    # J v rounded to fp32 from two fp64 values a few ulps apart: where they straddle a rounding boundary the two
    # intermediates differ by an fp32 ulp (a handful of pixels at most).  So h is held to the 80-digit J^T of the
    # restatement's own intermediate, and the intermediates to each other.
    off = jv32[pixels].view(np.int32).astype(np.int64) - want_jv.view(np.int32).astype(np.int64)
    assert np.abs(off).max() <= 1 and (off != 0).mean() < 1e-3, f"{(off != 0).sum()} of {off.size} fp32 intermediates differ"
    if (off != 0).any():
        want = dm.adjoint(seg, n, (w[pixels] * jv32[pixels]).astype(np.float32).astype(np.float64))
    rs += [_worst(ha, want["alpha"], want["scale_alpha"], "h_alpha", seed, record),
           _worst(hq, want["q"], want["scale_q"], "h_q", seed, record)]
    seen["elements"] += sum(r.size for r in rs)
    print(f"seed {seed} ({df.describe(s)}; {seg.n_segments} segments on {len(pixels)} pixels at 80 digits): "
          + ", ".join(f"{what} {r:.3g}" for r, what, _ in record) + "  [x 2^-52 x scale]")
    seen["worst"] += record
    return seen


@pytest.mark.parametrize("seed", SEEDS)
def test_restatements_against_80_digits(seed, scenes):
    for r, what, _ in scenes.scene(seed)["worst"]:
        assert r <= 64, (what, r)


def test_the_scenes_cover_every_class_and_both_branches(scenes):
    got = [scenes.scene(seed) for seed in SEEDS]
    seen = {"classes": sum(g["classes"] for g in got), "series": sum(g["series"] for g in got),
            "closed": sum(g["closed"] for g in got), "modes": set().union(*(g["modes"] for g in got)),
            "worst": [w for g in got for w in g["worst"]], "elements": sum(g["elements"] for g in got)}
    worst = max(seen["worst"])
    print(f"worst |numpy - mpmath| over {seen['elements']} elements: {worst[0]:.3g} x 2^-52 x scale ({worst[1]}, seed {worst[2]}); bar 64")
    print("alpha classes of the segments:", dict(zip(df.ALPHA_CLASSES, seen["classes"].tolist())),
          f"; active segments below a dz = 1/8: {seen['series']}, at or above: {seen['closed']}; modes {sorted(seen['modes'])}")
    assert (seen["classes"] > 0).all()
    assert seen["series"] > 1000 and seen["closed"] > 1000
    assert seen["modes"] == {"plain", "threshold", "underflow"}
    assert worst[0] <= 64


# ---- the second-order sweep's draws leave the scenes alone ---------------------------------------------------------------

def _same(a, b):
    if isinstance(a, (tuple, list)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return type(a) is type(b) and a == b


@pytest.mark.parametrize("seed", range(3000, 3040, 4))
def test_second_order_scene_is_derivative_scene_with_a_full_second_split(seed):
    """second_order_scene(seed) draws from a stream of its own: every field of derivative_scene(seed) is there bit for bit,
    and the second split of the rows covers rows 0..ry-1 exactly once, whichever kind was drawn."""
    base, s = df.derivative_scene(seed), df.second_order_scene(seed)
    for name, value in vars(base).items():
        assert _same(value, getattr(s, name)), (seed, name)
    assert set(vars(s)) - set(vars(base)) == {"compare_options", "second_split", "second_cut"}
    assert s.compare_options in df.COMPARE_OPTIONS and s.second_split in ("cyclic", "ranges")
    assert 0 < s.second_cut < s.res[1] and s.second_cut % 8
    for kind in ("cyclic", "ranges"):  # (both kinds, the drawn one included)
        s.second_split = kind
        rows = np.concatenate([r for _place, r in df.second_split(s)])
        assert np.array_equal(np.sort(rows), np.arange(s.res[1])), (seed, kind)


def test_the_second_split_covers_every_row_once_at_every_size():
    """Every image height of the fuzz scenes (20..500) with every tile height and world derivative_scene draws, and every
    cut off_tile_cut can return (no scene is built)."""
    import types
    for ry in (20, 21, 23, 24, 25, 31, 32, 33, 64, 65, 127, 263, 499, 500):
        for cut in range(1, ry):
            rng = types.SimpleNamespace(integers=lambda lo, hi, cut=cut: cut)
            got = df.off_tile_cut(rng, ry)
            assert 0 < got < ry and got % 8 and got in (cut, cut - 1)
        for tile_rows in (1, 3, 8, 16):
            for world in range(2, 6):
                for kind in ("cyclic", "ranges"):
                    s = types.SimpleNamespace(res=(40, ry), tile_rows=tile_rows, world=world, second_split=kind,
                                              second_cut=df.off_tile_cut(np.random.default_rng([ry, tile_rows, world]), ry))
                    rows = np.concatenate([r for _place, r in df.second_split(s)])
                    assert np.array_equal(np.sort(rows), np.arange(ry)), (ry, tile_rows, world, kind)


def test_the_second_order_draws_take_every_value():
    """Over the 40 pytest seeds every walk option of the comparison context and both kinds of second split are drawn (the
    stream alone: no scene is built)."""
    options, kinds = set(), set()
    for seed in range(3000, 3040):
        rng = np.random.default_rng([seed, 0x2E0])
        options.add(df.COMPARE_OPTIONS[int(rng.integers(len(df.COMPARE_OPTIONS)))])
        kinds.add(("cyclic", "ranges")[int(rng.integers(2))])
    assert options == set(df.COMPARE_OPTIONS) and kinds == {"cyclic", "ranges"}


# ---- the geometry restatements (motion tangent, vertex tangent, vertex adjoint) ----------------------------------------

# a "threshold" and an "underflow" scene (the latter a soup); 3003 and 3007 for their steep faces, a few rows each
GEOMETRY_SEEDS = (3001, 3006, 3003, 3007)
N_PIXELS = 90


@pytest.mark.parametrize("seed", GEOMETRY_SEEDS)
def test_geometry_restatements_against_80_digits(seed, oracle_port):
    """motion_reference, vertex_tangent_reference and vertex_adjoint_reference against derivative_reference_mp's geometry
    on N_PIXELS pixels of a scene of the geometry sweep, element by element within their own bars
    1e-9 scale + dz_err sens + 2^-970 - the sens term because the 80-digit chord is the difference of the two depths, not
    the double the restatements carry.  In 3003 and 3007 the pixels are those of the rows about the steepest face."""
    _geometry_against_80_digits(seed, oracle_port, fuzz_scenes.scene, seed in (3003, 3007))


def _geometry_against_80_digits(seed, oracle_port, mesh, steep_rows):
    """The body of the test above for one scene of `mesh` (tests/test_unstructured_scenes_cpu.py sends one of its family
    through here).  Returns the steepest face among the chosen pixels' segments."""
    s = df.geometry_scene(seed, mesh)
    assert df.qualify(s, oracle_port) is None
    rx, ry = s.res
    n_pts = len(s.xyz)
    pix, _cell, _zh, _dz, slope = s.segments
    rows = None
    if steep_rows:
        r = int(pix[slope.argmax()] // rx)
        rows = np.arange(max(r - 2, 0), min(r + 3, ry))
    m = ar.ray_matrices(s.xyz, s.cells, s.alpha, s.q, s.rots, rx, ry, B, s.limit, rows)
    geo = vr.segment_faces(s.xyz, s.cells, s.rots, rx, ry, B, rows)
    covered = np.flatnonzero(m["valid"].any(1))
    steep = np.flatnonzero((m["F"] * m["valid"]).max(1) > 100.0)
    rng = np.random.default_rng([seed, 80])
    pixels = np.unique(np.concatenate([steep[:N_PIXELS // 3], rng.choice(covered, min(N_PIXELS, len(covered)), replace=False)]))[:N_PIXELS]
    rays = dm.GeometryRays(ar.rotate(s.xyz, s.rots), s.cells, geo, s.alpha, s.q, s.limit, pixels)
    if steep_rows:
        assert rays.steepest > 100.0
    M = vr.view_matrix(s.rots)
    e = df.dz_err(s)
    worst = {}

    def hold(kind, got, want, scale, sens):
        r = df.ratio(got, want, scale, sens, e)
        worst[kind] = max(worst.get(kind, 0.0), float(r.max()))
        assert (r <= 1.0).all(), (kind, float(r.max()))

    at = s.motion_at
    for j in (0, at["base"], at["base"] + 2, at["up"]):  # a rotation, a drawn field, the z-scale, the drawn field x 2^20
        td, Id, x = mr.motion_of(m, geo, s.motion[j], with_scale=True)
        want = dm.motion_tangent(rays, s.motion[j])
        flat = lambda a: a.reshape(-1)[pixels]  # noqa: E731
        hold("motion tau_dot", flat(td), want[0], flat(x["scale_tau"]), flat(x["sens_tau"]))
        hold("motion I_dot", flat(Id), want[1], flat(x["scale_I"]), flat(x["sens_I"]))
    for j in s.v_compare:
        td, Id, x = vt.tangent_of(m, geo, s.cells, s.rots, s.v_fields[j], with_scale=True)
        want = dm.vertex_tangent(rays, s.v_fields[j], M)
        hold("vertex tau_dot", flat(td), want[0], flat(x["scale_tau"]), flat(x["sens_tau"]))
        hold("vertex I_dot", flat(Id), want[1], flat(x["scale_I"]), flat(x["sens_I"]))
    chosen = np.zeros(m["n_px"], bool)
    chosen[pixels] = True
    for g in s.vg:  # the upstream image on the chosen pixels, zero elsewhere
        g = g if rows is None else g[rows]
        w = np.where(chosen[:, None], g.reshape(-1, 2).astype(np.float64), 0.0)
        ref = vr.gradients_of(m, geo, s.cells, n_pts, s.rots, w)
        hold("vertex adjoint", ref["raw"], dm.vertex_adjoint(rays, w[pixels], n_pts, M), ref["scale_raw"], ref["sens_raw"])
    print(f"seed {seed} ({df.describe(s)}; {rays.n_segments} segments on {len(pixels)} pixels at 80 digits, steepest face "
          f"{rays.steepest:.3g}): worst error / bar " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    return rays.steepest

"""The exact vertex adjoint sums without a GPU: the six symbols and the header's text, the wrappers' argument checks, the
restatement (tests/vertex_exact_reference.py) - additive over rows, one rounding per slot, and through steps 2 to 4 the
gradient of tests/vertex_adjoint_reference.py - and fit.RowShards.shape_operators / shape_step / shape_gradient on
stand-in contexts made from that restatement."""
import ctypes as C
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from course5_amd import build, capi, fit
from course5_amd import meshgen as mg
from tests import adjoint_reference as ar
from tests import exact_sum_reference as er
from tests import vertex_adjoint_reference as vr
from tests import vertex_exact_reference as vx
from tests.fake_library import RecordingLibrary, bare_context

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "course5_hip.h")
RX, RY = 29, 21
M = er.word_bits(RX, RY)
B = mg.REFERENCE_BOUNDS
ROTS = mg.view_rotations(0.13, 0.21)


# ---- symbols and header ------------------------------------------------------------------------------------------------
def test_the_six_symbols_are_exported_with_the_binding_table_s_signatures():
    lib = capi.load_library()
    with open(HEADER) as f:
        text = f.read()
    vp, dp, fp, ip, lp = C.c_void_p, capi._dp_t, capi._fp_t, capi._ip_t, capi._lp_t
    want = {"c5_render_vertex_exact_bounds": [vp, fp, ip],
            "c5_render_vertex_exact_bounds_device": [vp, vp, vp],
            "c5_render_vertex_exact_sums": [vp, fp, ip, lp],
            "c5_render_vertex_exact_sums_device": [vp, vp, vp, vp],
            "c5_vertex_exact_finish": [vp, ip, lp, dp],
            "c5_vertex_exact_finish_device": [vp, vp, vp, vp]}
    for name, args in want.items():
        assert hasattr(lib, name) and name in capi.EXPORTS
        assert capi.SIGNATURES[name] == args and getattr(lib, name).argtypes == args
        declared = re.search(r"\bint " + name + r"\(([^;]*)\);", text)
        assert declared and len(declared.group(1).split(",")) == len(args), name


def test_the_header_names_the_option_and_the_abi_and_the_source_hash_stay():
    with open(HEADER) as f:
        text = f.read()
    assert "#define C5_ABI_VERSION 2\n" in text
    lib = capi.load_library()
    lib.c5_abi_version.restype = C.c_int
    assert lib.c5_abi_version() == 2
    assert build.kernel_source_hash() == "63c90aeb24365e47"  # (re-stamped with next_entry: profiles/component_fuzz.md)
    assert '"vertex_exact"' in text and "SPLIT CONTRACT" in text
    assert "c5_render_vertex_adjoint* ignores both options" in text  # ("adjoint_exact" / "exact_sums": still true)


# ---- the wrappers' argument checks -------------------------------------------------------------------------------------
def test_argument_checks_before_the_library():
    ctx = bare_context()  # 7 cells, 9 points, images of 5 x 6
    g = np.zeros((5, 6, 2), np.float32)
    exps, sums = np.zeros((7, 12), np.int32), np.zeros((7, 12, 2), np.int64)
    for bad in (np.zeros((4, 6, 2)), np.zeros((5, 6)), np.zeros((1, 5, 6, 2))):  # wrong image shape
        with pytest.raises(ValueError, match=r"grad_out must be \[5, 6, 2\]"):
            ctx.render_vertex_exact_bounds(bad)
        with pytest.raises(ValueError, match=r"grad_out must be \[5, 6, 2\]"):
            ctx.render_vertex_exact_sums(bad, exps)
    for bad in (np.zeros((7, 12), np.int64), np.zeros((7,), np.int32), np.zeros((6, 12), np.int32), np.zeros((12, 7), np.int32).T):
        with pytest.raises(ValueError, match=r"exps must be a contiguous int32 array \[7, 12\]"):
            ctx.render_vertex_exact_sums(g, bad)
        with pytest.raises(ValueError, match="exps must be"):
            ctx.vertex_exact_finish(bad, sums)
    for bad in (np.zeros((7, 12, 2), np.int32), np.zeros((7, 2), np.int64), np.zeros((7, 12, 3), np.int64), np.zeros((7, 24), np.int64)):
        with pytest.raises(ValueError, match=r"sums must be a contiguous int64 array \[7, 12, 2\]"):
            ctx.vertex_exact_finish(exps, bad)
    # a host array for a _device form
    with pytest.raises(ValueError, match="on the GPU"):
        ctx.render_vertex_exact_bounds_device(g, 0x2000)
    with pytest.raises(ValueError, match="on the GPU"):
        ctx.render_vertex_exact_sums_device(0x1000, exps, 0x3000)
    with pytest.raises(ValueError, match="on the GPU"):
        ctx.vertex_exact_finish_device(0x1000, sums, 0x3000)
    with pytest.raises(ValueError, match="on the GPU"):
        ctx.vertex_exact_finish_device(0x1000, 0x2000, np.zeros((9, 3)))


def test_one_recorded_call_per_entry():
    ctx = bare_context()
    g = np.ones((5, 6, 2))  # (converted to float32 on the way)
    exps, sums = np.zeros((7, 12), np.int32), np.zeros((7, 12, 2), np.int64)
    ctx.lib = RecordingLibrary()
    out = ctx.render_vertex_exact_bounds(g)
    assert out.dtype == np.int32 and out.shape == (7, 12)
    out = ctx.render_vertex_exact_sums(g, exps)
    assert out.dtype == np.int64 and out.shape == (7, 12, 2)
    out = ctx.vertex_exact_finish(exps, sums)
    assert out.dtype == np.float64 and out.shape == (9, 3)
    ctx.render_vertex_exact_bounds_device(0x1000, 0x2000)
    ctx.render_vertex_exact_sums_device(0x1000, 0x2000, 0x3000)
    ctx.vertex_exact_finish_device(0x2000, 0x3000, 0x4000)
    assert ctx.lib.calls == [("c5_render_vertex_exact_bounds", (None, "ptr", "ptr")),
                             ("c5_render_vertex_exact_sums", (None, "ptr", "ptr", "ptr")),
                             ("c5_vertex_exact_finish", (None, "ptr", "ptr", "ptr")),
                             ("c5_render_vertex_exact_bounds_device", (None, 0x1000, 0x2000)),
                             ("c5_render_vertex_exact_sums_device", (None, 0x1000, 0x2000, 0x3000)),
                             ("c5_vertex_exact_finish_device", (None, 0x2000, 0x3000, 0x4000))]


# ---- the restatement ---------------------------------------------------------------------------------------------------
class _Scene:
    def __init__(self):
        self.xyz, self.cells = mg.kuhn_box(2, jitter=0.1)
        rng = np.random.default_rng(5)
        self.n, self.n_pts = len(self.cells), len(self.xyz)
        self.alpha, self.q = rng.uniform(0.1, 2.0, self.n), rng.uniform(0.0, 1.0, self.n)
        self.m = ar.ray_matrices(self.xyz, self.cells, self.alpha, self.q, ROTS, RX, RY, B, 2.5)
        self.geo = vr.segment_faces(self.xyz, self.cells, ROTS, RX, RY, B)
        self.residual = rng.normal(size=(RY, RX, 2)).astype(np.float32)
        self.weight = np.abs(rng.normal(size=(RY, RX, 2))).astype(np.float32)
        self.free = rng.random(self.n_pts) < 0.7

    def contributions(self, image):
        """(pixel row, cell, slot, value) of the whole image's segments for the upstream image [RY, RX, 2]."""
        pix, cell, slot, value = vx.contributions(self.m, self.geo, image)
        return pix // RX, cell, slot, value


@pytest.fixture(scope="module")
def scene():
    return _Scene()


def test_words_are_additive_over_rows_and_finish_with_one_rounding(scene):
    row, cell, slot, value = scene.contributions(scene.residual)
    whole = vx.per_slot(cell, slot, value, scene.n)
    exps = vx.exponents(whole)
    sums = vx.words(whole, exps, M)
    assert (exps != er.NONE).sum() > scene.n and sums.any()
    for parts in ((row < 13, row >= 13), ((row // 4) % 2 == 0, (row // 4) % 2 == 1)):  # rows [0,13)+[13,21); cyclic 4-row tiles
        lists = [vx.per_slot(cell, slot, value, scene.n, keep) for keep in parts]
        part_exps = [vx.exponents(p) for p in lists]
        assert np.array_equal(np.maximum(*part_exps), exps) and (part_exps[0] != part_exps[1]).any()
        part_sums = [vx.words(p, exps, M) for p in lists]
        assert np.array_equal(part_sums[0] + part_sums[1], sums) and all(s.any() for s in part_sums)
    w = vx.face_w(exps, sums, M)
    for c, (lists_c, exact_c) in enumerate(zip(whole, vx.exact_slot_sums(whole))):
        for s, (p, exact) in enumerate(zip(lists_c, exact_c)):
            if exact is None:
                assert exps[c, s] == er.NONE and w[c, s] == 0.0 and not math.copysign(1.0, w[c, s]) < 0
                continue
            v = float(w[c, s])
            assert abs(Fraction(v) - exact) <= len(p) * Fraction(2) ** (int(exps[c, s]) - 2 * M) + Fraction(math.ulp(v)) / 2


def test_the_restated_steps_give_the_gradient(scene):
    _row, cell, slot, value = scene.contributions(scene.residual)
    whole = vx.per_slot(cell, slot, value, scene.n)
    exps = vx.exponents(whole)
    got = vx.finish(exps, vx.words(whole, exps, M), scene.xyz, scene.cells, ROTS, M)
    ref = vr.gradients_of(scene.m, scene.geo, scene.cells, scene.n_pts, ROTS, scene.residual)
    assert np.abs(ref["raw"]).max() > 0
    assert (np.abs(got - ref["raw"]) <= 1e-12 * ref["scale_raw"]).all()


# ---- fit.RowShards.shape_operators on stand-ins -------------------------------------------------------------------------
class _Stub:
    """A context's face as RowShards' shape operators use it, over the global rows `rows` of the scene; every call is
    noted in `log`."""
    res_x, res_y, device = RX, RY, "cpu"

    def __init__(self, scene, rows, log, name):
        self.s, self.rows, self.log, self.name = scene, np.asarray(rows), log, name
        self.n_cells, self.n_pts, self.local_rows = scene.n, scene.n_pts, len(self.rows)
        self.scalars = self.points = None

    def update_scalars(self, alpha, q):
        self.scalars = (np.array(alpha), np.array(q))

    def update_points(self, xyz):
        self.points = np.array(xyz)

    def _whole(self, image):
        assert image.dtype == np.float32 and image.shape == (self.local_rows, RX, 2)
        whole = np.zeros((RY, RX, 2), np.float32)
        whole[self.rows] = image
        return whole

    def _lists(self, image):
        row, cell, slot, value = self.s.contributions(self._whole(image))
        return vx.per_slot(cell, slot, value, self.n_cells, np.isin(row, self.rows))

    def render_vertex_exact_bounds(self, image):
        self.log.append(("bounds", self.name))
        return vx.exponents(self._lists(image))

    def render_vertex_exact_sums(self, image, exps):
        self.log.append(("sums", self.name, np.array(exps)))
        return vx.words(self._lists(image), exps, M)

    def vertex_exact_finish(self, exps, sums):
        self.log.append(("finish", self.name))
        return vx.finish(exps, sums, self.s.xyz, self.s.cells, ROTS, M)

    def render_vertex_tangent(self, d):
        """J d on the stub's rows: any fixed linear function of d per pixel will do for the stand-in - the transpose of
        the contributions with unit upstream weights."""
        self.log.append(("tangent", self.name))
        assert d.shape == (self.n_pts, 3) and d.dtype == np.float64
        out = np.zeros((RY, RX, 2))
        u = (d @ vr.view_matrix(ROTS).T)[:, 2]  # (the z velocity alone: slopes left out)
        for ch in range(2):
            unit = np.zeros((RY, RX, 2), np.float32)
            unit[..., ch] = 1.0
            pix, cell, slot, value = vx.contributions(self.s.m, self.s.geo, unit)
            vid = np.asarray(self.s.cells)[cell, vx.FACES[slot // 3, slot % 3]]
            np.add.at(out[..., ch].reshape(-1), pix, value * u[vid])
        return out[self.rows].astype(np.float32)


ROW_SETS = ((np.arange(0, 13), np.arange(13, RY)), (np.array([r for r in range(RY) if (r // 4) % 2 == 0]), np.array([r for r in range(RY) if (r // 4) % 2 == 1])))


def _shards(scene, row_sets, log):
    return fit.RowShards([(_Stub(scene, r, log, k), r) for k, r in enumerate(row_sets)])


def test_row_shards_keep_accepting_stand_ins_without_points(scene):
    class _NoPoints:
        res_x, res_y, device, n_cells, local_rows = RX, RY, "cpu", 3, RY

    shards = fit.RowShards([(_NoPoints(), np.arange(RY))])
    assert shards.n_pts is None
    assert _shards(scene, ROW_SETS[0], []).n_pts == scene.n_pts


def test_bounds_come_first_every_part_gets_the_combined_exponents_and_finish_runs_once(scene):
    log = []
    shards = _shards(scene, ROW_SETS[1], log)
    ops = shards.shape_operators(torch.tensor(scene.alpha), torch.tensor(scene.q), torch.tensor(scene.weight))
    for ctx, _rows in shards.parts:  # (the scalars went to every context)
        assert np.array_equal(ctx.scalars[0], scene.alpha) and np.array_equal(ctx.scalars[1], scene.q)
    p = torch.tensor(np.random.default_rng(9).normal(size=(scene.n_pts, 3)))
    for name, call, lead in (("rhs", lambda: ops.rhs(torch.tensor(scene.residual)), []), ("product", lambda: ops.product(p), ["tangent", "tangent"])):
        del log[:]
        out = call()
        assert [e[0] for e in log] == lead + ["bounds", "bounds", "sums", "sums", "finish"], name
        tail = log[len(lead):]
        assert sorted(e[1] for e in tail[:2]) == sorted(e[1] for e in tail[2:4]) == [0, 1] and tail[4][1] == 0, name
        assert np.array_equal(tail[2][2], tail[3][2]), name  # the same exponents to every part ...
        assert isinstance(out, torch.Tensor) and out.dtype == torch.float64 and tuple(out.shape) == (scene.n_pts, 3), name
        assert float(out.abs().max()) > 0, name
    # ... and they are the elementwise max of the parts' own
    del log[:]
    ops.rhs(torch.tensor(scene.residual))
    g = scene.residual * scene.weight
    own = [vx.exponents(ctx._lists(np.ascontiguousarray(g[r]))) for ctx, r in shards.parts]
    assert np.array_equal(log[2][2], np.maximum(*own)) and (own[0] != own[1]).any()
    shards.update_points(scene.xyz + 1.0)
    assert all(np.array_equal(ctx.points, scene.xyz + 1.0) for ctx, _r in shards.parts)


def _bits(t):
    return np.ascontiguousarray(t.numpy() if isinstance(t, torch.Tensor) else t, np.float64).view(np.int64)


def test_two_parts_give_one_part_s_bits_and_the_steps_use_the_hook(scene):
    a, q, w, r = (torch.tensor(v) for v in (scene.alpha, scene.q, scene.weight, scene.residual))
    p = torch.tensor(np.random.default_rng(10).normal(size=(scene.n_pts, 3)))
    one = _shards(scene, (np.arange(RY),), [])
    ops = one.shape_operators(a, q, w)
    want_rhs, want_prod = ops.rhs(r), ops.product(p)
    want_loss, want_grad = fit.shape_gradient(one, a, q, r, w)
    want_step, want_models = fit.shape_step(one, a, q, r, w, iters=2, free=scene.free)
    assert np.array_equal(_bits(want_grad), _bits(want_rhs)) and want_loss > 0
    assert len(want_models) >= 1 and not want_step[~scene.free].numpy().any() and want_step[scene.free].numpy().any()
    for row_sets in ROW_SETS:
        log = []
        two = _shards(scene, row_sets, log)
        ops = two.shape_operators(a, q, w)
        assert np.array_equal(_bits(ops.rhs(r)), _bits(want_rhs)) and np.array_equal(_bits(ops.product(p)), _bits(want_prod))
        loss, grad = fit.shape_gradient(two, a, q, r, w)
        assert loss == want_loss and np.array_equal(_bits(grad), _bits(want_grad))
        del log[:]
        step, models = fit.shape_step(two, a, q, r, w, iters=2, free=scene.free)
        assert np.array_equal(_bits(step), _bits(want_step)) and models == want_models
        assert [e[0] for e in log].count("finish") >= 1 + len(models)  # (the right-hand side, and one product per iteration)


def test_without_the_hook_the_steps_go_to_the_library_as_before():
    class _Plain:  # no shape_operators: fit must take the library's path, which asks autograd for the context's device
        device, n_pts, n_cells, res_x, res_y, local_rows = 0, 4, 1, RX, RY, RY

    seen = []
    from course5_amd import autograd
    original = autograd._gn_enter
    autograd._gn_enter = lambda ctx, alpha, q, what: (seen.append(what), (_ for _ in ()).throw(RuntimeError("library path")))[1]
    try:
        for call in (fit.shape_gradient, fit.shape_step):
            with pytest.raises(RuntimeError, match="library path"):
                call(_Plain(), torch.zeros(1), torch.zeros(1), torch.zeros((RY, RX, 2)))
    finally:
        autograd._gn_enter = original
    assert seen == ["shape_gradient", "shape_step"]

"""The exact sums of a fit without a GPU: the four new symbols, the header's text, and fit.RowShards on stand-in contexts
whose render_exact_bounds / render_exact_sums are made from the per-segment terms of tests/gn_reference.py through
tests/exact_sum_reference.py - its refusals, the order of its calls, the exponents it hands on, and two parts giving the
bits of one."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from course5_amd import capi, fit
from course5_amd import meshgen as mg
from tests import exact_sum_reference as er
from tests import gn_reference as gn

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "course5_hip.h")
NEW = ("c5_render_exact_bounds", "c5_render_exact_bounds_device", "c5_render_exact_sums", "c5_render_exact_sums_device")
RX, RY = 9, 7
M = er.word_bits(RX, RY)


# ---- symbols and header ------------------------------------------------------------------------------------------------
def test_the_four_symbols_are_exported_with_the_binding_table_s_signatures():
    lib = capi.load_library()
    with open(HEADER) as f:
        text = f.read()
    vp, dp, fp, ip, lp = C.c_void_p, capi._dp_t, capi._fp_t, capi._ip_t, capi._lp_t
    want = {"c5_render_exact_bounds": [vp, C.c_int, dp, dp, fp, ip, ip],
            "c5_render_exact_bounds_device": [vp, C.c_int, vp, vp, vp, vp, vp],
            "c5_render_exact_sums": [vp, C.c_int, dp, dp, fp, ip, ip, lp, lp],
            "c5_render_exact_sums_device": [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp]}
    for name in NEW:
        assert hasattr(lib, name) and name in capi.EXPORTS
        assert capi.SIGNATURES[name] == want[name] and getattr(lib, name).argtypes == want[name]
        declared = re.search(r"\bint " + name + r"\(([^;]*)\);", text)
        assert declared and len(declared.group(1).split(",")) == len(want[name]), name
    assert (capi.C5_EXACT_ADJOINT, capi.C5_EXACT_GN_DIAGONAL, capi.C5_EXACT_HVP) == (0, 1, 2)


def test_the_header_names_the_option_and_the_kinds_and_the_abi_version_stays_2():
    with open(HEADER) as f:
        text = f.read()
    assert "#define C5_ABI_VERSION 2\n" in text
    lib = capi.load_library()
    lib.c5_abi_version.restype = C.c_int
    assert lib.c5_abi_version() == 2
    assert '"exact_sums"' in text
    assert re.search(r"enum\s*\{\s*C5_EXACT_ADJOINT = 0,\s*C5_EXACT_GN_DIAGONAL = 1,\s*C5_EXACT_HVP = 2\s*\}", text)
    assert "c5_render_vertex_adjoint* ignores both options" in text


# ---- fit.RowShards on stand-ins ----------------------------------------------------------------------------------------
class _Scene:
    def __init__(self):
        xyz, cells = mg.kuhn_box(2, jitter=0.1)
        rng = np.random.default_rng(5)
        self.n = len(cells)
        self.alpha, self.q = rng.uniform(0.1, 2.0, self.n), rng.uniform(0.0, 1.0, self.n)
        self.terms = gn.segment_terms(xyz, cells, self.alpha, self.q, mg.view_rotations(0.13, 0.21), RX, RY, mg.REFERENCE_BOUNDS)
        self.residual = rng.normal(size=(RY, RX, 2)).astype(np.float32)
        self.weight = np.abs(rng.normal(size=(RY, RX, 2))).astype(np.float32)
        self.va, self.vq = rng.normal(size=self.n), rng.normal(size=self.n)


@pytest.fixture(scope="module")
def scene():
    return _Scene()


class _Stub:
    """A context's face as RowShards uses it, over the global rows `rows` of the scene; every call is noted in `log`."""
    res_x, res_y, device = RX, RY, "cpu"

    def __init__(self, scene, rows, log, name):
        self.s, self.rows, self.log, self.name = scene, np.asarray(rows), log, name
        self.n_cells, self.local_rows = scene.n, len(self.rows)
        P, C_, dtau, dI_da, dI_dq = scene.terms
        row_of = P // RX
        local = {int(r): k for k, r in enumerate(self.rows)}
        keep = np.isin(row_of, self.rows)
        self.P = np.array([local[int(r)] for r in row_of[keep]], np.int64) * RX + P[keep] % RX  # the local pixel
        self.C, self.dtau, self.dI_da, self.dI_dq = C_[keep], dtau[keep], dI_da[keep], dI_dq[keep]
        self.scalars = None

    def update_scalars(self, alpha, q):
        self.scalars = (np.array(alpha), np.array(q))

    def render_tangent(self, d_alpha=None, d_q=None):
        va = np.zeros(self.n_cells) if d_alpha is None else d_alpha
        vq = np.zeros(self.n_cells) if d_q is None else d_q
        jv = np.zeros((self.local_rows * RX, 2))
        np.add.at(jv[:, 0], self.P, self.dtau * va[self.C])
        np.add.at(jv[:, 1], self.P, self.dI_da * va[self.C] + self.dI_dq * vq[self.C])
        return jv.reshape(self.local_rows, RX, 2).astype(np.float32)

    def _contributions(self, what, image, d_alpha, d_q):
        """Per segment (alpha's, q's), one fp64 value each - any fixed function of the segment will do for the stand-in."""
        if image is None:
            assert what == capi.C5_EXACT_GN_DIAGONAL
            image = np.ones((self.local_rows, RX, 2), np.float32)
        assert image.dtype == np.float32 and image.shape == (self.local_rows, RX, 2)
        g = image.reshape(-1, 2).astype(np.float64)[self.P]
        if what == capi.C5_EXACT_ADJOINT:
            assert d_alpha is None and d_q is None
            return g[:, 0] * self.dtau + g[:, 1] * self.dI_da, g[:, 1] * self.dI_dq
        if what == capi.C5_EXACT_GN_DIAGONAL:
            assert d_alpha is None and d_q is None
            return g[:, 0] * self.dtau ** 2 + g[:, 1] * self.dI_da ** 2, g[:, 1] * self.dI_dq ** 2
        assert what == capi.C5_EXACT_HVP and (d_alpha is not None or d_q is not None)
        va = np.zeros(self.n_cells) if d_alpha is None else d_alpha
        vq = np.zeros(self.n_cells) if d_q is None else d_q
        return g[:, 1] * self.dI_da * va[self.C], g[:, 1] * self.dI_dq * vq[self.C]

    def _per_cell(self, x):
        out = [[] for _ in range(self.n_cells)]
        for c, v in zip(self.C, x):
            out[c].append(float(v))
        return out

    def render_exact_bounds(self, what, image=None, d_alpha=None, d_q=None):
        self.log.append(("bounds", self.name, what))
        return tuple(np.array([er.exponent_over(p) for p in self._per_cell(x)], np.int32)
                     for x in self._contributions(what, image, d_alpha, d_q))

    def render_exact_sums(self, what, exp_alpha, exp_q, image=None, d_alpha=None, d_q=None):
        self.log.append(("sums", self.name, what, np.array(exp_alpha), np.array(exp_q)))
        return tuple(np.array([er.words(p, int(e), M) for p, e in zip(self._per_cell(x), exps)], np.int64).reshape(self.n_cells, 2)
                     for x, exps in zip(self._contributions(what, image, d_alpha, d_q), (exp_alpha, exp_q)))


def _operators(ops, s):
    t = torch.tensor
    return {"rhs": lambda: ops.rhs(t(s.residual)), "diagonal": ops.diagonal, "product": lambda: ops.product(t(s.va), t(s.vq)),
            "hvp": lambda: ops.hvp(t(s.va), None, t(s.residual))}


def test_row_sets_that_overlap_or_leave_a_row_out_are_refused(scene):
    def stubs(*row_sets):
        return [(_Stub(scene, rows, [], k), rows) for k, rows in enumerate(row_sets)]

    fit.RowShards(stubs(np.arange(0, 3), np.arange(3, RY)))
    fit.RowShards(stubs(np.array([0, 1, 4, 5]), np.array([2, 3, 6])))  # (row tiles)
    for bad in ((np.arange(0, 4), np.arange(3, RY)),       # row 3 twice
                (np.arange(0, 3), np.arange(4, RY)),       # row 3 left out
                (np.arange(0, 3), np.arange(3, RY + 1)),   # a row beyond the image
                (np.arange(0, 3), np.arange(2, RY - 1))):  # as many rows as the image has, one twice and one missing
        with pytest.raises(ValueError, match="partition"):
            fit.RowShards(stubs(*bad))
    with pytest.raises(ValueError):
        fit.RowShards([])
    part = _Stub(scene, np.arange(0, 3), [], 0)
    with pytest.raises(ValueError, match="rows"):
        fit.RowShards([(part, np.arange(0, 4)), (_Stub(scene, np.arange(4, RY), [], 1), np.arange(4, RY))])


def test_bounds_come_before_sums_and_every_part_gets_the_combined_exponents(scene):
    log = []
    rows = (np.array([0, 1, 4, 5]), np.array([2, 3, 6]))
    shards = fit.RowShards([(_Stub(scene, r, log, k), r) for k, r in enumerate(rows)])
    ops = shards.gn_operators(torch.tensor(scene.alpha), torch.tensor(scene.q), torch.tensor(scene.weight))
    for ctx, _rows in shards.parts:  # (the scalars went to every context)
        assert np.array_equal(ctx.scalars[0], scene.alpha) and np.array_equal(ctx.scalars[1], scene.q)
    kinds = {"rhs": capi.C5_EXACT_ADJOINT, "diagonal": capi.C5_EXACT_GN_DIAGONAL, "product": capi.C5_EXACT_ADJOINT, "hvp": capi.C5_EXACT_HVP}
    for name, call in _operators(ops, scene).items():
        del log[:]
        out = call()
        assert [e[0] for e in log] == ["bounds", "bounds", "sums", "sums"], name
        assert sorted(e[1] for e in log[:2]) == sorted(e[1] for e in log[2:]) == [0, 1], name
        assert all(e[2] == kinds[name] for e in log), name
        assert np.array_equal(log[2][3], log[3][3]) and np.array_equal(log[2][4], log[3][4]), name
        assert all(isinstance(t, torch.Tensor) and t.dtype == torch.float64 and t.shape == (scene.n,) for t in out), name


def test_the_exponents_handed_on_are_the_elementwise_max_of_the_parts(scene):
    log = []
    rows = (np.arange(0, 3), np.arange(3, RY))
    parts = [(_Stub(scene, r, log, k), r) for k, r in enumerate(rows)]
    ops = fit.RowShards(parts).gn_operators(torch.tensor(scene.alpha), torch.tensor(scene.q), torch.tensor(scene.weight))
    ops.diagonal()
    handed = log[2][3], log[2][4]
    own = [ctx.render_exact_bounds(capi.C5_EXACT_GN_DIAGONAL, image=scene.weight[r]) for ctx, r in parts]
    for k in range(2):
        assert np.array_equal(handed[k], np.maximum(own[0][k], own[1][k]))
    assert (own[0][0] != own[1][0]).any()  # (the parts do differ)


def test_two_parts_give_the_bits_of_one_over_the_whole_image(scene):
    a, q, w = torch.tensor(scene.alpha), torch.tensor(scene.q), torch.tensor(scene.weight)
    whole = fit.RowShards([(_Stub(scene, np.arange(RY), [], 0), np.arange(RY))]).gn_operators(a, q, w)
    want = {name: call() for name, call in _operators(whole, scene).items()}
    for rows in ((np.arange(0, 3), np.arange(3, RY)), (np.array([0, 1, 4, 5]), np.array([2, 3, 6]))):
        ops = fit.RowShards([(_Stub(scene, r, [], k), r) for k, r in enumerate(rows)]).gn_operators(a, q, w)
        for name, call in _operators(ops, scene).items():
            got = call()
            for g, t in zip(got, want[name]):
                assert np.array_equal(g.numpy().view(np.int64), t.numpy().view(np.int64)), name
            assert any(float(t.abs().max()) > 0 for t in got), name
    # the steps run through the hook unchanged
    (d_alpha, d_q), models = fit.gn_step(fit.RowShards([(_Stub(scene, np.arange(RY), [], 0), np.arange(RY))]), a, q,
                                         torch.tensor(scene.residual), w, fit=("alpha", "q"), iters=2)
    assert d_alpha.shape == (scene.n,) and d_q.shape == (scene.n,) and len(models) >= 1

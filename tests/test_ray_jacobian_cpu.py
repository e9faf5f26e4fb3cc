"""Ray Jacobian, no GPU: the C ABI's declarations, the library's exports and the capi wrappers' argument checks (they raise
before anything reaches the library), what the wrappers send, and fit.JacobianOperators - the operators fit.ExplicitJacobian
hands to gn_step - built from the restatement's per-segment terms on torch CPU tensors, against the restatement's own
product, diagonal and gradients.

The bar of the operator tests is fp64 summation and nothing else: both sides add the SAME doubles (gn_reference.
segment_terms'), in another order and grouping.  A sum of n terms t_i, whatever its order, lies within (n - 1) 2^-53 sum
|t_i| of the exact sum to first order; two such sums differ by at most twice that, and every term carries up to two
products' roundings of its own: n 2^-52 sum |t_i| per element covers both.  The product nests two sums: the bar of J v
per pixel, carried through |w| |J| into the cells, is added to the outer sum's own."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from course5_amd import capi, fit
from course5_amd import meshgen as mg
from tests import adjoint_reference as ar
from tests import gn_reference as gr
from tests.fake_library import RecordingLibrary, bare_context

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
U = 2.0 ** -52
B = mg.REFERENCE_BOUNDS
ROTS = mg.view_rotations(0.13, 0.21, 0.05)
DECLARATIONS = (
    ("c5_ray_jacobian_fill", r"c5_context\* ctx, const int64_t\* row_ptr_host, int64_t capacity, int32_t\* col_host, double\* dz_host,\s+"
                             r"double\* dI_dalpha_host, double\* dI_dq_host"),
    ("c5_ray_jacobian_fill_device", r"c5_context\* ctx, const void\* row_ptr_dev, int64_t capacity, void\* col_dev, void\* dz_dev,\s+"
                                    r"void\* dI_dalpha_dev, void\* dI_dq_dev"),
)


def test_header_declares_and_the_library_exports_the_two_symbols():
    text = open(os.path.join(ROOT, "include", "course5_hip.h")).read()
    assert "#define C5_ABI_VERSION 2" in text
    exported = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for name, args in DECLARATIONS:
        assert re.search(r"int " + name + r"\(" + args + r"\);", text), name
        assert name in capi.EXPORTS
        assert re.search(r" T " + name + r"$", exported, flags=re.M), name
    lib = capi.load_library()
    assert [len(getattr(lib, name).argtypes) for name, _ in DECLARATIONS] == [7, 7]
    for name in ("ray_jacobian_fill", "ray_jacobian_fill_device", "ray_jacobian"):
        assert callable(getattr(capi.Context, name)), name
    from course5_amd import autograd
    assert "ray_jacobian" in autograd.__all__ and callable(autograd.ray_jacobian)
    assert callable(fit.ExplicitJacobian(None).gn_operators)


def test_the_host_wrapper_rejects_bad_arguments_before_touching_a_gpu():
    ctx = bare_context(n_cells=11, rows=5, cols=7)
    n = 5 * 7 + 1
    for bad in (np.zeros(n, np.int32), np.zeros(n, np.float64), np.zeros(n - 1, np.int64), np.zeros((n, 1), np.int64), [0] * n, None):
        with pytest.raises(ValueError, match="row_ptr"):
            ctx.ray_jacobian_fill(bad)
    with pytest.raises(ValueError, match="capacity"):
        ctx.ray_jacobian_fill(np.zeros(n, np.int64), capacity=-1)


def test_the_device_wrapper_rejects_bad_arguments_before_touching_a_gpu():
    ctx = bare_context(n_cells=11, rows=5, cols=7)
    n = 5 * 7 + 1
    with pytest.raises(ValueError, match="dI_dalpha or dI_dq"):  # both value arrays missing
        ctx.ray_jacobian_fill_device(1, 2, 3, None, None, capacity=4)
    with pytest.raises(ValueError, match="row_ptr"):
        ctx.ray_jacobian_fill_device(None, 2, 3, 4, 5, capacity=4)
    with pytest.raises(ValueError, match="capacity"):
        ctx.ray_jacobian_fill_device(1, 2, 3, 4, 5, capacity=-1)
    with pytest.raises(ValueError, match="capacity"):  # raw pointers do not say how long they are
        ctx.ray_jacobian_fill_device(1, 2, 3, 4, 5)
    with pytest.raises(ValueError, match="capacity"):
        ctx.ray_jacobian_fill_device(1, None, None, None, 5)
    # (CPU tensors, wrong dtypes, wrong lengths: _device_ptr raises before the call)
    for bad in (torch.zeros(n, dtype=torch.int64), torch.zeros(n, dtype=torch.int32), torch.zeros(n - 1, dtype=torch.int64)):
        with pytest.raises(ValueError, match="expected a contiguous"):
            ctx.ray_jacobian_fill_device(bad, 0, 0, 4, 5, capacity=4)
    for bad in (torch.zeros(4, dtype=torch.float64), torch.zeros(4, dtype=torch.float32)):
        with pytest.raises(ValueError, match="expected a contiguous"):
            ctx.ray_jacobian_fill_device(1, None, None, bad, None)


def test_what_reaches_the_library():
    ctx = bare_context(n_cells=11, rows=2, cols=3)
    ctx.lib = lib = RecordingLibrary()
    rows = np.array([0, 1, 1, 2, 3, 3, 3], np.int64)
    out = ctx.ray_jacobian_fill(rows)
    assert [(a.dtype, a.shape) for a in out] == [(np.int32, (3,))] + [(np.float64, (3,))] * 3
    out = ctx.ray_jacobian_fill(rows, with_structure=False)
    assert [(a.dtype, a.shape) for a in out] == [(np.float64, (3,))] * 2
    out = ctx.ray_jacobian_fill(rows, 10)
    assert [a.shape for a in out] == [(10,)] * 4
    ctx.ray_jacobian_fill_device(101, 102, 103, 104, 105, capacity=9)
    ctx.ray_jacobian_fill_device(101, None, None, None, 105, capacity=9)
    out = ctx.ray_jacobian()
    assert len(out) == 5 and out[0].shape == (7,)
    assert lib.calls == [
        ("c5_ray_jacobian_fill", (None, "ptr", 3, "ptr", "ptr", "ptr", "ptr")),
        ("c5_ray_jacobian_fill", (None, "ptr", 3, None, None, "ptr", "ptr")),
        ("c5_ray_jacobian_fill", (None, "ptr", 10, "ptr", "ptr", "ptr", "ptr")),
        ("c5_ray_jacobian_fill_device", (None, 101, 9, 102, 103, 104, 105)),
        ("c5_ray_jacobian_fill_device", (None, 101, 9, None, None, None, 105)),
        ("c5_ray_matrix_rows", (None, "ptr", "ptr")),
        ("c5_ray_jacobian_fill", (None, "ptr", None, "ptr", "ptr", "ptr", "ptr")),
    ]


# ---- the operators from plain arrays ----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scene():
    """Kuhn box 3 at 13 x 11 under a three-axis view, with a clamped and an inactive cell the image sees."""
    xyz, cells = mg.kuhn_box(3, jitter=0.1)
    n, rx, ry = len(cells), 13, 11
    rng = np.random.default_rng(47)
    alpha = rng.uniform(0.3, 2.0, n)
    q = rng.uniform(0.1, 1.0, n)
    m0 = ar.ray_matrices(xyz, cells, alpha, q, ROTS, rx, ry, B)
    seen = np.unique(m0["C"][m0["valid"]])
    clamped, inactive = int(seen[len(seen) // 3]), int(seen[2 * len(seen) // 3])
    alpha[clamped] = 3.7           # above the limit of 2.5: dI/dalpha = 0, dtau/dalpha = dz
    alpha[inactive] = 0.5 * EPS    # below DBL_EPSILON: nothing in I
    m = ar.ray_matrices(xyz, cells, alpha, q, ROTS, rx, ry, B)
    terms = gr.terms_of(m)
    P, C, dz, da, dq = terms
    assert (da[C == clamped] == 0).all() and (dq[C == clamped] > 0).all() and (C == clamped).any()
    assert (da[C == inactive] == 0).all() and (dq[C == inactive] == 0).all() and (C == inactive).any()
    assert (np.diff(P) >= 0).all()  # (by pixel: CSR order)
    n_px = rx * ry
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(P, minlength=n_px))]).astype(np.int64)
    w = rng.uniform(0.0, 2.0, (ry, rx, 2)).astype(np.float32)
    w[3:5, 2:9] = 0.0
    return dict(n=n, n_px=n_px, rx=rx, ry=ry, m=m, terms=terms, row_ptr=row_ptr, w=w, rng=rng)


def _operators(s, weight):
    P, C, dz, da, dq = s["terms"]
    t = torch.from_numpy
    return fit.JacobianOperators(t(s["row_ptr"]), t(C.astype(np.int32)), t(dz), t(da), t(dq), s["n"],
                                 None if weight is None else torch.as_tensor(weight))


def _check(got, want, bar, what):
    got = got.numpy()
    assert got.dtype == np.float64 and got.shape == want.shape
    r = np.abs(got - want) / np.maximum(bar, 1e-300)
    print(f"{what}: worst error / bar {r.max():.3g}, largest |value| {np.abs(want).max():.3g}")
    assert np.abs(want).max() > 0 or not bar.any(), what  # (all zero only where nothing was summed: tau without d_alpha)
    assert (np.abs(got - want) <= bar).all(), what


@pytest.mark.parametrize("weighted", [False, True])
def test_product_and_diagonal_equal_the_restatement(scene, weighted):
    s = scene
    P, C, dz, da, dq = s["terms"]
    n, n_px = s["n"], s["n_px"]
    w = s["w"] if weighted else None
    w64 = np.ones((n_px, 2)) if w is None else w.astype(np.float64).reshape(n_px, 2)
    ops = _operators(s, w)
    count_c = np.bincount(C, minlength=n)
    count_p = np.bincount(P, minlength=n_px)
    # the diagonal
    want_a, want_q = gr.diagonal(s["terms"], n_px, n, w)
    got_a, got_q = ops.diagonal()
    abs_a = np.bincount(C, weights=w64[P, 0] * dz ** 2 + w64[P, 1] * da ** 2, minlength=n)
    abs_q = np.bincount(C, weights=w64[P, 1] * dq ** 2, minlength=n)
    _check(got_a, want_a, 2 * count_c * U * abs_a, "diag_alpha")
    _check(got_q, want_q, count_c * U * abs_q, "diag_q")
    # the product, both blocks and each alone
    va, vq = s["rng"].normal(size=n), s["rng"].normal(size=n)
    for a, b in ((va, vq), (va, None), (None, vq)):
        want_ha, want_hq, want_jv = gr.product(s["terms"], n_px, n, a, b, w)
        za, zq = (np.zeros(n) if v is None else v for v in (a, b))
        got_ha, got_hq = ops.product(None if a is None else torch.from_numpy(a), None if b is None else torch.from_numpy(b))
        tau, I = ops.jv(None if a is None else torch.from_numpy(a), None if b is None else torch.from_numpy(b))
        abs_tau = np.bincount(P, weights=np.abs(dz * za[C]), minlength=n_px)
        abs_I = np.bincount(P, weights=np.abs(da * za[C]) + np.abs(dq * zq[C]), minlength=n_px)
        e_tau, e_I = count_p * U * abs_tau, 2 * count_p * U * abs_I
        _check(tau, want_jv[:, 0], e_tau, "J v, tau")
        _check(I, want_jv[:, 1], e_I, "J v, I")
        g = np.abs(w64 * want_jv)
        outer_a = np.bincount(C, weights=g[P, 0] * dz + g[P, 1] * np.abs(da), minlength=n)
        outer_q = np.bincount(C, weights=g[P, 1] * dq, minlength=n)
        carried_a = np.bincount(C, weights=w64[P, 0] * e_tau[P] * dz + w64[P, 1] * e_I[P] * np.abs(da), minlength=n)
        carried_q = np.bincount(C, weights=w64[P, 1] * e_I[P] * dq, minlength=n)
        _check(got_ha, want_ha, 2 * count_c * U * outer_a + 2 * carried_a, "h_alpha")
        _check(got_hq, want_hq, 2 * count_c * U * outer_q + 2 * carried_q, "h_q")


def test_rhs_is_the_adjoint_of_the_weighted_residual(scene):
    s = scene
    P, C, dz, da, dq = s["terms"]
    n, n_px = s["n"], s["n_px"]
    r = s["rng"].normal(size=(s["ry"], s["rx"], 2)).astype(np.float32)
    count_c = np.bincount(C, minlength=n)
    for w in (None, s["w"]):
        g32 = r if w is None else r * w  # (one fp32 multiply per channel, as the library's right-hand side)
        want_a, want_q, _tau, _I = ar.gradients_of(s["m"], n, g32.astype(np.float64))
        got_a, got_q = _operators(s, w).rhs(torch.from_numpy(r))
        g = np.abs(g32.astype(np.float64).reshape(n_px, 2))
        _check(got_a, want_a, 2 * count_c * U * np.bincount(C, weights=g[P, 0] * dz + g[P, 1] * np.abs(da), minlength=n), "rhs alpha")
        _check(got_q, want_q, count_c * U * np.bincount(C, weights=g[P, 1] * dq, minlength=n), "rhs q")


def test_gn_step_runs_on_the_array_built_operators(scene):
    """fit.gn_step takes anything with gn_operators: here a stand-in that hands out the array-built operators.  The first
    iterate of preconditioned CG has a closed form, x_1 = -t z with z = g / diag(H) and t = z.g / z.Hz, and the model
    there is -t z.g / 2: both are evaluated a second time through the restatement.  Bar: g, diag(H) and H z are each
    within 2 n 2^-52 of their absolute sums (the tests above), n the most terms an element sums; an inner product of
    n_cells such elements adds n_cells 2^-52 of its own absolute sum; t and the model are a ratio and a product of the two
    inner products, so their relative error is at most the sum of the two inner products' (each: absolute sum / |sum|),
    doubled for the second order."""
    s = scene
    n, n_px = s["n"], s["n_px"]
    r = torch.from_numpy(s["rng"].normal(size=(s["ry"], s["rx"], 2)).astype(np.float32))
    w = torch.from_numpy(s["w"])

    class StandIn:
        def gn_operators(self, alpha, q, weight):
            return _operators(s, weight)

    (d_alpha, d_q), models = fit.gn_step(StandIn(), torch.zeros(n), torch.zeros(n), r, w, fit=("q",), iters=3)
    assert d_alpha is None and d_q.shape == (n,) and len(models) == 3
    assert all(b <= a for a, b in zip(models, models[1:])) and models[0] < 0
    (_none, x1), (m1,) = fit.gn_step(StandIn(), torch.zeros(n), torch.zeros(n), r, w, fit=("q",), iters=1)
    g32 = r.numpy() * s["w"]
    _ga, gq, _t, _i = ar.gradients_of(s["m"], n, g32.astype(np.float64))
    _da, diag = gr.diagonal(s["terms"], n_px, n, s["w"])
    z = np.where(diag > 0, gq / np.where(diag > 0, diag, 1.0), 0.0)
    _ha, hz, _jv = gr.product(s["terms"], n_px, n, None, z, s["w"])
    zg, zhz = z @ gq, z @ hz
    t = zg / zhz
    terms = int(np.bincount(s["terms"][1], minlength=n).max()) * int(np.bincount(s["terms"][0], minlength=n_px).max())
    rel = 2 * (2 * terms + n) * U * (np.abs(z * gq).sum() / abs(zg) + np.abs(z * hz).sum() / abs(zhz))
    print(f"first CG iterate: model {m1:.6g} against {-0.5 * t * zg:.6g}, relative bar {rel:.3g}")
    assert abs(m1 + 0.5 * t * zg) <= 2 * rel * abs(0.5 * t * zg)
    assert np.abs(x1.numpy() + t * z).max() <= 2 * rel * np.abs(t * z).max()


def test_array_built_operators_have_no_second_derivatives_and_check_their_shapes(scene):
    ops = _operators(scene, None)
    with pytest.raises(RuntimeError, match="second derivatives"):
        ops.hvp(None, None, None)
    P, C, dz, da, dq = scene["terms"]
    t = torch.from_numpy
    with pytest.raises(ValueError, match="elements each"):
        fit.JacobianOperators(t(scene["row_ptr"]), t(C.astype(np.int32)), t(dz[:-1]), t(da), t(dq), scene["n"])
    with pytest.raises(ValueError, match="weight"):
        fit.JacobianOperators(t(scene["row_ptr"]), t(C.astype(np.int32)), t(dz), t(da), t(dq), scene["n"], torch.zeros(3, 2))


# ---- the operators bit for bit: every product is the gather, the multiply and the segmented sum written out ---------------

def _small(kind):
    """(row_ptr, col, n_cells, n_px) of a matrix whose offsets are the awkward ones: `empty` has no nonzero at all; `gaps` an
    empty first row, an empty last row, an empty row between, and columns (0, 3 and the last) no row names."""
    if kind == "empty":
        return np.zeros(5, np.int64), np.zeros(0, np.int32), 3, 4
    return np.array([0, 0, 2, 2, 5, 6, 6], np.int64), np.array([4, 1, 2, 5, 1, 4], np.int32), 7, 6


def _written_out_cases(scene):
    P, C, dz, da, dq = scene["terms"]
    yield "scene", scene["row_ptr"], C.astype(np.int32), scene["n"], (dz, da, dq), scene["w"]
    rng = np.random.default_rng(5)
    for kind in ("empty", "gaps"):
        row_ptr, col, n, n_px = _small(kind)
        yield kind, row_ptr, col, n, tuple(rng.normal(size=len(col)) for _ in range(3)), rng.uniform(0.0, 2.0, (n_px, 2)).astype(np.float32)


def test_every_product_is_the_segmented_sum_written_out_bit_for_bit(scene):
    from tests import operators_written_out as wo
    t = torch.from_numpy
    for kind, row_ptr, col, n, values, w in _written_out_cases(scene):
        n_px = len(row_ptr) - 1
        dz, da, dq = (t(v) for v in values)
        m = wo.ByRowAndColumn(row_ptr, col, n)
        rng = np.random.default_rng(6)
        va, vq = t(rng.normal(size=n)), t(rng.normal(size=n))
        r = rng.normal(size=(n_px, 2)).astype(np.float32)
        zero = torch.zeros(n_px, dtype=torch.float64)
        for weight in (None, w):
            ops = fit.JacobianOperators(t(row_ptr), t(col), dz, da, dq, n, None if weight is None else t(weight))
            jt = lambda g_tau, g_I: (m.to_columns(dz, g_tau) + m.to_columns(da, g_I), m.to_columns(dq, g_I))  # noqa: E731
            for a, b in ((va, vq), (va, None), (None, vq)):
                tau = zero if a is None else m.to_rows(dz, a)
                I = zero.clone()
                if a is not None:
                    I = I + m.to_rows(da, a)
                if b is not None:
                    I = I + m.to_rows(dq, b)
                got = ops.jv(a, b)
                assert torch.equal(got[0], tau) and torch.equal(got[1], I), (kind, "jv")
                w_tau, w_I = wo.weights(weight, n_px)
                want = jt(tau if weight is None else w_tau * tau, I if weight is None else w_I * I)
                got = ops.product(a, b)
                assert got[0].shape == (n,) and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (kind, "product")
            g_tau, g_I = t(rng.normal(size=n_px)), t(rng.normal(size=n_px))
            got, want = ops.jt(g_tau, g_I), jt(g_tau, g_I)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (kind, "jt")
            got, want = ops.rhs(t(r)), jt(*wo.weighted_image(r, weight))
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (kind, "rhs")
            w_tau, w_I = wo.weights(weight, n_px)
            got = ops.diagonal()
            assert torch.equal(got[0], m.to_columns(dz * dz, w_tau) + m.to_columns(da * da, w_I)), (kind, "diag_alpha")
            assert torch.equal(got[1], m.to_columns(dq * dq, w_I)), (kind, "diag_q")
            if kind == "gaps":  # the rows and columns nothing names are exact zeros, the others are not
                named = torch.zeros(n, dtype=torch.bool)
                named[t(col).long()] = True
                assert not got[1][~named].any() and (got[1][named] > 0).all()
                assert not ops.jv(va, vq)[1][[0, 2, 5]].any()


def test_the_messages_of_the_four_checks(scene):
    P, C, dz, da, dq = scene["terms"]
    t = torch.from_numpy
    row_ptr, col, n, n_px = t(scene["row_ptr"]), t(C.astype(np.int32)), scene["n"], scene["n_px"]
    nnz = len(C)
    with pytest.raises(ValueError, match=re.escape(f"col, dz, dI_dalpha and dI_dq must hold row_ptr's {nnz} elements each")):
        fit.JacobianOperators(row_ptr, col, t(dz), t(da[:-1]), t(dq), n)
    with pytest.raises(ValueError, match=re.escape(f"col, dz, dI_dalpha and dI_dq must hold row_ptr's {nnz} elements each")):
        fit.JacobianOperators(row_ptr, col[:-1], t(dz), t(da), t(dq), n)
    with pytest.raises(ValueError, match=re.escape(f"col must name cells 0 .. {int(C.max()) - 1}")):
        fit.JacobianOperators(row_ptr, col, t(dz), t(da), t(dq), int(C.max()))
    bad = col.clone()
    bad[0] = -1
    with pytest.raises(ValueError, match=re.escape(f"col must name cells 0 .. {n - 1}")):
        fit.JacobianOperators(row_ptr, bad, t(dz), t(da), t(dq), n)
    with pytest.raises(ValueError, match=re.escape(f"weight must hold two values for each of the {n_px} pixels")):
        fit.JacobianOperators(row_ptr, col, t(dz), t(da), t(dq), n, torch.zeros(n_px + 1, 2))
    with pytest.raises(ValueError, match=re.escape(f"residual must hold two values for each of the {n_px} pixels")):
        _operators(scene, None).rhs(torch.zeros(n_px - 1, 2))

"""The batched vertex adjoint (c5_render_vertex_adjoint_batch*) without a GPU: the C ABI's declarations, the library's
symbols, the bindings and their argument checks, the pins that must not move, and the yardstick the GPU test compares
against - tests/vertex_adjoint_reference.py applied image by image over ONE set of ray and face matrices, which is linear
in the upstream image and dual to tests/vertex_tangent_reference.py.

Bars.  Linearity: the restatement is sums of products with g, so gradients_of(fp32(2 g_a - 3 g_b)) against 2 ref_a - 3 ref_b
is held at (2^-23 + 1e-12) x (2 scale_a + 3 scale_b), scale the sums of absolute values the restatement returns itself: the
mix is rounded to fp32 once (2^-24 of it, a factor 2 to spare) and the fp64 sums add 1e-12.  Duality: 1e-12 x sum |terms|,
tests/test_vertex_tangent_cpu.py's bar."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from course5_amd import build, capi, meshgen as mg
from tests import adjoint_reference as ar, motion_reference as mr
from tests import vertex_adjoint_reference as vr, vertex_tangent_reference as vt
from tests.fake_library import RecordingLibrary, bare_context

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS = (1.9, 0.1, 0.9, -0.9)
RX, RY = 24, 18
ROTS = np.array([[0.0, 0.31, 0.0], [1.0, 0.22, 1.0]])
NAMES = ("c5_render_vertex_adjoint_batch", "c5_render_vertex_adjoint_batch_device")


def stacked_gradients(m, geo, cells, n_pts, rots, images):
    """The restatement for K upstream images over one set of matrices: a list of gradients_of's dicts, one per image."""
    return [vr.gradients_of(m, geo, cells, n_pts, rots, g) for g in images]


# ---- the C ABI and the bindings ---------------------------------------------------------------------------------------

def test_header_declares_the_two_calls_inside_the_vertex_adjoint_section():
    text = open(os.path.join(ROOT, "include", "course5_hip.h")).read()
    h = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    decls = ("int c5_render_vertex_adjoint_batch(c5_context* ctx, int n_imgs, const float* grad_out_host, double* grad_xyz_host);",
             "int c5_render_vertex_adjoint_batch_device(c5_context* ctx, int n_imgs, const void* grad_out_dev, void* grad_xyz_dev);")
    for decl in decls:
        assert decl in h, decl
    # directly below the single call's _device form, before the next section begins
    single = "int c5_render_vertex_adjoint_device(c5_context* ctx, const void* grad_out_dev, void* grad_xyz_dev);"
    assert h.index(single) < h.index(decls[0]) < h.index(decls[1]) < h.index("int c5_render_vertex_tangent(")
    assert h[h.index(single) + len(single):h.index(decls[0])].strip() == ""
    section = text.split("--- vertex adjoint render")[1].split("--- vertex tangent render")[0]
    assert "c5_render_vertex_adjoint_batch" in section and "\"batch_width\"" in section


def test_library_and_bindings_have_them():
    lib = ctypes.CDLL(capi.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in capi.EXPORTS
    assert len(capi.SIGNATURES[NAMES[0]]) == len(capi.SIGNATURES[NAMES[1]]) == 4  # (ctx, n_imgs, two pointers)
    for name in ("render_vertex_adjoint_batch", "render_vertex_adjoint_batch_device"):
        assert callable(getattr(capi.Context, name)), name


def test_pins_still_hold():
    assert build.kernel_source_hash() == "63c90aeb24365e47"  # (re-stamped with next_entry: profiles/component_fuzz.md)
    assert ctypes.CDLL(capi.LIB_PATH).c5_abi_version() == 2
    assert "#define C5_ABI_VERSION 2" in open(os.path.join(ROOT, "include", "course5_hip.h")).read()


def test_argument_checks_before_the_library():
    import torch
    ctx = bare_context()  # 9 points, images of 5 x 6
    msg = r"grad_out must be \[5, 6, 2\] or \[K, 5, 6, 2\]"
    bad = (np.zeros(60), np.zeros((5, 6)), np.zeros((1, 2, 5, 6, 2)),  # wrong rank
           np.zeros((4, 6, 2)), np.zeros((3, 5, 7, 2)), np.zeros((3, 5, 6, 3)),  # wrong image shape
           np.zeros((0, 5, 6, 2)))  # K = 0
    for g in bad:
        with pytest.raises(ValueError, match=msg):
            ctx.render_vertex_adjoint_batch(g)
    with pytest.raises(ValueError, match="expected a contiguous"):  # (host tensors are not device arrays)
        ctx.render_vertex_adjoint_batch_device(torch.zeros((2, 5, 6, 2)), torch.zeros((2, 9, 3), dtype=torch.float64))
    with pytest.raises(ValueError, match="grad_xyz must be"):
        ctx.render_vertex_adjoint_batch_device(torch.zeros((5, 6, 2)), torch.zeros((9, 3), dtype=torch.float64))
    with pytest.raises(ValueError, match="grad_xyz must be"):
        ctx.render_vertex_adjoint_batch_device(1, 2, n=0)
    with pytest.raises(AssertionError, match="the library was entered"):  # (a good call does get there)
        ctx.render_vertex_adjoint_batch(np.zeros((3, 5, 6, 2)))


@pytest.mark.parametrize("shape, k", [((3, 5, 6, 2), 3), ((5, 6, 2), 1), ((1, 5, 6, 2), 1)])
def test_the_library_sees_one_batched_call(shape, k):
    ctx = bare_context()
    ctx.lib = RecordingLibrary()
    out = ctx.render_vertex_adjoint_batch(np.ones(shape, dtype=np.float64))  # (converted to float32 on the way)
    assert ctx.lib.calls == [("c5_render_vertex_adjoint_batch", (None, k, "ptr", "ptr"))]
    assert out.dtype == np.float64 and out.shape == (k, 9, 3)
    ctx.lib = RecordingLibrary()
    ctx.render_vertex_adjoint_batch_device(0x1000, 0x2000, n=k)
    assert ctx.lib.calls == [("c5_render_vertex_adjoint_batch_device", (None, k, 0x1000, 0x2000))]


# ---- the yardstick -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scene():
    xyz, cells = mg.kuhn_box(3, jitter=0.2)
    a, q = mr.scalars(len(cells), 7)
    alpha = 0.6 * a  # below the 2.5 clamp
    m = ar.ray_matrices(xyz, cells, alpha, q, ROTS, RX, RY, BOUNDS)
    geo = vr.segment_faces(xyz, cells, ROTS, RX, RY, BOUNDS)
    rng = np.random.default_rng(61)
    images = rng.normal(size=(5, RY, RX, 2)).astype(np.float32)
    images[1, ..., 1] = 0.0  # tau only
    images[2, ..., 0] = 0.0  # I only
    images[3] = 0.0
    return types.SimpleNamespace(xyz=xyz, cells=cells, alpha=alpha, q=q, m=m, geo=geo, images=images, fields=rng.normal(size=(2,) + xyz.shape))


def test_slices_of_the_stacked_restatement_are_the_single_applications(scene):
    s = scene
    stacked = stacked_gradients(s.m, s.geo, s.cells, len(s.xyz), ROTS, s.images)
    assert len(stacked) == len(s.images)
    for k, g in enumerate(s.images):
        alone = vr.vertex_gradients(s.xyz, s.cells, s.alpha, s.q, ROTS, RX, RY, BOUNDS, g)
        for key in ("raw", "scale_raw", "sens_raw"):
            assert np.array_equal(stacked[k][key], alone[key]), (k, key)
    assert not stacked[3]["raw"].any() and np.abs(stacked[0]["raw"]).max() > 0
    # tau-only and I-only images add up to the image that has both channels
    both = s.images[1] + s.images[2]
    ref = vr.gradients_of(s.m, s.geo, s.cells, len(s.xyz), ROTS, both)
    err = np.abs(ref["raw"] - (stacked[1]["raw"] + stacked[2]["raw"]))
    assert (err <= 1e-12 * ref["scale_raw"]).all()


def test_the_restatement_is_linear_in_the_upstream_image(scene):
    s = scene
    ga, gb = s.images[0], s.images[4]
    mix = (2.0 * ga.astype(np.float64) - 3.0 * gb.astype(np.float64)).astype(np.float32)  # (exact in fp64: ONE fp32 rounding)
    ra, rb, rm = (vr.gradients_of(s.m, s.geo, s.cells, len(s.xyz), ROTS, g) for g in (ga, gb, mix))
    # the fp32 rounding of the mix is 2^-24 of it: compare against the fp64 combination of the two at that bar
    want = 2.0 * ra["raw"] - 3.0 * rb["raw"]
    bound = 2.0 * ra["scale_raw"] + 3.0 * rb["scale_raw"]
    err = np.abs(rm["raw"] - want)
    print(f"linearity: worst error / bound {(err / bound).max():.3g}")
    assert np.abs(want).max() > 0 and (err <= (2.0 ** -23 + 1e-12) * bound).all()


def test_duality_of_every_slice_with_the_vertex_tangent_restatement(scene):
    s = scene
    stacked = stacked_gradients(s.m, s.geo, s.cells, len(s.xyz), ROTS, s.images)
    for j, d in enumerate(s.fields):
        tau_dot, I_dot = vt.tangent_of(s.m, s.geo, s.cells, ROTS, d)
        for k, g in enumerate(s.images):
            g64 = g.astype(np.float64)
            lhs = float((stacked[k]["raw"] * d).sum())
            terms = np.concatenate([(g64[..., 0] * tau_dot).ravel(), (g64[..., 1] * I_dot).ravel()])
            rhs, size = float(terms.sum()), float(np.abs(terms).sum())
            print(f"field {j} image {k}: <J^T g, d> = {lhs:.15g}, <g, J d> = {rhs:.15g}, |difference| = {abs(lhs - rhs):.3g}")
            assert abs(lhs - rhs) <= 1e-12 * size
            assert (abs(rhs) > 0) == bool(g.any())

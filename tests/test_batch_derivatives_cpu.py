"""Batched tangent / adjoint renders and the device scalar upload, no GPU: the C ABI declarations, exports and bindings;
the torch Functions' vmap rules and their refusals (batched scalar fields, second derivatives) before any GPU work."""
import os
import re
import types

import pytest

from course5_amd import build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLS = (
    ("c5_render_tangent_batch", r"c5_context\* ctx, int n_dirs, const double\* d_alpha_host, const double\* d_q_host, float\* out_host"),
    ("c5_render_tangent_batch_device", r"c5_context\* ctx, int n_dirs, const void\* d_alpha_dev, const void\* d_q_dev, void\* out_dev"),
    ("c5_render_adjoint_batch",
     r"c5_context\* ctx, int n_imgs, const float\* grad_out_host, double\* grad_alpha_host, double\* grad_q_host"),
    ("c5_render_adjoint_batch_device",
     r"c5_context\* ctx, int n_imgs, const void\* grad_out_dev, void\* grad_alpha_dev, void\* grad_q_dev"),
    ("c5_update_scalars_device", r"c5_context\* ctx, const void\* alpha_dev, const void\* q_dev, int64_t n_cells"),
)


def test_header_declares_the_batch_calls_and_the_library_exports_them():
    text = open(os.path.join(ROOT, "include", "course5_hip.h")).read()
    assert re.search(r"#define C5_ABI_VERSION 2\b", text)  # (purely additive)
    lib = capi.load_library()
    for name, args in DECLS:
        assert re.search(r"int " + name + r"\(" + args + r"\);", text), name
        assert name in capi.EXPORTS
        assert getattr(lib, name).restype is not None, name  # (the symbol is in the built library)
    assert len(lib.c5_render_tangent_batch.argtypes) == 5 and len(lib.c5_update_scalars_device.argtypes) == 4
    for m in ("render_tangent_batch", "render_tangent_batch_device", "render_adjoint_batch", "render_adjoint_batch_device",
              "update_scalars_device"):
        assert hasattr(capi.Context, m), m


def test_the_forward_kernels_are_untouched():
    # the forward kernels' sources as the walk refactor left them (same machine code as 688bc525360ea908, the edge-on rule of
    # face_plane: profiles/walk_refactor_isa.md; the committed r04 profiles were measured on 85a78f3eaf095461): the batches
    # live beside the derivative kernels only.  Since then walk_common.hpp: next_entry takes or flags every entry beyond the
    # one taken (profiles/component_fuzz.md): 8d8cb316b206ad86 before that change
    assert build.kernel_source_hash() == "63c90aeb24365e47"
    for name in ("scalar_derivative_kernels.hip", "geometry_derivative_kernels.hip", "ray_matrix_kernels.hip", "deriv_ray.hpp", "deriv_lists.hpp", "deriv_faces.hpp"):
        assert name not in build.DEVICE_SOURCES, name


def test_batch_argument_checks_before_the_library():
    fake = types.SimpleNamespace(n_cells=5, local_rows=3, res_x=4)
    with pytest.raises(ValueError, match="directions must be"):
        capi.Context._batch_directions(fake, [[1.0] * 4], None)
    with pytest.raises(ValueError, match="same number of directions"):
        capi.Context._batch_directions(fake, [[1.0] * 5], [[1.0] * 5] * 2)
    with pytest.raises(ValueError, match="give d_alpha and / or d_q"):
        capi.Context._batch_directions(fake, None, None)
    da, dq, k = capi.Context._batch_directions(fake, [[1.0] * 5] * 3, None)
    assert k == 3 and dq is None and da.shape == (3, 5)


def test_functions_have_vmap_rules_and_refuse_second_derivatives():
    import torch
    from course5_amd import autograd
    for fn in (autograd._Render, autograd._Tangent, autograd._Adjoint):
        for name in ("forward", "setup_context", "backward", "jvp", "vmap"):
            assert getattr(fn, name) is not getattr(torch.autograd.Function, name), (fn.__name__, name)  # (overridden below torch's)
    a, q = torch.zeros(4), torch.zeros(4)
    info = types.SimpleNamespace(batch_size=2, randomness="error")
    with pytest.raises(RuntimeError, match="a batch of scalar fields"):
        autograd._Render.vmap(info, (None, 0, None), None, torch.zeros(2, 4), q)
    with pytest.raises(RuntimeError, match="a batch of scalar fields"):
        autograd._Adjoint.vmap(info, (None, None, 0, 0), None, a, torch.zeros(2, 4), torch.zeros(2, 3, 2))
    with pytest.raises(RuntimeError, match="second derivatives are not supported"):
        autograd._Tangent.backward(None, torch.zeros(3))
    with pytest.raises(RuntimeError, match="second derivatives are not supported"):
        autograd._Adjoint.jvp(None, None, None, None)
    for fn, what in ((autograd._Tangent, "tangent"), (autograd._Adjoint, "adjoint"), (autograd._ViewTangent, "motion tangent"),
                     (autograd._ViewAdjoint, "motion tangent"), (autograd._VertexAdjoint, "vertex adjoint"),
                     (autograd._VertexTangent, "vertex tangent")):
        for refuse in (fn.backward, fn.jvp):
            with pytest.raises(RuntimeError, match=rf"second derivatives are not supported \(the {what} render has no"):
                refuse(None, torch.zeros(3))
    fctx = types.SimpleNamespace(levels=2, primals=(a, q))
    with pytest.raises(RuntimeError, match="second derivatives are not supported"):
        autograd._Render.backward(fctx, torch.zeros(3, 4, 2))
    # no torch.func transform around: nothing differentiates
    assert autograd._differentiating_levels() == 0

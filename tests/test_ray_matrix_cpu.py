"""Ray matrix, no GPU: the C ABI's declarations, the library's exports and the capi wrappers' checks of shapes and dtypes
(they raise before anything reaches the library)."""
import os
import re
import subprocess

import numpy as np
import pytest

from course5_amd import capi
from tests.fake_library import bare_context

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECLARATIONS = (
    ("c5_ray_matrix_rows", r"c5_context\* ctx, int64_t\* row_ptr_host, int64_t\* nnz"),
    ("c5_ray_matrix_rows_device", r"c5_context\* ctx, void\* row_ptr_dev, int64_t\* nnz"),
    ("c5_ray_matrix_fill", r"c5_context\* ctx, const int64_t\* row_ptr_host, int64_t capacity, int32_t\* col_host, double\* dz_host,\s+"
                           r"double\* z_exit_host"),
    ("c5_ray_matrix_fill_device", r"c5_context\* ctx, const void\* row_ptr_dev, int64_t capacity, void\* col_dev, void\* dz_dev,\s+"
                                  r"void\* z_exit_dev"),
)


def test_header_declares_and_the_library_exports_the_four_symbols():
    text = open(os.path.join(ROOT, "include", "course5_hip.h")).read()
    assert "#define C5_ABI_VERSION 2" in text
    exported = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for name, args in DECLARATIONS:
        assert re.search(r"int " + name + r"\(" + args + r"\);", text), name
        assert name in capi.EXPORTS
        assert re.search(r" T " + name + r"$", exported, flags=re.M), name
    lib = capi.load_library()
    assert [len(getattr(lib, name).argtypes) for name, _ in DECLARATIONS] == [3, 3, 6, 6]
    for name in ("ray_matrix_rows", "ray_matrix_rows_device", "ray_matrix_fill", "ray_matrix_fill_device", "ray_matrix"):
        assert hasattr(capi.Context, name), name
    from course5_amd import autograd
    assert "ray_matrix" in autograd.__all__


def test_fill_rejects_wrong_row_ptr_shapes_and_dtypes_before_touching_a_gpu():
    ctx = bare_context(n_cells=11, rows=5, cols=7)
    n = 5 * 7 + 1
    for bad in (np.zeros(n, np.int32), np.zeros(n, np.float64), np.zeros(n - 1, np.int64), np.zeros((n, 1), np.int64),
                [0] * n, None):
        with pytest.raises(ValueError, match="row_ptr"):
            ctx.ray_matrix_fill(bad)
    with pytest.raises(ValueError, match="capacity"):
        ctx.ray_matrix_fill(np.zeros(n, np.int64), capacity=-1)


def test_device_forms_reject_wrong_tensors_before_touching_a_gpu():
    import torch
    ctx = bare_context(n_cells=11, rows=5, cols=7)
    n = 5 * 7 + 1
    # (CPU tensors, wrong dtypes, wrong lengths: _device_ptr raises before the call)
    for bad in (torch.zeros(n, dtype=torch.int64), torch.zeros(n, dtype=torch.int32), torch.zeros(n - 1, dtype=torch.int64)):
        with pytest.raises(ValueError, match="expected a contiguous"):
            ctx.ray_matrix_rows_device(bad)
        with pytest.raises(ValueError, match="expected a contiguous"):
            ctx.ray_matrix_fill_device(bad, 0, 0, capacity=4)
    with pytest.raises(ValueError, match="capacity"):
        ctx.ray_matrix_fill_device(0, 0, 0)
    with pytest.raises(ValueError, match="capacity"):
        ctx.ray_matrix_fill_device(0, None, None)

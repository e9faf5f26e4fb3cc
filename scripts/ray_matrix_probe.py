"""Ray matrix on the C3 frame: c5_ray_matrix_rows_device and c5_ray_matrix_fill_device (without
and with z_exit) beside c5_render_adjoint_device in the same process.  Device arrays throughout; every call between two HIP
events on the context's stream (the per-view setup each call makes is inside), the variants alternated, one warm-up round,
median and spread of the repeats.  Prints one JSON line; `--json PATH` writes it too.  `--quick`: fewer repeats."""
import json
import statistics
import sys

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import numpy as np  # noqa: E402
import torch  # noqa: E402

from course5_amd import capi, meshgen as mg  # noqa: E402

REPEATS = 3 if "--quick" in sys.argv else 9

xyz, cells, alpha, q = mg.workload("c3")
ctx = capi.Context(0)
ctx.set_option("stage_timing", 0)
ctx.set_option("walk_timing", 0)
ctx.upload_grid(xyz, cells, alpha, q)
ctx.set_image(2400, 1800, mg.REFERENCE_BOUNDS)
ctx.set_view(mg.view_rotations(**mg.BENCH_VIEW))
rows, cols = ctx.local_rows, 2400
dev = torch.device("cuda", 0)
G = torch.tensor(np.random.default_rng(1).normal(size=(rows, cols, 2)).astype(np.float32), device=dev)
GA = torch.empty(len(cells), dtype=torch.float64, device=dev)
GQ = torch.empty(len(cells), dtype=torch.float64, device=dev)
ROW_PTR = torch.empty(rows * cols + 1, dtype=torch.int64, device=dev)
torch.cuda.synchronize()
STREAM = torch.cuda.Stream(dev)  # (not torch's null stream, which the library would take for "its own")
torch.cuda.set_stream(STREAM)
ctx.set_stream(STREAM.cuda_stream)

nnz = ctx.ray_matrix_rows_device(ROW_PTR)
COL = torch.empty(nnz, dtype=torch.int32, device=dev)
DZ = torch.empty(nnz, dtype=torch.float64, device=dev)
Z = torch.empty(nnz, dtype=torch.float64, device=dev)


def timed(fn):
    """ms of one call between two events on the context's stream."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(STREAM)
    fn()
    e1.record(STREAM)
    assert ctx.synchronize() == capi.C5_OK
    e1.synchronize()
    return e0.elapsed_time(e1)


variants = {
    "adjoint_device": lambda: ctx.render_adjoint_device(G, GA, GQ),
    "rows_device": lambda: ctx.ray_matrix_rows_device(ROW_PTR),
    "fill_device": lambda: ctx.ray_matrix_fill_device(ROW_PTR, COL, DZ),
    "fill_device_with_depth": lambda: ctx.ray_matrix_fill_device(ROW_PTR, COL, DZ, Z),
}
for fn in variants.values():
    timed(fn)
acc = {k: [] for k in variants}
for _ in range(REPEATS):
    for k, fn in variants.items():
        acc[k].append(timed(fn))
ms = {k: round(statistics.median(v), 4) for k, v in acc.items()}
result = {"frame": "c3 2400x1800", "cells": len(cells), "nnz": nnz, "library": capi.LIB_PATH.rsplit("/", 1)[-1], "repeats": REPEATS,
          "ms": ms, "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in acc.items()},
          "store_gb_per_s": {"fill_device": round(nnz * 12 / ms["fill_device"] / 1e6, 1),
                             "fill_device_with_depth": round(nnz * 20 / ms["fill_device_with_depth"] / 1e6, 1)},
          "row_ptr_total_matches": bool(int(ROW_PTR[-1].item()) == nnz)}
line = json.dumps(result)
print(line)
if "--json" in sys.argv:
    with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
        f.write(line + "\n")

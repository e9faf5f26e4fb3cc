"""Ray Jacobian on the C3 frame: c5_ray_jacobian_fill_device (all four arrays, and the two value
arrays alone) beside c5_ray_matrix_fill_device and c5_render_adjoint_device, and one product of fit.JacobianOperators
over the exported arrays beside c5_render_gn_product_device, in the same process.  Device arrays throughout; every call
between two HIP events on the context's stream (the per-view setup each library call makes is inside), the variants
alternated, one warm-up round, median and spread of the repeats.  Prints one JSON line; `--json PATH` writes it too.
`--quick`: fewer repeats."""
import json
import statistics
import sys

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import numpy as np  # noqa: E402
import torch  # noqa: E402

from course5_amd import capi, fit, meshgen as mg  # noqa: E402

REPEATS = 3 if "--quick" in sys.argv else 9

xyz, cells, alpha, q = mg.workload("c3")
n = len(cells)
ctx = capi.Context(0)
ctx.set_option("stage_timing", 0)
ctx.set_option("walk_timing", 0)
ctx.upload_grid(xyz, cells, alpha, q)
ctx.set_image(2400, 1800, mg.REFERENCE_BOUNDS)
ctx.set_view(mg.view_rotations(**mg.BENCH_VIEW))
rows, cols = ctx.local_rows, 2400
dev = torch.device("cuda", 0)
rng = np.random.default_rng(1)
G = torch.tensor(rng.normal(size=(rows, cols, 2)).astype(np.float32), device=dev)
W = torch.tensor(rng.uniform(0.0, 2.0, (rows, cols, 2)).astype(np.float32), device=dev)
VA, VQ = (torch.tensor(rng.normal(size=(1, n)), device=dev) for _ in range(2))
GA, GQ = (torch.empty(n, dtype=torch.float64, device=dev) for _ in range(2))
HA, HQ = (torch.empty((1, n), dtype=torch.float64, device=dev) for _ in range(2))
ROW_PTR = torch.empty(rows * cols + 1, dtype=torch.int64, device=dev)
torch.cuda.synchronize()
STREAM = torch.cuda.Stream(dev)  # (not torch's null stream, which the library would take for "its own")
torch.cuda.set_stream(STREAM)
ctx.set_stream(STREAM.cuda_stream)

nnz = ctx.ray_matrix_rows_device(ROW_PTR)
COL = torch.empty(nnz, dtype=torch.int32, device=dev)
DZ, DA, DQ = (torch.empty(nnz, dtype=torch.float64, device=dev) for _ in range(3))
ctx.ray_jacobian_fill_device(ROW_PTR, COL, DZ, DA, DQ)
assert ctx.synchronize() == capi.C5_OK
OPS = fit.JacobianOperators(ROW_PTR, COL, DZ, DA, DQ, n, W)
STREAM.synchronize()


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
    "matrix_fill_device": lambda: ctx.ray_matrix_fill_device(ROW_PTR, COL, DZ),
    "jacobian_fill_device": lambda: ctx.ray_jacobian_fill_device(ROW_PTR, COL, DZ, DA, DQ),
    "jacobian_fill_device_values_only": lambda: ctx.ray_jacobian_fill_device(ROW_PTR, None, None, DA, DQ),
    "gn_product_device": lambda: ctx.render_gn_product_device(VA, VQ, W, HA, HQ, None, n=1),
    "explicit_product": lambda: OPS.product(VA[0], VQ[0]),
}
for fn in variants.values():
    timed(fn)
acc = {k: [] for k in variants}
for _ in range(REPEATS):
    for k, fn in variants.items():
        acc[k].append(timed(fn))
ms = {k: round(statistics.median(v), 4) for k, v in acc.items()}
saved = ms["gn_product_device"] - ms["explicit_product"]
result = {"frame": "c3 2400x1800", "cells": n, "nnz": nnz, "library": capi.LIB_PATH.rsplit("/", 1)[-1], "repeats": REPEATS,
          "ms": ms, "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in acc.items()},
          "store_gb_per_s": {"jacobian_fill_device": round(nnz * 28 / ms["jacobian_fill_device"] / 1e6, 1)},
          # rows + fill once, against what every product saves: the iteration count from which the export pays
          "break_even_products": (None if saved <= 0 else
                                  round((ms["rows_device"] + ms["jacobian_fill_device"]) / saved, 2)),
          "row_ptr_total_matches": bool(int(ROW_PTR[-1].item()) == nnz)}
line = json.dumps(result)
print(line)
if "--json" in sys.argv:
    with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
        f.write(line + "\n")

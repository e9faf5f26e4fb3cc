"""Ray shape Jacobian on the C3 frame: c5_ray_shape_jacobian_fill_device (all three arrays, and
dI_ddz alone) and c5_face_gradients_device beside c5_render_vertex_adjoint_device and c5_render_vertex_gn_product_device
(K = 1) - the legs alternated within every repeat after one warm-up round, median of 7 repeats.  Device arrays throughout; R
calls back to back between two HIP events on the context's stream.  The break-even: the fill's time over one library
product's - from that many CG iterations on, an export per linearisation costs less walk time than the products it
replaces (the sparse products on the exported arrays are not counted: they are torch's).  Prints one JSON line; `--json
PATH` writes it too.  `--quick`: fewer repeats."""
import json
import statistics
import sys

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import numpy as np  # noqa: E402
import torch  # noqa: E402

from course5_amd import capi, meshgen as mg  # noqa: E402

quick = "--quick" in sys.argv
REPEATS, CALLS = (2, 2) if quick else (7, 3)

xyz, cells, alpha, q = mg.workload("c3")
alpha = alpha.copy()
alpha[(alpha >= np.finfo(np.float64).eps) & (alpha < 1e-6)] = 1e-6
ctx = capi.Context(0)
ctx.set_option("stage_timing", 0)
ctx.set_option("walk_timing", 0)
ctx.upload_grid(xyz, cells, alpha, q)
ctx.set_image(2400, 1800, mg.REFERENCE_BOUNDS)
ctx.set_view(mg.view_rotations(**mg.BENCH_VIEW))
rows, cols, n_pts = ctx.local_rows, 2400, len(xyz)
dev = torch.device("cuda", 0)
rng = np.random.default_rng(1)
ROW_PTR = torch.empty(rows * cols + 1, dtype=torch.int64, device=dev)
torch.cuda.synchronize()
STREAM = torch.cuda.Stream(dev)  # (not torch's null stream, which the library would take for "its own")
torch.cuda.set_stream(STREAM)
ctx.set_stream(STREAM.cuda_stream)
nnz = ctx.ray_matrix_rows_device(ROW_PTR)
DI = torch.empty(nnz, dtype=torch.float64, device=dev)
FACES = torch.empty(nnz, dtype=torch.uint8, device=dev)
BARY = torch.empty((nnz, 2, 3), dtype=torch.float64, device=dev)
FPTS = torch.empty((len(cells), 4, 3), dtype=torch.int32, device=dev)
DW = torch.empty((len(cells), 4, 3), dtype=torch.float64, device=dev)
G = torch.tensor(rng.normal(size=(rows, cols, 2)).astype(np.float32), device=dev)
W = torch.rand((rows, cols, 2), dtype=torch.float32, device=dev)
D = torch.tensor(rng.normal(size=(1, n_pts, 3)), device=dev)
H = torch.empty((1, n_pts, 3), dtype=torch.float64, device=dev)
GRAD = torch.empty((n_pts, 3), dtype=torch.float64, device=dev)
STREAM.synchronize()


def timed(fn):
    """ms per call of fn over CALLS back-to-back calls between two events on the context's stream."""
    begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    begin.record(STREAM)
    for _ in range(CALLS):
        fn()
    end.record(STREAM)
    assert ctx.synchronize() == capi.C5_OK
    end.synchronize()
    return begin.elapsed_time(end) / CALLS


variants = {
    "shape_jacobian_fill_device": lambda: ctx.ray_shape_jacobian_device(ROW_PTR, DI, FACES, BARY),
    "shape_jacobian_fill_device_dI_ddz_only": lambda: ctx.ray_shape_jacobian_device(ROW_PTR, DI, None, None),
    "face_gradients_device": lambda: ctx.face_gradients_device(FPTS, DW),
    "vertex_adjoint_device": lambda: ctx.render_vertex_adjoint_device(G, GRAD),
    "vertex_gn_product_device": lambda: ctx.render_vertex_gn_product_device(D, W, H, None, n=1),
}
for fn in variants.values():  # one warm-up round
    fn()
    assert ctx.synchronize() == capi.C5_OK
acc = {k: [] for k in variants}
for _ in range(REPEATS):
    for k, fn in variants.items():
        acc[k].append(timed(fn))
ms = {k: round(statistics.median(v), 4) for k, v in acc.items()}
found = int((FACES >> 4 == 3).sum())
result = {"frame": "c3 2400x1800", "cells": len(cells), "points": n_pts, "segments": nnz, "bytes": nnz * 57, "repeats": REPEATS,
          "calls": CALLS, "ms": ms, "min_max_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in acc.items()},
          "segments_with_both_faces": found,
          "fill_over_vertex_adjoint": round(ms["shape_jacobian_fill_device"] / ms["vertex_adjoint_device"], 3),
          "break_even_cg_iterations": round((ms["shape_jacobian_fill_device"] + ms["face_gradients_device"]) / ms["vertex_gn_product_device"], 3)}
line = json.dumps(result)
print(line)
if "--json" in sys.argv:
    with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
        f.write(line + "\n")

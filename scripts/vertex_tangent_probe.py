"""Vertex tangent render on the C3 frame: c5_render_vertex_tangent_device at K = 1, 3, 8 beside
c5_render_motion_tangent_device at the same K and c5_render_vertex_adjoint_device (which has no batched form: K calls) in
the same process.  Device arrays throughout; host clock around R back-to-back calls ending in a synchronise, the variants
alternated, median of the repeats.  The vertex tangent legs are guarded with hasattr, so the script also runs on a tree
without them (the other two: the baseline).  Prints one JSON line; `--json PATH` writes it too.  `--quick`: fewer repeats
(for a profiler run)."""
import json
import statistics
import sys
import time

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import numpy as np  # noqa: E402
import torch  # noqa: E402

from course5_amd import capi, meshgen as mg  # noqa: E402

quick = "--quick" in sys.argv
REPEATS, CALLS = (2, 2) if quick else (7, 5)
KS = (1, 3, 8)

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
G = torch.tensor(rng.normal(size=(rows, cols, 2)).astype(np.float32), device=dev)
GX = torch.empty((n_pts, 3), dtype=torch.float64, device=dev)
D = torch.tensor(rng.normal(size=(max(KS), n_pts, 3)), device=dev)
FIELDS = rng.normal(size=(max(KS), 12))
OUT = torch.empty((max(KS), rows, cols, 2), dtype=torch.float32, device=dev)
torch.cuda.synchronize()
STREAM = torch.cuda.Stream(dev)  # (not torch's null stream, which the library would take for "its own")
torch.cuda.set_stream(STREAM)
ctx.set_stream(STREAM.cuda_stream)
has_tangent = hasattr(ctx, "render_vertex_tangent_device")


def timed(fn):
    """ms per call of fn over CALLS back-to-back calls ending in a synchronise."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(CALLS):
        fn()
    assert ctx.synchronize() == capi.C5_OK
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / CALLS


def compare(variants):
    """{name: median ms per call}, the variants alternated within every repeat (one warm-up round first)."""
    for fn in variants.values():
        fn()
    assert ctx.synchronize() == capi.C5_OK
    acc = {k: [] for k in variants}
    for _ in range(REPEATS):
        for k, fn in variants.items():
            acc[k].append(timed(fn))
    return {k: round(statistics.median(v), 4) for k, v in acc.items()}


def adjoint_calls(k):
    def run():
        for _ in range(k):
            ctx.render_vertex_adjoint_device(G, GX)
    return run


variants = {}
for k in KS:
    variants[f"vertex_adjoint_x{k}"] = adjoint_calls(k)
    variants[f"motion_tangent_k{k}"] = lambda k=k: ctx.render_motion_tangent_device(FIELDS[:k], OUT[:k])
    if has_tangent:
        variants[f"vertex_tangent_k{k}"] = lambda k=k: ctx.render_vertex_tangent_device(D[:k], OUT[:k])
result = {"frame": "c3 2400x1800", "cells": len(cells), "points": n_pts, "vertex_tangent": has_tangent, "ms": compare(variants)}
if has_tangent:
    ms = result["ms"]
    result["k1_against_vertex_adjoint"] = round(ms["vertex_tangent_k1"] / ms["vertex_adjoint_x1"], 3)
    result["against_motion_tangent"] = {k: round(ms[f"vertex_tangent_k{k}"] / ms[f"motion_tangent_k{k}"], 3) for k in KS}
line = json.dumps(result)
print(line)
if "--json" in sys.argv:
    with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
        f.write(line + "\n")

"""Vertex adjoint render on the C3 frame: c5_render_vertex_adjoint_device against
c5_render_adjoint_device in the same process, and its two forms - every lane adding its own six values ("vertex_merge" 0)
and the lanes of a wavefront in one cell summed in LDS first ("vertex_merge" 1).  Device arrays throughout; host clock
around R back-to-back calls ending in a synchronise, the variants alternated, median of the repeats.  The vertex legs are
guarded with hasattr, so the script also runs on a tree without them (the adjoint: the baseline).  Prints one JSON line;
`--json PATH` writes it too.  `--quick`: fewer repeats (for a profiler run)."""
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

xyz, cells, alpha, q = mg.workload("c3")
alpha = alpha.copy()
alpha[(alpha >= np.finfo(np.float64).eps) & (alpha < 1e-6)] = 1e-6
ctx = capi.Context(0)
ctx.set_option("stage_timing", 0)
ctx.set_option("walk_timing", 0)
ctx.upload_grid(xyz, cells, alpha, q)
ctx.set_image(2400, 1800, mg.REFERENCE_BOUNDS)
ctx.set_view(mg.view_rotations(**mg.BENCH_VIEW))
rows, cols, n = ctx.local_rows, 2400, len(cells)
dev = torch.device("cuda", 0)
G = torch.tensor(np.random.default_rng(1).normal(size=(rows, cols, 2)).astype(np.float32), device=dev)
GA = torch.empty(n, dtype=torch.float64, device=dev)
GQ = torch.empty(n, dtype=torch.float64, device=dev)
GX = torch.empty((len(xyz), 3), dtype=torch.float64, device=dev)
torch.cuda.synchronize()
STREAM = torch.cuda.Stream(dev)  # (not torch's null stream, which the library would take for "its own")
torch.cuda.set_stream(STREAM)
ctx.set_stream(STREAM.cuda_stream)
has_vertex = hasattr(ctx, "render_vertex_adjoint_device")


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
    ctx.synchronize()
    acc = {k: [] for k in variants}
    for _ in range(REPEATS):
        for k, fn in variants.items():
            acc[k].append(timed(fn))
    return {k: round(statistics.median(v), 4) for k, v in acc.items()}


def vertex(merge):
    def run():
        ctx.set_option("vertex_merge", merge)
        ctx.render_vertex_adjoint_device(G, GX)
    return run


variants = {"adjoint": lambda: ctx.render_adjoint_device(G, GA, GQ)}
if has_vertex:
    variants["vertex_adjoint"] = vertex(0)
    variants["vertex_adjoint_merged"] = vertex(1)
result = {"frame": "c3 2400x1800", "cells": n, "points": len(xyz), "vertex": has_vertex, "ms": compare(variants)}
if has_vertex:
    ms = result["ms"]
    result["ratio"] = round(ms["vertex_adjoint"] / ms["adjoint"], 3)
    result["ratio_merged"] = round(ms["vertex_adjoint_merged"] / ms["adjoint"], 3)
    plain = GX.clone()
    vertex(1)()
    assert ctx.synchronize() == capi.C5_OK
    result["merged_vs_plain_max_rel"] = float((GX - plain).abs().max() / plain.abs().max())
line = json.dumps(result)
print(line)
if "--json" in sys.argv:
    with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
        f.write(line + "\n")

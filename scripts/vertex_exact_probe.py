"""Exact vertex adjoint sums on the C3 frame: c5_render_vertex_adjoint_device with "vertex_exact"
0 (fp64 atomics) and 1 (passes 1, E, S and the finish kernels) in one process, alternated; CALLS back-to-back calls between
two HIP events on the context's stream (the method of DESIGN.md section 4.5), median of the repeats.  Also the three staged
calls (bounds: passes 1 and E; sums: passes 1 and S; finish: a per-view setup and the finish kernels), whether two exact
calls give equal bits, and how far the exact result is from the atomic one.  Prints one JSON line; `--json PATH` writes it
too.  `--quick`: one repeat of two calls (for a profiler run).  `--atomic-only`: the option-0 call alone (it needs no
symbol of this feature: the same script times the parent commit's library)."""
import json
import statistics
import sys

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import numpy as np  # noqa: E402
import torch  # noqa: E402

from course5_amd import capi, meshgen as mg  # noqa: E402

quick = "--quick" in sys.argv
atomic_only = "--atomic-only" in sys.argv
REPEATS, CALLS = (1, 2) if quick else (5, 20)

xyz, cells, alpha, q = mg.workload("c3")
alpha = alpha.copy()
alpha[(alpha >= np.finfo(np.float64).eps) & (alpha < 1e-6)] = 1e-6
ctx = capi.Context(0)
ctx.set_option("stage_timing", 0)
ctx.set_option("walk_timing", 0)
ctx.upload_grid(xyz, cells, alpha, q)
ctx.set_image(2400, 1800, mg.REFERENCE_BOUNDS)
ctx.set_view(mg.view_rotations(**mg.BENCH_VIEW))
rows, cols, n, n_pts = ctx.local_rows, 2400, len(cells), len(xyz)
dev = torch.device("cuda", 0)
G = torch.tensor(np.random.default_rng(1).normal(size=(rows, cols, 2)).astype(np.float32), device=dev)
OUT = torch.empty((n_pts, 3), dtype=torch.float64, device=dev)
EXPS = torch.empty((n, 12), dtype=torch.int32, device=dev)
SUMS = torch.empty((n, 12, 2), dtype=torch.int64, device=dev)
torch.cuda.synchronize()
STREAM = torch.cuda.Stream(dev)  # (not torch's null stream, which the library would take for "its own")
torch.cuda.set_stream(STREAM)
ctx.set_stream(STREAM.cuda_stream)


def vertex_adjoint(exact):
    def run():
        if not atomic_only:
            ctx.set_option("vertex_exact", exact)
        ctx.render_vertex_adjoint_device(G, OUT)
    return run


variants = {"vertex_adjoint_atomic": vertex_adjoint(0)}
if not atomic_only:
    variants.update({
        "vertex_adjoint_exact": vertex_adjoint(1),
        "vertex_exact_bounds": lambda: ctx.render_vertex_exact_bounds_device(G, EXPS),
        "vertex_exact_sums": lambda: ctx.render_vertex_exact_sums_device(G, EXPS, SUMS),
        "vertex_exact_finish": lambda: ctx.vertex_exact_finish_device(EXPS, SUMS, OUT),
    })


def timed(fn):
    """ms per call of fn: CALLS back-to-back calls between two events on the stream."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(STREAM)
    for _ in range(CALLS):
        fn()
    t1.record(STREAM)
    assert ctx.synchronize() == capi.C5_OK
    t1.synchronize()
    return t0.elapsed_time(t1) / CALLS


for fn in variants.values():  # one warm-up round (allocations, the entry pool's size)
    fn()
    assert ctx.synchronize() in (capi.C5_OK, capi.C5_RETRY)
acc = {k: [] for k in variants}
for _ in range(REPEATS):
    for k, fn in variants.items():
        acc[k].append(timed(fn))
ms = {k: round(statistics.median(v), 4) for k, v in acc.items()}

result = {"frame": "c3 2400x1800", "cells": n, "points": n_pts, "calls": CALLS, "repeats": REPEATS, "ms": ms}
if not atomic_only:
    vertex_adjoint(0)()
    assert ctx.synchronize() == capi.C5_OK
    atomic = OUT.clone()
    vertex_adjoint(1)()
    assert ctx.synchronize() == capi.C5_OK
    first = OUT.clone()
    vertex_adjoint(1)()
    assert ctx.synchronize() == capi.C5_OK
    result.update({"exact_over_atomic": round(ms["vertex_adjoint_exact"] / ms["vertex_adjoint_atomic"], 3),
                   "exact_calls_equal_bits": bool(torch.equal(first.view(torch.int64), OUT.view(torch.int64))),
                   "max_rel_exact_to_atomic": float((first - atomic).abs().max() / atomic.abs().max())})
line = json.dumps(result)
print(line)
if "--json" in sys.argv:
    with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
        f.write(line + "\n")

"""Exact adjoint sums on the C3 frame: c5_render_adjoint_device with "adjoint_exact" 0 (fp64
atomics) and 1 (passes 1, E, S and the finish) in one process, alternated; CALLS back-to-back calls between two HIP events
on the context's stream (the method of DESIGN.md section 4.5), median of the repeats.  Also the two staged calls
(bounds: passes 1 and E; sums: passes 1 and S), whether two exact calls give equal bits, and how far the exact result is from
the atomic one.  Prints one JSON line; `--json PATH` writes it too.  `--quick`: one repeat of two calls (for a profiler run)."""
import json
import statistics
import sys

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import numpy as np  # noqa: E402
import torch  # noqa: E402

from course5_amd import capi, meshgen as mg  # noqa: E402

quick = "--quick" in sys.argv
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
rows, cols, n = ctx.local_rows, 2400, len(cells)
dev = torch.device("cuda", 0)
G = torch.tensor(np.random.default_rng(1).normal(size=(rows, cols, 2)).astype(np.float32), device=dev)
GA = torch.empty(n, dtype=torch.float64, device=dev)
GQ = torch.empty(n, dtype=torch.float64, device=dev)
EA = torch.empty(n, dtype=torch.int32, device=dev)
EQ = torch.empty(n, dtype=torch.int32, device=dev)
SA = torch.empty((n, 2), dtype=torch.int64, device=dev)
SQ = torch.empty((n, 2), dtype=torch.int64, device=dev)
torch.cuda.synchronize()
STREAM = torch.cuda.Stream(dev)  # (not torch's null stream, which the library would take for "its own")
torch.cuda.set_stream(STREAM)
ctx.set_stream(STREAM.cuda_stream)


def adjoint(exact):
    def run():
        ctx.set_option("adjoint_exact", exact)
        ctx.render_adjoint_device(G, GA, GQ)
    return run


variants = {
    "adjoint_atomic": adjoint(0),
    "adjoint_exact": adjoint(1),
    "exact_bounds": lambda: ctx.render_adjoint_exact_bounds_device(G, EA, EQ),
    "exact_sums": lambda: ctx.render_adjoint_exact_sums_device(G, EA, EQ, SA, SQ),
}


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

adjoint(0)()
assert ctx.synchronize() == capi.C5_OK
atomic = (GA.clone(), GQ.clone())
adjoint(1)()
assert ctx.synchronize() == capi.C5_OK
first = (GA.clone(), GQ.clone())
adjoint(1)()
assert ctx.synchronize() == capi.C5_OK
result = {"frame": "c3 2400x1800", "cells": n, "calls": CALLS, "repeats": REPEATS, "ms": ms,
          "exact_over_atomic": round(ms["adjoint_exact"] / ms["adjoint_atomic"], 3),
          "exact_calls_equal_bits": bool(torch.equal(first[0].view(torch.int64), GA.view(torch.int64))
                                         and torch.equal(first[1].view(torch.int64), GQ.view(torch.int64))),
          "max_rel_exact_to_atomic": [float((a - b).abs().max() / b.abs().max()) for a, b in zip(first, atomic)]}
line = json.dumps(result)
print(line)
if "--json" in sys.argv:
    with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
        f.write(line + "\n")

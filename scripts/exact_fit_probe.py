"""Exact sums of a fit's operators on the C3 frame: c5_render_gn_diagonal_device,
c5_render_gn_product_device (K = 1 and K = 8) and c5_render_hvp_device with "exact_sums" 0 (fp64 atomics) and 1 (pass 1 / A,
pass E, pass S and the finish) in one process, alternated; CALLS back-to-back calls between two HIP events on the context's
stream (the method of DESIGN.md section 4.5), median of the repeats.  Also the two staged calls of the two new kinds
(bounds: passes 1 and E; sums: passes 1 and S), whether two exact calls give equal bits, and how far the exact result is
from the atomic one.  Prints one JSON line; `--json PATH` writes it too.  `--quick`: one repeat of two calls (for a profiler
run).  `--atomic-only`: the four atomic calls alone, nothing that a library without "exact_sums" lacks (the same script
on an older checkout, for the atomic path's before and after)."""
import json
import statistics
import sys

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import numpy as np  # noqa: E402
import torch  # noqa: E402

from course5_amd import capi, meshgen as mg  # noqa: E402

quick, atomic_only = "--quick" in sys.argv, "--atomic-only" in sys.argv
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
rng = np.random.default_rng(1)
G = torch.tensor(rng.normal(size=(rows, cols, 2)).astype(np.float32), device=dev)
W = torch.tensor(np.abs(rng.normal(size=(rows, cols, 2))).astype(np.float32), device=dev)
VA = torch.tensor(rng.normal(size=(8, n)), device=dev)
VQ = torch.tensor(rng.normal(size=(8, n)), device=dev)
VA1, VQ1 = VA[:1].contiguous(), VQ[:1].contiguous()
HA = torch.empty((8, n), dtype=torch.float64, device=dev)
HQ = torch.empty((8, n), dtype=torch.float64, device=dev)
HA1, HQ1 = HA[:1], HQ[:1]
EA = torch.empty(n, dtype=torch.int32, device=dev)
EQ = torch.empty(n, dtype=torch.int32, device=dev)
SA = torch.empty((n, 2), dtype=torch.int64, device=dev)
SQ = torch.empty((n, 2), dtype=torch.int64, device=dev)
torch.cuda.synchronize()
STREAM = torch.cuda.Stream(dev)  # (not torch's null stream, which the library would take for "its own")
torch.cuda.set_stream(STREAM)
ctx.set_stream(STREAM.cuda_stream)

CALLS_OF = {
    "diagonal": lambda: ctx.render_gn_diagonal_device(W, HA[0], HQ[0]),
    "product_k1": lambda: ctx.render_gn_product_device(VA1, VQ1, W, HA1, HQ1, None, n=1),
    "product_k8": lambda: ctx.render_gn_product_device(VA, VQ, W, HA, HQ, None, n=8),
    "hvp": lambda: ctx.render_hvp_device(VA[0], VQ[0], G, HA[0], HQ[0]),
}


def mode(name, exact):
    def run():
        if not atomic_only:
            ctx.set_option("exact_sums", exact)
        CALLS_OF[name]()
    return run


variants = {f"{name}_atomic": mode(name, 0) for name in CALLS_OF}
if not atomic_only:
    DIAG, HVP = capi.C5_EXACT_GN_DIAGONAL, capi.C5_EXACT_HVP
    variants.update({f"{name}_exact": mode(name, 1) for name in CALLS_OF})
    variants.update({
        "diagonal_bounds": lambda: ctx.render_exact_bounds_device(DIAG, EA, EQ, image=W),
        "diagonal_sums": lambda: ctx.render_exact_sums_device(DIAG, EA, EQ, SA, SQ, image=W),
        "hvp_bounds": lambda: ctx.render_exact_bounds_device(HVP, EA, EQ, image=G, d_alpha=VA[0], d_q=VQ[0]),
        "hvp_sums": lambda: ctx.render_exact_sums_device(HVP, EA, EQ, SA, SQ, image=G, d_alpha=VA[0], d_q=VQ[0]),
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
result = {"frame": "c3 2400x1800", "cells": n, "calls": CALLS, "repeats": REPEATS, "atomic_only": atomic_only, "ms": ms,
          "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in acc.items()}}

if not atomic_only:
    def values(name, exact):
        mode(name, exact)()
        assert ctx.synchronize() == capi.C5_OK
        k = 8 if name == "product_k8" else 1
        return HA[:k].clone(), HQ[:k].clone()

    result["exact_over_atomic"], result["exact_calls_equal_bits"], result["max_rel_exact_to_atomic"] = {}, {}, {}
    for name in CALLS_OF:
        atomic, first, second = values(name, 0), values(name, 1), values(name, 1)
        result["exact_over_atomic"][name] = round(ms[f"{name}_exact"] / ms[f"{name}_atomic"], 3)
        result["exact_calls_equal_bits"][name] = all(bool(torch.equal(a.view(torch.int64), b.view(torch.int64))) for a, b in zip(first, second))
        result["max_rel_exact_to_atomic"][name] = [float((a - b).abs().max() / b.abs().max()) for a, b in zip(first, atomic)]
line = json.dumps(result)
print(line)
if "--json" in sys.argv:
    with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
        f.write(line + "\n")

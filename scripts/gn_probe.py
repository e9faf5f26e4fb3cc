"""Gauss-Newton renders on the C3 frame: the fused product c5_render_gn_product_device against the
composition it replaces (render_tangent_batch_device -> a torch multiply on the same stream -> render_adjoint_batch_device)
at K = 1 and K = 8, the diagonal c5_render_gn_diagonal_device against the single adjoint (the same two walks), and
course5_amd.autograd.gn_product per call with the scalars on the GPU.  Device arrays throughout; host clock around R
back-to-back calls ending in a synchronise, the variants alternated, median of the repeats.  The new legs are guarded with
hasattr, so the script also runs on a tree without them (the composition and the adjoint: the baselines).  Prints one JSON
line; `--json PATH` writes it too.  `--quick`: fewer repeats (for a profiler run)."""
import json
import statistics
import sys
import time

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import numpy as np  # noqa: E402
import torch  # noqa: E402

from course5_amd import autograd, capi, meshgen as mg  # noqa: E402

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
rng = np.random.default_rng(1)
KMAX = 8
DA = torch.tensor(alpha * rng.uniform(-0.5, 1.5, (KMAX, n)), device=dev)
DQ = torch.tensor(q * rng.uniform(-0.5, 1.5, (KMAX, n)), device=dev)
W = torch.rand((rows, cols, 2), dtype=torch.float32, device=dev)
T_OUT = torch.empty((KMAX, rows, cols, 2), dtype=torch.float32, device=dev)
HA = torch.empty((KMAX, n), dtype=torch.float64, device=dev)
HQ = torch.empty((KMAX, n), dtype=torch.float64, device=dev)
torch.cuda.synchronize()
STREAM = torch.cuda.Stream(dev)  # (not torch's null stream, which the library would take for "its own")
torch.cuda.set_stream(STREAM)
ctx.set_stream(STREAM.cuda_stream)  # (the multiply of the composition: the same stream as the renders)
has_gn = hasattr(ctx, "render_gn_product_device")


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


def composition(k):
    def run():
        ctx.render_tangent_batch_device(DA[:k], DQ[:k], T_OUT[:k])
        T_OUT[:k].mul_(W)
        ctx.render_adjoint_batch_device(T_OUT[:k], HA[:k], HQ[:k])
    return run


def fused(k):
    return lambda: ctx.render_gn_product_device(DA[:k], DQ[:k], W, HA[:k], HQ[:k])


result = {"frame": "c3 2400x1800", "cells": n, "gn": has_gn}
for k in (1, 8):
    v = {"composition": composition(k)}
    if has_gn:
        v["fused"] = fused(k)
    result[f"product K={k}"] = compare(v)
v = {"adjoint": lambda: ctx.render_adjoint_device(W, HA[0], HQ[0])}
if has_gn:
    v["gn_diagonal"] = lambda: ctx.render_gn_diagonal_device(W, HA[1], HQ[1])
result["diagonal"] = compare(v)
if hasattr(autograd, "gn_product"):
    a_gpu, q_gpu = torch.tensor(alpha, device=dev), torch.tensor(q, device=dev)
    result["autograd"] = compare({
        "gn_product K=1, scalars on the GPU": lambda: autograd.gn_product(ctx, a_gpu, q_gpu, DA[0], DQ[0], W),
        "gn_product K=8, scalars on the GPU": lambda: autograd.gn_product(ctx, a_gpu, q_gpu, DA, DQ, W),
        "gn_diagonal, scalars on the GPU": lambda: autograd.gn_diagonal(ctx, a_gpu, q_gpu, W),
    })
line = json.dumps(result)
print(line)
if "--json" in sys.argv:
    with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
        f.write(line + "\n")

"""Batched derivative renders on the C3 frame: K single tangents / adjoints against one batch of K
(K = 1, 4, 8; at K = 8 both chunk widths), and the forward of course5_amd.autograd.render with the scalars uploaded from
the GPU (c5_update_scalars_device) or through the host, against a plain render_device frame.  Device arrays throughout
(the _device forms); host clock around R back-to-back calls ending in a synchronise, the variants alternated, median of
the repeats.  Prints one JSON line; `--json PATH` writes it too.  `--quick`: fewer repeats (for a profiler run)."""
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
G = torch.rand((KMAX, rows, cols, 2), dtype=torch.float32, device=dev)
T_OUT = torch.empty((KMAX, rows, cols, 2), dtype=torch.float32, device=dev)
GA = torch.empty((KMAX, n), dtype=torch.float64, device=dev)
GQ = torch.empty((KMAX, n), dtype=torch.float64, device=dev)
IMG = torch.empty((rows, cols, 2), dtype=torch.float32, device=dev)


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


def singles_tangent(k):
    return lambda: [ctx.render_tangent_device(DA[j], DQ[j], T_OUT[j]) for j in range(k)]


def batch_tangent(k):
    return lambda: ctx.render_tangent_batch_device(DA[:k], DQ[:k], T_OUT[:k])


def singles_adjoint(k):
    return lambda: [ctx.render_adjoint_device(G[j], GA[j], GQ[j]) for j in range(k)]


def batch_adjoint(k):
    return lambda: ctx.render_adjoint_batch_device(G[:k], GA[:k], GQ[:k])


result = {"frame": "c3 2400x1800", "cells": n}
for kind, single, batch in (("tangent", singles_tangent, batch_tangent), ("adjoint", singles_adjoint, batch_adjoint)):
    for k in (1, 4, 8):
        v = {f"{k} singles": single(k), f"batch of {k}": batch(k)}
        if k == 8:
            v["batch of 8, width 4"] = lambda b=batch(8): (ctx.set_option("batch_width", 4), b(), ctx.set_option("batch_width", 0))
        result[f"{kind} K={k}"] = compare(v)

# the forward of autograd.render: scalars from the GPU, through the host, and a plain frame with the scalars in place
a_gpu, q_gpu = torch.tensor(alpha, device=dev), torch.tensor(q, device=dev)
a_cpu, q_cpu = torch.tensor(alpha), torch.tensor(q)
with torch.no_grad():
    result["forward"] = compare({
        "render_device": lambda: ctx.render_device(IMG.data_ptr()),
        "autograd.render, scalars on the GPU": lambda: autograd.render(ctx, a_gpu, q_gpu),
        "autograd.render, scalars on the host": lambda: autograd.render(ctx, a_cpu, q_cpu),
    })
line = json.dumps(result)
print(line)
if "--json" in sys.argv:
    with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
        f.write(line + "\n")

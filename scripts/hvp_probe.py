"""The Hessian-vector render on the C3 frame: c5_render_hvp_device against c5_render_adjoint_device
and c5_render_tangent_device in one process, the variants alternated.  The call replaces a central difference of two
adjoints, so the aim is below 2 single adjoints; the expectation from the code is one adjoint plus a tangent's extra work
per step.  Device arrays throughout (the _device forms); host clock around R back-to-back calls ending in a synchronise,
median of the repeats, as scripts/batch_probe.py.  Prints one JSON line; `--json PATH` writes it too.  `--quick`: fewer
repeats (for a profiler run: rocprofv3 --kernel-trace --stats -- python scripts/hvp_probe.py --quick)."""
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
rng = np.random.default_rng(1)
DA = torch.tensor(alpha * rng.uniform(-0.5, 1.5, n), device=dev)
DQ = torch.tensor(q * rng.uniform(-0.5, 1.5, n), device=dev)
G = torch.rand((rows, cols, 2), dtype=torch.float32, device=dev)
T_OUT = torch.empty((rows, cols, 2), dtype=torch.float32, device=dev)
HA = torch.empty(n, dtype=torch.float64, device=dev)
HQ = torch.empty(n, dtype=torch.float64, device=dev)


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


ms = compare({
    "adjoint": lambda: ctx.render_adjoint_device(G, HA, HQ),
    "tangent": lambda: ctx.render_tangent_device(DA, DQ, T_OUT),
    "hvp": lambda: ctx.render_hvp_device(DA, DQ, G, HA, HQ),
    "hvp, d_alpha only, h_alpha only": lambda: ctx.render_hvp_device(DA, None, G, HA, None),
})
result = {"frame": "c3 2400x1800", "cells": n, "ms": ms, "hvp / adjoint": round(ms["hvp"] / ms["adjoint"], 3),
          "below 2 adjoints": bool(ms["hvp"] < 2.0 * ms["adjoint"])}
line = json.dumps(result)
print(line)
if "--json" in sys.argv:
    with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
        f.write(line + "\n")

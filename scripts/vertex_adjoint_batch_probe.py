"""Batched vertex adjoint render on the C3 frame: c5_render_vertex_adjoint_batch_device at K = 1,
3 and 8 - at "batch_width" 4 and 8 where the two differ - beside K looped c5_render_vertex_adjoint_device calls in the same
process.  The single call's kernels are the ones the batch was added beside, so the looped leg is also the figure of the
tree before the batch.  Device arrays throughout; R calls back to back between two HIP events on the context's stream,
the variants alternated within every repeat after one warm-up round, median of 7 repeats.  Before the timing every slice
of a K = 8 batch is compared with its single call (rtol 1e-12, atol 1e-15 x max).  Prints one JSON line; `--json PATH`
writes it too.  `--quick`: fewer repeats, and `--ks 8`: that batch size alone (for a profiler run, so that a kernel's mean is
that of one batch size: `rocprofv3 --kernel-trace --stats -- python <this> --quick --ks 8`)."""
import json
import statistics
import sys

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import numpy as np  # noqa: E402
import torch  # noqa: E402

from course5_amd import capi, meshgen as mg  # noqa: E402

quick = "--quick" in sys.argv
REPEATS, CALLS = (2, 2) if quick else (7, 5)
KS = tuple(int(k) for k in sys.argv[sys.argv.index("--ks") + 1].split(",")) if "--ks" in sys.argv else (1, 3, 8)

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
G = torch.tensor(rng.normal(size=(max(KS), rows, cols, 2)).astype(np.float32), device=dev)
GX = torch.empty((max(KS), n_pts, 3), dtype=torch.float64, device=dev)
torch.cuda.synchronize()
STREAM = torch.cuda.Stream(dev)  # (not torch's null stream, which the library would take for "its own")
torch.cuda.set_stream(STREAM)
ctx.set_stream(STREAM.cuda_stream)


def looped(k):
    def run():
        for j in range(k):
            ctx.render_vertex_adjoint_device(G[j], GX[j])
    return run


WIDTH = [0]


def batched(k, width):
    def run():
        if WIDTH[0] != width:
            ctx.set_option("batch_width", width)
            WIDTH[0] = width
        ctx.render_vertex_adjoint_batch_device(G[:k], GX[:k], n=k)
    return run


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


def compare(variants):
    """{name: median ms per call}, the variants alternated within every repeat (one warm-up round first)."""
    for fn in variants.values():
        fn()
    assert ctx.synchronize() == capi.C5_OK
    acc = {k: [] for k in variants}
    for _ in range(REPEATS):
        for k, fn in variants.items():
            acc[k].append(timed(fn))
    return ({k: round(statistics.median(v), 4) for k, v in acc.items()},
            {k: [round(min(v), 4), round(max(v), 4)] for k, v in acc.items()})


# the same results first: every slice of the widest batch against its single call
looped(max(KS))()
assert ctx.synchronize() == capi.C5_OK
singles = GX.cpu().numpy().copy()
worst = {}
for width in (4, 8):
    GX.fill_(float("nan"))
    batched(max(KS), width)()
    assert ctx.synchronize() == capi.C5_OK
    got = GX.cpu().numpy()
    for j in range(max(KS)):
        np.testing.assert_allclose(got[j], singles[j], rtol=1e-12, atol=1e-15 * np.abs(singles[j]).max())
    worst[f"w{width}"] = float(np.abs(got - singles).max() / np.abs(singles).max())

variants = {}
for k in KS:
    variants[f"single_x{k}"] = looped(k)
    variants[f"batch_k{k}_w4"] = batched(k, 4)
    if k > 1:  # (a batch of one is the single call at either width)
        variants[f"batch_k{k}_w8"] = batched(k, 8)
ms, spread = compare(variants)
result = {"frame": "c3 2400x1800", "cells": len(cells), "points": n_pts, "repeats": REPEATS, "calls": CALLS, "ms": ms,
          "min_max_ms": spread, "worst_difference_over_max": worst,
          "against_looped": {f"k{k}_w{w}": round(ms[f"batch_k{k}_w{w}"] / ms[f"single_x{k}"], 3)
                             for k in KS for w in (4, 8) if f"batch_k{k}_w{w}" in ms}}
if 1 in KS:  # (the n == 1 path IS the single call)
    result["k1_against_single"] = round(ms["batch_k1_w4"] / ms["single_x1"], 3)
line = json.dumps(result)
print(line)
if "--json" in sys.argv:
    with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
        f.write(line + "\n")

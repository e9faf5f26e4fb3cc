"""Vertex Gauss-Newton product on the C3 frame: the fused c5_render_vertex_gn_product_device
against the composition it replaces - render_vertex_tangent_device -> a torch multiply on the same stream ->
render_vertex_adjoint_device (K = 1) or render_vertex_adjoint_batch_device (K = 8) - the two alternated within every repeat
after one warm-up round, median of 7 repeats.  Device arrays throughout; R calls back to back between two HIP events on the
context's stream.  The fused leg is guarded with hasattr, so the script also runs on a tree without it and gives the
composition's figure there.  Before the timing the fused result is compared with the composition's (1e-9 x max per
field; jv_out bit for bit).  Prints one JSON line; `--json PATH` writes it too.  `--quick`: fewer repeats, and `--ks 8`:
that size alone (for a profiler run, so that a kernel's mean is that of one size:
`rocprofv3 --kernel-trace --stats -- python <this> --quick --ks 8`)."""
import json
import statistics
import sys

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import numpy as np  # noqa: E402
import torch  # noqa: E402

from course5_amd import capi, meshgen as mg  # noqa: E402

quick = "--quick" in sys.argv
REPEATS, CALLS = (2, 2) if quick else (7, 5)
KS = tuple(int(k) for k in sys.argv[sys.argv.index("--ks") + 1].split(",")) if "--ks" in sys.argv else (1, 8)
KMAX = max(KS)

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
D = torch.tensor(rng.normal(size=(KMAX, n_pts, 3)), device=dev)
W = torch.rand((rows, cols, 2), dtype=torch.float32, device=dev)
T_OUT = torch.empty((KMAX, rows, cols, 2), dtype=torch.float32, device=dev)
H = torch.empty((KMAX, n_pts, 3), dtype=torch.float64, device=dev)
torch.cuda.synchronize()
STREAM = torch.cuda.Stream(dev)  # (not torch's null stream, which the library would take for "its own")
torch.cuda.set_stream(STREAM)
ctx.set_stream(STREAM.cuda_stream)  # (the multiply of the composition: the same stream as the renders)
has_fused = hasattr(ctx, "render_vertex_gn_product_device")


def composition(k):
    def run():
        ctx.render_vertex_tangent_device(D[:k], T_OUT[:k], n=k)
        T_OUT[:k].mul_(W)
        if k == 1:
            ctx.render_vertex_adjoint_device(T_OUT[0], H[0])
        else:
            ctx.render_vertex_adjoint_batch_device(T_OUT[:k], H[:k], n=k)
    return run


def fused(k, jv_out=None):
    return lambda: ctx.render_vertex_gn_product_device(D[:k], W, H[:k], jv_out, n=k)


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


result = {"frame": "c3 2400x1800", "cells": len(cells), "points": n_pts, "repeats": REPEATS, "calls": CALLS, "fused": has_fused}
if has_fused:  # the same results first
    worst = {}
    for k in KS:
        composition(k)()
        assert ctx.synchronize() == capi.C5_OK
        want, jv = H[:k].cpu().numpy().copy(), None
        ctx.render_vertex_tangent_device(D[:k], T_OUT[:k], n=k)
        assert ctx.synchronize() == capi.C5_OK
        jv = T_OUT[:k].clone()
        jv_out = torch.full_like(jv, float("nan"))
        H.fill_(float("nan"))
        fused(k, jv_out)()
        assert ctx.synchronize() == capi.C5_OK
        got = H[:k].cpu().numpy()
        assert torch.equal(jv_out.view(torch.int32), jv.view(torch.int32)), f"K = {k}: jv_out is not the tangent render's image"
        rel = max(float(np.abs(got[j] - want[j]).max() / np.abs(want[j]).max()) for j in range(k))
        assert rel <= 1e-9, f"K = {k}: the fused product differs from the composition by {rel:.3g} of the largest component"
        worst[f"k{k}"] = rel
        del jv, jv_out
    result["worst_difference_over_max"] = worst
for k in KS:
    v = {"composition": composition(k)}
    if has_fused:
        v["fused"] = fused(k)
    ms, spread = compare(v)
    result[f"K={k}"] = {"ms": ms, "min_max_ms": spread}
    if has_fused:
        result[f"K={k}"]["saved_ms"] = round(ms["composition"] - ms["fused"], 4)
line = json.dumps(result)
print(line)
if "--json" in sys.argv:
    with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
        f.write(line + "\n")

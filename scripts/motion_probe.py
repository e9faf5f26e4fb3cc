"""Motion tangent render on the C3 frame: c5_render_motion_tangent_device against
c5_render_tangent_batch_device at the same number of directions, K = 3 (the three angles of `course`'s view) and K = 8, and
K = 1 against the single tangent.  Device arrays throughout; host clock around R back-to-back calls ending in a synchronise,
the variants alternated, median of the repeats.  The motion legs are guarded with hasattr, so the script also runs on a
tree without them (the tangent batch: the baseline).  Prints one JSON line; `--json PATH` writes it too.  `--quick`: fewer
repeats (for a profiler run)."""
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
rots = mg.view_rotations(**mg.BENCH_VIEW)
ctx.set_view(rots)
rows, cols, n = ctx.local_rows, 2400, len(cells)
dev = torch.device("cuda", 0)
rng = np.random.default_rng(1)
KMAX = 8
DA = torch.tensor(alpha * rng.uniform(-0.5, 1.5, (KMAX, n)), device=dev)
DQ = torch.tensor(q * rng.uniform(-0.5, 1.5, (KMAX, n)), device=dev)
OUT = torch.empty((KMAX, rows, cols, 2), dtype=torch.float32, device=dev)
torch.cuda.synchronize()
STREAM = torch.cuda.Stream(dev)  # (not torch's null stream, which the library would take for "its own")
torch.cuda.set_stream(STREAM)
ctx.set_stream(STREAM.cuda_stream)
has_motion = hasattr(ctx, "render_motion_tangent_device")
if has_motion:
    FIELDS = np.vstack([[capi.rotation_motion(rots, i) for i in range(3)], rng.normal(size=(KMAX - 3, 12))])


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


result = {"frame": "c3 2400x1800", "cells": n, "motion": has_motion}
for k in (1, 3, 8):
    v = {"tangent_batch": (lambda k=k: ctx.render_tangent_batch_device(DA[:k], DQ[:k], OUT[:k]))}
    if has_motion:
        v["motion_tangent"] = (lambda k=k: ctx.render_motion_tangent_device(FIELDS[:k], OUT[:k]))
    r = compare(v)
    if has_motion:
        r["ratio"] = round(r["motion_tangent"] / r["tangent_batch"], 3)
    result[f"K={k}"] = r
line = json.dumps(result)
print(line)
if "--json" in sys.argv:
    with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
        f.write(line + "\n")

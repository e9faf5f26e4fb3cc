"""The shape prior on the C3 grid: what its operators cost beside a CG iteration of a shape fit.

Measured with HIP events on the context's stream (a torch stream the context is set to), 30 warm calls and then 100 timed
ones, one event pair per call: best and median; and once more back to back between one pair of events.  Reported: the rest
shape's build (host clock: it ends in a wait), every operator under both energies, quality, the bytes the formula below
counts and the rate they give, the same product composed in torch on the same GPU and stream (batched F from gathered
points, the energy summed, the product as autograd's double backward), and fit.shape_step(iters=10) on the C3 frame
without and with the prior - and, where --parent-lib names a library built from the parent commit, the same step without
the prior on that library in a child process of the same session.

Bytes per operator, gathers counted once per cell (in Morton order they mostly hit cache): the cell launch reads 16 (point
ids) + 72 (B) + 8 (V0) + 96 per point set it gathers (the point, the direction) and writes 96 (shares); the point launch
reads the 96 of shares again and 16 of incidence entries per cell, and per point 4 of offsets, and writes 24 per point.

    python scripts/shape_prior_probe.py [--out profiles/shape_prior.md] [--parent-lib PATH] [--quick]"""
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import numpy as np  # noqa: E402
import torch  # noqa: E402

from course5_amd import capi, fit, meshgen as mg  # noqa: E402
from course5_amd import build as c5build  # noqa: E402

quick = "--quick" in sys.argv
step_only = "--step-only" in sys.argv
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else "profiles/shape_prior.md"
PARENT = sys.argv[sys.argv.index("--parent-lib") + 1] if "--parent-lib" in sys.argv else None
WARM, CALLS = (3, 10) if quick else (30, 100)

if step_only:  # (a library from before the shape prior has none of its symbols: the binding is not asked for them)
    for name in [k for k in capi.SIGNATURES if k.startswith("c5_shape_prior")]:
        del capi.SIGNATURES[name]

xyz, cells, alpha, q = mg.workload("c3" if not quick else "c2")
n, n_pts = len(cells), len(xyz)
dev = torch.device("cuda", 0)
STREAM = torch.cuda.Stream(dev)  # (not torch's null stream, which the library would take for "its own")
torch.cuda.set_stream(STREAM)

ctx = capi.Context(0)
ctx.set_option("stage_timing", 0)
ctx.set_option("walk_timing", 0)
ctx.upload_grid(xyz, cells, alpha, q)
ctx.set_stream(STREAM.cuda_stream)


def shape_steps(with_prior: bool):
    """{label: (median ms, iterations done)} of fit.shape_step(iters=10) on the C3 frame."""
    ctx.set_image(2400, 1800, mg.REFERENCE_BOUNDS)
    ctx.set_view(mg.view_rotations(**mg.BENCH_VIEW))
    residual = torch.rand((ctx.local_rows, 2400, 2), dtype=torch.float32, device=dev) - 0.5
    a, b = torch.tensor(alpha, device=dev), torch.tensor(q, device=dev)
    ways = [("without a prior", ctx)]
    if with_prior:
        ways.append(("with a Neo-Hookean prior", fit.WithShapePrior(ctx, fit.ShapePrior(ctx, 1e-3))))
        ways.append(("with a Dirichlet prior", fit.WithShapePrior(ctx, fit.ShapePrior(ctx, 1e-3, energy="dirichlet", rest=False))))
    out = {}
    for label, obj in ways:
        fit.shape_step(obj, a, b, residual, iters=2)
        ms = []
        for _ in range(1 if quick else 3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _d, models = fit.shape_step(obj, a, b, residual, iters=10)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        out[label] = (statistics.median(ms), len(models))
    return out


if step_only:  # the child process on another library (C5_LIB): the step without the prior, one JSON line
    print(json.dumps(shape_steps(False)))
    sys.exit(0)


def events(fn):
    """(best, median, back to back) ms of one call of fn."""
    for _ in range(WARM):
        fn()
    STREAM.synchronize()
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(CALLS)]
    for a, b in pairs:
        a.record(STREAM)
        fn()
        b.record(STREAM)
    STREAM.synchronize()
    ms = [a.elapsed_time(b) for a, b in pairs]
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(STREAM)
    for _ in range(CALLS):
        fn()
    b.record(STREAM)
    STREAM.synchronize()
    return min(ms), statistics.median(ms), a.elapsed_time(b) / CALLS


def bytes_moved(point_sets, per_point=True):
    cell = 16 + 72 + 8 + 96 * point_sets
    if not per_point:
        return n * (cell + 8)  # quality: the ratio out
    return n * (cell + 96 + 96 + 16) + n_pts * (4 + 24)


rows = []  # (what, best ms, median ms, back to back, bytes or None)
build_ms = []
for _ in range(2 if quick else 5):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n_degenerate = ctx.shape_prior_rest_device(None)
    build_ms.append((time.perf_counter() - t0) * 1e3)
rows.append(("rest shape (the context's points; host clock, ends in a wait)", min(build_ms), statistics.median(build_ms), None, None))

rng = np.random.default_rng(1)
X = torch.tensor(xyz, device=dev)
h = (xyz.max(0) - xyz.min(0)).max() / round(n / 6) ** (1 / 3)
XD = (X + 0.05 * h * torch.sin(7.0 * X.flip(1))).contiguous()  # a smooth displacement of 5 % of the cell size
V = torch.tensor(rng.normal(size=(n_pts, 3)), device=dev)
OUTV = torch.empty((n_pts, 3), dtype=torch.float64, device=dev)
VALUE = torch.empty(1, dtype=torch.float64, device=dev)
NINV = torch.zeros(1, dtype=torch.int64, device=dev)
RATIO = torch.empty(n, dtype=torch.float64, device=dev)
ctx.shape_prior_gradient_device(capi.ShapePrior(capi.C5_SHAPE_NEO_HOOKEAN, 1.0, 1.0), XD, VALUE, NINV, OUTV)  # (builds the incidence table)
STREAM.synchronize()
inverted_at_xd = int(NINV.item())

for energy, name in ((capi.C5_SHAPE_DIRICHLET, "Dirichlet"), (capi.C5_SHAPE_NEO_HOOKEAN, "Neo-Hookean")):
    P = capi.ShapePrior(energy, 1.0, 1.0)
    nh = energy == capi.C5_SHAPE_NEO_HOOKEAN
    rows.append((f"gradient + value + count, {name}", *events(lambda: ctx.shape_prior_gradient_device(P, XD, VALUE, NINV, OUTV)), bytes_moved(1)))
    rows.append((f"gradient, {name}", *events(lambda: ctx.shape_prior_gradient_device(P, XD, None, None, OUTV)), bytes_moved(1)))
    rows.append((f"product, {name}", *events(lambda: ctx.shape_prior_product_device(P, XD, V, OUTV)), bytes_moved(2 if nh else 1)))
    rows.append((f"diagonal, {name}", *events(lambda: ctx.shape_prior_diagonal_device(P, XD, OUTV)), bytes_moved(1 if nh else 0)))
rows.append(("quality (ratio and count)", *events(lambda: ctx.shape_prior_quality_device(XD, RATIO, NINV)), bytes_moved(1, per_point=False)))

# the same product composed in torch: batched F from gathered points, the energy, double backward
binv_t = torch.empty((n, 3, 3), dtype=torch.float64, device=dev)
vol_t = torch.empty(n, dtype=torch.float64, device=dev)
vert_t = torch.empty((n, 4), dtype=torch.int32, device=dev)
ctx.shape_prior_rest_data_device(binv_t, vol_t, vert_t)
STREAM.synchronize()
idx = vert_t.to(torch.int64)


def torch_energy(x, energy):
    p = x[idx]  # [n, 4, 3]
    Ds = (p[:, 1:] - p[:, :1]).transpose(1, 2)
    F = Ds @ binv_t
    if energy == capi.C5_SHAPE_DIRICHLET:
        psi = 0.5 * ((F - torch.eye(3, dtype=torch.float64, device=dev)) ** 2).sum(dim=(1, 2))
    else:
        lnJ = torch.log(torch.linalg.det(F))
        psi = 0.5 * ((F ** 2).sum(dim=(1, 2)) - 3.0) - lnJ + 0.5 * lnJ ** 2
    return (vol_t * psi).sum()


def torch_product(energy):
    x = XD.detach().requires_grad_()
    (g,) = torch.autograd.grad(torch_energy(x, energy), x, create_graph=True)
    (hv,) = torch.autograd.grad((g * V).sum(), x)
    return hv


diffs = {}
for energy, name in ((capi.C5_SHAPE_DIRICHLET, "Dirichlet"), (capi.C5_SHAPE_NEO_HOOKEAN, "Neo-Hookean")):
    ctx.shape_prior_product_device(capi.ShapePrior(energy, 1.0, 1.0), XD, V, OUTV)
    STREAM.synchronize()
    diffs[name] = float((torch_product(energy) - OUTV).abs().max() / OUTV.abs().max())
    rows.append((f"product in torch, {name}: gather, batched F, double backward", *events(lambda: torch_product(energy)), None))

steps = shape_steps(True)
parent_steps = None
if PARENT:
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--step-only"] + (["--quick"] if quick else []),
                           env=dict(os.environ, C5_LIB=os.path.abspath(PARENT)), capture_output=True, text=True, timeout=900)
    if child.returncode != 0:
        raise SystemExit(f"the child process on {PARENT} failed ({child.returncode}):\n{child.stdout}\n{child.stderr}")
    parent_steps = json.loads(child.stdout.strip().splitlines()[-1])

lines = ["# Shape prior: what the operators cost (scripts/shape_prior_probe.py)", "",
         f"Grid: {n} cells, {n_pts} points, {n_degenerate} degenerate rest cells; x = rest + a smooth 5 % displacement ({inverted_at_xd} inverted);",
         f"kernel sources {c5build.kernel_source_hash()}.  HIP events on the context's stream around every call, {WARM} warm calls, then {CALLS}",
         "timed.  Bytes: the script's formula (cell launch: ids 16, B 72, V0 8, 96 per gathered point set, shares 96 out; point launch:",
         "shares 96 and incidence 16 per cell, offsets 4 and 24 out per point).", "",
         "| call | best ms | median ms | back to back ms | MB counted | TB/s, back to back |", "|---|---|---|---|---|---|"]
for what, best, med, b2b, nbytes in rows:
    mb = "-" if nbytes is None else f"{nbytes / 1e6:.1f}"
    rate = "-" if nbytes is None or b2b is None else f"{nbytes / (b2b * 1e-3) / 1e12:.2f}"
    lines.append(f"| {what} | {best:.4f} | {med:.4f} | {'-' if b2b is None else format(b2b, '.4f')} | {mb} | {rate} |")
lines += ["", "The torch composition differs from the library's product by " +
          ", ".join(f"{d:.2g} ({name})" for name, d in diffs.items()) + " of the largest element (another order of sums).", "",
          "| fit.shape_step(iters=10), 2400 x 1800 | median ms | iterations done |", "|---|---|---|"]
lines += [f"| {label} | {ms:.1f} | {it} |" for label, (ms, it) in steps.items()]
if parent_steps:
    lines += [f"| {label}, the parent commit's library (child process, same session) | {ms:.1f} | {it} |" for label, (ms, it) in parent_steps.items()]
text = "\n".join(lines) + "\n"
print(text)
with open(OUT, "w") as f:
    f.write(text)

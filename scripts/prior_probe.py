"""The smoothness prior on the C3 grid: what its operators cost beside a CG iteration.

Measured with HIP events on the context's stream (a torch stream the context is set to), 30 warm calls and then 100 timed
ones, one event pair per call: best and median; and once more back to back between one pair of events.  Reported: the
weights' build (host clock: it ends in a wait), gradient (with and without the value), product and diagonal for both penalties, the bytes the formula below counts and the rate
they give, the same product composed in torch (a CSR Laplacian from c5_face_adjacency and the library's weights, torch's
sparse matvec, same GPU and stream), the product with the caller's ids permuted at random (the worst case for the
gathers), and fit.gn_step(iters=10) with and without a prior.

Bytes per launch over both fields, gathers not counted (in Morton order they mostly hit cache): per cell 16 (adjacency) + 32
(weights) + 4 (permutation), and per field 8 out + 8 per array read at the cell itself (the point, the direction).

    python scripts/prior_probe.py [--out profiles/prior.md] [--quick]"""
import statistics
import sys
import time

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import numpy as np  # noqa: E402
import torch  # noqa: E402

from course5_amd import capi, fit, meshgen as mg  # noqa: E402
from course5_amd import build as c5build  # noqa: E402

quick = "--quick" in sys.argv
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else "profiles/prior.md"
WARM, CALLS = (3, 10) if quick else (30, 100)
BUILD_RECORDS_TBS = "5.1-5.7"  # build_records as a streaming kernel on this frame

xyz, cells, alpha, q = mg.workload("c3" if not quick else "c2")
n = len(cells)
dev = torch.device("cuda", 0)
STREAM = torch.cuda.Stream(dev)  # (not torch's null stream, which the library would take for "its own")
torch.cuda.set_stream(STREAM)


def context(cell_ids):
    ctx = capi.Context(0)
    ctx.set_option("stage_timing", 0)
    ctx.set_option("walk_timing", 0)
    ctx.upload_grid(xyz, cell_ids, alpha, q)
    ctx.set_stream(STREAM.cuda_stream)
    return ctx


def events(fn):
    """(best, median) ms of one call of fn, from an event pair around each of CALLS calls after WARM warm ones."""
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
    # and the calls back to back between ONE pair of events: what a call costs when the host keeps the stream fed
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(STREAM)
    for _ in range(CALLS):
        fn()
    b.record(STREAM)
    STREAM.synchronize()
    return min(ms), statistics.median(ms), a.elapsed_time(b) / CALLS


def bytes_moved(fields, reads_per_field):
    return n * (16 + 32 + 4 + fields * (8 + 8 * reads_per_field))


rng = np.random.default_rng(1)
X, XQ = torch.tensor(alpha, device=dev), torch.tensor(q, device=dev)
V, VQ = (torch.tensor(rng.normal(size=n), device=dev) for _ in range(2))
OA, OQ = (torch.empty(n, dtype=torch.float64, device=dev) for _ in range(2))
VALUE = torch.empty(2, dtype=torch.float64, device=dev)
ctx = context(cells)
rows = []  # (what, best ms, median ms, MB counted or None)

# the weights' build: stale after update_points, rebuilt by the next call that wants them (ends in a wait)
build_ms = []
for _ in range(2 if quick else 5):
    ctx.update_points(xyz)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ctx.prior_weights_device(capi.C5_PRIOR_TPFA, None)
    build_ms.append((time.perf_counter() - t0) * 1e3)
n_interior, n_degenerate = ctx.prior_weights_device(capi.C5_PRIOR_TPFA, None)
rows.append(("weights build (TPFA; host clock, ends in a wait)", min(build_ms), statistics.median(build_ms), None, None))

for penalty, name in ((capi.C5_PRIOR_QUADRATIC, "quadratic"), (capi.C5_PRIOR_PSEUDO_HUBER, "pseudo-Huber")):
    P = capi.Prior(penalty, capi.C5_PRIOR_TPFA, 1.0, 1.0, 0.5, 0.5)
    point = penalty == capi.C5_PRIOR_PSEUDO_HUBER
    rows.append((f"gradient + value, {name}", *events(lambda: ctx.prior_gradient_device(P, X, XQ, VALUE, OA, OQ)), bytes_moved(2, 1)))
    rows.append((f"gradient, {name}", *events(lambda: ctx.prior_gradient_device(P, X, XQ, None, OA, OQ)), bytes_moved(2, 1)))
    rows.append((f"product, {name}", *events(lambda: ctx.prior_product_device(P, X, XQ, V, VQ, OA, OQ)), bytes_moved(2, 2 if point else 1)))
    rows.append((f"diagonal, {name}", *events(lambda: ctx.prior_diagonal_device(P, X, XQ, OA, OQ)), bytes_moved(2, 1 if point else 0)))
P = capi.Prior(capi.C5_PRIOR_QUADRATIC, capi.C5_PRIOR_TPFA, 1.0, 0.0)
rows.append(("product, quadratic, one field", *events(lambda: ctx.prior_product_device(P, None, None, V, None, OA, None)), bytes_moved(1, 1)))

# the same product composed in torch: L = D - W as CSR over the caller's ids, one sparse matvec per field
P2 = capi.Prior(capi.C5_PRIOR_QUADRATIC, capi.C5_PRIOR_TPFA, 1.0, 1.0)
w_lib = torch.empty((n, 4), dtype=torch.float64, device=dev)
ctx.prior_weights_device(capi.C5_PRIOR_TPFA, w_lib)
STREAM.synchronize()
t0 = time.perf_counter()
adj, _nb = capi.face_adjacency(cells, len(xyz))
adj_t = torch.tensor(adj, device=dev, dtype=torch.int64)
has = adj_t >= 0
r_idx = torch.arange(n, device=dev).repeat_interleave(4)[has.reshape(-1)]
c_idx = adj_t.reshape(-1)[has.reshape(-1)]
off = -w_lib.reshape(-1)[has.reshape(-1)]
diag = w_lib.sum(dim=1)
L = torch.sparse_coo_tensor(torch.stack([torch.cat([r_idx, torch.arange(n, device=dev)]), torch.cat([c_idx, torch.arange(n, device=dev)])]),
                            torch.cat([off, diag]), (n, n)).coalesce().to_sparse_csr()
STREAM.synchronize()
csr_build_ms = (time.perf_counter() - t0) * 1e3


def torch_product():
    L @ V
    L @ VQ


ctx.prior_product_device(P2, None, None, V, VQ, OA, OQ)
STREAM.synchronize()
diff = float(((L @ V) - OA).abs().max() / OA.abs().max())
rows.append(("product in torch: two CSR matvecs (float64, int64 indices)", *events(torch_product), None))

# the caller's ids permuted at random: every gather and every store scattered
perm = np.random.default_rng(2).permutation(n)
shuffled = context(cells[perm])
shuffled.prior_weights_device(capi.C5_PRIOR_TPFA, None)
rows.append(("product, quadratic, caller's ids permuted at random", *events(lambda: shuffled.prior_product_device(P2, None, None, V, VQ, OA, OQ)),
             bytes_moved(2, 1)))
shuffled.close()

# a Gauss-Newton step with and without the prior
ctx.set_image(2400, 1800, mg.REFERENCE_BOUNDS)
ctx.set_view(mg.view_rotations(**mg.BENCH_VIEW))
residual = torch.rand((ctx.local_rows, 2400, 2), dtype=torch.float32, device=dev) - 0.5
prior = fit.SmoothnessPrior(ctx, lambda_q=1e-3)
steps = {}
for label, kw in (("without a prior", {}), ("with a quadratic TPFA prior on q", {"prior": prior})):
    fit.gn_step(ctx, X, XQ, residual, fit=("q",), iters=2, **kw)
    ms = []
    for _ in range(1 if quick else 3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _d, models = fit.gn_step(ctx, X, XQ, residual, fit=("q",), iters=10, **kw)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    steps[label] = (statistics.median(ms), len(models))

lines = ["# Smoothness prior: what the operators cost (scripts/prior_probe.py)", "",
         f"Grid: {n} cells, {n_interior} interior faces, {n_degenerate} degenerate; kernel sources {c5build.kernel_source_hash()}.",
         f"HIP events on the context's stream around every call, {WARM} warm calls, then {CALLS} timed.  Bytes: the script's formula",
         "(adjacency 16, weights 32, permutation 4 per cell; per field 8 out and 8 per array read at the cell; gathers not counted).",
         f"For scale: build_records streams at {BUILD_RECORDS_TBS} TB/s on this GPU, and one gn_product of a CG iteration takes 5.8 ms.", "",
         "| call | best ms | median ms | back to back ms | MB counted | TB/s, back to back |", "|---|---|---|---|---|---|"]
for what, best, med, b2b, nbytes in rows:
    mb = "-" if nbytes is None else f"{nbytes / 1e6:.1f}"
    rate = "-" if nbytes is None or b2b is None else f"{nbytes / (b2b * 1e-3) / 1e12:.2f}"
    lines.append(f"| {what} | {best:.4f} | {med:.4f} | {'-' if b2b is None else format(b2b, '.4f')} | {mb} | {rate} |")
lines += ["", f"The torch composition needs its matrix first: {csr_build_ms:.1f} ms for c5_face_adjacency on the host and the CSR on the GPU (once per",
          f"grid and set of weights); its product differs from the library's by {diff:.2g} of the largest element (another order of sums).", "",
          "| fit.gn_step(iters=10, fit=(\"q\",)), 2400 x 1800 | median ms | iterations done |", "|---|---|---|"]
lines += [f"| {label} | {ms:.1f} | {it} |" for label, (ms, it) in steps.items()]
text = "\n".join(lines) + "\n"
print(text)
with open(OUT, "w") as f:
    f.write(text)

// ------------------------------------------------------------------------------------------
// Derivative renders (scalar_derivative_kernels.hip, geometry_derivative_kernels.hip, ray_matrix_kernels.hip): the frame
// c5_render would produce now, differentiated.  All share one per-view setup on the context's stream into slot 0's buffers -
// records of "integration" 0 (the reference's order, whatever the option says), whole rays (no "depth_split"), the entry
// lists, the solid mask; or bin_sort_resolve's lists - then run their own kernels.  They leave the options alone and the
// frames' statistics and failure words too (counters and sticky words of their own); the slot's per-view data are marked
// stale, so the next frame builds its own ("view_cache").
// ------------------------------------------------------------------------------------------
#include "context.hpp"
#include "exact_sum.hpp"

using namespace c5api;

namespace {

struct DerivativeView {
    bool no_cells = false;  // a scene of solids only: nothing was set up (there is no cell to differentiate)
    bool bin_sort = false;  // "algorithm" 1: bin_sort_resolve's lists in ctx->offs64 / ctx->segs; else the walk's in w
    hipStream_t s = nullptr;        // the context's stream: everything of a derivative runs on it
    int64_t n_px = 0, padded = 0;   // pixels of the context's rows; rounded up to the scan's 1024
    const int32_t* perm = nullptr;  // cell_perm on the device (device order -> the caller's), or nullptr: the identity
    const uint32_t* mask = nullptr;  // solid-marked pixels, or nullptr
    c5::WalkParams w{};
    c5::ResolveParams r{};     // (bin_sort) what every *_resolve kernel reads
    c5::MotionGeometry geo{};  // the cells' vertices in view space
};

int setup_derivative(c5_context* ctx, DerivativeView& v) {
    if (nothing_to_render(ctx)) return fail(ctx, C5_ERR_STATE, "plane initializer. empty set of objects to render");  // plane.cpp:269-271
    if (!ctx->have_image) return fail(ctx, C5_ERR_STATE, "critical error. empty plane");  // plane.cpp:151-153
    int rc = bind_device(ctx);
    if (rc) return rc;
    FrameSlot& fs = ctx->slots[0];
    hipStream_t s = v.s = ctx->stream;
    const c5::ImageParams& im = ctx->im;
    v.n_px = local_pixels(im);
    const int64_t padded = v.padded = padded_pixels(im);
    if (ctx->n_cells <= 0) {  // (solids only: no cell to differentiate)
        v.no_cells = true;
        return C5_OK;
    }
    if (c5::segment_bytes() != c5::adjoint_segment_bytes())
        return fail(ctx, C5_ERR_STATE, "bin_sort_resolve's segment layout differs from the adjoint's");
    // everything below runs on the context's stream: frames set up on the others ("pipeline", "overlap_setup") must be done
    if (ctx->pipeline || ctx->overlap_setup) {
        rc = drain(ctx);
        if (rc) return rc;
    }

    C5_HIP(ctx, ctx->adj_counters.ensure(kCountersBytes));
    C5_HIP(ctx, ctx->adj_sticky.ensure(kStickyWords * sizeof(unsigned)));
    if (!ctx->adj_status) {
        C5_HIP(ctx, hipHostMalloc(reinterpret_cast<void**>(&ctx->adj_status), 5 * sizeof(unsigned), hipHostMallocDefault));
        ctx->adj_status[3] = 0;  // (rows a ray matrix fill found changed: written by that call alone, cleared by finish_adjoint)
        ctx->adj_status[4] = 0;  // (contributions an exact sum found beyond their cell's exponent: the same)
    }
    rc = ensure_device_perm(ctx);
    if (rc) return rc;
    v.perm = ctx->cell_perm.empty() ? nullptr : ctx->adj_perm.as<int32_t>();
    c5::FrameCounters* const counters = ctx->adj_counters.as<c5::FrameCounters>();
    C5_HIP(ctx, hipMemsetAsync(ctx->adj_sticky.ptr, 0, kStickyWords * sizeof(unsigned), s));

    const c5::GridView g = grid_view(ctx, fs);
    v.geo = c5::MotionGeometry{g.cell_vert, g.vx, g.vy, g.vz};
    // the slot's per-view data are about to hold the derivative's: no frame may take them for its own
    fs.setup_epoch = 0;
    fs.setup_kept = false;
    fs.flags_valid = false;

    c5::launch_transform_soa(s, g.px, g.py, g.pz, g.vx, g.vy, g.vz, g.n_pts, ctx->view, counters);
    c5::SolidTable table{};
    bool any_solid = false;
    v.bin_sort = uses_bin_sort(ctx);
    if (v.bin_sort) {
        int64_t total = 0;
        rc = enqueue_bin_lists(ctx, fs, g, s, counters, total);
        if (rc) return rc;
        rc = enqueue_solids(ctx, fs, 0, s, table, any_solid);
        if (rc) return rc;
        v.mask = any_solid ? fs.mask.as<uint32_t>() : nullptr;
        v.r = c5::ResolveParams{g, im, ctx->xtab.as<double>(), ctx->ytab.as<double>(), ctx->offs64.as<int64_t>(), ctx->segs.ptr,
                                v.mask, ctx->alpha_limit};
    } else {
        const double key_slack = entry_key_slack(ctx);
        c5::launch_build_records(s, g, ctx->alpha_limit, 0);
        if (!fs.head_clean) C5_HIP(ctx, hipMemsetAsync(fs.head.ptr, 0, static_cast<size_t>(padded) * sizeof(c5::EntryHead), s));
        fs.head_clean = false;
        c5::launch_entry_lists(s, g, ctx->xtab.as<double>(), ctx->ytab.as<double>(), im, fs.head.as<c5::EntryHead>(),
                               fs.first.as<c5::Entry>(), fs.pool.as<c5::Entry>(), fs.entry_capacity, counters,
                               ctx->adj_sticky.as<unsigned>(), 0, key_slack);
        rc = enqueue_solids(ctx, fs, 0, s, table, any_solid);
        if (rc) return rc;
        v.mask = any_solid ? fs.mask.as<uint32_t>() : nullptr;
        c5::WalkParams& wp = v.w;
        wp.xrec = g.xrec;
        wp.entry_head = fs.head.as<c5::EntryHead>();
        wp.entry_first = fs.first.as<c5::Entry>();
        wp.entry_pool = fs.pool.as<c5::Entry>();
        wp.pool_capacity = fs.entry_capacity;
        wp.key_slack = key_slack > 0.0 ? key_slack : 0.0;
        wp.mask = v.mask;
        wp.solids = table;
        wp.Xtab = ctx->xtab.as<double>();
        wp.Ytab = ctx->ytab.as<double>();
        wp.im = im;
        wp.max_steps = static_cast<uint32_t>(ctx->n_cells + 64);
        wp.counters = counters;
        wp.sticky = ctx->adj_sticky.as<unsigned>();
    }
    return C5_OK;
}

// After a derivative's kernels: its status words to the host for finish_adjoint, at the next wait.
int commit_derivative(c5_context* ctx, const char* what) {
    FrameSlot& fs = ctx->slots[0];
    hipStream_t s = ctx->stream;
    C5_HIP(ctx, hipGetLastError());
    C5_HIP(ctx, hipMemcpyAsync(ctx->adj_status, &ctx->adj_counters.as<c5::FrameCounters>()->walk_overflow,
                               kStatusWords * sizeof(unsigned), hipMemcpyDeviceToHost, s));
    if (ctx->pipeline) {  // (the next frame's setup on the auxiliary stream waits for slot 0's buffers)
        C5_HIP(ctx, hipEventRecord(fs.walk_done, s));
        fs.walk_recorded = true;
    }
    ctx->adjoint_pending = true;
    ctx->adj_what = what;
    return C5_OK;
}

// The adjoint's parameters over the view's walk, with Lambda's buffer (pass 1 -> pass 2); the weights and where the sums
// go are the caller's to fill in.
int adjoint_params(c5_context* ctx, const DerivativeView& v, c5::AdjointParams& ap) {
    C5_HIP(ctx, ctx->adj_lambda.ensure(static_cast<size_t>(v.padded) * sizeof(double)));
    ap = c5::AdjointParams{};
    ap.w = v.w;
    ap.lambda = ctx->adj_lambda.as<double>();
    return C5_OK;
}

// One adjoint over the view: the per-cell sums zeroed, two passes of the walk (or the resolve over bin_sort_resolve's
// lists), and the permutation into the caller's order.  squared: the Gauss-Newton diagonal's kernels, `weights` may
// then be null (ones).
int adjoint_one(c5_context* ctx, const DerivativeView& v, bool squared, const float2* weights, double* ga_out, double* gq_out) {
    const size_t n_cells = static_cast<size_t>(ctx->n_cells);
    C5_HIP(ctx, ctx->adj_grad.ensure(2 * n_cells * sizeof(double)));
    double* const ga_dev = ctx->adj_grad.as<double>();
    double* const gq_dev = ga_dev + n_cells;
    C5_HIP(ctx, hipMemsetAsync(ga_dev, 0, 2 * n_cells * sizeof(double), v.s));
    if (v.bin_sort) {
        const auto resolve = squared ? c5::launch_gn_diag_resolve : c5::launch_adjoint_resolve;
        resolve(v.s, v.r, weights, ga_dev, gq_dev);
    } else {
        c5::AdjointParams ap;
        int rc = adjoint_params(ctx, v, ap);
        if (rc) return rc;
        ap.grad_out = weights;
        ap.grad_a = ga_dev;
        ap.grad_q = gq_dev;
        c5::launch_adjoint_walk(v.s, ap, 1);
        if (squared) c5::launch_gn_diag_walk(v.s, ap);
        else c5::launch_adjoint_walk(v.s, ap, 2);
        ctx->slots[0].head_clean = true;  // (the second pass hands every head back cleared)
    }
    c5::launch_adjoint_permute(v.s, ga_dev, gq_dev, v.perm, ctx->n_cells, ga_out, gq_out);
    return C5_OK;
}

// The exact sums' word width m for an image of res_x x res_y pixels (exact_sum.hpp), refused where it leaves too few bits.
// ctx may be null (the pure host functions).
int exact_word_bits(c5_context* ctx, int res_x, int res_y, int& m) {
    m = c5::exact::word_bits(static_cast<int64_t>(res_x) * res_y);
    if (m < c5::exact::kMinWordBits)
        return fail(ctx, C5_ERR_INVALID, "exact sums: an image of %d x %d pixels leaves %d bits per word", res_x, res_y, m);
    return C5_OK;
}

// The exact sums' buffer over the context's cells - 40 bytes per cell and the misfit word, allocated here at the first
// exact call - with the word width of the WHOLE image (c5_set_image): the same for every rank of a split.
int exact_sums(c5_context* ctx, c5::ExactSums& x) {
    const size_t n_cells = static_cast<size_t>(ctx->n_cells);
    int m;
    if (const int rc = exact_word_bits(ctx, ctx->im.res_x, ctx->im.res_y, m)) return rc;
    C5_HIP(ctx, ctx->adj_exact.ensure(n_cells * 40 + 8));
    x = c5::ExactSums{};
    x.words = ctx->adj_exact.as<long long>();
    x.exps = reinterpret_cast<int2*>(x.words + 4 * n_cells);
    x.misfits = reinterpret_cast<unsigned*>(x.exps + n_cells);
    x.word_bits = m;
    return C5_OK;
}

// The exact passes over the view for one upstream image: pass 1 (unless Lambda is there: `have_lambda`, a batch's later
// images), pass E into x.exps (`bounds`: cleared here first) and pass S against x.exps into x.words (`sums`: cleared here
// first, the misfit word with them where `first`) - the walk's, or the resolve's over bin_sort_resolve's lists.  keep: the
// walk's pass S leaves the entry heads in place (another image follows); without pass S they stay in place anyway, and the
// next per-view setup clears them.  squared: the Gauss-Newton diagonal's kernels, `weights` may then be null (ones).
int exact_passes(c5_context* ctx, const DerivativeView& v, c5::ExactSums x, const float2* weights, bool bounds, bool sums,
                 bool have_lambda, bool keep, bool first, bool squared = false) {
    c5::launch_exact_clear(v.s, x, ctx->n_cells, bounds, sums, sums && first);
    const auto walk = squared ? c5::launch_gn_diag_exact_walk : c5::launch_adjoint_exact_walk;
    if (v.bin_sort) {
        const auto resolve = squared ? c5::launch_gn_diag_exact_resolve : c5::launch_adjoint_exact_resolve;
        if (bounds) resolve(v.s, v.r, weights, x, false);
        if (sums) resolve(v.s, v.r, weights, x, true);
        return C5_OK;
    }
    c5::AdjointParams ap;
    int rc = adjoint_params(ctx, v, ap);
    if (rc) return rc;
    ap.grad_out = weights;
    if (!have_lambda) c5::launch_adjoint_walk(v.s, ap, 1);
    if (bounds) walk(v.s, ap, x, false);
    x.keep_entries = keep ? 1 : 0;
    if (sums) {
        walk(v.s, ap, x, true);
        if (!keep) ctx->slots[0].head_clean = true;  // (pass S hands every head back cleared)
    }
    return C5_OK;
}

// commit_derivative for a call that ran pass S: the misfit word (on the device: the scalar sums' or the vertex sums')
// travels to the host behind the status words
int commit_exact(c5_context* ctx, const unsigned* misfits, const char* what) {
    int rc = commit_derivative(ctx, what);
    if (rc) return rc;
    C5_HIP(ctx, hipMemcpyAsync(ctx->adj_status + 4, misfits, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    return C5_OK;
}

// "adjoint_exact" 1: n upstream images -> ga_out / gq_out [n][n_cells], every image through passes E and S and the
// finish, one after the other (the host loop "algorithm" 1 uses for its batches); pass 1 runs once for all of them.
int exact_images(c5_context* ctx, const DerivativeView& v, int n, const float2* grad_out, double* ga_out, double* gq_out, const char* what) {
    c5::ExactSums x;
    int rc = exact_sums(ctx, x);
    const int64_t n_cells = ctx->n_cells;
    for (int j = 0; j < n && !rc; ++j) {
        rc = exact_passes(ctx, v, x, grad_out + j * v.n_px, true, true, j > 0, j + 1 < n, j == 0);
        if (!rc) c5::launch_exact_finish(v.s, x, v.perm, n_cells, ga_out + j * n_cells, gq_out + j * n_cells);
    }
    return rc ? rc : commit_exact(ctx, x.misfits, what);
}

// The Hessian-vector render's parameters: the direction into device order (the tangent's buffer: the gather is launched
// here) and, over the view's walk, Lambda's and Lambda_dot's buffers (pass 1 -> pass 2); where the sums go is the caller's
// to fill in.  On bin_sort_resolve's lists hvp_resolve takes hp.dir and hp.grad_out alone.
int hvp_params(c5_context* ctx, const DerivativeView& v, const double* d_alpha, const double* d_q, const float2* grad_out,
               c5::HvpParams& hp) {
    C5_HIP(ctx, ctx->tan_dir.ensure(static_cast<size_t>(ctx->n_cells) * sizeof(double2)));
    hp = c5::HvpParams{};
    hp.dir = ctx->tan_dir.as<double2>();
    c5::launch_tangent_gather(v.s, d_alpha, d_q, v.perm, ctx->n_cells, ctx->tan_dir.as<double2>());
    hp.grad_out = grad_out;
    if (v.bin_sort) return C5_OK;
    C5_HIP(ctx, ctx->adj_lambda.ensure(static_cast<size_t>(v.padded) * sizeof(double)));
    C5_HIP(ctx, ctx->hvp_lambda_dot.ensure(static_cast<size_t>(v.padded) * sizeof(double)));
    hp.w = v.w;
    hp.lambda = ctx->adj_lambda.as<double>();
    hp.lambda_dot = ctx->hvp_lambda_dot.as<double>();
    return C5_OK;
}

// The exact passes of the Hessian-vector render: the direction into device order (the tangent's buffer), pass 1 (Lambda
// and Lambda_dot per pixel), pass E into x.exps (`bounds`: cleared here first) and pass S against x.exps into x.words
// (`sums`: cleared here first, with the misfit word) - the walk's, or hvp_resolve's over bin_sort_resolve's lists.
int hvp_exact_passes(c5_context* ctx, const DerivativeView& v, c5::ExactSums x, const double* d_alpha, const double* d_q,
                     const float2* grad_out, bool bounds, bool sums) {
    c5::HvpParams hp;
    if (const int rc = hvp_params(ctx, v, d_alpha, d_q, grad_out, hp)) return rc;
    c5::launch_exact_clear(v.s, x, ctx->n_cells, bounds, sums, sums);
    if (v.bin_sort) {
        if (bounds) c5::launch_hvp_exact_resolve(v.s, v.r, hp.dir, grad_out, x, false);
        if (sums) c5::launch_hvp_exact_resolve(v.s, v.r, hp.dir, grad_out, x, true);
        return C5_OK;
    }
    c5::launch_hvp_walk(v.s, hp, 1);
    if (bounds) c5::launch_hvp_exact_walk(v.s, hp, x, false);
    x.keep_entries = 0;
    if (sums) {
        c5::launch_hvp_exact_walk(v.s, hp, x, true);
        ctx->slots[0].head_clean = true;  // (pass S hands every head back cleared)
    }
    return C5_OK;
}

// The passes of one kind of exact sum (C5_EXACT_*) over the view; `image`: the upstream image, or the diagonal's weights
int exact_passes_of(c5_context* ctx, const DerivativeView& v, const c5::ExactSums& x, int what, const double* d_alpha,
                    const double* d_q, const float2* image, bool bounds, bool sums) {
    if (what == C5_EXACT_HVP) return hvp_exact_passes(ctx, v, x, d_alpha, d_q, image, bounds, sums);
    return exact_passes(ctx, v, x, image, bounds, sums, false, false, sums, what == C5_EXACT_GN_DIAGONAL);
}

const char* const kExactBoundsName[] = {"adjoint exact bounds", "gn diagonal exact bounds", "hvp exact bounds"};
const char* const kExactSumsName[] = {"adjoint exact sums", "gn diagonal exact sums", "hvp exact sums"};

// c5_render_exact_bounds: pass 1 and pass E over the context's rows; the exponents in the caller's order
int enqueue_exact_bounds(c5_context* ctx, int what, const double* d_alpha, const double* d_q, const float2* image, int32_t* exp_a,
                         int32_t* exp_q) {
    DerivativeView v;
    int rc = setup_derivative(ctx, v);
    if (rc || v.no_cells) return rc;
    c5::ExactSums x;
    rc = exact_sums(ctx, x);
    if (!rc) rc = exact_passes_of(ctx, v, x, what, d_alpha, d_q, image, true, false);
    if (rc) return rc;
    c5::launch_exact_emit_exps(v.s, x, v.perm, ctx->n_cells, exp_a, exp_q);
    return commit_derivative(ctx, kExactBoundsName[what]);
}

// c5_render_exact_sums: the caller's exponents into device order, pass 1 and pass S against them; the words in the
// caller's order
int enqueue_exact_sums(c5_context* ctx, int what, const double* d_alpha, const double* d_q, const float2* image, const int32_t* exp_a,
                       const int32_t* exp_q, int64_t* sums_a, int64_t* sums_q) {
    DerivativeView v;
    int rc = setup_derivative(ctx, v);
    if (rc || v.no_cells) return rc;
    c5::ExactSums x;
    rc = exact_sums(ctx, x);
    if (rc) return rc;
    c5::launch_exact_gather_exps(v.s, exp_a, exp_q, v.perm, ctx->n_cells, x);
    rc = exact_passes_of(ctx, v, x, what, d_alpha, d_q, image, false, true);
    if (rc) return rc;
    c5::launch_exact_emit_words(v.s, x, v.perm, ctx->n_cells, sums_a, sums_q);
    return commit_exact(ctx, x.misfits, kExactSumsName[what]);
}

// The adjoint: adjoint_one on the upstream image; with "adjoint_exact" or "exact_sums", the exact sums.
int enqueue_adjoint(c5_context* ctx, const float2* grad_out, double* ga_out, double* gq_out) {
    DerivativeView v;
    int rc = setup_derivative(ctx, v);
    if (rc || v.no_cells) return rc;
    if (ctx->adjoint_exact || ctx->exact_sums) return exact_images(ctx, v, 1, grad_out, ga_out, gq_out, "adjoint");
    rc = adjoint_one(ctx, v, false, grad_out, ga_out, gq_out);
    return rc ? rc : commit_derivative(ctx, "adjoint");
}

// One tangent over the view: the caller's direction into device order, then one walk (or tangent_resolve over
// bin_sort_resolve's lists) that writes (tau_dot, I_dot) per pixel.
int tangent_one(c5_context* ctx, const DerivativeView& v, const double* d_alpha, const double* d_q, float2* out) {
    C5_HIP(ctx, ctx->tan_dir.ensure(static_cast<size_t>(ctx->n_cells) * sizeof(double2)));
    double2* const dir = ctx->tan_dir.as<double2>();
    c5::launch_tangent_gather(v.s, d_alpha, d_q, v.perm, ctx->n_cells, dir);
    if (v.bin_sort) {
        c5::launch_tangent_resolve(v.s, v.r, dir, out);
    } else {
        c5::TangentParams tp{};
        tp.w = v.w;
        tp.dir = dir;
        tp.out = out;
        c5::launch_tangent_walk(v.s, tp);
        ctx->slots[0].head_clean = true;  // (the walk hands every head back cleared)
    }
    return C5_OK;
}

// nothing but solids: n tangent images do not depend on any cell
int zero_tangents(c5_context* ctx, const DerivativeView& v, int n, float2* out) {
    if (out && v.n_px > 0) C5_HIP(ctx, hipMemsetAsync(out, 0, static_cast<size_t>(n) * v.n_px * sizeof(float2), v.s));
    return C5_OK;
}

// The tangent: tangent_one on the direction.
int enqueue_tangent(c5_context* ctx, const double* d_alpha, const double* d_q, float2* out) {
    DerivativeView v;
    int rc = setup_derivative(ctx, v);
    if (rc) return rc;
    if (v.no_cells) return zero_tangents(ctx, v, 1, out);
    rc = tangent_one(ctx, v, d_alpha, d_q, out);
    return rc ? rc : commit_derivative(ctx, "tangent");
}

// Batches: the chunk width (4 or 8 directions / upstream images per walk; "batch_width").
int batch_width(const c5_context* ctx, int n) {
    if (ctx->batch_width) return ctx->batch_width;
    return n <= 4 ? 4 : 8;
}

// directions k0 .. k0 + n_used - 1 of the caller's [n][n_cells] arrays into bat_dirs (ensured by the caller): `width`
// interleaved pairs per cell in device order
void gather_chunk(c5_context* ctx, const DerivativeView& v, int width, const double* d_alpha, const double* d_q, int k0, int n_used) {
    c5::launch_tangent_gather_batch(v.s, width, d_alpha, d_q, v.perm, ctx->n_cells, k0, n_used, ctx->bat_dirs.as<double2>());
}

// The batched pass 2 over the view's walk: its buffers (Lambda's, and [n_cells][2 width] sums in device order) and its
// parameters but for the chunk's (grad_out, n_used, keep_entries).
int adjoint_batch_params(c5_context* ctx, const DerivativeView& v, int width, c5::AdjointBatchParams& ab) {
    C5_HIP(ctx, ctx->adj_lambda.ensure(static_cast<size_t>(v.padded) * sizeof(double)));
    C5_HIP(ctx, ctx->bat_grad.ensure(static_cast<size_t>(ctx->n_cells) * 2 * width * sizeof(double)));
    ab = c5::AdjointBatchParams{};
    ab.w = v.w;
    ab.image_px = v.n_px;
    ab.lambda = ctx->adj_lambda.as<double>();
    ab.grad = ctx->bat_grad.as<double>();
    return C5_OK;
}

// ... and one chunk of it: the sums zeroed, the walk, the permutation into rows k0_out .. of the caller's arrays
int adjoint_chunk(c5_context* ctx, const DerivativeView& v, int width, const c5::AdjointBatchParams& ab, int k0_out, double* ga_out,
                  double* gq_out) {
    C5_HIP(ctx, hipMemsetAsync(ab.grad, 0, static_cast<size_t>(ctx->n_cells) * 2 * width * sizeof(double), v.s));
    c5::launch_adjoint_walk_batch(v.s, width, ab);
    c5::launch_adjoint_permute_batch(v.s, width, ab.grad, v.perm, ctx->n_cells, k0_out, ab.n_used, ga_out, gq_out);
    return C5_OK;
}

// n directions ([n][n_cells] fp64 each, the caller's order; null: zero) -> out[n][local_rows][res_x]: one per-view setup,
// then per chunk of up to `width` directions a gather into device order and one walk; the entry heads stay in place
// between the chunks and the last walk hands them back cleared.  On bin_sort_resolve's lists: tangent_one per direction
// (the first sorts the lists, the others find them sorted).  A batch of one is the single tangent.
int enqueue_tangent_batch(c5_context* ctx, int n, const double* d_alpha, const double* d_q, float2* out) {
    if (n == 1) return enqueue_tangent(ctx, d_alpha, d_q, out);
    DerivativeView v;
    int rc = setup_derivative(ctx, v);
    if (rc) return rc;
    if (v.no_cells) return zero_tangents(ctx, v, n, out);
    const int64_t n_cells = ctx->n_cells;
    if (v.bin_sort) {
        for (int j = 0; j < n && !rc; ++j)
            rc = tangent_one(ctx, v, d_alpha ? d_alpha + j * n_cells : nullptr, d_q ? d_q + j * n_cells : nullptr,
                             out + j * v.n_px);
        return rc ? rc : commit_derivative(ctx, "tangent batch");
    }
    const int width = batch_width(ctx, n);
    C5_HIP(ctx, ctx->bat_dirs.ensure(static_cast<size_t>(n_cells) * width * sizeof(double2)));
    c5::TangentBatchParams tb{};
    tb.w = v.w;
    tb.dirs = ctx->bat_dirs.as<double2>();
    tb.image_px = v.n_px;
    for (int k0 = 0; k0 < n; k0 += width) {
        tb.n_used = std::min(width, n - k0);
        tb.out = out + k0 * v.n_px;
        tb.keep_entries = k0 + width < n;
        gather_chunk(ctx, v, width, d_alpha, d_q, k0, tb.n_used);
        c5::launch_tangent_walk_batch(v.s, width, tb);
    }
    ctx->slots[0].head_clean = true;  // (the last chunk's walk hands every head back cleared)
    return commit_derivative(ctx, "tangent batch");
}

// n upstream images ([n][local_rows][res_x] float2) -> ga_out / gq_out [n][n_cells] in the caller's order: one per-view
// setup and ONE pass 1 (Lambda does not depend on the weights), then per chunk of up to `width` images the batched pass 2
// into [n_cells][2 width] and its permutation.  On bin_sort_resolve's lists: adjoint_one per image.  A batch of one is the
// single adjoint.  With "adjoint_exact" or "exact_sums": the single exact path per image (exact_images).
int enqueue_adjoint_batch(c5_context* ctx, int n, const float2* grad_out, double* ga_out, double* gq_out) {
    if (n == 1) return enqueue_adjoint(ctx, grad_out, ga_out, gq_out);
    DerivativeView v;
    int rc = setup_derivative(ctx, v);
    if (rc || v.no_cells) return rc;
    if (ctx->adjoint_exact || ctx->exact_sums) return exact_images(ctx, v, n, grad_out, ga_out, gq_out, "adjoint batch");
    const int64_t n_cells = ctx->n_cells;
    if (v.bin_sort) {
        for (int j = 0; j < n && !rc; ++j)
            rc = adjoint_one(ctx, v, false, grad_out + j * v.n_px, ga_out + j * n_cells, gq_out + j * n_cells);
        return rc ? rc : commit_derivative(ctx, "adjoint batch");
    }
    const int width = batch_width(ctx, n);
    c5::AdjointParams ap;
    c5::AdjointBatchParams ab;
    rc = adjoint_params(ctx, v, ap);
    if (!rc) rc = adjoint_batch_params(ctx, v, width, ab);
    if (rc) return rc;
    c5::launch_adjoint_walk(v.s, ap, 1);
    for (int k0 = 0; k0 < n; k0 += width) {
        ab.n_used = std::min(width, n - k0);
        ab.grad_out = grad_out + k0 * v.n_px;
        ab.keep_entries = k0 + width < n;
        rc = adjoint_chunk(ctx, v, width, ab, k0, ga_out, gq_out);
        if (rc) return rc;
    }
    ctx->slots[0].head_clean = true;  // (the last chunk's pass 2 hands every head back cleared)
    return commit_derivative(ctx, "adjoint batch");
}

// The Gauss-Newton product H v = J^T W J v for n directions: one per-view setup, then per chunk of up to `width` directions
// the gather, pass A (gn_walk_a: the tangent walk that is also the adjoint's pass 1; g = w * J v in fp32 and Lambda), the
// batched pass 2 on g, and its permutation.  The heads stay in place from pass A to pass B and between the chunks; the
// last pass B hands them back cleared.  On bin_sort_resolve's lists: tangent_one -> gn_weight -> adjoint_one per
// direction.  ha_out / hq_out: either may be null (then that block goes to a spare buffer); jv_out may be null.
// With "exact_sums": pass A per chunk as it is, then every direction's g through the single exact path - passes E and S
// on Lambda as pass A left it, and the finish - one after the other (exact_images' loop): bit for bit the exact adjoint
// of g.  Pass S leaves the heads in place for all but the last direction of the call.
int enqueue_gn_product(c5_context* ctx, int n, const double* d_alpha, const double* d_q, const float2* weight, double* ha_out,
                       double* hq_out, float2* jv_out) {
    DerivativeView v;
    int rc = setup_derivative(ctx, v);
    if (rc) return rc;
    if (v.no_cells) return zero_tangents(ctx, v, n, jv_out);
    const int64_t n_cells = ctx->n_cells, n_px = v.n_px;
    const int width = v.bin_sort ? 1 : batch_width(ctx, n);
    const bool exact = ctx->exact_sums != 0;
    c5::ExactSums x{};
    if (exact) {
        rc = exact_sums(ctx, x);
        if (rc) return rc;
    }
    // direction j's g through passes E and S and the finish (a null output is not written)
    auto exact_one = [&](int j, const float2* g) -> int {
        const int rc1 = exact_passes(ctx, v, x, g, true, true, true, j + 1 < n, j == 0);
        if (rc1) return rc1;
        c5::launch_exact_finish(v.s, x, v.perm, n_cells, ha_out ? ha_out + j * n_cells : nullptr, hq_out ? hq_out + j * n_cells : nullptr);
        return C5_OK;
    };
    if (!exact && (!ha_out || !hq_out)) C5_HIP(ctx, ctx->gn_spare.ensure(static_cast<size_t>(n_cells) * width * sizeof(double)));
    double* const spare = ctx->gn_spare.as<double>();
    if (v.bin_sort) {
        C5_HIP(ctx, ctx->gn_g.ensure(2 * static_cast<size_t>(n_px) * sizeof(float2) + 16));
        float2* const g = ctx->gn_g.as<float2>();
        for (int j = 0; j < n; ++j) {
            float2* const t = jv_out ? jv_out + j * n_px : g + n_px;
            rc = tangent_one(ctx, v, d_alpha ? d_alpha + j * n_cells : nullptr, d_q ? d_q + j * n_cells : nullptr, t);
            if (rc) return rc;
            c5::launch_gn_weight(v.s, t, weight, n_px, 1, g);
            rc = exact ? exact_one(j, g)
                       : adjoint_one(ctx, v, false, g, ha_out ? ha_out + j * n_cells : spare, hq_out ? hq_out + j * n_cells : spare);
            if (rc) return rc;
        }
        return exact ? commit_exact(ctx, x.misfits, "gn product") : commit_derivative(ctx, "gn product");
    }
    c5::AdjointBatchParams ab{};
    if (exact) C5_HIP(ctx, ctx->adj_lambda.ensure(static_cast<size_t>(v.padded) * sizeof(double)));
    else rc = adjoint_batch_params(ctx, v, width, ab);
    if (rc) return rc;
    C5_HIP(ctx, ctx->bat_dirs.ensure(static_cast<size_t>(n_cells) * width * sizeof(double2)));
    C5_HIP(ctx, ctx->gn_g.ensure(static_cast<size_t>(width) * n_px * sizeof(float2) + 16));
    c5::GnWalkParams ga{};
    ga.w = v.w;
    ga.dirs = ctx->bat_dirs.as<double2>();
    ga.weight = weight;
    ga.lambda = ctx->adj_lambda.as<double>();
    ga.g = ctx->gn_g.as<float2>();
    ga.image_px = n_px;
    ab.grad_out = ga.g;
    for (int k0 = 0; k0 < n; k0 += width) {
        ga.n_used = ab.n_used = std::min(width, n - k0);
        ga.jv_out = jv_out ? jv_out + k0 * n_px : nullptr;
        ab.keep_entries = k0 + width < n;
        gather_chunk(ctx, v, width, d_alpha, d_q, k0, ga.n_used);
        c5::launch_gn_walk_a(v.s, width, ga);
        if (exact) {
            for (int j = 0; j < ga.n_used && !rc; ++j) rc = exact_one(k0 + j, ga.g + j * n_px);
        } else {
            rc = adjoint_chunk(ctx, v, width, ab, 0, ha_out ? ha_out + k0 * n_cells : spare, hq_out ? hq_out + k0 * n_cells : spare);
        }
        if (rc) return rc;
    }
    ctx->slots[0].head_clean = true;  // (the last chunk's pass B - or the last direction's pass S - hands every head back cleared)
    return exact ? commit_exact(ctx, x.misfits, "gn product") : commit_derivative(ctx, "gn product");
}

// The motion tangent: n velocity fields (host memory, [n][12]: A row-major then b, view space) -> out[n][local_rows][res_x]:
// one per-view setup, then per chunk of up to `width` fields one walk; the heads stay in place between the chunks and the
// last walk hands them back cleared.  The derivative's records are those of "integration" 0, whose walk coordinate IS
// view z (walk_common.hpp: to_exit_record, sign +1): the fields go to the kernels as they are.  On bin_sort_resolve's
// lists: motion_resolve per field (the first sorts the lists, the others find them sorted).
int enqueue_motion(c5_context* ctx, int n, const double* fields, float2* out) {
    DerivativeView v;
    int rc = setup_derivative(ctx, v);
    if (rc) return rc;
    if (v.no_cells) return zero_tangents(ctx, v, n, out);
    if (v.bin_sort) {
        for (int j = 0; j < n; ++j) {
            c5::MotionField f;
            std::copy(fields + 12 * j, fields + 12 * j + 12, f.f);
            c5::launch_motion_resolve(v.s, v.r, f, out + j * v.n_px);
        }
        return commit_derivative(ctx, "motion tangent");
    }
    const int width = batch_width(ctx, n);
    c5::MotionParams mp{};
    mp.w = v.w;
    mp.geo = v.geo;
    mp.image_px = v.n_px;
    for (int k0 = 0; k0 < n; k0 += width) {
        mp.n_used = std::min(width, n - k0);
        mp.out = out + k0 * v.n_px;
        mp.keep_entries = k0 + width < n;
        for (int j = 0; j < c5::kMotionWidth; ++j)
            for (int i = 0; i < 12; ++i) mp.field[j][i] = j < mp.n_used ? fields[12 * (k0 + j) + i] : 0.0;
        c5::launch_motion_walk(v.s, width, mp);
    }
    ctx->slots[0].head_clean = true;  // (the last chunk's walk hands every head back cleared)
    return commit_derivative(ctx, "motion tangent");
}

// ---- exact vertex adjoint sums ("vertex_exact", c5_render_vertex_exact_*)

// The exact vertex sums' buffer over the context's cells - 240 bytes per cell (192 of words, 48 of exponents) and the
// misfit word, allocated here at the first exact vertex call - with the word width of the WHOLE image (c5_set_image).
int vertex_exact_sums(c5_context* ctx, c5::VertexExactSums& x) {
    const size_t n_cells = static_cast<size_t>(ctx->n_cells);
    int m;
    if (const int rc = exact_word_bits(ctx, ctx->im.res_x, ctx->im.res_y, m)) return rc;
    C5_HIP(ctx, ctx->vtx_exact.ensure(n_cells * 240 + 8));
    x = c5::VertexExactSums{};
    x.words = ctx->vtx_exact.as<long long>();
    x.exps = reinterpret_cast<int32_t*>(x.words + 24 * n_cells);  // (192 n_cells bytes on: 16-byte aligned)
    x.misfits = reinterpret_cast<unsigned*>(x.exps + 12 * n_cells);
    x.word_bits = m;
    return C5_OK;
}

// The point -> (cell, local vertex) incidence table of the grid on the device, built by the host at the first exact vertex
// call after an upload: per point its entries 4 * (device cell) + (vertex) in ascending order of the CALLER's cell index,
// so that the per-point sums do not depend on "cell_order".  Connectivity only: c5_update_points keeps it.  Cells name
// the representatives of welded points: the others' lists are empty.
int vertex_incidence(c5_context* ctx, c5::VertexIncidence& inc) {
    const int64_t n_pts = ctx->n_pts, n_cells = ctx->n_cells;
    if (ctx->vtx_inc_serial != ctx->grid_serial || !ctx->vtx_inc.ptr) {
        const std::vector<int32_t>& cv = ctx->host_cell_vert;  // (device order)
        std::vector<int32_t> tab(static_cast<size_t>(n_pts + 1 + 4 * n_cells), 0);
        int32_t* const ptr = tab.data();
        int32_t* const idx = ptr + n_pts + 1;
        for (int64_t i = 0; i < 4 * n_cells; ++i) ++ptr[cv[static_cast<size_t>(i)] + 1];
        for (int64_t p = 0; p < n_pts; ++p) ptr[p + 1] += ptr[p];
        std::vector<int32_t> at(ptr, ptr + n_pts), of_caller;  // where a point's next entry goes; caller's index -> the device's
        if (!ctx->cell_perm.empty()) {
            of_caller.resize(static_cast<size_t>(n_cells));
            for (int64_t d = 0; d < n_cells; ++d) of_caller[static_cast<size_t>(ctx->cell_perm[static_cast<size_t>(d)])] = static_cast<int32_t>(d);
        }
        for (int64_t c = 0; c < n_cells; ++c) {
            const int64_t d = of_caller.empty() ? c : of_caller[static_cast<size_t>(c)];
            for (int k = 0; k < 4; ++k) idx[at[static_cast<size_t>(cv[static_cast<size_t>(4 * d + k)])]++] = static_cast<int32_t>(4 * d + k);
        }
        C5_HIP(ctx, ctx->vtx_inc.ensure(tab.size() * sizeof(int32_t)));
        C5_HIP(ctx, hipMemcpy(ctx->vtx_inc.ptr, tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        ctx->vtx_inc_serial = ctx->grid_serial;
    }
    inc.ptr = ctx->vtx_inc.as<int32_t>();
    inc.idx = inc.ptr + n_pts + 1;
    return C5_OK;
}

// The vertex adjoint's parameters over the view's walk for one upstream image, and pass 1's on the same Lambda (its buffer
// is ensured here, by adjoint_params); where the sums go (vp.face_w, or the exact sums) is the caller's to fill in.
int vertex_params(c5_context* ctx, const DerivativeView& v, const float2* grad_out, c5::AdjointParams& ap, c5::VertexParams& vp) {
    if (const int rc = adjoint_params(ctx, v, ap)) return rc;
    vp = c5::VertexParams{};
    vp.w = v.w;
    vp.geo = v.geo;
    vp.grad_out = grad_out;
    vp.lambda = ap.lambda;
    return C5_OK;
}

// nothing but solids: n gradients [n_pts][3] do not depend on any point
int zero_vertex_grads(c5_context* ctx, const DerivativeView& v, int n, double* grad_xyz) {
    const size_t n_pts = static_cast<size_t>(ctx->n_pts);
    if (n_pts > 0) C5_HIP(ctx, hipMemsetAsync(grad_xyz, 0, 3 * n * n_pts * sizeof(double), v.s));
    return C5_OK;
}

// The exact passes of the vertex adjoint over the view for one upstream image - exact_passes with the vertex kernels:
// pass 1 (unless Lambda is there: `have_lambda`), pass E into x.exps (`bounds`: cleared here first) and pass S against
// x.exps into x.words (`sums`: cleared here first, the misfit word with them where `first`); keep: the walk's pass S
// leaves the entry heads in place (another image follows).
int vertex_exact_passes(c5_context* ctx, const DerivativeView& v, c5::VertexExactSums x, const float2* grad_out, bool bounds, bool sums,
                        bool have_lambda, bool keep, bool first) {
    c5::launch_vertex_exact_clear(v.s, x, ctx->n_cells, bounds, sums, sums && first);
    if (v.bin_sort) {
        if (bounds) c5::launch_vertex_exact_resolve(v.s, v.r, grad_out, x, false);
        if (sums) c5::launch_vertex_exact_resolve(v.s, v.r, grad_out, x, true);
        return C5_OK;
    }
    c5::AdjointParams ap;
    c5::VertexParams vp;
    if (const int rc = vertex_params(ctx, v, grad_out, ap, vp)) return rc;
    if (!have_lambda) c5::launch_adjoint_walk(v.s, ap, 1);
    if (bounds) c5::launch_vertex_exact_walk(v.s, vp, x, false);
    x.keep_entries = keep ? 1 : 0;
    if (sums) {
        c5::launch_vertex_exact_walk(v.s, vp, x, true);
        if (!keep) ctx->slots[0].head_clean = true;  // (pass S hands every head back cleared)
    }
    return C5_OK;
}

// Steps 1 (the finish of the words) to 4 of the exact vertex adjoint on x's exponents and words (device order): face_w,
// the per-cell triples, the per-point gather over the incidence table and the view's M^T, into grad_xyz [n_pts][3].
int vertex_exact_finish(c5_context* ctx, const DerivativeView& v, const c5::VertexExactSums& x, double* grad_xyz) {
    const size_t n_cells = static_cast<size_t>(ctx->n_cells);
    C5_HIP(ctx, ctx->vtx_face.ensure(12 * n_cells * sizeof(double)));
    C5_HIP(ctx, ctx->vtx_triples.ensure(12 * n_cells * sizeof(double)));
    c5::VertexIncidence inc;
    int rc = vertex_incidence(ctx, inc);
    if (rc) return rc;
    c5::launch_vertex_exact_finish(v.s, x, v.geo, ctx->n_cells, ctx->vtx_face.as<double>(), ctx->vtx_triples.as<double>(), inc, ctx->n_pts,
                                   ctx->view, grad_xyz);
    return C5_OK;
}

// "vertex_exact" 1: images k0 .. k0 + n - 1 of a call of n_total upstream images (grad_out: image k0) -> rows k0 .. of
// grad_xyz [n_total][n_pts][3], every image through passes E and S and the finish, one after the other; pass 1 runs once,
// before the call's first image - or not at all where Lambda is there (`have_lambda`: the vertex Gauss-Newton product's
// pass A left it).  The call's last image hands the heads back cleared, and behind it the call is committed under the name
// `what` (commit_exact: the misfit word travels).  "vertex_merge" has no say here.
int vertex_exact_images(c5_context* ctx, const DerivativeView& v, int n, const float2* grad_out, double* grad_xyz, const char* what,
                        bool have_lambda = false, int k0 = 0, int n_total = -1) {
    if (n_total < 0) n_total = n;
    c5::VertexExactSums x;
    int rc = vertex_exact_sums(ctx, x);
    const int64_t n_pts = ctx->n_pts;
    for (int j = 0; j < n && !rc; ++j) {
        const int k = k0 + j;
        rc = vertex_exact_passes(ctx, v, x, grad_out + j * v.n_px, true, true, have_lambda || k > 0, k + 1 < n_total, k == 0);
        if (!rc) rc = vertex_exact_finish(ctx, v, x, grad_xyz + 3 * k * n_pts);
    }
    if (rc || k0 + n < n_total) return rc;
    return commit_exact(ctx, x.misfits, what);
}

// c5_render_vertex_exact_bounds: pass 1 and pass E over the context's rows; the exponents in the caller's cell order
int enqueue_vertex_exact_bounds(c5_context* ctx, const float2* grad_out, int32_t* exps) {
    DerivativeView v;
    int rc = setup_derivative(ctx, v);
    if (rc || v.no_cells) return rc;
    c5::VertexExactSums x;
    rc = vertex_exact_sums(ctx, x);
    if (!rc) rc = vertex_exact_passes(ctx, v, x, grad_out, true, false, false, false, false);
    if (rc) return rc;
    c5::launch_vertex_exact_emit(v.s, x, v.perm, ctx->n_cells, exps, nullptr);
    return commit_derivative(ctx, "vertex exact bounds");
}

// c5_render_vertex_exact_sums: the caller's exponents into device order, pass 1 and pass S against them; the words in the
// caller's cell order
int enqueue_vertex_exact_sums(c5_context* ctx, const float2* grad_out, const int32_t* exps, int64_t* sums) {
    DerivativeView v;
    int rc = setup_derivative(ctx, v);
    if (rc || v.no_cells) return rc;
    c5::VertexExactSums x;
    rc = vertex_exact_sums(ctx, x);
    if (rc) return rc;
    c5::launch_vertex_exact_gather(v.s, exps, nullptr, v.perm, ctx->n_cells, x);
    rc = vertex_exact_passes(ctx, v, x, grad_out, false, true, false, false, true);
    if (rc) return rc;
    c5::launch_vertex_exact_emit(v.s, x, v.perm, ctx->n_cells, nullptr, sums);
    return commit_exact(ctx, x.misfits, "vertex exact sums");
}

// c5_vertex_exact_finish: the per-view setup (the finish wants the points in view space), the caller's exponents and words
// into device order, and the finish.  No walk: the entry lists the setup built stay unused.
int enqueue_vertex_exact_finish(c5_context* ctx, const int32_t* exps, const int64_t* sums, double* grad_xyz) {
    DerivativeView v;
    int rc = setup_derivative(ctx, v);
    if (rc) return rc;
    if (v.no_cells) return zero_vertex_grads(ctx, v, 1, grad_xyz);
    c5::VertexExactSums x;
    rc = vertex_exact_sums(ctx, x);
    if (rc) return rc;
    c5::launch_vertex_exact_gather(v.s, exps, sums, v.perm, ctx->n_cells, x);
    rc = vertex_exact_finish(ctx, v, x, grad_xyz);
    return rc ? rc : commit_derivative(ctx, "vertex exact finish");
}

// One vertex adjoint over the view: the per-face weights and the view-space gradient zeroed, the adjoint's pass 1 and
// vertex_walk (or vertex_resolve over bin_sort_resolve's lists), then vertex_finish into the caller's [n_pts][3] (the
// caller's point order is the device's: only the cells are reordered).  have_lambda: Lambda is there (the vertex
// Gauss-Newton product's pass A left it, with the heads in place): pass 1 is not launched.
int vertex_one(c5_context* ctx, const DerivativeView& v, const float2* grad_out, double* grad_xyz, bool have_lambda = false) {
    const size_t n_cells = static_cast<size_t>(ctx->n_cells), n_pts = static_cast<size_t>(ctx->n_pts);
    C5_HIP(ctx, ctx->vtx_face.ensure(12 * n_cells * sizeof(double)));
    C5_HIP(ctx, ctx->vtx_grad.ensure(3 * n_pts * sizeof(double)));
    double* const face_w = ctx->vtx_face.as<double>();
    double* const grad_view = ctx->vtx_grad.as<double>();
    C5_HIP(ctx, hipMemsetAsync(face_w, 0, 12 * n_cells * sizeof(double), v.s));
    C5_HIP(ctx, hipMemsetAsync(grad_view, 0, 3 * n_pts * sizeof(double), v.s));
    if (v.bin_sort) {
        c5::launch_vertex_resolve(v.s, v.r, grad_out, face_w);
    } else {
        c5::AdjointParams ap;
        c5::VertexParams vp;
        if (const int rc = vertex_params(ctx, v, grad_out, ap, vp)) return rc;
        if (!have_lambda) c5::launch_adjoint_walk(v.s, ap, 1);
        vp.face_w = face_w;
        c5::launch_vertex_walk(v.s, vp, ctx->vertex_merge != 0);
        ctx->slots[0].head_clean = true;  // (vertex_walk hands every head back cleared)
    }
    c5::launch_vertex_finish(v.s, v.geo, ctx->n_cells, face_w, grad_view, ctx->n_pts, ctx->view, grad_xyz);
    return C5_OK;
}

// The vertex adjoint: vertex_one on the upstream image; with "vertex_exact", the exact sums (vertex_exact_images).
int enqueue_vertex_adjoint(c5_context* ctx, const float2* grad_out, double* grad_xyz) {
    DerivativeView v;
    int rc = setup_derivative(ctx, v);
    if (rc) return rc;
    if (v.no_cells) return zero_vertex_grads(ctx, v, 1, grad_xyz);
    if (ctx->vertex_exact) return vertex_exact_images(ctx, v, 1, grad_out, grad_xyz, "vertex adjoint");
    rc = vertex_one(ctx, v, grad_out, grad_xyz);
    return rc ? rc : commit_derivative(ctx, "vertex adjoint");
}

// The batched vertex walk over the view: its buffers (Lambda's, [n_cells][width][12] weights and [n_pts][3][width] view-space
// sums) and its parameters but for the chunk's (grad_out, n_used, keep_entries).
int vertex_batch_params(c5_context* ctx, const DerivativeView& v, int width, c5::VertexBatchParams& vb) {
    const size_t n_cells = static_cast<size_t>(ctx->n_cells), n_pts = static_cast<size_t>(ctx->n_pts);
    C5_HIP(ctx, ctx->adj_lambda.ensure(static_cast<size_t>(v.padded) * sizeof(double)));
    C5_HIP(ctx, ctx->vtx_bat_face.ensure(12 * n_cells * width * sizeof(double)));
    C5_HIP(ctx, ctx->vtx_bat_grad.ensure(3 * n_pts * width * sizeof(double)));
    vb = c5::VertexBatchParams{};
    vb.w = v.w;
    vb.geo = v.geo;
    vb.image_px = v.n_px;
    vb.lambda = ctx->adj_lambda.as<double>();
    vb.face_w = ctx->vtx_bat_face.as<double>();
    return C5_OK;
}

// ... and one chunk of it: the two buffers zeroed, the walk, the batched finish into rows k0 .. of the caller's array
int vertex_chunk(c5_context* ctx, const DerivativeView& v, int width, const c5::VertexBatchParams& vb, int k0, double* grad_xyz) {
    const size_t n_cells = static_cast<size_t>(ctx->n_cells), n_pts = static_cast<size_t>(ctx->n_pts);
    double* const grad_view = ctx->vtx_bat_grad.as<double>();
    C5_HIP(ctx, hipMemsetAsync(vb.face_w, 0, 12 * n_cells * width * sizeof(double), v.s));
    C5_HIP(ctx, hipMemsetAsync(grad_view, 0, 3 * n_pts * width * sizeof(double), v.s));
    c5::launch_vertex_walk_batch(v.s, width, vb);
    c5::launch_vertex_finish_batch(v.s, width, v.geo, ctx->n_cells, vb.face_w, grad_view, ctx->n_pts, ctx->view, k0, vb.n_used, grad_xyz);
    return C5_OK;
}

// The batched vertex adjoint: n upstream images ([n][local_rows][res_x] float2) -> grad_xyz [n][n_pts][3] in the caller's
// point order: one per-view setup and ONE pass 1 (Lambda does not depend on the weights), then per chunk of up to `width`
// images the two buffers zeroed, vertex_walk_batch and the batched finish; the heads stay in place between the chunks and
// the last walk hands them back cleared.  On bin_sort_resolve's lists: vertex_one per image (the first sorts the lists,
// the others find them sorted).  A batch of one is the single vertex adjoint.  Always merged
// ("vertex_merge" is the single call's); the chunk's buffers - 96 width bytes per cell, 24 width per point - are
// allocated here, at the first batched call.
int enqueue_vertex_adjoint_batch(c5_context* ctx, int n, const float2* grad_out, double* grad_xyz) {
    if (n == 1) return enqueue_vertex_adjoint(ctx, grad_out, grad_xyz);
    DerivativeView v;
    int rc = setup_derivative(ctx, v);
    if (rc) return rc;
    if (v.no_cells) return zero_vertex_grads(ctx, v, n, grad_xyz);
    // "vertex_exact": ONE pass 1, then the single exact path image by image - every slice bit for bit the single call's
    if (ctx->vertex_exact) return vertex_exact_images(ctx, v, n, grad_out, grad_xyz, "vertex adjoint batch");
    const size_t n_pts = static_cast<size_t>(ctx->n_pts);
    if (v.bin_sort) {
        for (int j = 0; j < n && !rc; ++j) rc = vertex_one(ctx, v, grad_out + j * v.n_px, grad_xyz + 3 * j * n_pts);
        return rc ? rc : commit_derivative(ctx, "vertex adjoint batch");
    }
    const int width = batch_width(ctx, n);
    c5::AdjointParams ap;
    c5::VertexBatchParams vb;
    rc = adjoint_params(ctx, v, ap);
    if (!rc) rc = vertex_batch_params(ctx, v, width, vb);
    if (rc) return rc;
    c5::launch_adjoint_walk(v.s, ap, 1);
    for (int k0 = 0; k0 < n; k0 += width) {
        vb.n_used = std::min(width, n - k0);
        vb.grad_out = grad_out + k0 * v.n_px;
        vb.keep_entries = k0 + width < n;
        rc = vertex_chunk(ctx, v, width, vb, k0, grad_xyz);
        if (rc) return rc;
    }
    ctx->slots[0].head_clean = true;  // (the last chunk's walk hands every head back cleared)
    return commit_derivative(ctx, "vertex adjoint batch");
}

// The vertex tangent: n displacement fields ([n][n_pts][3] fp64 on the device, the caller's point order, the coordinates of
// the upload) -> out[n][local_rows][res_x]: one per-view setup, then per chunk of up to `width` fields vertex_velocity (the
// fields into view space, `width` per point) and one walk; the heads stay in place between the chunks and the last walk
// hands them back cleared.  On bin_sort_resolve's lists: vertex_tangent_resolve per field (the first sorts the lists, the
// others find them sorted).  The velocity buffer is allocated here, at the first call.
int enqueue_vertex_tangent(c5_context* ctx, int n, const double* d_xyz, float2* out) {
    DerivativeView v;
    int rc = setup_derivative(ctx, v);
    if (rc) return rc;
    if (v.no_cells) return zero_tangents(ctx, v, n, out);
    const int width = batch_width(ctx, n);
    C5_HIP(ctx, ctx->vtx_vel.ensure(3 * static_cast<size_t>(width) * static_cast<size_t>(ctx->n_pts) * sizeof(double)));
    double* const u_view = ctx->vtx_vel.as<double>();
    c5::VertexTangentParams vt{};
    vt.w = v.w;
    vt.geo = v.geo;
    vt.u_view = u_view;
    vt.image_px = v.n_px;
    for (int k0 = 0; k0 < n; k0 += width) {
        vt.n_used = std::min(width, n - k0);
        c5::launch_vertex_velocity(v.s, width, d_xyz, ctx->n_pts, k0, vt.n_used, ctx->view, u_view);
        if (v.bin_sort) {
            for (int j = 0; j < vt.n_used; ++j)
                c5::launch_vertex_tangent_resolve(v.s, v.r, u_view, width, j, out + (k0 + j) * v.n_px);
            continue;
        }
        vt.out = out + k0 * v.n_px;
        vt.keep_entries = k0 + width < n;
        c5::launch_vertex_tangent_walk(v.s, width, vt);
    }
    if (!v.bin_sort) ctx->slots[0].head_clean = true;  // (the last chunk's walk hands every head back cleared)
    return commit_derivative(ctx, "vertex tangent");
}

// The vertex Gauss-Newton product H v = J^T W J v for n per-point fields, J the vertex tangent's map: one per-view setup,
// then per chunk of up to `width` fields vertex_velocity, pass A (vertex_gn_walk_a: the vertex tangent's walk that is also
// the adjoint's pass 1; g = w * J v in fp32 and Lambda) and pass B on g with pass A's Lambda - pass 1 is never launched.
// Pass B: one field goes through vertex_one ("vertex_merge" has its say), several through the batched walk and finish, and
// under "vertex_exact" every field's g through the single exact path (vertex_exact_images) - bit for bit the exact vertex
// adjoint of g.  The heads stay in place from pass A to pass B and between the chunks; the last pass B hands them back
// cleared.  On bin_sort_resolve's lists: vertex_tangent_resolve -> gn_weight -> vertex_one (or the exact passes) per field.
// jv_out may be null.
int enqueue_vertex_gn_product(c5_context* ctx, int n, const double* d_xyz, const float2* weight, double* h_xyz, float2* jv_out) {
    DerivativeView v;
    int rc = setup_derivative(ctx, v);
    if (rc) return rc;
    if (v.no_cells) {
        rc = zero_vertex_grads(ctx, v, n, h_xyz);
        return rc ? rc : zero_tangents(ctx, v, n, jv_out);
    }
    const int64_t n_px = v.n_px, n_pts = ctx->n_pts;
    const int width = batch_width(ctx, n);
    const bool exact = ctx->vertex_exact != 0;
    const char* const what = "vertex gn product";
    C5_HIP(ctx, ctx->vtx_vel.ensure(3 * static_cast<size_t>(width) * static_cast<size_t>(n_pts) * sizeof(double)));
    double* const u_view = ctx->vtx_vel.as<double>();
    if (v.bin_sort) {
        C5_HIP(ctx, ctx->gn_g.ensure(2 * static_cast<size_t>(n_px) * sizeof(float2) + 16));
        float2* const g = ctx->gn_g.as<float2>();
        for (int k0 = 0; k0 < n; k0 += width) {
            const int n_used = std::min(width, n - k0);
            c5::launch_vertex_velocity(v.s, width, d_xyz, n_pts, k0, n_used, ctx->view, u_view);
            for (int j = k0; j < k0 + n_used; ++j) {
                float2* const t = jv_out ? jv_out + j * n_px : g + n_px;
                c5::launch_vertex_tangent_resolve(v.s, v.r, u_view, width, j - k0, t);
                c5::launch_gn_weight(v.s, t, weight, n_px, 1, g);
                rc = exact ? vertex_exact_images(ctx, v, 1, g, h_xyz, what, true, j, n) : vertex_one(ctx, v, g, h_xyz + 3 * j * n_pts);
                if (rc) return rc;
            }
        }
        return exact ? C5_OK : commit_derivative(ctx, what);  // (exact: the last field's vertex_exact_images committed)
    }
    const bool batched = !exact && n > 1;
    c5::VertexBatchParams vb{};
    if (batched) rc = vertex_batch_params(ctx, v, width, vb);
    else C5_HIP(ctx, ctx->adj_lambda.ensure(static_cast<size_t>(v.padded) * sizeof(double)));
    if (rc) return rc;
    C5_HIP(ctx, ctx->gn_g.ensure(static_cast<size_t>(width) * n_px * sizeof(float2) + 16));
    c5::VertexGnWalkParams ga{};
    ga.w = v.w;
    ga.geo = v.geo;
    ga.u_view = u_view;
    ga.weight = weight;
    ga.lambda = ctx->adj_lambda.as<double>();
    ga.g = ctx->gn_g.as<float2>();
    ga.image_px = n_px;
    vb.grad_out = ga.g;
    for (int k0 = 0; k0 < n; k0 += width) {
        ga.n_used = vb.n_used = std::min(width, n - k0);
        ga.jv_out = jv_out ? jv_out + k0 * n_px : nullptr;
        vb.keep_entries = k0 + width < n;
        c5::launch_vertex_velocity(v.s, width, d_xyz, n_pts, k0, ga.n_used, ctx->view, u_view);
        c5::launch_vertex_gn_walk_a(v.s, width, ga);
        if (exact) rc = vertex_exact_images(ctx, v, ga.n_used, ga.g, h_xyz, what, true, k0, n);
        else if (batched) rc = vertex_chunk(ctx, v, width, vb, k0, h_xyz);
        else rc = vertex_one(ctx, v, ga.g, h_xyz, true);
        if (rc) return rc;
    }
    if (exact) return C5_OK;          // (the last field's pass S handed the heads back; vertex_exact_images committed)
    ctx->slots[0].head_clean = true;  // (the last chunk's pass B hands every head back cleared)
    return commit_derivative(ctx, what);
}

// The ray matrix's own buffer: the count per pixel ([padded] int32) and, behind them, the fill's word of changed rows.
int ray_matrix_buffer(c5_context* ctx, const DerivativeView& v, int32_t*& count, unsigned*& changed_rows) {
    C5_HIP(ctx, ctx->rm_count.ensure(static_cast<size_t>(v.padded + 1) * sizeof(int32_t)));
    count = ctx->rm_count.as<int32_t>();
    changed_rows = reinterpret_cast<unsigned*>(count + v.padded);
    return C5_OK;
}

// The ray matrix's rows: one per-view setup, the count per pixel (segment_walk<1>, which leaves the entry heads in place,
// or segment_count_resolve over bin_sort_resolve's lists) and the scan into row_ptr [n_px + 1] on the device.
int enqueue_ray_matrix_rows(c5_context* ctx, int64_t* row_ptr) {
    DerivativeView v;
    int rc = setup_derivative(ctx, v);
    if (rc) return rc;
    if (v.no_cells || v.n_px <= 0) C5_HIP(ctx, hipMemsetAsync(row_ptr, 0, static_cast<size_t>(v.n_px + 1) * sizeof(int64_t), v.s));
    if (v.no_cells) return C5_OK;  // (solids only: every row is empty)
    int32_t* count;
    unsigned* changed_rows;
    rc = ray_matrix_buffer(ctx, v, count, changed_rows);
    if (rc) return rc;
    C5_HIP(ctx, ctx->scratch64.ensure(static_cast<size_t>(v.padded / 1024 + 1024) * sizeof(int64_t)));
    if (v.bin_sort) {
        c5::launch_segment_count_resolve(v.s, v.r, count);
    } else {
        c5::RayMatrixParams m{};
        m.w = v.w;
        m.count = count;
        c5::launch_segment_walk(v.s, m, 1);
    }
    c5::launch_scan64(v.s, count, row_ptr, v.n_px, ctx->scratch64.as<int64_t>());
    return commit_derivative(ctx, "ray matrix rows");
}

// The ray matrix's arrays: a per-view setup of its own, then segment_walk<2> (or segment_fill_resolve), which writes only
// inside [0, capacity) and counts the rows that differ from row_ptr; that count travels to the host behind the status words.
int enqueue_ray_matrix_fill(c5_context* ctx, const int64_t* row_ptr, int64_t capacity, int32_t* col, double* dz, double* z_exit) {
    DerivativeView v;
    int rc = setup_derivative(ctx, v);
    if (rc) return rc;
    if (v.no_cells) {  // (solids only: every row is empty, and a row_ptr that says otherwise is another frame's; this waits)
        int64_t total = 0;
        C5_HIP(ctx, hipMemcpyAsync(&total, row_ptr + v.n_px, sizeof total, hipMemcpyDeviceToHost, v.s));
        C5_HIP(ctx, hipStreamSynchronize(v.s));
        if (total != 0)
            return fail(ctx, C5_ERR_STATE, "ray matrix fill: the frame changed between c5_ray_matrix_rows and c5_ray_matrix_fill: "
                        "row_ptr holds %lld segments, the scene has no cells", static_cast<long long>(total));
        return C5_OK;
    }
    int32_t* count;
    unsigned* changed_rows;
    rc = ray_matrix_buffer(ctx, v, count, changed_rows);
    if (rc) return rc;
    C5_HIP(ctx, hipMemsetAsync(changed_rows, 0, sizeof(unsigned), v.s));
    c5::RayMatrixParams m{};
    m.w = v.w;
    m.row_ptr = row_ptr;
    m.capacity = capacity;
    m.perm = v.perm;
    m.col = col;
    m.dz = dz;
    m.z_exit = z_exit;
    m.changed_rows = changed_rows;
    if (v.bin_sort) {
        c5::launch_segment_fill_resolve(v.s, v.r, m);
    } else {
        c5::launch_segment_walk(v.s, m, 2);
        ctx->slots[0].head_clean = true;  // (the fill hands every head back cleared)
    }
    rc = commit_derivative(ctx, "ray matrix fill");
    if (rc) return rc;
    C5_HIP(ctx, hipMemcpyAsync(ctx->adj_status + 3, changed_rows, sizeof(unsigned), hipMemcpyDeviceToHost, v.s));
    return C5_OK;
}

// The Hessian-vector render: the direction into device order (the tangent's buffer), the per-cell sums zeroed (the
// adjoint's buffer), two passes of the walk - Lambda and Lambda_dot per pixel, then the scatter - or hvp_resolve over
// bin_sort_resolve's lists, and the permutation into the caller's order.  ha_out / hq_out: either may be null.
int enqueue_hvp(c5_context* ctx, const double* d_alpha, const double* d_q, const float2* grad_out, double* ha_out, double* hq_out) {
    DerivativeView v;
    int rc = setup_derivative(ctx, v);
    if (rc || v.no_cells) return rc;
    if (ctx->exact_sums) {  // pass 1, pass E, pass S and the finish
        c5::ExactSums x;
        rc = exact_sums(ctx, x);
        if (!rc) rc = hvp_exact_passes(ctx, v, x, d_alpha, d_q, grad_out, true, true);
        if (rc) return rc;
        c5::launch_exact_finish(v.s, x, v.perm, ctx->n_cells, ha_out, hq_out);
        return commit_exact(ctx, x.misfits, "hvp");
    }
    const size_t n_cells = static_cast<size_t>(ctx->n_cells);
    C5_HIP(ctx, ctx->adj_grad.ensure(2 * n_cells * sizeof(double)));
    double* const ha_dev = ctx->adj_grad.as<double>();
    double* const hq_dev = ha_dev + n_cells;
    c5::HvpParams hp;
    rc = hvp_params(ctx, v, d_alpha, d_q, grad_out, hp);
    if (rc) return rc;
    C5_HIP(ctx, hipMemsetAsync(ha_dev, 0, 2 * n_cells * sizeof(double), v.s));
    if (v.bin_sort) {
        c5::launch_hvp_resolve(v.s, v.r, hp.dir, grad_out, ha_dev, hq_dev);
    } else {
        hp.h_a = ha_dev;
        hp.h_q = hq_dev;
        c5::launch_hvp_walk(v.s, hp, 1);
        c5::launch_hvp_walk(v.s, hp, 2);
        ctx->slots[0].head_clean = true;  // (the second pass hands every head back cleared)
    }
    c5::launch_hvp_permute(v.s, ha_dev, hq_dev, v.perm, ctx->n_cells, ha_out, hq_out);
    return commit_derivative(ctx, "hvp");
}

// diag(J^T W J): adjoint_one with the squared kernels.  weight null: ones.
int enqueue_gn_diagonal(c5_context* ctx, const float2* weight, double* da_out, double* dq_out) {
    DerivativeView v;
    int rc = setup_derivative(ctx, v);
    if (rc || v.no_cells) return rc;
    if (ctx->exact_sums) {  // pass 1, pass E on the squares, pass S and the finish
        c5::ExactSums x;
        rc = exact_sums(ctx, x);
        if (!rc) rc = exact_passes(ctx, v, x, weight, true, true, false, false, true, true);
        if (rc) return rc;
        c5::launch_exact_finish(v.s, x, v.perm, ctx->n_cells, da_out, dq_out);
        return commit_exact(ctx, x.misfits, "gn diagonal");
    }
    rc = adjoint_one(ctx, v, true, weight, da_out, dq_out);
    return rc ? rc : commit_derivative(ctx, "gn diagonal");
}

}  // namespace

namespace c5api __attribute__((visibility("hidden"))) {
// After the stream drained: the failure words of the last adjoint or tangent (as finish_frame treats a frame's).
int finish_adjoint(c5_context* ctx) {
    if (!ctx->adjoint_pending) return C5_OK;
    ctx->adjoint_pending = false;
    const unsigned lost_rays = ctx->adj_status[0], refused = ctx->adj_status[1], overlap_rays = ctx->adj_status[2];
    const unsigned changed_rows = ctx->adj_status[3];  // (a ray matrix fill's; short rows of a call that has to be run again anyway come last)
    ctx->adj_status[3] = 0;
    const unsigned misfits = ctx->adj_status[4];  // (an exact sum's pass S; the same)
    ctx->adj_status[4] = 0;
    if (refused) {
        int rc = drain(ctx);
        if (rc) return rc;
        rc = grow_entry_pools(ctx, std::min<int64_t>(2 * (ctx->slots[0].entry_capacity + refused) + 8192, kMaxEntryPool));
        if (rc) return rc;
        return fail(ctx, C5_RETRY, "%s: %u boundary entries found no room in the overflow pool (now %lld records): run it again",
                    ctx->adj_what, refused, static_cast<long long>(ctx->slots[0].entry_capacity));
    }
    if (lost_rays) return fail(ctx, C5_ERR_WALK, "%s: %u rays exceeded the walk step bound (malformed grid?)", ctx->adj_what, lost_rays);
    if (overlap_rays) {
        ctx->overlap_seen = true;  // (what the next frame would find out for itself: bin_sort_resolve from now on)
        ++ctx->setup_epoch;
        return fail(ctx, C5_RETRY,
                    "%s: %u rays met a boundary entry inside a stretch of cells they had walked: components of the grid "
                    "interpenetrate; run it again (bin_sort_resolve from now on)", ctx->adj_what, overlap_rays);
    }
    if (changed_rows)
        return fail(ctx, C5_ERR_STATE,
                    "%s: the frame changed between c5_ray_matrix_rows and c5_ray_matrix_fill: %u rows differ from row_ptr's or found no "
                    "room below capacity", ctx->adj_what, changed_rows);
    if (misfits)
        return fail(ctx, C5_ERR_INVALID,
                    "%s: %u contributions lie beyond their cell's exponent and were added nowhere: the exponents given are too small "
                    "(take the elementwise max of c5_render_exact_bounds - the vertex sums: c5_render_vertex_exact_bounds - over "
                    "every part of the image)", ctx->adj_what, misfits);
    return C5_OK;
}
}  // namespace c5api

namespace {

// What the forty derivative entry points check before anything else, in this order: the context; a batch's size; the
// call's own pointers (`required_ok`, and `per_cell_ok` where the grid has cells); no c5_render_host_async frame
// outstanding; and for the host-pointer forms the image, after which the device is bound.
struct DerivativeCall {
    const char* name;         // as the messages spell it: "c5_render_tangent_batch" also for its _device form
    bool host;                // a host-pointer form
    int n;                    // a batch's size (1: not a batch)
    const char* batch_of;     // "direction" / "upstream image"
    bool required_ok, per_cell_ok;
    const char* pointer_msg;
    bool refuse_async = true;
};

int check_derivative(c5_context* ctx, const DerivativeCall& c) {
    if (!ctx) return fail(nullptr, C5_ERR_INVALID, "null context");
    if (c.n < 1) return fail(ctx, C5_ERR_INVALID, "a batch needs at least one %s (%d)", c.batch_of, c.n);
    if (!c.required_ok || (ctx->n_cells > 0 && !c.per_cell_ok)) return fail(ctx, C5_ERR_INVALID, "%s", c.pointer_msg);
    if (c.refuse_async && ctx->hr_count) return fail(ctx, C5_ERR_STATE, "%s while c5_render_host_async frames are outstanding", c.name);
    if (!c.host) return C5_OK;
    if (!ctx->have_image) return fail(ctx, C5_ERR_STATE, "critical error. empty plane");  // plane.cpp:151-153
    return bind_device(ctx);
}

// One block of a host-pointer derivative call's staging buffer: uploaded from `src` before the work, downloaded to `dst`
// after it (either may be null).  dev: its place on the device, or nullptr where the caller gave neither - the enqueue
// then sees the null pointer the caller passed.
struct Staged {
    const void* src;
    void* dst;
    size_t bytes;
    char* dev = nullptr;
    template <class T>
    T* as() const { return reinterpret_cast<T*>(dev); }
};

// The host-pointer form of a derivative: the blocks laid out in deriv_io (256-byte aligned), the uploads on the context's
// stream, `enqueue` and c5_synchronize - again while the entry pool had to grow (C5_RETRY) - and the downloads.
template <size_t N, class Enqueue>
int run_staged(c5_context* ctx, const char* what, Staged (&blocks)[N], Enqueue enqueue) {
    auto room = [](const Staged& b) { return (b.bytes + 255) / 256 * 256; };
    size_t total = 0;
    for (const Staged& b : blocks) total += room(b);
    C5_HIP(ctx, ctx->deriv_io.ensure(total + 256));
    char* at = ctx->deriv_io.as<char>();
    for (Staged& b : blocks) {
        if (b.src || b.dst) b.dev = at;
        at += room(b);
        if (b.src && b.bytes > 0) C5_HIP(ctx, hipMemcpyAsync(b.dev, b.src, b.bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    for (int attempt = 0; attempt < 3; ++attempt) {
        int rc = enqueue();
        if (rc) return rc;
        rc = c5_synchronize(ctx);
        if (rc == C5_RETRY) continue;
        if (rc) return rc;
        for (const Staged& b : blocks)
            if (b.dst && b.bytes > 0) C5_HIP(ctx, hipMemcpy(b.dst, b.dev, b.bytes, hipMemcpyDeviceToHost));
        return C5_OK;
    }
    return fail(ctx, C5_ERR_STATE, "%s: entry buffer kept overflowing", what);
}

size_t cells_bytes(const c5_context* ctx) { return static_cast<size_t>(ctx->n_cells) * sizeof(double); }

// What c5_render_exact_bounds / _sums check of their kind and its inputs (`arrays_ok`: the call's own exponent and word
// arrays), in check_derivative's terms.
DerivativeCall exact_call(const char* name, bool host, int what, const void* d_alpha, const void* d_q, const void* image, bool arrays_ok) {
    const bool known = what == C5_EXACT_ADJOINT || what == C5_EXACT_GN_DIAGONAL || what == C5_EXACT_HVP;
    const bool dirs_ok = what == C5_EXACT_HVP ? (d_alpha || d_q) : (!d_alpha && !d_q);
    const bool image_ok = what == C5_EXACT_GN_DIAGONAL || image != nullptr;
    const char* const msg = !known      ? "unknown kind of exact sum: C5_EXACT_ADJOINT, C5_EXACT_GN_DIAGONAL or C5_EXACT_HVP"
                            : !dirs_ok  ? "directions belong to C5_EXACT_HVP alone (d_alpha, d_q or both); the other kinds take NULL"
                            : !image_ok ? "null upstream image"
                                        : "null exact bounds or sums pointer";
    return {name, host, 1, nullptr, known && dirs_ok && image_ok, arrays_ok, msg};
}
}  // namespace

extern "C" {

// The only derivative entry point that does not refuse while c5_render_host_async frames are outstanding (it never has).
int c5_render_adjoint_device(c5_context* ctx, const void* grad_out_device, void* grad_alpha_device, void* grad_q_device) {
    int rc = check_derivative(ctx, {"c5_render_adjoint", false, 1, nullptr, grad_out_device != nullptr,
                                    grad_alpha_device && grad_q_device, "null adjoint pointer", false});
    if (rc) return rc;
    return enqueue_adjoint(ctx, static_cast<const float2*>(grad_out_device), static_cast<double*>(grad_alpha_device),
                           static_cast<double*>(grad_q_device));
}

int c5_render_adjoint(c5_context* ctx, const float* grad_out_host, double* grad_alpha_host, double* grad_q_host) {
    int rc = check_derivative(ctx, {"c5_render_adjoint", true, 1, nullptr, grad_out_host != nullptr, grad_alpha_host && grad_q_host,
                                    "null adjoint pointer"});
    if (rc) return rc;
    Staged b[] = {{grad_out_host, nullptr, image_bytes(ctx)},
                  {nullptr, grad_alpha_host, cells_bytes(ctx)},
                  {nullptr, grad_q_host, cells_bytes(ctx)}};
    return run_staged(ctx, "adjoint", b, [&] {
        return enqueue_adjoint(ctx, b[0].as<const float2>(), b[1].as<double>(), b[2].as<double>());
    });
}

int c5_render_exact_bounds_device(c5_context* ctx, int what, const void* d_alpha_dev, const void* d_q_dev, const void* image_dev,
                                  void* exp_alpha_dev, void* exp_q_dev) {
    int rc = check_derivative(ctx, exact_call("c5_render_exact_bounds", false, what, d_alpha_dev, d_q_dev, image_dev, exp_alpha_dev && exp_q_dev));
    if (rc) return rc;
    return enqueue_exact_bounds(ctx, what, static_cast<const double*>(d_alpha_dev), static_cast<const double*>(d_q_dev),
                                static_cast<const float2*>(image_dev), static_cast<int32_t*>(exp_alpha_dev), static_cast<int32_t*>(exp_q_dev));
}

int c5_render_exact_bounds(c5_context* ctx, int what, const double* d_alpha_host, const double* d_q_host, const float* image_host,
                           int32_t* exp_alpha_host, int32_t* exp_q_host) {
    int rc = check_derivative(ctx, exact_call("c5_render_exact_bounds", true, what, d_alpha_host, d_q_host, image_host, exp_alpha_host && exp_q_host));
    if (rc) return rc;
    const size_t exp_bytes = static_cast<size_t>(ctx->n_cells) * sizeof(int32_t);
    Staged b[] = {{image_host, nullptr, image_bytes(ctx)},
                  {d_alpha_host, nullptr, cells_bytes(ctx)},
                  {d_q_host, nullptr, cells_bytes(ctx)},
                  {nullptr, exp_alpha_host, exp_bytes},
                  {nullptr, exp_q_host, exp_bytes}};
    return run_staged(ctx, kExactBoundsName[what], b, [&] {
        return enqueue_exact_bounds(ctx, what, b[1].as<const double>(), b[2].as<const double>(), b[0].as<const float2>(), b[3].as<int32_t>(),
                                    b[4].as<int32_t>());
    });
}

int c5_render_exact_sums_device(c5_context* ctx, int what, const void* d_alpha_dev, const void* d_q_dev, const void* image_dev,
                                const void* exp_alpha_dev, const void* exp_q_dev, void* sums_alpha_dev, void* sums_q_dev) {
    int rc = check_derivative(ctx, exact_call("c5_render_exact_sums", false, what, d_alpha_dev, d_q_dev, image_dev,
                                              exp_alpha_dev && exp_q_dev && sums_alpha_dev && sums_q_dev));
    if (rc) return rc;
    return enqueue_exact_sums(ctx, what, static_cast<const double*>(d_alpha_dev), static_cast<const double*>(d_q_dev),
                              static_cast<const float2*>(image_dev), static_cast<const int32_t*>(exp_alpha_dev),
                              static_cast<const int32_t*>(exp_q_dev), static_cast<int64_t*>(sums_alpha_dev), static_cast<int64_t*>(sums_q_dev));
}

int c5_render_exact_sums(c5_context* ctx, int what, const double* d_alpha_host, const double* d_q_host, const float* image_host,
                         const int32_t* exp_alpha_host, const int32_t* exp_q_host, int64_t* sums_alpha_host, int64_t* sums_q_host) {
    int rc = check_derivative(ctx, exact_call("c5_render_exact_sums", true, what, d_alpha_host, d_q_host, image_host,
                                              exp_alpha_host && exp_q_host && sums_alpha_host && sums_q_host));
    if (rc) return rc;
    const size_t exp_bytes = static_cast<size_t>(ctx->n_cells) * sizeof(int32_t), word_bytes = static_cast<size_t>(ctx->n_cells) * 2 * sizeof(int64_t);
    Staged b[] = {{image_host, nullptr, image_bytes(ctx)},
                  {d_alpha_host, nullptr, cells_bytes(ctx)},
                  {d_q_host, nullptr, cells_bytes(ctx)},
                  {exp_alpha_host, nullptr, exp_bytes},
                  {exp_q_host, nullptr, exp_bytes},
                  {nullptr, sums_alpha_host, word_bytes},
                  {nullptr, sums_q_host, word_bytes}};
    return run_staged(ctx, kExactSumsName[what], b, [&] {
        return enqueue_exact_sums(ctx, what, b[1].as<const double>(), b[2].as<const double>(), b[0].as<const float2>(),
                                  b[3].as<const int32_t>(), b[4].as<const int32_t>(), b[5].as<int64_t>(), b[6].as<int64_t>());
    });
}

// The adjoint's own pair: C5_EXACT_ADJOINT of the generic one.
int c5_render_adjoint_exact_bounds_device(c5_context* ctx, const void* grad_out_device, void* exp_alpha_device, void* exp_q_device) {
    return c5_render_exact_bounds_device(ctx, C5_EXACT_ADJOINT, nullptr, nullptr, grad_out_device, exp_alpha_device, exp_q_device);
}

int c5_render_adjoint_exact_bounds(c5_context* ctx, const float* grad_out_host, int32_t* exp_alpha_host, int32_t* exp_q_host) {
    return c5_render_exact_bounds(ctx, C5_EXACT_ADJOINT, nullptr, nullptr, grad_out_host, exp_alpha_host, exp_q_host);
}

int c5_render_adjoint_exact_sums_device(c5_context* ctx, const void* grad_out_device, const void* exp_alpha_device,
                                        const void* exp_q_device, void* sums_alpha_device, void* sums_q_device) {
    return c5_render_exact_sums_device(ctx, C5_EXACT_ADJOINT, nullptr, nullptr, grad_out_device, exp_alpha_device, exp_q_device,
                                       sums_alpha_device, sums_q_device);
}

int c5_render_adjoint_exact_sums(c5_context* ctx, const float* grad_out_host, const int32_t* exp_alpha_host, const int32_t* exp_q_host,
                                 int64_t* sums_alpha_host, int64_t* sums_q_host) {
    return c5_render_exact_sums(ctx, C5_EXACT_ADJOINT, nullptr, nullptr, grad_out_host, exp_alpha_host, exp_q_host, sums_alpha_host,
                                sums_q_host);
}

// A pure host function: no context, no GPU.
int c5_exact_sums_finish(const int32_t* exp, const int64_t* sums, int64_t n, int res_x, int res_y, double* out_fp64) {
    if (n < 0 || (n > 0 && (!exp || !sums || !out_fp64))) return fail(nullptr, C5_ERR_INVALID, "c5_exact_sums_finish: null pointer");
    if (res_x < 1 || res_y < 1) return fail(nullptr, C5_ERR_INVALID, "c5_exact_sums_finish: an image of %d x %d pixels", res_x, res_y);
    int m;
    if (const int rc = exact_word_bits(nullptr, res_x, res_y, m)) return rc;
    for (int64_t i = 0; i < n; ++i) out_fp64[i] = c5::exact::finish(exp[i], sums[2 * i], sums[2 * i + 1], m);
    return C5_OK;
}

// Testing: the host side of exact_sum.hpp's quantise.
int c5_exact_quantise(const double* x, int64_t n, int32_t exp, int res_x, int res_y, int64_t* words) {
    if (n < 0 || (n > 0 && (!x || !words)) || res_x < 1 || res_y < 1) return fail(nullptr, C5_ERR_INVALID, "c5_exact_quantise: bad arguments");
    int m;
    if (const int rc = exact_word_bits(nullptr, res_x, res_y, m)) return rc;
    int64_t misfits = 0;
    for (int64_t i = 0; i < n; ++i) misfits += !c5::exact::quantise(x[i], exp, m, words[2 * i], words[2 * i + 1]);
    if (misfits)
        return fail(nullptr, C5_ERR_INVALID, "c5_exact_quantise: %lld values lie beyond the exponent %d", static_cast<long long>(misfits),
                    static_cast<int>(exp));
    return C5_OK;
}

int c5_render_tangent_device(c5_context* ctx, const void* d_alpha_dev, const void* d_q_dev, void* out_device) {
    int rc = check_derivative(ctx, {"c5_render_tangent", false, 1, nullptr, out_device != nullptr, true, "null output pointer"});
    if (rc) return rc;
    return enqueue_tangent(ctx, static_cast<const double*>(d_alpha_dev), static_cast<const double*>(d_q_dev),
                           static_cast<float2*>(out_device));
}

int c5_render_tangent(c5_context* ctx, const double* d_alpha_host, const double* d_q_host, float* out_host) {
    int rc = check_derivative(ctx, {"c5_render_tangent", true, 1, nullptr, out_host != nullptr, true, "null output pointer"});
    if (rc) return rc;
    Staged b[] = {{d_alpha_host, nullptr, cells_bytes(ctx)},
                  {d_q_host, nullptr, cells_bytes(ctx)},
                  {nullptr, out_host, image_bytes(ctx)}};
    return run_staged(ctx, "tangent", b, [&] {
        return enqueue_tangent(ctx, b[0].as<const double>(), b[1].as<const double>(), b[2].as<float2>());
    });
}

int c5_render_tangent_batch_device(c5_context* ctx, int n_dirs, const void* d_alpha_dev, const void* d_q_dev, void* out_dev) {
    int rc = check_derivative(ctx, {"c5_render_tangent_batch", false, n_dirs, "direction", out_dev != nullptr, true,
                                    "null output pointer"});
    if (rc) return rc;
    return enqueue_tangent_batch(ctx, n_dirs, static_cast<const double*>(d_alpha_dev), static_cast<const double*>(d_q_dev),
                                 static_cast<float2*>(out_dev));
}

int c5_render_tangent_batch(c5_context* ctx, int n_dirs, const double* d_alpha_host, const double* d_q_host, float* out_host) {
    int rc = check_derivative(ctx, {"c5_render_tangent_batch", true, n_dirs, "direction", out_host != nullptr, true,
                                    "null output pointer"});
    if (rc) return rc;
    const size_t dir_bytes = n_dirs * cells_bytes(ctx);
    Staged b[] = {{d_alpha_host, nullptr, dir_bytes},
                  {d_q_host, nullptr, dir_bytes},
                  {nullptr, out_host, n_dirs * image_bytes(ctx)}};
    return run_staged(ctx, "tangent batch", b, [&] {
        return enqueue_tangent_batch(ctx, n_dirs, b[0].as<const double>(), b[1].as<const double>(), b[2].as<float2>());
    });
}

int c5_render_adjoint_batch_device(c5_context* ctx, int n_imgs, const void* grad_out_dev, void* grad_alpha_dev, void* grad_q_dev) {
    int rc = check_derivative(ctx, {"c5_render_adjoint_batch", false, n_imgs, "upstream image", grad_out_dev != nullptr,
                                    grad_alpha_dev && grad_q_dev, "null adjoint pointer"});
    if (rc) return rc;
    return enqueue_adjoint_batch(ctx, n_imgs, static_cast<const float2*>(grad_out_dev), static_cast<double*>(grad_alpha_dev),
                                 static_cast<double*>(grad_q_dev));
}

int c5_render_adjoint_batch(c5_context* ctx, int n_imgs, const float* grad_out_host, double* grad_alpha_host, double* grad_q_host) {
    int rc = check_derivative(ctx, {"c5_render_adjoint_batch", true, n_imgs, "upstream image", grad_out_host != nullptr,
                                    grad_alpha_host && grad_q_host, "null adjoint pointer"});
    if (rc) return rc;
    const size_t grad_bytes = n_imgs * cells_bytes(ctx);
    Staged b[] = {{grad_out_host, nullptr, n_imgs * image_bytes(ctx)},
                  {nullptr, grad_alpha_host, grad_bytes},
                  {nullptr, grad_q_host, grad_bytes}};
    return run_staged(ctx, "adjoint batch", b, [&] {
        return enqueue_adjoint_batch(ctx, n_imgs, b[0].as<const float2>(), b[1].as<double>(), b[2].as<double>());
    });
}

int c5_render_gn_product_device(c5_context* ctx, int n_dirs, const void* d_alpha_dev, const void* d_q_dev, const void* weight_dev,
                                void* h_alpha_dev, void* h_q_dev, void* jv_out_dev) {
    int rc = check_derivative(ctx, {"c5_render_gn_product", false, n_dirs, "direction", h_alpha_dev || h_q_dev, true,
                                    "null output pointers: give h_alpha, h_q or both"});
    if (rc) return rc;
    return enqueue_gn_product(ctx, n_dirs, static_cast<const double*>(d_alpha_dev), static_cast<const double*>(d_q_dev),
                              static_cast<const float2*>(weight_dev), static_cast<double*>(h_alpha_dev), static_cast<double*>(h_q_dev),
                              static_cast<float2*>(jv_out_dev));
}

int c5_render_gn_product(c5_context* ctx, int n_dirs, const double* d_alpha_host, const double* d_q_host, const float* weight_host,
                         double* h_alpha_host, double* h_q_host, float* jv_out_host) {
    int rc = check_derivative(ctx, {"c5_render_gn_product", true, n_dirs, "direction", h_alpha_host || h_q_host, true,
                                    "null output pointers: give h_alpha, h_q or both"});
    if (rc) return rc;
    const size_t dir_bytes = n_dirs * cells_bytes(ctx);
    Staged b[] = {{weight_host, nullptr, image_bytes(ctx)},
                  {d_alpha_host, nullptr, dir_bytes},
                  {d_q_host, nullptr, dir_bytes},
                  {nullptr, h_alpha_host, dir_bytes},
                  {nullptr, h_q_host, dir_bytes},
                  {nullptr, jv_out_host, n_dirs * image_bytes(ctx)}};
    return run_staged(ctx, "gn product", b, [&] {
        return enqueue_gn_product(ctx, n_dirs, b[1].as<const double>(), b[2].as<const double>(), b[0].as<const float2>(),
                                  b[3].as<double>(), b[4].as<double>(), b[5].as<float2>());
    });
}

int c5_render_gn_diagonal_device(c5_context* ctx, const void* weight_dev, void* diag_alpha_dev, void* diag_q_dev) {
    int rc = check_derivative(ctx, {"c5_render_gn_diagonal", false, 1, nullptr, true, diag_alpha_dev && diag_q_dev,
                                    "null diagonal pointer"});
    if (rc) return rc;
    return enqueue_gn_diagonal(ctx, static_cast<const float2*>(weight_dev), static_cast<double*>(diag_alpha_dev),
                               static_cast<double*>(diag_q_dev));
}

int c5_render_gn_diagonal(c5_context* ctx, const float* weight_host, double* diag_alpha_host, double* diag_q_host) {
    int rc = check_derivative(ctx, {"c5_render_gn_diagonal", true, 1, nullptr, true, diag_alpha_host && diag_q_host,
                                    "null diagonal pointer"});
    if (rc) return rc;
    Staged b[] = {{weight_host, nullptr, image_bytes(ctx)},
                  {nullptr, diag_alpha_host, cells_bytes(ctx)},
                  {nullptr, diag_q_host, cells_bytes(ctx)}};
    return run_staged(ctx, "gn diagonal", b, [&] {
        return enqueue_gn_diagonal(ctx, b[0].as<const float2>(), b[1].as<double>(), b[2].as<double>());
    });
}

int c5_render_hvp_device(c5_context* ctx, const void* d_alpha_dev, const void* d_q_dev, const void* grad_out_dev, void* h_alpha_dev,
                         void* h_q_dev) {
    int rc = check_derivative(ctx, {"c5_render_hvp", false, 1, nullptr,
                                    grad_out_dev && (d_alpha_dev || d_q_dev) && (h_alpha_dev || h_q_dev), true,
                                    "null hvp pointer: give grad_out, d_alpha or d_q (or both), and h_alpha or h_q (or both)"});
    if (rc) return rc;
    return enqueue_hvp(ctx, static_cast<const double*>(d_alpha_dev), static_cast<const double*>(d_q_dev),
                       static_cast<const float2*>(grad_out_dev), static_cast<double*>(h_alpha_dev), static_cast<double*>(h_q_dev));
}

int c5_render_hvp(c5_context* ctx, const double* d_alpha_host, const double* d_q_host, const float* grad_out_host, double* h_alpha_host,
                  double* h_q_host) {
    int rc = check_derivative(ctx, {"c5_render_hvp", true, 1, nullptr,
                                    grad_out_host && (d_alpha_host || d_q_host) && (h_alpha_host || h_q_host), true,
                                    "null hvp pointer: give grad_out, d_alpha or d_q (or both), and h_alpha or h_q (or both)"});
    if (rc) return rc;
    Staged b[] = {{grad_out_host, nullptr, image_bytes(ctx)},
                  {d_alpha_host, nullptr, cells_bytes(ctx)},
                  {d_q_host, nullptr, cells_bytes(ctx)},
                  {nullptr, h_alpha_host, cells_bytes(ctx)},
                  {nullptr, h_q_host, cells_bytes(ctx)}};
    return run_staged(ctx, "hvp", b, [&] {
        return enqueue_hvp(ctx, b[1].as<const double>(), b[2].as<const double>(), b[0].as<const float2>(), b[3].as<double>(),
                           b[4].as<double>());
    });
}

// The fields are host memory in both forms: they travel as kernel arguments.
int c5_render_motion_tangent_device(c5_context* ctx, int n_dirs, const double* fields_host, void* out_dev) {
    int rc = check_derivative(ctx, {"c5_render_motion_tangent", false, n_dirs, "field", fields_host && out_dev, true,
                                    "null field or output pointer"});
    if (rc) return rc;
    return enqueue_motion(ctx, n_dirs, fields_host, static_cast<float2*>(out_dev));
}

int c5_render_motion_tangent(c5_context* ctx, int n_dirs, const double* fields_host, float* out_host) {
    int rc = check_derivative(ctx, {"c5_render_motion_tangent", true, n_dirs, "field", fields_host && out_host, true,
                                    "null field or output pointer"});
    if (rc) return rc;
    Staged b[] = {{nullptr, out_host, n_dirs * image_bytes(ctx)}};
    return run_staged(ctx, "motion tangent", b, [&] { return enqueue_motion(ctx, n_dirs, fields_host, b[0].as<float2>()); });
}

int c5_render_vertex_adjoint_device(c5_context* ctx, const void* grad_out_dev, void* grad_xyz_dev) {
    int rc = check_derivative(ctx, {"c5_render_vertex_adjoint", false, 1, nullptr, grad_out_dev && grad_xyz_dev, true,
                                    "null vertex adjoint pointer"});
    if (rc) return rc;
    return enqueue_vertex_adjoint(ctx, static_cast<const float2*>(grad_out_dev), static_cast<double*>(grad_xyz_dev));
}

int c5_render_vertex_adjoint(c5_context* ctx, const float* grad_out_host, double* grad_xyz_host) {
    int rc = check_derivative(ctx, {"c5_render_vertex_adjoint", true, 1, nullptr, grad_out_host && grad_xyz_host, true,
                                    "null vertex adjoint pointer"});
    if (rc) return rc;
    Staged b[] = {{grad_out_host, nullptr, image_bytes(ctx)},
                  {nullptr, grad_xyz_host, 3 * static_cast<size_t>(ctx->n_pts) * sizeof(double)}};
    return run_staged(ctx, "vertex adjoint", b, [&] { return enqueue_vertex_adjoint(ctx, b[0].as<const float2>(), b[1].as<double>()); });
}

int c5_render_vertex_adjoint_batch_device(c5_context* ctx, int n_imgs, const void* grad_out_dev, void* grad_xyz_dev) {
    int rc = check_derivative(ctx, {"c5_render_vertex_adjoint_batch", false, n_imgs, "upstream image", grad_out_dev && grad_xyz_dev, true,
                                    "null vertex adjoint pointer"});
    if (rc) return rc;
    return enqueue_vertex_adjoint_batch(ctx, n_imgs, static_cast<const float2*>(grad_out_dev), static_cast<double*>(grad_xyz_dev));
}

int c5_render_vertex_adjoint_batch(c5_context* ctx, int n_imgs, const float* grad_out_host, double* grad_xyz_host) {
    int rc = check_derivative(ctx, {"c5_render_vertex_adjoint_batch", true, n_imgs, "upstream image", grad_out_host && grad_xyz_host, true,
                                    "null vertex adjoint pointer"});
    if (rc) return rc;
    Staged b[] = {{grad_out_host, nullptr, n_imgs * image_bytes(ctx)},
                  {nullptr, grad_xyz_host, 3 * static_cast<size_t>(n_imgs) * static_cast<size_t>(ctx->n_pts) * sizeof(double)}};
    return run_staged(ctx, "vertex adjoint batch", b,
                      [&] { return enqueue_vertex_adjoint_batch(ctx, n_imgs, b[0].as<const float2>(), b[1].as<double>()); });
}

// The exact vertex adjoint's staged calls ("vertex_exact" makes c5_render_vertex_adjoint* return them finished).
int c5_render_vertex_exact_bounds_device(c5_context* ctx, const void* grad_out_dev, void* exps_dev) {
    int rc = check_derivative(ctx, {"c5_render_vertex_exact_bounds", false, 1, nullptr, grad_out_dev != nullptr, exps_dev != nullptr,
                                    "null upstream image or exponent pointer"});
    if (rc) return rc;
    return enqueue_vertex_exact_bounds(ctx, static_cast<const float2*>(grad_out_dev), static_cast<int32_t*>(exps_dev));
}

int c5_render_vertex_exact_bounds(c5_context* ctx, const float* grad_out_host, int32_t* exps_host) {
    int rc = check_derivative(ctx, {"c5_render_vertex_exact_bounds", true, 1, nullptr, grad_out_host != nullptr, exps_host != nullptr,
                                    "null upstream image or exponent pointer"});
    if (rc) return rc;
    Staged b[] = {{grad_out_host, nullptr, image_bytes(ctx)},
                  {nullptr, exps_host, 12 * static_cast<size_t>(ctx->n_cells) * sizeof(int32_t)}};
    return run_staged(ctx, "vertex exact bounds", b,
                      [&] { return enqueue_vertex_exact_bounds(ctx, b[0].as<const float2>(), b[1].as<int32_t>()); });
}

int c5_render_vertex_exact_sums_device(c5_context* ctx, const void* grad_out_dev, const void* exps_dev, void* sums_dev) {
    int rc = check_derivative(ctx, {"c5_render_vertex_exact_sums", false, 1, nullptr, grad_out_dev != nullptr, exps_dev && sums_dev,
                                    "null upstream image, exponent or sums pointer"});
    if (rc) return rc;
    return enqueue_vertex_exact_sums(ctx, static_cast<const float2*>(grad_out_dev), static_cast<const int32_t*>(exps_dev),
                                     static_cast<int64_t*>(sums_dev));
}

int c5_render_vertex_exact_sums(c5_context* ctx, const float* grad_out_host, const int32_t* exps_host, int64_t* sums_host) {
    int rc = check_derivative(ctx, {"c5_render_vertex_exact_sums", true, 1, nullptr, grad_out_host != nullptr, exps_host && sums_host,
                                    "null upstream image, exponent or sums pointer"});
    if (rc) return rc;
    const size_t slots = 12 * static_cast<size_t>(ctx->n_cells);
    Staged b[] = {{grad_out_host, nullptr, image_bytes(ctx)},
                  {exps_host, nullptr, slots * sizeof(int32_t)},
                  {nullptr, sums_host, slots * 2 * sizeof(int64_t)}};
    return run_staged(ctx, "vertex exact sums", b, [&] {
        return enqueue_vertex_exact_sums(ctx, b[0].as<const float2>(), b[1].as<const int32_t>(), b[2].as<int64_t>());
    });
}

int c5_vertex_exact_finish_device(c5_context* ctx, const void* exps_dev, const void* sums_dev, void* grad_xyz_dev) {
    int rc = check_derivative(ctx, {"c5_vertex_exact_finish", false, 1, nullptr, grad_xyz_dev != nullptr, exps_dev && sums_dev,
                                    "null exponent, sums or gradient pointer"});
    if (rc) return rc;
    return enqueue_vertex_exact_finish(ctx, static_cast<const int32_t*>(exps_dev), static_cast<const int64_t*>(sums_dev),
                                       static_cast<double*>(grad_xyz_dev));
}

int c5_vertex_exact_finish(c5_context* ctx, const int32_t* exps_host, const int64_t* sums_host, double* grad_xyz_host) {
    int rc = check_derivative(ctx, {"c5_vertex_exact_finish", true, 1, nullptr, grad_xyz_host != nullptr, exps_host && sums_host,
                                    "null exponent, sums or gradient pointer"});
    if (rc) return rc;
    const size_t slots = 12 * static_cast<size_t>(ctx->n_cells);
    Staged b[] = {{exps_host, nullptr, slots * sizeof(int32_t)},
                  {sums_host, nullptr, slots * 2 * sizeof(int64_t)},
                  {nullptr, grad_xyz_host, 3 * static_cast<size_t>(ctx->n_pts) * sizeof(double)}};
    return run_staged(ctx, "vertex exact finish", b, [&] {
        return enqueue_vertex_exact_finish(ctx, b[0].as<const int32_t>(), b[1].as<const int64_t>(), b[2].as<double>());
    });
}

int c5_render_vertex_tangent_device(c5_context* ctx, int n_dirs, const void* d_xyz_dev, void* out_dev) {
    int rc = check_derivative(ctx, {"c5_render_vertex_tangent", false, n_dirs, "displacement field", d_xyz_dev && out_dev, true,
                                    "null displacement or output pointer"});
    if (rc) return rc;
    return enqueue_vertex_tangent(ctx, n_dirs, static_cast<const double*>(d_xyz_dev), static_cast<float2*>(out_dev));
}

int c5_render_vertex_tangent(c5_context* ctx, int n_dirs, const double* d_xyz_host, float* out_host) {
    int rc = check_derivative(ctx, {"c5_render_vertex_tangent", true, n_dirs, "displacement field", d_xyz_host && out_host, true,
                                    "null displacement or output pointer"});
    if (rc) return rc;
    Staged b[] = {{d_xyz_host, nullptr, 3 * static_cast<size_t>(n_dirs) * static_cast<size_t>(ctx->n_pts) * sizeof(double)},
                  {nullptr, out_host, n_dirs * image_bytes(ctx)}};
    return run_staged(ctx, "vertex tangent", b,
                      [&] { return enqueue_vertex_tangent(ctx, n_dirs, b[0].as<const double>(), b[1].as<float2>()); });
}

int c5_render_vertex_gn_product_device(c5_context* ctx, int n_dirs, const void* d_xyz_dev, const void* weight_dev, void* h_xyz_dev,
                                       void* jv_out_dev) {
    int rc = check_derivative(ctx, {"c5_render_vertex_gn_product", false, n_dirs, "displacement field", d_xyz_dev && h_xyz_dev, true,
                                    "null displacement or output pointer"});
    if (rc) return rc;
    return enqueue_vertex_gn_product(ctx, n_dirs, static_cast<const double*>(d_xyz_dev), static_cast<const float2*>(weight_dev),
                                     static_cast<double*>(h_xyz_dev), static_cast<float2*>(jv_out_dev));
}

int c5_render_vertex_gn_product(c5_context* ctx, int n_dirs, const double* d_xyz_host, const float* weight_host, double* h_xyz_host,
                                float* jv_out_host) {
    int rc = check_derivative(ctx, {"c5_render_vertex_gn_product", true, n_dirs, "displacement field", d_xyz_host && h_xyz_host, true,
                                    "null displacement or output pointer"});
    if (rc) return rc;
    const size_t field_bytes = 3 * static_cast<size_t>(n_dirs) * static_cast<size_t>(ctx->n_pts) * sizeof(double);
    Staged b[] = {{weight_host, nullptr, image_bytes(ctx)},
                  {d_xyz_host, nullptr, field_bytes},
                  {nullptr, h_xyz_host, field_bytes},
                  {nullptr, jv_out_host, n_dirs * image_bytes(ctx)}};
    return run_staged(ctx, "vertex gn product", b, [&] {
        return enqueue_vertex_gn_product(ctx, n_dirs, b[1].as<const double>(), b[0].as<const float2>(), b[2].as<double>(), b[3].as<float2>());
    });
}

// Waits for the stream: *nnz is valid on return.
int c5_ray_matrix_rows_device(c5_context* ctx, void* row_ptr_dev, int64_t* nnz) {
    int rc = check_derivative(ctx, {"c5_ray_matrix_rows", false, 1, nullptr, row_ptr_dev && nnz, true, "null row_ptr or nnz pointer"});
    if (rc) return rc;
    *nnz = 0;
    int64_t* const row_ptr = static_cast<int64_t*>(row_ptr_dev);
    rc = enqueue_ray_matrix_rows(ctx, row_ptr);
    if (rc) return rc;
    C5_HIP(ctx, hipMemcpyAsync(nnz, row_ptr + local_pixels(ctx->im), sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    return c5_synchronize(ctx);
}

int c5_ray_matrix_rows(c5_context* ctx, int64_t* row_ptr_host, int64_t* nnz) {
    int rc = check_derivative(ctx, {"c5_ray_matrix_rows", true, 1, nullptr, row_ptr_host && nnz, true, "null row_ptr or nnz pointer"});
    if (rc) return rc;
    *nnz = 0;
    const int64_t n_px = local_pixels(ctx->im);
    Staged b[] = {{nullptr, row_ptr_host, static_cast<size_t>(n_px + 1) * sizeof(int64_t)}};
    rc = run_staged(ctx, "ray matrix rows", b, [&] { return enqueue_ray_matrix_rows(ctx, b[0].as<int64_t>()); });
    if (rc) return rc;
    *nnz = row_ptr_host[n_px];
    return C5_OK;
}

int c5_ray_matrix_fill_device(c5_context* ctx, const void* row_ptr_dev, int64_t capacity, void* col_dev, void* dz_dev, void* z_exit_dev) {
    int rc = check_derivative(ctx, {"c5_ray_matrix_fill", false, 1, nullptr, row_ptr_dev && col_dev && dz_dev, true,
                                    "null row_ptr, col or dz pointer"});
    if (rc) return rc;
    if (capacity < 0) return fail(ctx, C5_ERR_INVALID, "c5_ray_matrix_fill: negative capacity (%lld)", static_cast<long long>(capacity));
    return enqueue_ray_matrix_fill(ctx, static_cast<const int64_t*>(row_ptr_dev), capacity, static_cast<int32_t*>(col_dev),
                                   static_cast<double*>(dz_dev), static_cast<double*>(z_exit_dev));
}

// The arrays are staged for row_ptr's total, which is also the capacity the kernel is given: nothing beyond it is written
// on the device or copied back.
int c5_ray_matrix_fill(c5_context* ctx, const int64_t* row_ptr_host, int64_t capacity, int32_t* col_host, double* dz_host,
                       double* z_exit_host) {
    int rc = check_derivative(ctx, {"c5_ray_matrix_fill", true, 1, nullptr, row_ptr_host && col_host && dz_host, true,
                                    "null row_ptr, col or dz pointer"});
    if (rc) return rc;
    if (capacity < 0) return fail(ctx, C5_ERR_INVALID, "c5_ray_matrix_fill: negative capacity (%lld)", static_cast<long long>(capacity));
    const int64_t n_px = local_pixels(ctx->im), need = row_ptr_host[n_px];
    if (need < 0 || need > capacity)
        return fail(ctx, C5_ERR_INVALID, "c5_ray_matrix_fill: row_ptr asks for %lld elements, capacity is %lld", static_cast<long long>(need),
                    static_cast<long long>(capacity));
    const size_t n = static_cast<size_t>(need);
    Staged b[] = {{row_ptr_host, nullptr, static_cast<size_t>(n_px + 1) * sizeof(int64_t)},
                  {nullptr, col_host, n * sizeof(int32_t)},
                  {nullptr, dz_host, n * sizeof(double)},
                  {nullptr, z_exit_host, z_exit_host ? n * sizeof(double) : 0}};
    return run_staged(ctx, "ray matrix fill", b, [&] {
        return enqueue_ray_matrix_fill(ctx, b[0].as<const int64_t>(), need, b[1].as<int32_t>(), b[2].as<double>(), b[3].as<double>());
    });
}

// Host only.  The view is p -> R_n(... R_1(p)), R_k(p) = M_k (p - o_k) + o_k (axis 0: about the x axis, o = 0; axis 1: about
// the line x = x0, z = 0).  With s the point after rotation `index` and L = R_n ... R_{index+1} = (M_L, t_L) the rest:
//   d s / d angle = G (s - o), G = M' M^T the generator (axis 0: (0, -z, y); axis 1: (-z, 0, x - x0));
//   d s / d x0    = (I - M) e_x = (1 - cos, 0, -sin)  (axis 1; axis 0 has no x0: the zero field);
// and in view space, s = M_L^T (p - t_L): u(p) = M_L G M_L^T (p - t_L) - M_L G o, or the constant M_L d.
int c5_rotation_motion(const c5_rotation* rots, int n_rots, int index, int what, double field[12]) {
    if (!rots || !field || n_rots < 1 || n_rots > c5::kMaxRotations || index < 0 || index >= n_rots || (what != 0 && what != 1))
        return fail(nullptr, C5_ERR_INVALID, "c5_rotation_motion: bad rotation list, index or what");
    for (int k = 0; k < n_rots; ++k)
        if (rots[k].axis != 0 && rots[k].axis != 1) return fail(nullptr, C5_ERR_INVALID, "rotation axis must be 0 (x) or 1 (y)");
    double M[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}}, t[3] = {0, 0, 0};  // L so far: p -> M p + t
    for (int k = index + 1; k < n_rots; ++k) {
        const double c = std::cos(rots[k].angle), s = std::sin(rots[k].angle), x0 = rots[k].axis == 1 ? rots[k].x0 : 0.0;
        const int i = rots[k].axis == 0 ? 1 : 0;  // the rotation mixes rows i and 2: (r_i, r_2) <- (c r_i - s r_2, s r_i + c r_2)
        t[0] -= x0;
        for (int j = 0; j < 3; ++j) {
            const double a = M[i][j], b = M[2][j];
            M[i][j] = c * a - s * b;
            M[2][j] = s * a + c * b;
        }
        const double a = t[i], b = t[2];
        t[i] = c * a - s * b;
        t[2] = s * a + c * b;
        t[0] += x0;
    }
    const c5_rotation& r = rots[index];
    double A[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, bb[3] = {0, 0, 0};
    if (what == 0) {
        const int i = r.axis == 0 ? 1 : 0;  // G: u_i = -s_2, u_2 = s_i - o_i
        const double o[3] = {r.axis == 1 ? r.x0 : 0.0, 0.0, 0.0};
        double MG[3][3];  // M G: column 2 = -M[:, i], column i = M[:, 2]
        for (int a = 0; a < 3; ++a)
            for (int j = 0; j < 3; ++j) MG[a][j] = j == 2 ? -M[a][i] : (j == i ? M[a][2] : 0.0);
        for (int a = 0; a < 3; ++a)
            for (int j = 0; j < 3; ++j) A[a][j] = MG[a][0] * M[j][0] + MG[a][1] * M[j][1] + MG[a][2] * M[j][2];
        for (int a = 0; a < 3; ++a)
            bb[a] = -(A[a][0] * t[0] + A[a][1] * t[1] + A[a][2] * t[2]) - (MG[a][0] * o[0] + MG[a][1] * o[1] + MG[a][2] * o[2]);
    } else if (r.axis == 1) {
        const double d[3] = {1.0 - std::cos(r.angle), 0.0, -std::sin(r.angle)};
        for (int a = 0; a < 3; ++a) bb[a] = M[a][0] * d[0] + M[a][1] * d[1] + M[a][2] * d[2];
    }
    for (int a = 0; a < 3; ++a) {
        for (int j = 0; j < 3; ++j) field[3 * a + j] = A[a][j];
        field[9 + a] = bb[a];
    }
    return C5_OK;
}

}  // extern "C"

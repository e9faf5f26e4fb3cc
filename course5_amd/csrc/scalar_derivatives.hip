// ------------------------------------------------------------------------------------------
// Derivative renders in the cells' scalars (scalar_derivative_kernels.hip): the adjoint, the tangent, their batches, the
// Gauss-Newton product and diagonal, the Hessian-vector render and the exact sums of all of them - the enqueue functions
// over derivative_host.hpp and, next to them, their entry points.
// ------------------------------------------------------------------------------------------
#include "derivative_host.hpp"
#include "exact_sum.hpp"

using namespace c5api;

namespace {

// One adjoint over the view: the per-cell sums zeroed, two passes of the walk (or the resolve over bin_sort_resolve's
// lists), and the permutation into the caller's order.  squared: the Gauss-Newton diagonal's kernels, `weights` may
// then be null (ones).
int adjoint_one(c5_context* ctx, DerivativeView& v, bool squared, const float2* weights, double* ga_out, double* gq_out) {
    const size_t n_cells = static_cast<size_t>(ctx->n_cells);
    C5_HIP(ctx, ctx->deriv.adj_grad.ensure(2 * n_cells * sizeof(double)));
    double* const ga_dev = ctx->deriv.adj_grad.as<double>();
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
        v.keep(false);  // (the second pass hands every head back cleared)
        if (squared) c5::launch_gn_diag_walk(v.s, ap);
        else c5::launch_adjoint_walk(v.s, ap, 2);
    }
    c5::launch_adjoint_permute(v.s, ga_dev, gq_dev, v.perm, ctx->n_cells, ga_out, gq_out);
    return C5_OK;
}

// The exact sums' buffer over the context's cells - 40 bytes per cell and the misfit word, allocated here at the first
// exact call - with the word width of the WHOLE image (c5_set_image): the same for every rank of a split.
int exact_sums(c5_context* ctx, c5::ExactSums& x) {
    const size_t n_cells = static_cast<size_t>(ctx->n_cells);
    int m;
    if (const int rc = exact_word_bits(ctx, ctx->im.res_x, ctx->im.res_y, m)) return rc;
    C5_HIP(ctx, ctx->deriv.adj_exact.ensure(n_cells * 40 + 8));
    x = c5::ExactSums{};
    x.words = ctx->deriv.adj_exact.as<long long>();
    x.exps = reinterpret_cast<int2*>(x.words + 4 * n_cells);
    x.misfits = reinterpret_cast<unsigned*>(x.exps + n_cells);
    x.word_bits = m;
    return C5_OK;
}

void clear_exact(const DerivativeView& v, const c5::ExactSums& x, int64_t n_cells, unsigned flags) {
    c5::launch_exact_clear(v.s, x, n_cells, flags & kBounds, flags & kSums, (flags & kSums) && (flags & kFirst));
}

// exact_passes' family of the adjoint, and (kSquared) of the Gauss-Newton diagonal: the weights may then be null (ones)
template <bool kSquared>
struct AdjointExact {
    using Sums = c5::ExactSums;
    c5::AdjointParams ap{};  // (on the lists: grad_out alone)
    int init(c5_context* ctx, const DerivativeView& v, const float2* weights) {
        if (!v.bin_sort)
            if (const int rc = adjoint_params(ctx, v, ap)) return rc;
        ap.grad_out = weights;
        return C5_OK;
    }
    void clear(const DerivativeView& v, const Sums& x, int64_t n_cells, unsigned flags) const { clear_exact(v, x, n_cells, flags); }
    void pass1(const DerivativeView& v) const { c5::launch_adjoint_walk(v.s, ap, 1); }
    void walk(const DerivativeView& v, const Sums& x, bool sums) const {
        (kSquared ? c5::launch_gn_diag_exact_walk : c5::launch_adjoint_exact_walk)(v.s, ap, x, sums);
    }
    void resolve(const DerivativeView& v, const Sums& x, bool sums) const {
        (kSquared ? c5::launch_gn_diag_exact_resolve : c5::launch_adjoint_exact_resolve)(v.s, v.r, ap.grad_out, x, sums);
    }
};

template <bool kSquared>
int adjoint_exact_passes(c5_context* ctx, DerivativeView& v, const c5::ExactSums& x, const float2* weights, unsigned flags) {
    AdjointExact<kSquared> f;
    if (const int rc = f.init(ctx, v, weights)) return rc;
    exact_passes(ctx, v, f, x, flags);
    return C5_OK;
}

// "adjoint_exact" / "exact_sums": images k0 .. k0 + n - 1 of a call of n_total upstream images (g: image k0) -> rows k0 ..
// of ga_out / gq_out [n_total][n_cells] (a null output is not written), every image through passes E and S and the
// finish, one after the other (the host loop "algorithm" 1 uses for its batches); pass 1 runs once, before the call's first
// image - or not at all where Lambda is there (`have_lambda`: the Gauss-Newton product's pass A left it).  The call's
// last image hands the heads back cleared; the caller commits (commit_exact).
int exact_images(c5_context* ctx, DerivativeView& v, const c5::ExactSums& x, int n, const float2* g, double* ga_out, double* gq_out,
                 bool have_lambda = false, int k0 = 0, int n_total = -1) {
    if (n_total < 0) n_total = n;
    const int64_t n_cells = ctx->n_cells;
    for (int j = 0; j < n; ++j) {
        const int k = k0 + j;
        if (const int rc = adjoint_exact_passes<false>(ctx, v, x, g + j * v.n_px, exact_image_flags(k, n_total, have_lambda))) return rc;
        c5::launch_exact_finish(v.s, x, v.perm, n_cells, row_of(ga_out, k, n_cells), row_of(gq_out, k, n_cells));
    }
    return C5_OK;
}

// ... as a whole call: the sums' buffer, the n images, the commit
int enqueue_exact_images(c5_context* ctx, DerivativeView& v, int n, const float2* grad_out, double* ga_out, double* gq_out, const char* what) {
    c5::ExactSums x;
    int rc = exact_sums(ctx, x);
    if (!rc) rc = exact_images(ctx, v, x, n, grad_out, ga_out, gq_out);
    return rc ? rc : commit_exact(ctx, v, x.misfits, what);
}

// The Hessian-vector render's parameters: the direction into device order (the tangent's buffer: the gather is launched
// here) and, over the view's walk, Lambda's and Lambda_dot's buffers (pass 1 -> pass 2); where the sums go is the caller's
// to fill in.  On bin_sort_resolve's lists hvp_resolve takes hp.dir and hp.grad_out alone.
int hvp_params(c5_context* ctx, const DerivativeView& v, const double* d_alpha, const double* d_q, const float2* grad_out,
               c5::HvpParams& hp) {
    DerivativeState& d = ctx->deriv;
    C5_HIP(ctx, d.tan_dir.ensure(static_cast<size_t>(ctx->n_cells) * sizeof(double2)));
    hp = c5::HvpParams{};
    hp.dir = d.tan_dir.as<double2>();
    c5::launch_tangent_gather(v.s, d_alpha, d_q, v.perm, ctx->n_cells, d.tan_dir.as<double2>());
    hp.grad_out = grad_out;
    if (v.bin_sort) return C5_OK;
    C5_HIP(ctx, d.adj_lambda.ensure(static_cast<size_t>(v.padded) * sizeof(double)));
    C5_HIP(ctx, d.hvp_lambda_dot.ensure(static_cast<size_t>(v.padded) * sizeof(double)));
    hp.w = v.w;
    hp.lambda = d.adj_lambda.as<double>();
    hp.lambda_dot = d.hvp_lambda_dot.as<double>();
    return C5_OK;
}

// exact_passes' family of the Hessian-vector render: pass 1 is hvp_walk's (Lambda and Lambda_dot per pixel), behind
// hvp_params' gather
struct HvpExact {
    using Sums = c5::ExactSums;
    c5::HvpParams hp{};
    void clear(const DerivativeView& v, const Sums& x, int64_t n_cells, unsigned flags) const { clear_exact(v, x, n_cells, flags); }
    void pass1(const DerivativeView& v) const { c5::launch_hvp_walk(v.s, hp, 1); }
    void walk(const DerivativeView& v, const Sums& x, bool sums) const { c5::launch_hvp_exact_walk(v.s, hp, x, sums); }
    void resolve(const DerivativeView& v, const Sums& x, bool sums) const {
        c5::launch_hvp_exact_resolve(v.s, v.r, hp.dir, hp.grad_out, x, sums);
    }
};

// The passes of one kind of exact sum (C5_EXACT_*) over the view for a call of one image: `image` is the upstream image,
// or the diagonal's weights; flags: kBounds, kSums or both
int exact_passes_of(c5_context* ctx, DerivativeView& v, const c5::ExactSums& x, int what, const double* d_alpha, const double* d_q,
                    const float2* image, unsigned flags) {
    flags |= kFirst;
    if (what == C5_EXACT_HVP) {
        HvpExact f;
        if (const int rc = hvp_params(ctx, v, d_alpha, d_q, image, f.hp)) return rc;
        exact_passes(ctx, v, f, x, flags);
        return C5_OK;
    }
    return what == C5_EXACT_GN_DIAGONAL ? adjoint_exact_passes<true>(ctx, v, x, image, flags)
                                        : adjoint_exact_passes<false>(ctx, v, x, image, flags);
}

// ... as a whole call behind the setup: passes E and S, the finish into the caller's order, the commit
int enqueue_exact_of(c5_context* ctx, DerivativeView& v, int what, const double* d_alpha, const double* d_q, const float2* image,
                     double* a_out, double* q_out, const char* name) {
    c5::ExactSums x;
    int rc = exact_sums(ctx, x);
    if (!rc) rc = exact_passes_of(ctx, v, x, what, d_alpha, d_q, image, kBounds | kSums);
    if (rc) return rc;
    c5::launch_exact_finish(v.s, x, v.perm, ctx->n_cells, a_out, q_out);
    return commit_exact(ctx, v, x.misfits, name);
}

const char* const kExactBoundsName[] = {"adjoint exact bounds", "gn diagonal exact bounds", "hvp exact bounds"};
const char* const kExactSumsName[] = {"adjoint exact sums", "gn diagonal exact sums", "hvp exact sums"};

// c5_render_exact_bounds: pass 1 and pass E over the context's rows; the exponents in the caller's order.  Pass E leaves
// the heads in place: the next per-view setup clears them.
int enqueue_exact_bounds(c5_context* ctx, int what, const double* d_alpha, const double* d_q, const float2* image, int32_t* exp_a,
                         int32_t* exp_q) {
    DerivativeView v;
    int rc = setup_derivative(ctx, v);
    if (rc || v.no_cells) return rc;
    c5::ExactSums x;
    rc = exact_sums(ctx, x);
    if (!rc) rc = exact_passes_of(ctx, v, x, what, d_alpha, d_q, image, kBounds);
    if (rc) return rc;
    c5::launch_exact_emit_exps(v.s, x, v.perm, ctx->n_cells, exp_a, exp_q);
    return commit_derivative(ctx, v, kExactBoundsName[what]);
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
    rc = exact_passes_of(ctx, v, x, what, d_alpha, d_q, image, kSums);
    if (rc) return rc;
    c5::launch_exact_emit_words(v.s, x, v.perm, ctx->n_cells, sums_a, sums_q);
    return commit_exact(ctx, v, x.misfits, kExactSumsName[what]);
}

// The adjoint: adjoint_one on the upstream image; with "adjoint_exact" or "exact_sums", the exact sums.
int enqueue_adjoint(c5_context* ctx, const float2* grad_out, double* ga_out, double* gq_out) {
    DerivativeView v;
    int rc = setup_derivative(ctx, v);
    if (rc || v.no_cells) return rc;
    if (ctx->deriv.adjoint_exact || ctx->deriv.exact_sums) return enqueue_exact_images(ctx, v, 1, grad_out, ga_out, gq_out, "adjoint");
    rc = adjoint_one(ctx, v, false, grad_out, ga_out, gq_out);
    return rc ? rc : commit_derivative(ctx, v, "adjoint");
}

// One tangent over the view: the caller's direction into device order, then one walk (or tangent_resolve over
// bin_sort_resolve's lists) that writes (tau_dot, I_dot) per pixel.
int tangent_one(c5_context* ctx, DerivativeView& v, const double* d_alpha, const double* d_q, float2* out) {
    C5_HIP(ctx, ctx->deriv.tan_dir.ensure(static_cast<size_t>(ctx->n_cells) * sizeof(double2)));
    double2* const dir = ctx->deriv.tan_dir.as<double2>();
    c5::launch_tangent_gather(v.s, d_alpha, d_q, v.perm, ctx->n_cells, dir);
    if (v.bin_sort) {
        c5::launch_tangent_resolve(v.s, v.r, dir, out);
    } else {
        c5::TangentParams tp{};
        tp.w = v.w;
        tp.dir = dir;
        tp.out = out;
        v.keep(false);  // (the walk hands every head back cleared)
        c5::launch_tangent_walk(v.s, tp);
    }
    return C5_OK;
}

// The tangent: tangent_one on the direction.
int enqueue_tangent(c5_context* ctx, const double* d_alpha, const double* d_q, float2* out) {
    DerivativeView v;
    int rc = setup_derivative(ctx, v);
    if (rc) return rc;
    if (v.no_cells) return zero_tangents(ctx, v, 1, out);
    rc = tangent_one(ctx, v, d_alpha, d_q, out);
    return rc ? rc : commit_derivative(ctx, v, "tangent");
}

// directions c.k0 .. c.k0 + c.n_used - 1 of the caller's [n][n_cells] arrays into bat_dirs (ensured by the caller): `width`
// interleaved pairs per cell in device order
void gather_chunk(c5_context* ctx, const DerivativeView& v, int width, const double* d_alpha, const double* d_q, const Chunk& c) {
    c5::launch_tangent_gather_batch(v.s, width, d_alpha, d_q, v.perm, ctx->n_cells, c.k0, c.n_used, ctx->deriv.bat_dirs.as<double2>());
}

// The batched pass 2 over the view's walk: its buffers (Lambda's, and [n_cells][2 width] sums in device order) and its
// parameters but for the chunk's (grad_out, n_used, keep_entries).
int adjoint_batch_params(c5_context* ctx, const DerivativeView& v, int width, c5::AdjointBatchParams& ab) {
    DerivativeState& d = ctx->deriv;
    C5_HIP(ctx, d.adj_lambda.ensure(static_cast<size_t>(v.padded) * sizeof(double)));
    C5_HIP(ctx, d.bat_grad.ensure(static_cast<size_t>(ctx->n_cells) * 2 * width * sizeof(double)));
    ab = c5::AdjointBatchParams{};
    ab.w = v.w;
    ab.image_px = v.n_px;
    ab.lambda = d.adj_lambda.as<double>();
    ab.grad = d.bat_grad.as<double>();
    return C5_OK;
}

// ... and one chunk of it: the sums zeroed, the walk (which hands the heads back unless c.more), the permutation into rows
// k0_out .. of the caller's arrays
int adjoint_chunk(c5_context* ctx, DerivativeView& v, int width, c5::AdjointBatchParams& ab, const Chunk& c, int k0_out, double* ga_out,
                  double* gq_out) {
    ab.n_used = c.n_used;
    ab.keep_entries = v.keep(c.more);
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
        for (int j = 0; j < n && !rc; ++j) rc = tangent_one(ctx, v, row_of(d_alpha, j, n_cells), row_of(d_q, j, n_cells), out + j * v.n_px);
        return rc ? rc : commit_derivative(ctx, v, "tangent batch");
    }
    const int width = batch_width(ctx, n);
    C5_HIP(ctx, ctx->deriv.bat_dirs.ensure(static_cast<size_t>(n_cells) * width * sizeof(double2)));
    c5::TangentBatchParams tb{};
    tb.w = v.w;
    tb.dirs = ctx->deriv.bat_dirs.as<double2>();
    tb.image_px = v.n_px;
    for (const Chunk c : Chunks{n, width}) {
        tb.n_used = c.n_used;
        tb.out = out + c.k0 * v.n_px;
        tb.keep_entries = v.keep(c.more);
        gather_chunk(ctx, v, width, d_alpha, d_q, c);
        c5::launch_tangent_walk_batch(v.s, width, tb);
    }
    return commit_derivative(ctx, v, "tangent batch");
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
    if (ctx->deriv.adjoint_exact || ctx->deriv.exact_sums) return enqueue_exact_images(ctx, v, n, grad_out, ga_out, gq_out, "adjoint batch");
    const int64_t n_cells = ctx->n_cells;
    if (v.bin_sort) {
        for (int j = 0; j < n && !rc; ++j)
            rc = adjoint_one(ctx, v, false, grad_out + j * v.n_px, ga_out + j * n_cells, gq_out + j * n_cells);
        return rc ? rc : commit_derivative(ctx, v, "adjoint batch");
    }
    const int width = batch_width(ctx, n);
    c5::AdjointParams ap;
    c5::AdjointBatchParams ab;
    rc = adjoint_params(ctx, v, ap);
    if (!rc) rc = adjoint_batch_params(ctx, v, width, ab);
    if (rc) return rc;
    c5::launch_adjoint_walk(v.s, ap, 1);
    for (const Chunk c : Chunks{n, width}) {
        ab.grad_out = grad_out + c.k0 * v.n_px;
        rc = adjoint_chunk(ctx, v, width, ab, c, c.k0, ga_out, gq_out);
        if (rc) return rc;
    }
    return commit_derivative(ctx, v, "adjoint batch");
}

// The Gauss-Newton product H v = J^T W J v for n directions: one per-view setup, then per chunk of up to `width` directions
// the gather, pass A (gn_walk_a: the tangent walk that is also the adjoint's pass 1; g = w * J v in fp32 and Lambda), the
// batched pass 2 on g, and its permutation.  The heads stay in place from pass A to pass B and between the chunks; the
// last pass B hands them back cleared.  On bin_sort_resolve's lists: tangent_one -> gn_weight -> adjoint_one per
// direction.  ha_out / hq_out: either may be null (then that block goes to a spare buffer); jv_out may be null.
// With "exact_sums": pass A per chunk as it is, then every direction's g through the single exact path - passes E and S
// on Lambda as pass A left it, and the finish - one after the other (exact_images): bit for bit the exact adjoint of g.
// Pass S leaves the heads in place for all but the last direction of the call.
int enqueue_gn_product(c5_context* ctx, int n, const double* d_alpha, const double* d_q, const float2* weight, double* ha_out,
                       double* hq_out, float2* jv_out) {
    DerivativeView v;
    int rc = setup_derivative(ctx, v);
    if (rc) return rc;
    if (v.no_cells) return zero_tangents(ctx, v, n, jv_out);
    DerivativeState& d = ctx->deriv;
    const int64_t n_cells = ctx->n_cells, n_px = v.n_px;
    const int width = v.bin_sort ? 1 : batch_width(ctx, n);
    const bool exact = d.exact_sums != 0;
    c5::ExactSums x{};
    if (exact) {
        rc = exact_sums(ctx, x);
        if (rc) return rc;
    }
    if (!exact && (!ha_out || !hq_out)) C5_HIP(ctx, d.gn_spare.ensure(static_cast<size_t>(n_cells) * width * sizeof(double)));
    // rows j .. of a block of H v, or the spare buffer for the block the caller did not ask for
    auto rows = [&](double* h_out, int j) { return h_out ? h_out + j * n_cells : d.gn_spare.as<double>(); };
    auto commit = [&] { return exact ? commit_exact(ctx, v, x.misfits, "gn product") : commit_derivative(ctx, v, "gn product"); };
    if (v.bin_sort) {
        C5_HIP(ctx, d.gn_g.ensure(2 * static_cast<size_t>(n_px) * sizeof(float2) + 16));
        float2* const g = d.gn_g.as<float2>();
        for (int j = 0; j < n; ++j) {
            float2* const t = jv_out ? jv_out + j * n_px : g + n_px;
            rc = tangent_one(ctx, v, row_of(d_alpha, j, n_cells), row_of(d_q, j, n_cells), t);
            if (rc) return rc;
            c5::launch_gn_weight(v.s, t, weight, n_px, 1, g);
            rc = exact ? exact_images(ctx, v, x, 1, g, ha_out, hq_out, true, j, n) : adjoint_one(ctx, v, false, g, rows(ha_out, j), rows(hq_out, j));
            if (rc) return rc;
        }
        return commit();
    }
    c5::AdjointBatchParams ab{};
    if (exact) C5_HIP(ctx, d.adj_lambda.ensure(static_cast<size_t>(v.padded) * sizeof(double)));
    else rc = adjoint_batch_params(ctx, v, width, ab);
    if (rc) return rc;
    C5_HIP(ctx, d.bat_dirs.ensure(static_cast<size_t>(n_cells) * width * sizeof(double2)));
    C5_HIP(ctx, d.gn_g.ensure(static_cast<size_t>(width) * n_px * sizeof(float2) + 16));
    c5::GnWalkParams ga{};
    ga.w = v.w;
    ga.dirs = d.bat_dirs.as<double2>();
    ga.weight = weight;
    ga.lambda = d.adj_lambda.as<double>();
    ga.g = d.gn_g.as<float2>();
    ga.image_px = n_px;
    ab.grad_out = ga.g;
    for (const Chunk c : Chunks{n, width}) {
        ga.n_used = c.n_used;
        ga.jv_out = jv_out ? jv_out + c.k0 * n_px : nullptr;
        gather_chunk(ctx, v, width, d_alpha, d_q, c);
        c5::launch_gn_walk_a(v.s, width, ga);
        rc = exact ? exact_images(ctx, v, x, c.n_used, ga.g, ha_out, hq_out, true, c.k0, n)
                   : adjoint_chunk(ctx, v, width, ab, c, 0, rows(ha_out, c.k0), rows(hq_out, c.k0));
        if (rc) return rc;
    }
    return commit();
}

// The Hessian-vector render: the direction into device order (the tangent's buffer), the per-cell sums zeroed (the
// adjoint's buffer), two passes of the walk - Lambda and Lambda_dot per pixel, then the scatter - or hvp_resolve over
// bin_sort_resolve's lists, and the permutation into the caller's order.  ha_out / hq_out: either may be null.
int enqueue_hvp(c5_context* ctx, const double* d_alpha, const double* d_q, const float2* grad_out, double* ha_out, double* hq_out) {
    DerivativeView v;
    int rc = setup_derivative(ctx, v);
    if (rc || v.no_cells) return rc;
    // "exact_sums": pass 1, pass E, pass S and the finish
    if (ctx->deriv.exact_sums) return enqueue_exact_of(ctx, v, C5_EXACT_HVP, d_alpha, d_q, grad_out, ha_out, hq_out, "hvp");
    const size_t n_cells = static_cast<size_t>(ctx->n_cells);
    C5_HIP(ctx, ctx->deriv.adj_grad.ensure(2 * n_cells * sizeof(double)));
    double* const ha_dev = ctx->deriv.adj_grad.as<double>();
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
        v.keep(false);  // (the second pass hands every head back cleared)
        c5::launch_hvp_walk(v.s, hp, 2);
    }
    c5::launch_hvp_permute(v.s, ha_dev, hq_dev, v.perm, ctx->n_cells, ha_out, hq_out);
    return commit_derivative(ctx, v, "hvp");
}

// diag(J^T W J): adjoint_one with the squared kernels.  weight null: ones.
int enqueue_gn_diagonal(c5_context* ctx, const float2* weight, double* da_out, double* dq_out) {
    DerivativeView v;
    int rc = setup_derivative(ctx, v);
    if (rc || v.no_cells) return rc;
    // "exact_sums": pass 1, pass E on the squares, pass S and the finish
    if (ctx->deriv.exact_sums) return enqueue_exact_of(ctx, v, C5_EXACT_GN_DIAGONAL, nullptr, nullptr, weight, da_out, dq_out, "gn diagonal");
    rc = adjoint_one(ctx, v, true, weight, da_out, dq_out);
    return rc ? rc : commit_derivative(ctx, v, "gn diagonal");
}

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

}  // extern "C"

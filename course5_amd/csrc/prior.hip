// ------------------------------------------------------------------------------------------
// Cell-field smoothness prior, host side (include/course5_hip.h: c5_prior_*; the kernels: prior_kernels.hip).
// The weights live on the context per weighting and are rebuilt when the grid or (TPFA) the points moved on; every
// operator call is one launch over the cells on the context's stream, and the value one more over its blocks' partials.
// ------------------------------------------------------------------------------------------
#include "context.hpp"
#include "prior_kernels.hpp"

using namespace c5api;

namespace {

inline size_t cells_bytes(const c5_context* ctx) { return static_cast<size_t>(ctx->n_cells) * sizeof(double); }

// What every prior call checks first.  done: there is no cell, and rc is the answer (the derivative renders': C5_ERR_STATE
// where there is nothing at all, C5_OK where there are only solids).
int check_grid(c5_context* ctx, const char* name, bool& done) {
    done = true;
    if (ctx->n_cells <= 0) {
        if (nothing_to_render(ctx)) return fail(ctx, C5_ERR_STATE, "plane initializer. empty set of objects to render");
        return C5_OK;
    }
    if (!ctx->grid_conforming)
        return fail(ctx, C5_ERR_MESH, "%s: the grid was uploaded as non-conforming (a face is shared by more than two cells): it has no adjacency", name);
    done = false;
    return bind_device(ctx);
}

int check_weighting(c5_context* ctx, const char* name, int weighting) {
    if (weighting != C5_PRIOR_UNIT && weighting != C5_PRIOR_TPFA) return fail(ctx, C5_ERR_INVALID, "%s: unknown weighting %d", name, weighting);
    return C5_OK;
}

int check_prior(c5_context* ctx, const char* name, const c5_prior* p) {
    if (!p) return fail(ctx, C5_ERR_INVALID, "%s: null prior", name);
    if (p->penalty != C5_PRIOR_QUADRATIC && p->penalty != C5_PRIOR_PSEUDO_HUBER)
        return fail(ctx, C5_ERR_INVALID, "%s: unknown penalty %d", name, p->penalty);
    int rc = check_weighting(ctx, name, p->weighting);
    if (rc) return rc;
    const double lambda[2] = {p->lambda_alpha, p->lambda_q}, delta[2] = {p->delta_alpha, p->delta_q};
    for (int k = 0; k < 2; ++k) {
        if (!(lambda[k] >= 0.0) || !std::isfinite(lambda[k]))
            return fail(ctx, C5_ERR_INVALID, "%s: lambda_%s = %g is not finite and >= 0", name, k ? "q" : "alpha", lambda[k]);
        if (p->penalty == C5_PRIOR_PSEUDO_HUBER && lambda[k] > 0.0 && (!(delta[k] > 0.0) || !std::isfinite(delta[k])))
            return fail(ctx, C5_ERR_INVALID, "%s: delta_%s = %g is not finite and > 0", name, k ? "q" : "alpha", delta[k]);
    }
    return C5_OK;
}

// The weights of `weighting` on the device, for the grid and the points as they are now.
int ensure_weights(c5_context* ctx, int weighting) {
    PriorState& ps = ctx->prior;
    const bool fresh = ps.w[weighting].ptr && ps.w_grid[weighting] == ctx->grid_serial &&
                       (weighting == C5_PRIOR_UNIT || ps.w_points[weighting] == ctx->points_serial);
    if (fresh) return C5_OK;
    int rc = ensure_device_perm(ctx);
    if (rc) return rc;
    C5_HIP(ctx, ps.w[weighting].ensure(static_cast<size_t>(ctx->n_cells) * 4 * sizeof(double)));
    C5_HIP(ctx, ps.counts.ensure(2 * sizeof(unsigned long long)));
    hipStream_t s = ctx->stream;
    unsigned long long* const counts = ps.counts.as<unsigned long long>();
    C5_HIP(ctx, hipMemsetAsync(counts, 0, 2 * sizeof(unsigned long long), s));
    const c5::PriorGrid g{ctx->cell_vert.as<int4>(), ctx->cell_adj.as<int4>(), ctx->px.as<double>(), ctx->py.as<double>(),
                          ctx->pz.as<double>(), ctx->n_cells};
    c5::launch_prior_weights(s, g, weighting, ps.w[weighting].as<double>(), counts);
    C5_HIP(ctx, hipGetLastError());
    unsigned long long host[2] = {0, 0};
    C5_HIP(ctx, hipMemcpyAsync(host, counts, sizeof host, hipMemcpyDeviceToHost, s));
    C5_HIP(ctx, hipStreamSynchronize(s));
    ps.n_interior[weighting] = static_cast<int64_t>(host[0] / 2);  // (every face was seen from both its cells)
    ps.n_degenerate[weighting] = static_cast<int64_t>(host[1] / 2);
    ps.w_grid[weighting] = ctx->grid_serial;
    ps.w_points[weighting] = ctx->points_serial;
    return C5_OK;
}

int weights_device(c5_context* ctx, const char* name, int weighting, double* w_dev, int64_t* n_interior, int64_t* n_degenerate, bool& done) {
    if (!ctx) return fail(nullptr, C5_ERR_INVALID, "null context");
    int rc = check_weighting(ctx, name, weighting);
    if (rc) return rc;
    rc = check_grid(ctx, name, done);
    if (rc || done) {
        if (!rc && n_interior) *n_interior = 0;
        if (!rc && n_degenerate) *n_degenerate = 0;
        return rc;
    }
    rc = ensure_weights(ctx, weighting);
    if (rc) return rc;
    const PriorState& ps = ctx->prior;
    if (w_dev) {
        c5::launch_prior_weights_scatter(ctx->stream, ps.w[weighting].as<double>(), ctx->cell_perm.empty() ? nullptr : ctx->adj_perm.as<int32_t>(),
                                         ctx->n_cells, w_dev);
        C5_HIP(ctx, hipGetLastError());
    }
    if (n_interior) *n_interior = ps.n_interior[weighting];
    if (n_degenerate) *n_degenerate = ps.n_degenerate[weighting];
    return C5_OK;
}

// One operator call over device pointers.  x: the point, p: the product's direction, out: the result, each per field.
int apply_device(c5_context* ctx, const char* name, int op, const c5_prior* prior, const double* const x[2], const double* const p[2],
                 double* const out[2], double* value_dev, bool& done) {
    if (!ctx) return fail(nullptr, C5_ERR_INVALID, "null context");
    int rc = check_prior(ctx, name, prior);
    if (rc) return rc;
    const double lambda[2] = {prior->lambda_alpha, prior->lambda_q}, delta[2] = {prior->delta_alpha, prior->delta_q};
    const bool need_x = op == c5::kPriorGradient || prior->penalty == C5_PRIOR_PSEUDO_HUBER;
    for (int k = 0; k < 2; ++k)
        if (lambda[k] > 0.0 && ctx->n_cells > 0 && (!out[k] || (need_x && !x[k]) || (op == c5::kPriorProduct && !p[k])))
            return fail(ctx, C5_ERR_INVALID, "%s: null array for %s, whose lambda is not 0", name, k ? "q" : "alpha");
    rc = check_grid(ctx, name, done);
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    if (done) {
        if (value_dev) C5_HIP(ctx, hipMemsetAsync(value_dev, 0, 2 * sizeof(double), s));
        return C5_OK;
    }
    rc = ensure_weights(ctx, prior->weighting);
    if (rc) return rc;
    PriorState& ps = ctx->prior;
    const int64_t n_blocks = c5::prior_blocks(ctx->n_cells);
    if (value_dev) C5_HIP(ctx, ps.partials.ensure(static_cast<size_t>(2 * n_blocks) * sizeof(double)));
    c5::PriorArgs a{};
    a.adj = ctx->cell_adj.as<int4>();
    a.w = ps.w[prior->weighting].as<double>();
    a.perm = ctx->cell_perm.empty() ? nullptr : ctx->adj_perm.as<int32_t>();
    a.n_cells = ctx->n_cells;
    for (int k = 0; k < 2; ++k) a.f[k] = c5::PriorField{x[k], p[k], out[k], lambda[k], delta[k]};
    a.partials = ps.partials.as<double>();
    c5::launch_prior_apply(s, op, prior->penalty, value_dev != nullptr, a);
    C5_HIP(ctx, hipGetLastError());
    if (value_dev) {
        c5::launch_prior_value(s, a.partials, n_blocks, lambda[0], lambda[1], value_dev);
        C5_HIP(ctx, hipGetLastError());
    }
    return C5_OK;
}

// The host-pointer form of an operator: the arrays through the context's staging buffer, one wait at the end.
int apply_host(c5_context* ctx, const char* name, int op, const c5_prior* prior, const double* const x[2], const double* const p[2],
               double* const out[2], double* value) {
    if (!ctx) return fail(nullptr, C5_ERR_INVALID, "null context");
    int rc = check_prior(ctx, name, prior);  // (before anything is staged)
    if (rc) return rc;
    const size_t cb = (cells_bytes(ctx) + 255) / 256 * 256;
    rc = bind_device(ctx);
    if (rc) return rc;
    C5_HIP(ctx, ctx->prior.io.ensure(6 * cb + 256));
    char* const base = ctx->prior.io.as<char>();
    hipStream_t s = ctx->stream;
    const double *xd[2], *pd[2];
    double* od[2];
    for (int k = 0; k < 2; ++k) {
        xd[k] = x[k] ? reinterpret_cast<const double*>(base + k * cb) : nullptr;
        pd[k] = p[k] ? reinterpret_cast<const double*>(base + (2 + k) * cb) : nullptr;
        od[k] = out[k] ? reinterpret_cast<double*>(base + (4 + k) * cb) : nullptr;
        if (x[k] && ctx->n_cells > 0) C5_HIP(ctx, hipMemcpyAsync(base + k * cb, x[k], cells_bytes(ctx), hipMemcpyHostToDevice, s));
        if (p[k] && ctx->n_cells > 0) C5_HIP(ctx, hipMemcpyAsync(base + (2 + k) * cb, p[k], cells_bytes(ctx), hipMemcpyHostToDevice, s));
    }
    double* const value_dev = value ? reinterpret_cast<double*>(base + 6 * cb) : nullptr;
    bool done = false;
    rc = apply_device(ctx, name, op, prior, xd, pd, od, value_dev, done);
    if (rc) return rc;
    if (!done)
        for (int k = 0; k < 2; ++k)
            if (out[k]) C5_HIP(ctx, hipMemcpyAsync(out[k], od[k], cells_bytes(ctx), hipMemcpyDeviceToHost, s));
    if (value) C5_HIP(ctx, hipMemcpyAsync(value, value_dev, 2 * sizeof(double), hipMemcpyDeviceToHost, s));
    C5_HIP(ctx, hipStreamSynchronize(s));
    return C5_OK;
}

const double* dptr(const void* p) { return static_cast<const double*>(p); }
double* dptr(void* p) { return static_cast<double*>(p); }

}  // namespace

extern "C" {

int c5_prior_weights_device(c5_context* ctx, int weighting, void* w_dev, int64_t* n_interior_faces, int64_t* n_degenerate) {
    bool done = false;
    return weights_device(ctx, "c5_prior_weights", weighting, dptr(w_dev), n_interior_faces, n_degenerate, done);
}

int c5_prior_weights(c5_context* ctx, int weighting, double* w_host, int64_t* n_interior_faces, int64_t* n_degenerate) {
    if (!ctx) return fail(nullptr, C5_ERR_INVALID, "null context");
    const size_t bytes = 4 * cells_bytes(ctx);
    double* w_dev = nullptr;
    if (w_host && ctx->n_cells > 0 && ctx->grid_conforming) {
        int rc = bind_device(ctx);
        if (rc) return rc;
        C5_HIP(ctx, ctx->prior.io.ensure(bytes));
        w_dev = ctx->prior.io.as<double>();
    }
    bool done = false;
    int rc = weights_device(ctx, "c5_prior_weights", weighting, w_dev, n_interior_faces, n_degenerate, done);
    if (rc || done) return rc;
    if (w_dev) C5_HIP(ctx, hipMemcpyAsync(w_host, w_dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    C5_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return C5_OK;
}

int c5_prior_gradient_device(c5_context* ctx, const c5_prior* prior, const void* alpha_dev, const void* q_dev, void* value_dev,
                             void* grad_alpha_dev, void* grad_q_dev) {
    const double* const x[2] = {dptr(alpha_dev), dptr(q_dev)};
    const double* const p[2] = {nullptr, nullptr};
    double* const out[2] = {dptr(grad_alpha_dev), dptr(grad_q_dev)};
    bool done = false;
    return apply_device(ctx, "c5_prior_gradient", c5::kPriorGradient, prior, x, p, out, dptr(value_dev), done);
}

int c5_prior_gradient(c5_context* ctx, const c5_prior* prior, const double* alpha_host, const double* q_host, double value_host[2],
                      double* grad_alpha_host, double* grad_q_host) {
    const double* const x[2] = {alpha_host, q_host};
    const double* const p[2] = {nullptr, nullptr};
    double* const out[2] = {grad_alpha_host, grad_q_host};
    return apply_host(ctx, "c5_prior_gradient", c5::kPriorGradient, prior, x, p, out, value_host);
}

int c5_prior_product_device(c5_context* ctx, const c5_prior* prior, const void* alpha_dev, const void* q_dev, const void* v_alpha_dev,
                            const void* v_q_dev, void* h_alpha_dev, void* h_q_dev) {
    const double* const x[2] = {dptr(alpha_dev), dptr(q_dev)};
    const double* const p[2] = {dptr(v_alpha_dev), dptr(v_q_dev)};
    double* const out[2] = {dptr(h_alpha_dev), dptr(h_q_dev)};
    bool done = false;
    return apply_device(ctx, "c5_prior_product", c5::kPriorProduct, prior, x, p, out, nullptr, done);
}

int c5_prior_product(c5_context* ctx, const c5_prior* prior, const double* alpha_host, const double* q_host, const double* v_alpha_host,
                     const double* v_q_host, double* h_alpha_host, double* h_q_host) {
    const double* const x[2] = {alpha_host, q_host};
    const double* const p[2] = {v_alpha_host, v_q_host};
    double* const out[2] = {h_alpha_host, h_q_host};
    return apply_host(ctx, "c5_prior_product", c5::kPriorProduct, prior, x, p, out, nullptr);
}

int c5_prior_diagonal_device(c5_context* ctx, const c5_prior* prior, const void* alpha_dev, const void* q_dev, void* diag_alpha_dev,
                             void* diag_q_dev) {
    const double* const x[2] = {dptr(alpha_dev), dptr(q_dev)};
    const double* const p[2] = {nullptr, nullptr};
    double* const out[2] = {dptr(diag_alpha_dev), dptr(diag_q_dev)};
    bool done = false;
    return apply_device(ctx, "c5_prior_diagonal", c5::kPriorDiagonal, prior, x, p, out, nullptr, done);
}

int c5_prior_diagonal(c5_context* ctx, const c5_prior* prior, const double* alpha_host, const double* q_host, double* diag_alpha_host,
                      double* diag_q_host) {
    const double* const x[2] = {alpha_host, q_host};
    const double* const p[2] = {nullptr, nullptr};
    double* const out[2] = {diag_alpha_host, diag_q_host};
    return apply_host(ctx, "c5_prior_diagonal", c5::kPriorDiagonal, prior, x, p, out, nullptr);
}

}  // extern "C"

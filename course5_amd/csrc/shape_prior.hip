// ------------------------------------------------------------------------------------------
// Shape prior, host side (include/course5_hip.h: c5_shape_prior_*; the kernels: shape_prior_kernels.hip).
// The rest data (B and V0 per cell, device order) live on the context from c5_shape_prior_rest to the next c5_upload_grid;
// every operator call is one launch over the cells and one over the points on the context's stream - the latter over the
// incidence table the exact vertex sums use (geometry_derivatives.hip: vertex_incidence) - and the value one more over
// the blocks' partials.
// ------------------------------------------------------------------------------------------
#include "context.hpp"
#include "shape_prior_kernels.hpp"

using namespace c5api;

namespace {

inline size_t pad256(size_t b) { return (b + 255) / 256 * 256; }
inline size_t points_bytes(const c5_context* ctx) { return static_cast<size_t>(ctx->n_pts) * 3 * sizeof(double); }

int check_prior(c5_context* ctx, const char* name, const c5_shape_prior* p) {
    if (!p) return fail(ctx, C5_ERR_INVALID, "%s: null prior", name);
    if (p->energy != C5_SHAPE_DIRICHLET && p->energy != C5_SHAPE_NEO_HOOKEAN) return fail(ctx, C5_ERR_INVALID, "%s: unknown energy %d", name, p->energy);
    if (p->reserved != 0) return fail(ctx, C5_ERR_INVALID, "%s: reserved = %d is not 0", name, p->reserved);
    if (!(p->lambda >= 0.0) || !std::isfinite(p->lambda)) return fail(ctx, C5_ERR_INVALID, "%s: lambda = %g is not finite and >= 0", name, p->lambda);
    if (!(p->kappa >= 0.0) || !std::isfinite(p->kappa)) return fail(ctx, C5_ERR_INVALID, "%s: kappa = %g is not finite and >= 0", name, p->kappa);
    return C5_OK;
}

// What every call checks before it touches the device.  done: there is no cell, and rc is the answer (the c5_prior_*
// calls': C5_ERR_STATE where there is nothing at all, C5_OK where there are only solids).
int check_grid(c5_context* ctx, const char* name, bool& done) {
    done = true;
    if (ctx->hr_count) return fail(ctx, C5_ERR_STATE, "%s while c5_render_host_async frames are outstanding", name);
    if (ctx->n_cells <= 0) {
        if (nothing_to_render(ctx)) return fail(ctx, C5_ERR_STATE, "plane initializer. empty set of objects to render");
        return C5_OK;
    }
    done = false;
    return bind_device(ctx);
}

int check_rest(c5_context* ctx, const char* name) {
    if (!ctx->shape.have_rest) return fail(ctx, C5_ERR_STATE, "%s: no rest shape is set (c5_shape_prior_rest; c5_upload_grid drops it)", name);
    return C5_OK;
}

c5::ShapeRest rest_view(const c5_context* ctx) {
    return c5::ShapeRest{ctx->cell_vert.as<int4>(), ctx->shape.binv.as<double>(), ctx->shape.vol.as<double>(), ctx->n_cells};
}

// c5_shape_prior_rest over device memory (xyz_dev null: the context's own points).  checked: the caller has looked at
// every coordinate already.
int rest_device(c5_context* ctx, const char* name, const double* xyz_dev, int64_t n_pts, int64_t* n_degenerate, bool checked) {
    if (n_pts != ctx->n_pts) return fail(ctx, C5_ERR_INVALID, "%s: point count differs from the uploaded grid", name);
    bool done = false;
    int rc = check_grid(ctx, name, done);
    if (rc) return rc;
    ShapeState& sh = ctx->shape;
    if (done) {
        sh.have_rest = true;
        sh.n_degenerate = 0;
        if (n_degenerate) *n_degenerate = 0;
        return C5_OK;
    }
    hipStream_t s = ctx->stream;
    C5_HIP(ctx, sh.counts.ensure(2 * sizeof(unsigned long long)));
    unsigned long long* const counts = sh.counts.as<unsigned long long>();
    unsigned long long host[2] = {0, 0};
    C5_HIP(ctx, hipMemsetAsync(counts, 0, sizeof host, s));
    if (xyz_dev && !checked) {
        c5::launch_shape_check_finite(s, xyz_dev, 3 * n_pts, counts);
        C5_HIP(ctx, hipGetLastError());
        C5_HIP(ctx, hipMemcpyAsync(host, counts, sizeof host, hipMemcpyDeviceToHost, s));
        C5_HIP(ctx, hipStreamSynchronize(s));
        if (host[0]) return fail(ctx, C5_ERR_INVALID, "%s: %llu rest coordinates are not finite", name, host[0]);
    }
    const size_t n_cells = static_cast<size_t>(ctx->n_cells);
    C5_HIP(ctx, sh.binv.ensure(9 * n_cells * sizeof(double)));
    C5_HIP(ctx, sh.vol.ensure(n_cells * sizeof(double)));
    const c5::ShapePoints X = xyz_dev ? c5::shape_points_aos(xyz_dev)
                                      : c5::ShapePoints{{ctx->px.as<double>(), ctx->py.as<double>(), ctx->pz.as<double>()}, 1};
    c5::launch_shape_rest(s, ctx->cell_vert.as<int4>(), ctx->n_cells, X, sh.binv.as<double>(), sh.vol.as<double>(), counts);
    C5_HIP(ctx, hipGetLastError());
    C5_HIP(ctx, hipMemcpyAsync(host, counts, sizeof host, hipMemcpyDeviceToHost, s));
    C5_HIP(ctx, hipStreamSynchronize(s));
    sh.have_rest = true;
    sh.n_degenerate = static_cast<int64_t>(host[1]);
    if (n_degenerate) *n_degenerate = sh.n_degenerate;
    return C5_OK;
}

int rest_data_device(c5_context* ctx, const char* name, double* binv, double* vol, int32_t* vert, bool& done) {
    int rc = check_grid(ctx, name, done);
    if (rc || done) return rc;
    rc = check_rest(ctx, name);
    if (rc) return rc;
    rc = ensure_device_perm(ctx);
    if (rc) return rc;
    c5::launch_shape_rest_scatter(ctx->stream, rest_view(ctx), ctx->cell_perm.empty() ? nullptr : ctx->adj_perm.as<int32_t>(), binv, vol, vert);
    C5_HIP(ctx, hipGetLastError());
    return C5_OK;
}

// One operator call over device pointers: xyz the point, v the product's direction, out the result, [n_pts][3] each in the
// caller's point order; value_dev / n_inverted_dev: a device double / int64, or null.
int apply_device(c5_context* ctx, const char* name, int op, const c5_shape_prior* prior, const double* xyz, const double* v, double* out,
                 double* value_dev, long long* n_inverted_dev, bool& done) {
    int rc = check_prior(ctx, name, prior);
    if (rc) return rc;
    const bool need_x = op == c5::kShapeGradient || prior->energy == C5_SHAPE_NEO_HOOKEAN;
    if (!out || (need_x && !xyz) || (op == c5::kShapeProduct && !v)) return fail(ctx, C5_ERR_INVALID, "%s: null array", name);
    rc = check_grid(ctx, name, done);
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    if (done) {
        if (value_dev) C5_HIP(ctx, hipMemsetAsync(value_dev, 0, sizeof(double), s));
        if (n_inverted_dev) C5_HIP(ctx, hipMemsetAsync(n_inverted_dev, 0, sizeof(long long), s));
        return C5_OK;
    }
    rc = check_rest(ctx, name);
    if (rc) return rc;
    ShapeState& sh = ctx->shape;
    const bool with_value = value_dev || n_inverted_dev;
    const int64_t n_blocks = c5::shape_blocks(ctx->n_cells);
    C5_HIP(ctx, sh.shares.ensure(static_cast<size_t>(ctx->n_cells) * 12 * sizeof(double)));
    if (with_value) C5_HIP(ctx, sh.partials.ensure(static_cast<size_t>(2 * n_blocks) * sizeof(double)));
    c5::VertexIncidence inc;
    rc = vertex_incidence(ctx, inc);
    if (rc) return rc;
    c5::ShapeArgs a{};
    a.rest = rest_view(ctx);
    a.x = c5::shape_points_aos(xyz);
    a.v = c5::shape_points_aos(v);
    a.kappa = prior->kappa;
    a.shares = sh.shares.as<double>();
    a.value_partials = sh.partials.as<double>();
    a.inv_partials = reinterpret_cast<long long*>(a.value_partials + n_blocks);
    c5::launch_shape_cells(s, op, prior->energy, with_value, a);
    C5_HIP(ctx, hipGetLastError());
    c5::launch_shape_points(s, a.shares, inc, ctx->n_pts, prior->lambda, out);
    C5_HIP(ctx, hipGetLastError());
    if (with_value) {
        c5::launch_shape_value(s, a.value_partials, a.inv_partials, n_blocks, prior->lambda, prior->energy == C5_SHAPE_NEO_HOOKEAN, value_dev,
                               n_inverted_dev);
        C5_HIP(ctx, hipGetLastError());
    }
    return C5_OK;
}

int quality_device(c5_context* ctx, const char* name, const double* xyz, double* ratio_dev, long long* n_inverted_dev, bool& done) {
    if (!xyz) return fail(ctx, C5_ERR_INVALID, "%s: null array", name);
    int rc = check_grid(ctx, name, done);
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    if (done) {
        if (n_inverted_dev) C5_HIP(ctx, hipMemsetAsync(n_inverted_dev, 0, sizeof(long long), s));
        return C5_OK;
    }
    rc = check_rest(ctx, name);
    if (rc) return rc;
    rc = ensure_device_perm(ctx);
    if (rc) return rc;
    ShapeState& sh = ctx->shape;
    const int64_t n_blocks = c5::shape_blocks(ctx->n_cells);
    C5_HIP(ctx, sh.partials.ensure(static_cast<size_t>(2 * n_blocks) * sizeof(double)));
    c5::ShapeArgs a{};
    a.rest = rest_view(ctx);
    a.x = c5::shape_points_aos(xyz);
    a.value_partials = sh.partials.as<double>();
    a.inv_partials = reinterpret_cast<long long*>(a.value_partials + n_blocks);
    a.ratio = ratio_dev;
    a.perm = ctx->cell_perm.empty() ? nullptr : ctx->adj_perm.as<int32_t>();
    c5::launch_shape_cells(s, c5::kShapeQuality, C5_SHAPE_DIRICHLET, true, a);
    C5_HIP(ctx, hipGetLastError());
    if (n_inverted_dev) {
        c5::launch_shape_value(s, a.value_partials, a.inv_partials, n_blocks, 0.0, false, nullptr, n_inverted_dev);
        C5_HIP(ctx, hipGetLastError());
    }
    return C5_OK;
}

// The host-pointer form of an operator: the arrays through the context's staging buffer, one wait at the end.
int apply_host(c5_context* ctx, const char* name, int op, const c5_shape_prior* prior, const double* xyz, const double* v, double* out,
               double* value, int64_t* n_inverted) {
    if (!ctx) return fail(nullptr, C5_ERR_INVALID, "null context");
    int rc = check_prior(ctx, name, prior);  // (before anything is staged)
    if (rc) return rc;
    rc = bind_device(ctx);
    if (rc) return rc;
    const size_t pb = pad256(points_bytes(ctx));
    C5_HIP(ctx, ctx->shape.io.ensure(3 * pb + 256));
    char* const base = ctx->shape.io.as<char>();
    hipStream_t s = ctx->stream;
    const bool cells = ctx->n_cells > 0 && ctx->n_pts > 0;
    if (xyz && cells) C5_HIP(ctx, hipMemcpyAsync(base, xyz, points_bytes(ctx), hipMemcpyHostToDevice, s));
    if (v && cells) C5_HIP(ctx, hipMemcpyAsync(base + pb, v, points_bytes(ctx), hipMemcpyHostToDevice, s));
    double* const value_dev = value ? reinterpret_cast<double*>(base + 3 * pb) : nullptr;
    long long* const inv_dev = n_inverted ? reinterpret_cast<long long*>(base + 3 * pb + 8) : nullptr;
    double* const out_dev = out ? reinterpret_cast<double*>(base + 2 * pb) : nullptr;
    bool done = false;
    rc = apply_device(ctx, name, op, prior, xyz ? reinterpret_cast<const double*>(base) : nullptr,
                      v ? reinterpret_cast<const double*>(base + pb) : nullptr, out_dev, value_dev, inv_dev, done);
    if (rc) return rc;
    if (!done && ctx->n_pts > 0) C5_HIP(ctx, hipMemcpyAsync(out, out_dev, points_bytes(ctx), hipMemcpyDeviceToHost, s));
    if (value) C5_HIP(ctx, hipMemcpyAsync(value, value_dev, sizeof(double), hipMemcpyDeviceToHost, s));
    if (n_inverted) C5_HIP(ctx, hipMemcpyAsync(n_inverted, inv_dev, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    C5_HIP(ctx, hipStreamSynchronize(s));
    return C5_OK;
}

const double* dptr(const void* p) { return static_cast<const double*>(p); }
double* dptr(void* p) { return static_cast<double*>(p); }

}  // namespace

extern "C" {

int c5_shape_prior_rest_device(c5_context* ctx, const void* xyz_dev, int64_t n_pts, int64_t* n_degenerate) {
    if (!ctx) return fail(nullptr, C5_ERR_INVALID, "null context");
    return rest_device(ctx, "c5_shape_prior_rest", dptr(xyz_dev), n_pts, n_degenerate, false);
}

int c5_shape_prior_rest(c5_context* ctx, const double* xyz_host, int64_t n_pts, int64_t* n_degenerate) {
    if (!ctx) return fail(nullptr, C5_ERR_INVALID, "null context");
    const char* const name = "c5_shape_prior_rest";
    if (n_pts != ctx->n_pts) return fail(ctx, C5_ERR_INVALID, "%s: point count differs from the uploaded grid", name);
    if (!xyz_host || ctx->n_cells <= 0 || ctx->hr_count) return rest_device(ctx, name, nullptr, n_pts, n_degenerate, true);
    for (int64_t i = 0; i < 3 * n_pts; ++i)
        if (!std::isfinite(xyz_host[i])) return fail(ctx, C5_ERR_INVALID, "%s: point %lld has a non-finite rest coordinate", name, static_cast<long long>(i / 3));
    int rc = bind_device(ctx);
    if (rc) return rc;
    C5_HIP(ctx, ctx->shape.io.ensure(3 * pad256(points_bytes(ctx)) + 256));
    C5_HIP(ctx, hipMemcpyAsync(ctx->shape.io.ptr, xyz_host, points_bytes(ctx), hipMemcpyHostToDevice, ctx->stream));
    return rest_device(ctx, name, ctx->shape.io.as<double>(), n_pts, n_degenerate, true);
}

int c5_shape_prior_rest_data_device(c5_context* ctx, void* binv_dev, void* vol_dev, void* vert_dev) {
    if (!ctx) return fail(nullptr, C5_ERR_INVALID, "null context");
    bool done = false;
    return rest_data_device(ctx, "c5_shape_prior_rest_data", dptr(binv_dev), dptr(vol_dev), static_cast<int32_t*>(vert_dev), done);
}

int c5_shape_prior_rest_data(c5_context* ctx, double* binv_host, double* vol_host, int32_t* vert_host) {
    if (!ctx) return fail(nullptr, C5_ERR_INVALID, "null context");
    const char* const name = "c5_shape_prior_rest_data";
    const size_t n = static_cast<size_t>(std::max<int64_t>(ctx->n_cells, 0));
    char* base = nullptr;
    if (n > 0 && !ctx->hr_count) {
        int rc = bind_device(ctx);
        if (rc) return rc;
        C5_HIP(ctx, ctx->shape.io.ensure(std::max(96 * n, 3 * pad256(points_bytes(ctx)) + 256)));
        base = ctx->shape.io.as<char>();
    }
    double* const binv_dev = binv_host && base ? reinterpret_cast<double*>(base) : nullptr;
    double* const vol_dev = vol_host && base ? reinterpret_cast<double*>(base + 72 * n) : nullptr;
    int32_t* const vert_dev = vert_host && base ? reinterpret_cast<int32_t*>(base + 80 * n) : nullptr;
    bool done = false;
    int rc = rest_data_device(ctx, name, binv_dev, vol_dev, vert_dev, done);
    if (rc || done) return rc;
    hipStream_t s = ctx->stream;
    if (binv_dev) C5_HIP(ctx, hipMemcpyAsync(binv_host, binv_dev, 72 * n, hipMemcpyDeviceToHost, s));
    if (vol_dev) C5_HIP(ctx, hipMemcpyAsync(vol_host, vol_dev, 8 * n, hipMemcpyDeviceToHost, s));
    if (vert_dev) C5_HIP(ctx, hipMemcpyAsync(vert_host, vert_dev, 16 * n, hipMemcpyDeviceToHost, s));
    C5_HIP(ctx, hipStreamSynchronize(s));
    return C5_OK;
}

int c5_shape_prior_gradient_device(c5_context* ctx, const c5_shape_prior* prior, const void* xyz_dev, void* value_dev, void* n_inverted_dev,
                                   void* grad_xyz_dev) {
    if (!ctx) return fail(nullptr, C5_ERR_INVALID, "null context");
    bool done = false;
    return apply_device(ctx, "c5_shape_prior_gradient", c5::kShapeGradient, prior, dptr(xyz_dev), nullptr, dptr(grad_xyz_dev), dptr(value_dev),
                        static_cast<long long*>(n_inverted_dev), done);
}

int c5_shape_prior_gradient(c5_context* ctx, const c5_shape_prior* prior, const double* xyz_host, double* value_host, int64_t* n_inverted,
                            double* grad_xyz_host) {
    return apply_host(ctx, "c5_shape_prior_gradient", c5::kShapeGradient, prior, xyz_host, nullptr, grad_xyz_host, value_host, n_inverted);
}

int c5_shape_prior_product_device(c5_context* ctx, const c5_shape_prior* prior, const void* xyz_dev, const void* v_xyz_dev, void* h_xyz_dev) {
    if (!ctx) return fail(nullptr, C5_ERR_INVALID, "null context");
    bool done = false;
    return apply_device(ctx, "c5_shape_prior_product", c5::kShapeProduct, prior, dptr(xyz_dev), dptr(v_xyz_dev), dptr(h_xyz_dev), nullptr, nullptr,
                        done);
}

int c5_shape_prior_product(c5_context* ctx, const c5_shape_prior* prior, const double* xyz_host, const double* v_xyz_host, double* h_xyz_host) {
    return apply_host(ctx, "c5_shape_prior_product", c5::kShapeProduct, prior, xyz_host, v_xyz_host, h_xyz_host, nullptr, nullptr);
}

int c5_shape_prior_diagonal_device(c5_context* ctx, const c5_shape_prior* prior, const void* xyz_dev, void* diag_xyz_dev) {
    if (!ctx) return fail(nullptr, C5_ERR_INVALID, "null context");
    bool done = false;
    return apply_device(ctx, "c5_shape_prior_diagonal", c5::kShapeDiagonal, prior, dptr(xyz_dev), nullptr, dptr(diag_xyz_dev), nullptr, nullptr, done);
}

int c5_shape_prior_diagonal(c5_context* ctx, const c5_shape_prior* prior, const double* xyz_host, double* diag_xyz_host) {
    return apply_host(ctx, "c5_shape_prior_diagonal", c5::kShapeDiagonal, prior, xyz_host, nullptr, diag_xyz_host, nullptr, nullptr);
}

int c5_shape_prior_quality_device(c5_context* ctx, const void* xyz_dev, void* ratio_dev, void* n_inverted_dev) {
    if (!ctx) return fail(nullptr, C5_ERR_INVALID, "null context");
    bool done = false;
    return quality_device(ctx, "c5_shape_prior_quality", dptr(xyz_dev), dptr(ratio_dev), static_cast<long long*>(n_inverted_dev), done);
}

int c5_shape_prior_quality(c5_context* ctx, const double* xyz_host, double* ratio_host, int64_t* n_inverted) {
    if (!ctx) return fail(nullptr, C5_ERR_INVALID, "null context");
    const char* const name = "c5_shape_prior_quality";
    if (!xyz_host) return fail(ctx, C5_ERR_INVALID, "%s: null array", name);
    int rc = bind_device(ctx);
    if (rc) return rc;
    const size_t pb = pad256(points_bytes(ctx)), cb = pad256(static_cast<size_t>(std::max<int64_t>(ctx->n_cells, 0)) * sizeof(double));
    C5_HIP(ctx, ctx->shape.io.ensure(std::max(pb + cb + 256, 3 * pb + 256)));
    char* const base = ctx->shape.io.as<char>();
    hipStream_t s = ctx->stream;
    if (ctx->n_cells > 0 && ctx->n_pts > 0) C5_HIP(ctx, hipMemcpyAsync(base, xyz_host, points_bytes(ctx), hipMemcpyHostToDevice, s));
    double* const ratio_dev = ratio_host ? reinterpret_cast<double*>(base + pb) : nullptr;
    long long* const inv_dev = n_inverted ? reinterpret_cast<long long*>(base + pb + cb) : nullptr;
    bool done = false;
    rc = quality_device(ctx, name, reinterpret_cast<const double*>(base), ratio_dev, inv_dev, done);
    if (rc) return rc;
    if (!done && ratio_dev) C5_HIP(ctx, hipMemcpyAsync(ratio_host, ratio_dev, static_cast<size_t>(ctx->n_cells) * sizeof(double), hipMemcpyDeviceToHost, s));
    if (n_inverted) C5_HIP(ctx, hipMemcpyAsync(n_inverted, inv_dev, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    C5_HIP(ctx, hipStreamSynchronize(s));
    return C5_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------
// Derivative renders in the geometry (geometry_derivative_kernels.hip): the motion tangent, the vertex adjoint (single,
// batched, and its exact sums), the vertex tangent and the vertex Gauss-Newton product - the enqueue functions over
// derivative_host.hpp and, next to them, their entry points; and the host-only c5_rotation_motion.
// ------------------------------------------------------------------------------------------
#include "derivative_host.hpp"

using namespace c5api;

// The point -> (cell, local vertex) incidence table of the grid on the device, built by the host at the first exact vertex or shape prior
// call after an upload: per point its entries 4 * (device cell) + (vertex) in ascending order of the CALLER's cell index,
// so that the per-point sums do not depend on "cell_order".  Connectivity only: c5_update_points keeps it.  Cells name
// the representatives of welded points: the others' lists are empty.
int c5api::vertex_incidence(c5_context* ctx, c5::VertexIncidence& inc) {
    const int64_t n_pts = ctx->n_pts, n_cells = ctx->n_cells;
    if (ctx->deriv.vtx_inc_serial != ctx->grid_serial || !ctx->deriv.vtx_inc.ptr) {
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
        C5_HIP(ctx, ctx->deriv.vtx_inc.ensure(tab.size() * sizeof(int32_t)));
        C5_HIP(ctx, hipMemcpy(ctx->deriv.vtx_inc.ptr, tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        ctx->deriv.vtx_inc_serial = ctx->grid_serial;
    }
    inc.ptr = ctx->deriv.vtx_inc.as<int32_t>();
    inc.idx = inc.ptr + n_pts + 1;
    return C5_OK;
}

namespace {

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
        return commit_derivative(ctx, v, "motion tangent");
    }
    const int width = batch_width(ctx, n);
    c5::MotionParams mp{};
    mp.w = v.w;
    mp.geo = v.geo;
    mp.image_px = v.n_px;
    for (const Chunk c : Chunks{n, width}) {
        mp.n_used = c.n_used;
        mp.out = out + c.k0 * v.n_px;
        mp.keep_entries = v.keep(c.more);
        for (int j = 0; j < c5::kMotionWidth; ++j)
            for (int i = 0; i < 12; ++i) mp.field[j][i] = j < mp.n_used ? fields[12 * (c.k0 + j) + i] : 0.0;
        c5::launch_motion_walk(v.s, width, mp);
    }
    return commit_derivative(ctx, v, "motion tangent");
}

// ---- exact vertex adjoint sums ("vertex_exact", c5_render_vertex_exact_*)

// The exact vertex sums' buffer over the context's cells - 240 bytes per cell (192 of words, 48 of exponents) and the
// misfit word, allocated here at the first exact vertex call - with the word width of the WHOLE image (c5_set_image).
int vertex_exact_sums(c5_context* ctx, c5::VertexExactSums& x) {
    const size_t n_cells = static_cast<size_t>(ctx->n_cells);
    int m;
    if (const int rc = exact_word_bits(ctx, ctx->im.res_x, ctx->im.res_y, m)) return rc;
    C5_HIP(ctx, ctx->deriv.vtx_exact.ensure(n_cells * 240 + 8));
    x = c5::VertexExactSums{};
    x.words = ctx->deriv.vtx_exact.as<long long>();
    x.exps = reinterpret_cast<int32_t*>(x.words + 24 * n_cells);  // (192 n_cells bytes on: 16-byte aligned)
    x.misfits = reinterpret_cast<unsigned*>(x.exps + 12 * n_cells);
    x.word_bits = m;
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

// exact_passes' family of the vertex adjoint: pass 1 is the adjoint's
struct VertexExact {
    using Sums = c5::VertexExactSums;
    c5::AdjointParams ap{};
    c5::VertexParams vp{};  // (on the lists: grad_out alone)
    int init(c5_context* ctx, const DerivativeView& v, const float2* grad_out) {
        if (!v.bin_sort) return vertex_params(ctx, v, grad_out, ap, vp);
        vp.grad_out = grad_out;
        return C5_OK;
    }
    void clear(const DerivativeView& v, const Sums& x, int64_t n_cells, unsigned flags) const {
        c5::launch_vertex_exact_clear(v.s, x, n_cells, flags & kBounds, flags & kSums, (flags & kSums) && (flags & kFirst));
    }
    void pass1(const DerivativeView& v) const { c5::launch_adjoint_walk(v.s, ap, 1); }
    void walk(const DerivativeView& v, const Sums& x, bool sums) const { c5::launch_vertex_exact_walk(v.s, vp, x, sums); }
    void resolve(const DerivativeView& v, const Sums& x, bool sums) const { c5::launch_vertex_exact_resolve(v.s, v.r, vp.grad_out, x, sums); }
};

int vertex_exact_passes(c5_context* ctx, DerivativeView& v, const c5::VertexExactSums& x, const float2* grad_out, unsigned flags) {
    VertexExact f;
    if (const int rc = f.init(ctx, v, grad_out)) return rc;
    exact_passes(ctx, v, f, x, flags);
    return C5_OK;
}

// Steps 1 (the finish of the words) to 4 of the exact vertex adjoint on x's exponents and words (device order): face_w,
// the per-cell triples, the per-point gather over the incidence table and the view's M^T, into grad_xyz [n_pts][3].
int vertex_exact_finish(c5_context* ctx, const DerivativeView& v, const c5::VertexExactSums& x, double* grad_xyz) {
    DerivativeState& d = ctx->deriv;
    const size_t n_cells = static_cast<size_t>(ctx->n_cells);
    C5_HIP(ctx, d.vtx_face.ensure(12 * n_cells * sizeof(double)));
    C5_HIP(ctx, d.vtx_triples.ensure(12 * n_cells * sizeof(double)));
    c5::VertexIncidence inc;
    int rc = vertex_incidence(ctx, inc);
    if (rc) return rc;
    c5::launch_vertex_exact_finish(v.s, x, v.geo, ctx->n_cells, d.vtx_face.as<double>(), d.vtx_triples.as<double>(), inc, ctx->n_pts,
                                   ctx->view, grad_xyz);
    return C5_OK;
}

// "vertex_exact" 1: images k0 .. k0 + n - 1 of a call of n_total upstream images (grad_out: image k0) -> rows k0 .. of
// grad_xyz [n_total][n_pts][3], every image through passes E and S and the finish, one after the other; pass 1 runs once,
// before the call's first image - or not at all where Lambda is there (`have_lambda`: the vertex Gauss-Newton product's
// pass A left it).  The call's last image hands the heads back cleared; the caller commits (commit_exact).
// "vertex_merge" has no say here.
int vertex_exact_images(c5_context* ctx, DerivativeView& v, const c5::VertexExactSums& x, int n, const float2* grad_out, double* grad_xyz,
                        bool have_lambda = false, int k0 = 0, int n_total = -1) {
    if (n_total < 0) n_total = n;
    for (int j = 0; j < n; ++j) {
        const int k = k0 + j;
        int rc = vertex_exact_passes(ctx, v, x, grad_out + j * v.n_px, exact_image_flags(k, n_total, have_lambda));
        if (!rc) rc = vertex_exact_finish(ctx, v, x, grad_xyz + 3 * k * ctx->n_pts);
        if (rc) return rc;
    }
    return C5_OK;
}

// ... as a whole call: the sums' buffer, the n images, the commit
int enqueue_vertex_exact_images(c5_context* ctx, DerivativeView& v, int n, const float2* grad_out, double* grad_xyz, const char* what) {
    c5::VertexExactSums x;
    int rc = vertex_exact_sums(ctx, x);
    if (!rc) rc = vertex_exact_images(ctx, v, x, n, grad_out, grad_xyz);
    return rc ? rc : commit_exact(ctx, v, x.misfits, what);
}

// c5_render_vertex_exact_bounds: pass 1 and pass E over the context's rows; the exponents in the caller's cell order.
// Pass E leaves the heads in place: the next per-view setup clears them.
int enqueue_vertex_exact_bounds(c5_context* ctx, const float2* grad_out, int32_t* exps) {
    DerivativeView v;
    int rc = setup_derivative(ctx, v);
    if (rc || v.no_cells) return rc;
    c5::VertexExactSums x;
    rc = vertex_exact_sums(ctx, x);
    if (!rc) rc = vertex_exact_passes(ctx, v, x, grad_out, kBounds);
    if (rc) return rc;
    c5::launch_vertex_exact_emit(v.s, x, v.perm, ctx->n_cells, exps, nullptr);
    return commit_derivative(ctx, v, "vertex exact bounds");
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
    rc = vertex_exact_passes(ctx, v, x, grad_out, kSums | kFirst);
    if (rc) return rc;
    c5::launch_vertex_exact_emit(v.s, x, v.perm, ctx->n_cells, nullptr, sums);
    return commit_exact(ctx, v, x.misfits, "vertex exact sums");
}

// c5_vertex_exact_finish: the per-view setup (the finish wants the points in view space), the caller's exponents and words
// into device order, and the finish.  No walk: the entry lists the setup built stay unused, and the next setup clears them.
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
    return rc ? rc : commit_derivative(ctx, v, "vertex exact finish");
}

// One vertex adjoint over the view: the per-face weights and the view-space gradient zeroed, the adjoint's pass 1 and
// vertex_walk (or vertex_resolve over bin_sort_resolve's lists), then vertex_finish into the caller's [n_pts][3] (the
// caller's point order is the device's: only the cells are reordered).  have_lambda: Lambda is there (the vertex
// Gauss-Newton product's pass A left it, with the heads in place): pass 1 is not launched.
int vertex_one(c5_context* ctx, DerivativeView& v, const float2* grad_out, double* grad_xyz, bool have_lambda = false) {
    DerivativeState& d = ctx->deriv;
    const size_t n_cells = static_cast<size_t>(ctx->n_cells), n_pts = static_cast<size_t>(ctx->n_pts);
    C5_HIP(ctx, d.vtx_face.ensure(12 * n_cells * sizeof(double)));
    C5_HIP(ctx, d.vtx_grad.ensure(3 * n_pts * sizeof(double)));
    double* const face_w = d.vtx_face.as<double>();
    double* const grad_view = d.vtx_grad.as<double>();
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
        v.keep(false);  // (vertex_walk hands every head back cleared)
        c5::launch_vertex_walk(v.s, vp, d.vertex_merge != 0);
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
    if (ctx->deriv.vertex_exact) return enqueue_vertex_exact_images(ctx, v, 1, grad_out, grad_xyz, "vertex adjoint");
    rc = vertex_one(ctx, v, grad_out, grad_xyz);
    return rc ? rc : commit_derivative(ctx, v, "vertex adjoint");
}

// The batched vertex walk over the view: its buffers (Lambda's, [n_cells][width][12] weights and [n_pts][3][width] view-space
// sums) and its parameters but for the chunk's (grad_out, n_used, keep_entries).
int vertex_batch_params(c5_context* ctx, const DerivativeView& v, int width, c5::VertexBatchParams& vb) {
    DerivativeState& d = ctx->deriv;
    const size_t n_cells = static_cast<size_t>(ctx->n_cells), n_pts = static_cast<size_t>(ctx->n_pts);
    C5_HIP(ctx, d.adj_lambda.ensure(static_cast<size_t>(v.padded) * sizeof(double)));
    C5_HIP(ctx, d.vtx_bat_face.ensure(12 * n_cells * width * sizeof(double)));
    C5_HIP(ctx, d.vtx_bat_grad.ensure(3 * n_pts * width * sizeof(double)));
    vb = c5::VertexBatchParams{};
    vb.w = v.w;
    vb.geo = v.geo;
    vb.image_px = v.n_px;
    vb.lambda = d.adj_lambda.as<double>();
    vb.face_w = d.vtx_bat_face.as<double>();
    return C5_OK;
}

// ... and one chunk of it: the two buffers zeroed, the walk (which hands the heads back unless c.more), the batched finish
// into rows c.k0 .. of the caller's array
int vertex_chunk(c5_context* ctx, DerivativeView& v, int width, c5::VertexBatchParams& vb, const Chunk& c, double* grad_xyz) {
    const size_t n_cells = static_cast<size_t>(ctx->n_cells), n_pts = static_cast<size_t>(ctx->n_pts);
    double* const grad_view = ctx->deriv.vtx_bat_grad.as<double>();
    vb.n_used = c.n_used;
    vb.keep_entries = v.keep(c.more);
    C5_HIP(ctx, hipMemsetAsync(vb.face_w, 0, 12 * n_cells * width * sizeof(double), v.s));
    C5_HIP(ctx, hipMemsetAsync(grad_view, 0, 3 * n_pts * width * sizeof(double), v.s));
    c5::launch_vertex_walk_batch(v.s, width, vb);
    c5::launch_vertex_finish_batch(v.s, width, v.geo, ctx->n_cells, vb.face_w, grad_view, ctx->n_pts, ctx->view, c.k0, vb.n_used, grad_xyz);
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
    if (ctx->deriv.vertex_exact) return enqueue_vertex_exact_images(ctx, v, n, grad_out, grad_xyz, "vertex adjoint batch");
    const size_t n_pts = static_cast<size_t>(ctx->n_pts);
    if (v.bin_sort) {
        for (int j = 0; j < n && !rc; ++j) rc = vertex_one(ctx, v, grad_out + j * v.n_px, grad_xyz + 3 * j * n_pts);
        return rc ? rc : commit_derivative(ctx, v, "vertex adjoint batch");
    }
    const int width = batch_width(ctx, n);
    c5::AdjointParams ap;
    c5::VertexBatchParams vb;
    rc = adjoint_params(ctx, v, ap);
    if (!rc) rc = vertex_batch_params(ctx, v, width, vb);
    if (rc) return rc;
    c5::launch_adjoint_walk(v.s, ap, 1);
    for (const Chunk c : Chunks{n, width}) {
        vb.grad_out = grad_out + c.k0 * v.n_px;
        rc = vertex_chunk(ctx, v, width, vb, c, grad_xyz);
        if (rc) return rc;
    }
    return commit_derivative(ctx, v, "vertex adjoint batch");
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
    C5_HIP(ctx, ctx->deriv.vtx_vel.ensure(3 * static_cast<size_t>(width) * static_cast<size_t>(ctx->n_pts) * sizeof(double)));
    double* const u_view = ctx->deriv.vtx_vel.as<double>();
    c5::VertexTangentParams vt{};
    vt.w = v.w;
    vt.geo = v.geo;
    vt.u_view = u_view;
    vt.image_px = v.n_px;
    for (const Chunk c : Chunks{n, width}) {
        vt.n_used = c.n_used;
        c5::launch_vertex_velocity(v.s, width, d_xyz, ctx->n_pts, c.k0, vt.n_used, ctx->view, u_view);
        if (v.bin_sort) {
            for (int j = 0; j < vt.n_used; ++j)
                c5::launch_vertex_tangent_resolve(v.s, v.r, u_view, width, j, out + (c.k0 + j) * v.n_px);
            continue;
        }
        vt.out = out + c.k0 * v.n_px;
        vt.keep_entries = v.keep(c.more);
        c5::launch_vertex_tangent_walk(v.s, width, vt);
    }
    return commit_derivative(ctx, v, "vertex tangent");
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
    DerivativeState& d = ctx->deriv;
    const int64_t n_px = v.n_px, n_pts = ctx->n_pts;
    const int width = batch_width(ctx, n);
    const bool exact = d.vertex_exact != 0;
    c5::VertexExactSums x{};
    if (exact) {
        rc = vertex_exact_sums(ctx, x);
        if (rc) return rc;
    }
    auto commit = [&] { return exact ? commit_exact(ctx, v, x.misfits, "vertex gn product") : commit_derivative(ctx, v, "vertex gn product"); };
    C5_HIP(ctx, d.vtx_vel.ensure(3 * static_cast<size_t>(width) * static_cast<size_t>(n_pts) * sizeof(double)));
    double* const u_view = d.vtx_vel.as<double>();
    if (v.bin_sort) {
        C5_HIP(ctx, d.gn_g.ensure(2 * static_cast<size_t>(n_px) * sizeof(float2) + 16));
        float2* const g = d.gn_g.as<float2>();
        for (const Chunk c : Chunks{n, width}) {
            c5::launch_vertex_velocity(v.s, width, d_xyz, n_pts, c.k0, c.n_used, ctx->view, u_view);
            for (int j = c.k0; j < c.k0 + c.n_used; ++j) {
                float2* const t = jv_out ? jv_out + j * n_px : g + n_px;
                c5::launch_vertex_tangent_resolve(v.s, v.r, u_view, width, j - c.k0, t);
                c5::launch_gn_weight(v.s, t, weight, n_px, 1, g);
                rc = exact ? vertex_exact_images(ctx, v, x, 1, g, h_xyz, true, j, n) : vertex_one(ctx, v, g, h_xyz + 3 * j * n_pts);
                if (rc) return rc;
            }
        }
        return commit();
    }
    const bool batched = !exact && n > 1;
    c5::VertexBatchParams vb{};
    if (batched) rc = vertex_batch_params(ctx, v, width, vb);
    else C5_HIP(ctx, d.adj_lambda.ensure(static_cast<size_t>(v.padded) * sizeof(double)));
    if (rc) return rc;
    C5_HIP(ctx, d.gn_g.ensure(static_cast<size_t>(width) * n_px * sizeof(float2) + 16));
    c5::VertexGnWalkParams ga{};
    ga.w = v.w;
    ga.geo = v.geo;
    ga.u_view = u_view;
    ga.weight = weight;
    ga.lambda = d.adj_lambda.as<double>();
    ga.g = d.gn_g.as<float2>();
    ga.image_px = n_px;
    vb.grad_out = ga.g;
    for (const Chunk c : Chunks{n, width}) {
        ga.n_used = c.n_used;
        ga.jv_out = jv_out ? jv_out + c.k0 * n_px : nullptr;
        c5::launch_vertex_velocity(v.s, width, d_xyz, n_pts, c.k0, ga.n_used, ctx->view, u_view);
        c5::launch_vertex_gn_walk_a(v.s, width, ga);
        if (exact) rc = vertex_exact_images(ctx, v, x, c.n_used, ga.g, h_xyz, true, c.k0, n);
        else if (batched) rc = vertex_chunk(ctx, v, width, vb, c, h_xyz);
        else rc = vertex_one(ctx, v, ga.g, h_xyz, true);
        if (rc) return rc;
    }
    return commit();
}

}  // namespace

extern "C" {

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

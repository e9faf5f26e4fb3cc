// ------------------------------------------------------------------------------------------
// Derivative renders, host side: the per-view setup every derivative starts with, the commit it ends with and what the
// wait behind it makes of its status words (derivative_host.hpp).
// ------------------------------------------------------------------------------------------
#include "derivative_host.hpp"
#include "exact_sum.hpp"

namespace c5api __attribute__((visibility("hidden"))) {

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

    C5_HIP(ctx, ctx->deriv.adj_counters.ensure(kCountersBytes));
    C5_HIP(ctx, ctx->deriv.adj_sticky.ensure(kStickyWords * sizeof(unsigned)));
    if (!ctx->deriv.adj_status) {
        C5_HIP(ctx, hipHostMalloc(reinterpret_cast<void**>(&ctx->deriv.adj_status), 5 * sizeof(unsigned), hipHostMallocDefault));
        ctx->deriv.adj_status[3] = 0;  // (rows a ray matrix fill found changed: written by that call alone, cleared by finish_adjoint)
        ctx->deriv.adj_status[4] = 0;  // (contributions an exact sum found beyond their cell's exponent: the same)
    }
    rc = ensure_device_perm(ctx);
    if (rc) return rc;
    v.perm = ctx->cell_perm.empty() ? nullptr : ctx->adj_perm.as<int32_t>();
    c5::FrameCounters* const counters = ctx->deriv.adj_counters.as<c5::FrameCounters>();
    C5_HIP(ctx, hipMemsetAsync(ctx->deriv.adj_sticky.ptr, 0, kStickyWords * sizeof(unsigned), s));

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
        v.heads_cleared = fs.head_clean;  // (nothing on the lists touches the heads)
        v.r = c5::ResolveParams{g, im, ctx->xtab.as<double>(), ctx->ytab.as<double>(), ctx->offs64.as<int64_t>(), ctx->segs.ptr,
                                v.mask, ctx->alpha_limit};
    } else {
        const double key_slack = entry_key_slack(ctx);
        c5::launch_build_records(s, g, ctx->alpha_limit, 0);
        if (!fs.head_clean) C5_HIP(ctx, hipMemsetAsync(fs.head.ptr, 0, static_cast<size_t>(padded) * sizeof(c5::EntryHead), s));
        fs.head_clean = false;  // (the raster's heads are live until a walk hands them back: DerivativeView::keep)
        c5::launch_entry_lists(s, g, ctx->xtab.as<double>(), ctx->ytab.as<double>(), im, fs.head.as<c5::EntryHead>(),
                               fs.first.as<c5::Entry>(), fs.pool.as<c5::Entry>(), fs.entry_capacity, counters,
                               ctx->deriv.adj_sticky.as<unsigned>(), 0, key_slack);
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
        wp.sticky = ctx->deriv.adj_sticky.as<unsigned>();
    }
    return C5_OK;
}

int commit_derivative(c5_context* ctx, const DerivativeView& v, const char* what) {
    FrameSlot& fs = ctx->slots[0];
    hipStream_t s = ctx->stream;
    C5_HIP(ctx, hipGetLastError());
    C5_HIP(ctx, hipMemcpyAsync(ctx->deriv.adj_status, &ctx->deriv.adj_counters.as<c5::FrameCounters>()->walk_overflow,
                               kStatusWords * sizeof(unsigned), hipMemcpyDeviceToHost, s));
    if (ctx->pipeline) {  // (the next frame's setup on the auxiliary stream waits for slot 0's buffers)
        C5_HIP(ctx, hipEventRecord(fs.walk_done, s));
        fs.walk_recorded = true;
    }
    fs.head_clean = v.heads_cleared;
    ctx->deriv.adjoint_pending = true;
    ctx->deriv.adj_what = what;
    return C5_OK;
}

int commit_exact(c5_context* ctx, const DerivativeView& v, const unsigned* misfits, const char* what) {
    int rc = commit_derivative(ctx, v, what);
    if (rc) return rc;
    C5_HIP(ctx, hipMemcpyAsync(ctx->deriv.adj_status + 4, misfits, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    return C5_OK;
}

int adjoint_params(c5_context* ctx, const DerivativeView& v, c5::AdjointParams& ap) {
    C5_HIP(ctx, ctx->deriv.adj_lambda.ensure(static_cast<size_t>(v.padded) * sizeof(double)));
    ap = c5::AdjointParams{};
    ap.w = v.w;
    ap.lambda = ctx->deriv.adj_lambda.as<double>();
    return C5_OK;
}

int exact_word_bits(c5_context* ctx, int res_x, int res_y, int& m) {
    m = c5::exact::word_bits(static_cast<int64_t>(res_x) * res_y);
    if (m < c5::exact::kMinWordBits)
        return fail(ctx, C5_ERR_INVALID, "exact sums: an image of %d x %d pixels leaves %d bits per word", res_x, res_y, m);
    return C5_OK;
}

int zero_tangents(c5_context* ctx, const DerivativeView& v, int n, float2* out) {
    if (out && v.n_px > 0) C5_HIP(ctx, hipMemsetAsync(out, 0, static_cast<size_t>(n) * v.n_px * sizeof(float2), v.s));
    return C5_OK;
}

int batch_width(const c5_context* ctx, int n) {
    if (ctx->deriv.batch_width) return ctx->deriv.batch_width;
    return n <= 4 ? 4 : 8;
}

int check_derivative(c5_context* ctx, const DerivativeCall& c) {
    if (!ctx) return fail(nullptr, C5_ERR_INVALID, "null context");
    if (c.n < 1) return fail(ctx, C5_ERR_INVALID, "a batch needs at least one %s (%d)", c.batch_of, c.n);
    if (!c.required_ok || (ctx->n_cells > 0 && !c.per_cell_ok)) return fail(ctx, C5_ERR_INVALID, "%s", c.pointer_msg);
    if (c.refuse_async && ctx->hr_count) return fail(ctx, C5_ERR_STATE, "%s while c5_render_host_async frames are outstanding", c.name);
    if (!c.host) return C5_OK;
    if (!ctx->have_image) return fail(ctx, C5_ERR_STATE, "critical error. empty plane");  // plane.cpp:151-153
    return bind_device(ctx);
}

// After the stream drained: the failure words of the last adjoint or tangent (as finish_frame treats a frame's).
int finish_adjoint(c5_context* ctx) {
    if (!ctx->deriv.adjoint_pending) return C5_OK;
    ctx->deriv.adjoint_pending = false;
    const unsigned lost_rays = ctx->deriv.adj_status[0], refused = ctx->deriv.adj_status[1], overlap_rays = ctx->deriv.adj_status[2];
    const unsigned changed_rows = ctx->deriv.adj_status[3];  // (a ray matrix fill's; short rows of a call that has to be run again anyway come last)
    ctx->deriv.adj_status[3] = 0;
    const unsigned misfits = ctx->deriv.adj_status[4];  // (an exact sum's pass S; the same)
    ctx->deriv.adj_status[4] = 0;
    if (refused) {
        int rc = drain(ctx);
        if (rc) return rc;
        rc = grow_entry_pools(ctx, std::min<int64_t>(2 * (ctx->slots[0].entry_capacity + refused) + 8192, kMaxEntryPool));
        if (rc) return rc;
        return fail(ctx, C5_RETRY, "%s: %u boundary entries found no room in the overflow pool (now %lld records): run it again",
                    ctx->deriv.adj_what, refused, static_cast<long long>(ctx->slots[0].entry_capacity));
    }
    if (lost_rays) return fail(ctx, C5_ERR_WALK, "%s: %u rays exceeded the walk step bound (malformed grid?)", ctx->deriv.adj_what, lost_rays);
    if (overlap_rays) {
        ctx->overlap_seen = true;  // (what the next frame would find out for itself: bin_sort_resolve from now on)
        ++ctx->setup_epoch;
        return fail(ctx, C5_RETRY,
                    "%s: %u rays met a boundary entry inside a stretch of cells they had walked: components of the grid "
                    "interpenetrate; run it again (bin_sort_resolve from now on)", ctx->deriv.adj_what, overlap_rays);
    }
    if (changed_rows)
        return fail(ctx, C5_ERR_STATE,
                    "%s: the frame changed between c5_ray_matrix_rows and c5_ray_matrix_fill: %u rows differ from row_ptr's or found no "
                    "room below capacity", ctx->deriv.adj_what, changed_rows);
    if (misfits)
        return fail(ctx, C5_ERR_INVALID,
                    "%s: %u contributions lie beyond their cell's exponent and were added nowhere: the exponents given are too small "
                    "(take the elementwise max of c5_render_exact_bounds - the vertex sums: c5_render_vertex_exact_bounds - over "
                    "every part of the image)", ctx->deriv.adj_what, misfits);
    return C5_OK;
}

}  // namespace c5api

// Context, image, solids and options of the C ABI (include/course5_hip.h); what every file of the library uses to report
// a failure.  No exceptions cross the ABI; every entry point returns a status and leaves a message for c5_last_error().
#include "context.hpp"

namespace c5api __attribute__((visibility("hidden"))) {

namespace {
std::string g_create_error;
}

int fail(c5_context* ctx, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx)
        ctx->error = buf;
    else
        g_create_error = buf;
    return code;
}

int bind_device(c5_context* ctx) {
    C5_HIP(ctx, hipSetDevice(ctx->device));
    return C5_OK;
}

int to_rotation_list(c5_context* ctx, const c5_rotation* rots, int n, c5::RotationList& out) {
    if (n < 0 || n > C5_MAX_ROTATIONS) return fail(ctx, C5_ERR_INVALID, "rotation count %d out of range", n);
    if (n > 0 && !rots) return fail(ctx, C5_ERR_INVALID, "null rotation list");
    out.n = n;
    for (int k = 0; k < n; ++k) {
        if (rots[k].axis != 0 && rots[k].axis != 1)
            return fail(ctx, C5_ERR_INVALID, "rotation axis must be 0 (x) or 1 (y)");
        out.axis[k] = rots[k].axis;
        // libm on the host, like tetra.cpp:46-47,58-59
        out.cosv[k] = std::cos(rots[k].angle);
        out.sinv[k] = std::sin(rots[k].angle);
        out.x0[k] = rots[k].x0;
    }
    return C5_OK;
}

// tetra.cpp:44-62 on the host (what rotate_point does on the device), for bounding boxes and centres
void rotate_host(const c5::RotationList& R, double c[3]) {
    for (int r = 0; r < R.n; ++r) {
        const double co = R.cosv[r], si = R.sinv[r];
        if (R.axis[r] == 0) {
            const double y_old = c[1];
            c[1] = c[1] * co - c[2] * si;
            c[2] = y_old * si + c[2] * co;
        } else {
            c[0] -= R.x0[r];
            const double x_old = c[0];
            c[0] = c[0] * co - c[2] * si;
            c[2] = x_old * si + c[2] * co;
            c[0] += R.x0[r];
        }
    }
}

// Wait until nothing of this context is running (both streams).
int drain(c5_context* ctx) {
    C5_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->aux_stream) C5_HIP(ctx, hipStreamSynchronize(ctx->aux_stream));
    if (ctx->side_stream) C5_HIP(ctx, hipStreamSynchronize(ctx->side_stream));
    return C5_OK;
}

int grow_entry_pools(c5_context* ctx, int64_t want) {
    for (int k = 0; k < (ctx->pipeline ? kFrameSlots : 1); ++k) {
        FrameSlot& o = ctx->slots[k];
        if (o.entry_capacity >= want) continue;
        o.entry_capacity = want;
        C5_HIP(ctx, o.pool.ensure(static_cast<size_t>(want) * sizeof(c5::Entry)));
        ++ctx->setup_epoch;  // (the entry lists lived in the old pool)
    }
    return C5_OK;
}
}  // namespace c5api

using namespace c5api;

namespace {

int recompute_rows(c5_context* ctx) {
    c5::ImageParams& im = ctx->im;
    im.tile_rows = (ctx->cfg_tile_rows > 0) ? ctx->cfg_tile_rows : (im.res_y > 0 ? im.res_y : 1);
    im.rank = ctx->cfg_rank;
    im.world = ctx->cfg_world;
    im.row_begin = ctx->cfg_row_begin;
    im.row_count = (ctx->cfg_row_count < 0) ? im.res_y - im.row_begin : ctx->cfg_row_count;
    if (im.row_begin < 0 || im.row_count < 0 || im.row_begin + im.row_count > im.res_y)
        return fail(ctx, C5_ERR_INVALID, "row range [%d, %d) outside the image of %d rows", im.row_begin,
                    im.row_begin + im.row_count, im.res_y);
    int n = 0;
    for (int r = 0; r < im.res_y; ++r)
        if (c5::local_row_of(im, r) >= 0) ++n;
    im.n_local_rows = n;
    ctx->row_costs_collected = false;
    return C5_OK;
}

int ensure_image_buffers(c5_context* ctx) {
    const c5::ImageParams& im = ctx->im;
    const int64_t n_px = static_cast<int64_t>(im.n_local_rows) * im.res_x;
    const int64_t padded = ((n_px + 1023) / 1024) * 1024;
    C5_HIP(ctx, ctx->out.ensure(static_cast<size_t>(padded) * sizeof(float) * 2));
    for (int k = 0; k < (ctx->pipeline ? kFrameSlots : 1); ++k) {
        FrameSlot& fs = ctx->slots[k];
        C5_HIP(ctx, fs.count.ensure(static_cast<size_t>(padded + 1024) * sizeof(int32_t)));
        C5_HIP(ctx, fs.head.ensure(static_cast<size_t>(padded) * sizeof(c5::EntryHead)));
        fs.head_clean = false;
        C5_HIP(ctx, fs.first.ensure(static_cast<size_t>(padded) * sizeof(c5::Entry)));
        C5_HIP(ctx, fs.mask.ensure(static_cast<size_t>(padded) * sizeof(uint32_t)));
        C5_HIP(ctx, fs.row_cost.ensure(static_cast<size_t>(im.n_local_rows + 64) * sizeof(uint32_t)));
        // overflow pool: second and further entries of a ray only.  A frame overflows iff its total demand
        // exceeds the capacity (entry_raster); finish_frame keeps the capacity at twice the demand of the
        // last frame it has seen, so only a jump of the demand between two looks can cost a C5_RETRY.
        if (fs.entry_capacity < n_px / 4 + 8192) {
            fs.entry_capacity = n_px / 4 + 8192;
            C5_HIP(ctx, fs.pool.ensure(static_cast<size_t>(fs.entry_capacity) * sizeof(c5::Entry)));
            ++ctx->setup_epoch;
        }
    }
    return C5_OK;
}

// whatever mask of its own a solid has is stale: every solid is rastered anew ("solid_cache", enqueue_solids)
void forget_solid_masks(c5_context* ctx) {
    for (Solid& so : ctx->solids) so.own_mask_ready = false, so.unchanged_frames = 0, so.seen_generation = ~uint64_t{0};
}
}  // namespace

extern "C" {

int c5_abi_version(void) { return C5_ABI_VERSION; }

int c5_device_count(int* count) {
    if (!count) return fail(nullptr, C5_ERR_INVALID, "null count");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return fail(nullptr, C5_ERR_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    *count = n;
    return C5_OK;
}

int c5_create(int device_ordinal, c5_context** out_ctx) {
    if (!out_ctx) return fail(nullptr, C5_ERR_INVALID, "null out_ctx");
    *out_ctx = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(nullptr, C5_ERR_NO_DEVICE, "no HIP device available (%s)",
                    e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
    if (device_ordinal < 0 || device_ordinal >= n)
        return fail(nullptr, C5_ERR_INVALID, "device ordinal %d out of range [0, %d)", device_ordinal, n);
    c5_context* ctx = new (std::nothrow) c5_context();
    if (!ctx) return fail(nullptr, C5_ERR_INVALID, "out of host memory");
    ctx->device = device_ordinal;
    auto bail = [&](hipError_t err, const char* what) {
        fail(nullptr, C5_ERR_HIP, "%s: %s", what, hipGetErrorString(err));
        c5_destroy(ctx);
        return C5_ERR_HIP;
    };
    if ((e = hipSetDevice(device_ordinal)) != hipSuccess) return bail(e, "hipSetDevice");
    {
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        if ((e = hipStreamCreateWithPriority(&ctx->own_stream, hipStreamNonBlocking, hi)) != hipSuccess)
            return bail(e, "hipStreamCreate");
    }
    ctx->stream = ctx->own_stream;
    {   // the setup stream only fills what the walk leaves idle: lowest priority
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        if ((e = hipStreamCreateWithPriority(&ctx->aux_stream, hipStreamNonBlocking, lo)) != hipSuccess)
            return bail(e, "hipStreamCreate");
    }
    if ((e = hipStreamCreateWithFlags(&ctx->side_stream, hipStreamNonBlocking)) != hipSuccess)
        return bail(e, "hipStreamCreate");
    if ((e = hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking)) != hipSuccess)
        return bail(e, "hipStreamCreate");
    for (c5_context::HostFrame& h : ctx->hring) {
        if ((e = hipEventCreateWithFlags(&h.rendered, hipEventDisableTiming)) != hipSuccess) return bail(e, "hipEventCreate");
        if ((e = hipEventCreateWithFlags(&h.copied, hipEventDisableTiming)) != hipSuccess) return bail(e, "hipEventCreate");
        if ((e = hipHostMalloc(reinterpret_cast<void**>(&h.status), 4 * sizeof(unsigned), hipHostMallocDefault)) != hipSuccess)
            return bail(e, "hipHostMalloc");
        h.status[0] = h.status[1] = h.status[2] = h.status[3] = 0;
    }
    for (int k = 0; k < 2; ++k)
        if ((e = hipEventCreateWithFlags(&ctx->stage_ev[k], hipEventDisableTiming)) != hipSuccess) return bail(e, "hipEventCreate");
    if ((e = hipEventCreateWithFlags(&ctx->fork_ev, hipEventDisableTiming)) != hipSuccess) return bail(e, "hipEventCreate");
    if ((e = hipEventCreateWithFlags(&ctx->join_ev, hipEventDisableTiming)) != hipSuccess) return bail(e, "hipEventCreate");
    for (FrameSlot& fs : ctx->slots) {
        for (auto& ev : fs.ev)
            if ((e = hipEventCreate(&ev)) != hipSuccess) return bail(e, "hipEventCreate");
        if ((e = hipEventCreateWithFlags(&fs.setup_done, hipEventDisableTiming)) != hipSuccess) return bail(e, "hipEventCreate");
        if ((e = hipEventCreateWithFlags(&fs.walk_done, hipEventDisableTiming)) != hipSuccess) return bail(e, "hipEventCreate");
        if ((e = fs.counters.ensure(kCountersBytes)) != hipSuccess) return bail(e, "hipMalloc");
        if ((e = hipHostMalloc(reinterpret_cast<void**>(&fs.host_counters), kCountersBytes, hipHostMallocDefault)) !=
            hipSuccess)
            return bail(e, "hipHostMalloc");
        std::memset(fs.host_counters, 0, kCountersBytes);
    }
    for (int k = 0; k < kWalkEventPool; ++k) {
        ctx->walk_a[k] = ctx->walk_b[k] = nullptr;
    }
    for (int k = 0; k < kWalkEventPool; ++k) {
        if ((e = hipEventCreate(&ctx->walk_a[k])) != hipSuccess) return bail(e, "hipEventCreate");
        if ((e = hipEventCreate(&ctx->walk_b[k])) != hipSuccess) return bail(e, "hipEventCreate");
    }
    // (a line of its own; cleared in the context's own stream and waited for — see finish_frame)
    if ((e = ctx->sticky.ensure(256)) != hipSuccess) return bail(e, "hipMalloc");
    if ((e = hipMemsetAsync(ctx->sticky.ptr, 0, 256, ctx->own_stream)) != hipSuccess) return bail(e, "hipMemsetAsync");
    if ((e = hipStreamSynchronize(ctx->own_stream)) != hipSuccess) return bail(e, "hipStreamSynchronize");
    if ((e = hipHostMalloc(reinterpret_cast<void**>(&ctx->host_sticky), 4 * sizeof(unsigned), hipHostMallocDefault)) != hipSuccess)
        return bail(e, "hipHostMalloc");
    for (int k = 0; k < 4; ++k) ctx->host_sticky[k] = 0;
    if ((e = hipHostMalloc(reinterpret_cast<void**>(&ctx->host_sb), c5::kMaxSbRows * sizeof(uint32_t), hipHostMallocDefault)) != hipSuccess)
        ctx->host_sb = nullptr;  // (the walk then starts its rows in image order)
    else
        std::memset(ctx->host_sb, 0, c5::kMaxSbRows * sizeof(uint32_t));
    ctx->view.n = 0;
    for (Solid& s : ctx->solids) s.rots.n = 0;
    *out_ctx = ctx;
    return C5_OK;
}

void c5_destroy(c5_context* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->aux_stream) (void)hipStreamSynchronize(ctx->aux_stream);
    DeviceBuffer* bufs[] = {&ctx->px, &ctx->py, &ctx->pz, &ctx->cell_vert, &ctx->cell_adj, &ctx->alpha,
                            &ctx->q, &ctx->bface, &ctx->xtab, &ctx->ytab, &ctx->out, &ctx->sticky,
                            &ctx->offs64, &ctx->scratch64, &ctx->segs, &ctx->adj_perm, &ctx->scal_stats};
    ctx->deriv.release();
    ctx->prior.release();
    ctx->shape.release();
    if (ctx->host_sticky) (void)hipHostFree(ctx->host_sticky);
    if (ctx->scal_host) (void)hipHostFree(ctx->scal_host);
    if (ctx->host_sb) (void)hipHostFree(ctx->host_sb);
    for (DeviceBuffer* b : bufs) b->release();
    for (FrameSlot& fs : ctx->slots) {
        DeviceBuffer* sb[] = {&fs.vx, &fs.vy, &fs.vz, &fs.rec, &fs.count, &fs.head, &fs.first, &fs.pool,
                              &fs.mask, &fs.counters, &fs.row_cost, &fs.sb, &fs.plane_cell, &fs.straddle, &fs.straddle_count,
                              &fs.partials, &fs.arrivals, &fs.bfrec};
        for (DeviceBuffer* b : sb) b->release();
        if (fs.host_counters) (void)hipHostFree(fs.host_counters);
        for (auto& ev : fs.ev)
            if (ev) (void)hipEventDestroy(ev);
        if (fs.setup_done) (void)hipEventDestroy(fs.setup_done);
        if (fs.walk_done) (void)hipEventDestroy(fs.walk_done);
    }
    for (Solid& so : ctx->solids) {
        so.raw.release();
        so.faces.release();
        for (DeviceBuffer& v : so.view) v.release();
        so.own_mask.release();
    }
    for (int k = 0; k < kWalkEventPool; ++k) {
        if (ctx->walk_a[k]) (void)hipEventDestroy(ctx->walk_a[k]);
        if (ctx->walk_b[k]) (void)hipEventDestroy(ctx->walk_b[k]);
    }
    if (ctx->copy_stream) (void)hipStreamSynchronize(ctx->copy_stream);
    for (c5_context::HostFrame& h : ctx->hring) {
        h.img.release();
        h.counters.release();
        if (h.rendered) (void)hipEventDestroy(h.rendered);
        if (h.copied) (void)hipEventDestroy(h.copied);
        if (h.status) (void)hipHostFree(h.status);
    }
    for (int k = 0; k < 2; ++k) {
        if (ctx->stage[k]) (void)hipHostFree(ctx->stage[k]);
        if (ctx->stage_ev[k]) (void)hipEventDestroy(ctx->stage_ev[k]);
    }
    if (ctx->copy_stream) (void)hipStreamDestroy(ctx->copy_stream);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    if (ctx->aux_stream) (void)hipStreamDestroy(ctx->aux_stream);
    if (ctx->side_stream) (void)hipStreamDestroy(ctx->side_stream);
    if (ctx->fork_ev) (void)hipEventDestroy(ctx->fork_ev);
    if (ctx->join_ev) (void)hipEventDestroy(ctx->join_ev);
    delete ctx;
}

int c5_set_stream(c5_context* ctx, void* hip_stream) {
    if (!ctx) return fail(nullptr, C5_ERR_INVALID, "null context");
    ++ctx->setup_epoch;  // whatever was built per view is stale ("view_cache")
    int rc = bind_device(ctx);
    if (rc) return rc;
    rc = wait_and_collect(ctx);
    ctx->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->own_stream;
    ctx->using_caller_stream = hip_stream != nullptr;
    return rc;  // C5_RETRY included: the stream IS switched, but the frames before the switch must be rendered again
}

const char* c5_last_error(const c5_context* ctx) { return ctx ? ctx->error.c_str() : g_create_error.c_str(); }

int c5_set_solid(c5_context* ctx, int slot, const double* tets, int64_t n_tets, double colour) {
    if (!ctx) return fail(nullptr, C5_ERR_INVALID, "null context");
    if (slot < 0 || slot >= C5_MAX_SOLIDS) return fail(ctx, C5_ERR_INVALID, "solid slot %d out of range", slot);
    if (n_tets < 0 || (n_tets > 0 && !tets)) return fail(ctx, C5_ERR_INVALID, "bad solid array");
    int rc = bind_device(ctx);
    if (rc) return rc;
    C5_HIP(ctx, hipStreamSynchronize(ctx->stream));
    Solid& s = ctx->solids[slot];
    int64_t others = 0;
    for (int k = 0; k < C5_MAX_SOLIDS; ++k)
        if (k != slot) others += ctx->solids[k].n_tets;
    if (others + n_tets >= static_cast<int64_t>(c5::kNoCell))
        return fail(ctx, C5_ERR_INVALID, "solid cell count does not fit 28 bits");
    s.n_tets = n_tets;
    s.colour = colour;
    s.n_points = s.n_faces = 0;
    s.n_interior = 0;
    s.groups.clear();
    ++s.generation;  // whatever mask of its own the slot had is stale
    s.own_mask_ready = false;
    if (n_tets > 0) {
        std::vector<double> pts;
        std::vector<int32_t> faces;
        c5::unique_solid_faces(tets, n_tets, pts, faces);
        s.n_points = static_cast<int64_t>(pts.size() / 3);
        s.n_faces = static_cast<int64_t>(faces.size() / 4);
        s.n_interior = 0;
        while (s.n_interior < s.n_faces && faces[4 * static_cast<size_t>(s.n_interior) + 3] != 0) ++s.n_interior;
        {   // bounding sphere about the centre of the bounding box (no rotation makes the solid reach further)
            double lo[3] = {pts[0], pts[1], pts[2]}, hi[3] = {pts[0], pts[1], pts[2]};
            for (size_t i = 0; i < pts.size(); i += 3)
                for (int d = 0; d < 3; ++d) lo[d] = std::min(lo[d], pts[i + d]), hi[d] = std::max(hi[d], pts[i + d]);
            for (int d = 0; d < 3; ++d) s.centre[d] = 0.5 * (lo[d] + hi[d]);
            double r2 = 0.0;
            for (size_t i = 0; i < pts.size(); i += 3) {
                double q = 0.0;
                for (int d = 0; d < 3; ++d) q += (pts[i + d] - s.centre[d]) * (pts[i + d] - s.centre[d]);
                r2 = std::max(r2, q);
            }
            s.radius = std::sqrt(r2);
        }
        {   // groups of faces of about the same size (see Solid::FaceGroup), the generator's order kept inside a group:
            // consecutive cells of init_polar are angular neighbours, their faces cover neighbouring pixels
            const size_t nf = faces.size() / 4;
            std::vector<double> edge(nf);
            std::vector<int> cls(nf);
            for (size_t f = 0; f < nf; ++f) {
                const double* a = &pts[3 * static_cast<size_t>(faces[4 * f])];
                const double* b = &pts[3 * static_cast<size_t>(faces[4 * f + 1])];
                const double* c = &pts[3 * static_cast<size_t>(faces[4 * f + 2])];
                auto d2 = [](const double* u, const double* v) {
                    return (u[0] - v[0]) * (u[0] - v[0]) + (u[1] - v[1]) * (u[1] - v[1]) + (u[2] - v[2]) * (u[2] - v[2]);
                };
                edge[f] = std::sqrt(std::max(d2(a, b), std::max(d2(b, c), d2(a, c))));
                int e = -1000;
                if (edge[f] > 0.0 && std::isfinite(edge[f])) (void)std::frexp(edge[f], &e);
                cls[f] = e;
            }
            std::vector<uint32_t> order(nf);
            for (size_t f = 0; f < nf; ++f) order[f] = static_cast<uint32_t>(f);
            std::stable_sort(order.begin(), order.end(), [&](uint32_t l, uint32_t r) {
                const bool li = static_cast<int64_t>(l) < s.n_interior, ri = static_cast<int64_t>(r) < s.n_interior;
                if (li != ri) return li;
                return cls[l] > cls[r];
            });
            std::vector<int32_t> sorted(faces.size());
            s.groups.clear();
            for (size_t k = 0; k < nf; ++k) {
                const uint32_t f = order[k];
                for (int d = 0; d < 4; ++d) sorted[4 * k + d] = faces[4 * static_cast<size_t>(f) + d];
                const bool interior = static_cast<int64_t>(f) < s.n_interior;
                const bool was_interior = k > 0 && static_cast<int64_t>(order[k - 1]) < s.n_interior;
                if (k == 0 || cls[f] != cls[order[k - 1]] || interior != was_interior)
                    s.groups.push_back(Solid::FaceGroup{static_cast<int64_t>(k), 0, 0.0});
                s.groups.back().count += 1;
                s.groups.back().longest = std::max(s.groups.back().longest, edge[f]);
            }
            faces.swap(sorted);
        }
        const size_t bytes = pts.size() * sizeof(double);
        C5_HIP(ctx, s.raw.ensure(bytes));
        C5_HIP(ctx, s.faces.ensure(faces.size() * sizeof(int32_t)));
        for (int k = 0; k < (ctx->pipeline ? kFrameSlots : 1); ++k) C5_HIP(ctx, s.view[k].ensure(bytes));
        C5_HIP(ctx, hipMemcpy(s.raw.ptr, pts.data(), bytes, hipMemcpyHostToDevice));
        C5_HIP(ctx, hipMemcpy(s.faces.ptr, faces.data(), faces.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    return C5_OK;
}

int c5_set_image(c5_context* ctx, int res_x, int res_y, const double* bounds4) {
    if (!ctx) return fail(nullptr, C5_ERR_INVALID, "null context");
    ++ctx->setup_epoch;  // whatever was built per view is stale ("view_cache")
    if (!bounds4) return fail(ctx, C5_ERR_INVALID, "plane initializer. wrong manual boundaries");  // plane.cpp:262-264
    if (res_x < 2 || res_y < 2) return fail(ctx, C5_ERR_INVALID, "critical error. empty plane");
    int rc = bind_device(ctx);
    if (rc) return rc;
    rc = drain(ctx);
    if (rc) return rc;
    std::memcpy(ctx->bounds, bounds4, sizeof ctx->bounds);
    c5::ImageParams& im = ctx->im;
    im.res_x = res_x;
    im.res_y = res_y;
    im.x_min = bounds4[1];
    im.y_min = bounds4[3];
    // plane.cpp:295-302
    im.step_x = (bounds4[0] - bounds4[1]) / (static_cast<double>(res_x) - 1.);
    im.step_y = (bounds4[2] - bounds4[3]) / (static_cast<double>(res_y) - 1.);
    for (im.fit_shift = 3;; ++im.fit_shift) {  // the depth sample (DepthSamples): the finest raster of at most kFitSlots boxes
        im.fit_cols = (res_x >> im.fit_shift) + 1;
        if (static_cast<int64_t>(im.fit_cols) * ((res_y >> im.fit_shift) + 1) <= c5::kFitSlots) break;
    }
    // plane.cpp:304-314: coordinates are running sums
    std::vector<double> X(static_cast<size_t>(res_x)), Y(static_cast<size_t>(res_y));
    double cx = bounds4[1];
    for (int i = 0; i < res_x; ++i) {
        X[static_cast<size_t>(i)] = cx;
        cx = cx + im.step_x;
    }
    double cy = bounds4[3];
    for (int j = 0; j < res_y; ++j) {
        Y[static_cast<size_t>(j)] = cy;
        cy = cy + im.step_y;
    }
    C5_HIP(ctx, ctx->xtab.ensure(X.size() * 8));
    C5_HIP(ctx, ctx->ytab.ensure(Y.size() * 8));
    C5_HIP(ctx, hipMemcpy(ctx->xtab.ptr, X.data(), X.size() * 8, hipMemcpyHostToDevice));
    C5_HIP(ctx, hipMemcpy(ctx->ytab.ptr, Y.data(), Y.size() * 8, hipMemcpyHostToDevice));
    ctx->host_ytab = Y;
    ctx->have_image = true;
    rc = recompute_rows(ctx);
    if (rc) return rc;
    return ensure_image_buffers(ctx);
}

int c5_set_row_tiles(c5_context* ctx, int tile_rows, int rank, int world) {
    if (!ctx) return fail(nullptr, C5_ERR_INVALID, "null context");
    ++ctx->setup_epoch;  // whatever was built per view is stale ("view_cache")
    if (world < 1 || rank < 0 || rank >= world) return fail(ctx, C5_ERR_INVALID, "bad rank/world %d/%d", rank, world);
    if (tile_rows < 0) return fail(ctx, C5_ERR_INVALID, "bad tile_rows");
    if (world > 1 && tile_rows == 0) return fail(ctx, C5_ERR_INVALID, "tile_rows must be > 0 when world > 1");
    ctx->cfg_tile_rows = tile_rows;
    ctx->cfg_rank = rank;
    ctx->cfg_world = world;
    if (ctx->have_image) {
        int rc = bind_device(ctx);
        if (rc) return rc;
        C5_HIP(ctx, hipStreamSynchronize(ctx->stream));
        rc = recompute_rows(ctx);
        if (rc) return rc;
        return ensure_image_buffers(ctx);
    }
    return C5_OK;
}

int c5_set_row_range(c5_context* ctx, int row_begin, int row_count) {
    if (!ctx) return fail(nullptr, C5_ERR_INVALID, "null context");
    ++ctx->setup_epoch;  // whatever was built per view is stale ("view_cache")
    if (row_begin < 0 || row_count < -1) return fail(ctx, C5_ERR_INVALID, "bad row range");
    const int old_begin = ctx->cfg_row_begin, old_count = ctx->cfg_row_count;
    ctx->cfg_row_begin = row_begin;
    ctx->cfg_row_count = row_count;
    if (ctx->have_image) {
        int rc = bind_device(ctx);
        if (rc) return rc;
        C5_HIP(ctx, hipStreamSynchronize(ctx->stream));
        rc = recompute_rows(ctx);
        if (rc) {
            ctx->cfg_row_begin = old_begin;
            ctx->cfg_row_count = old_count;
            recompute_rows(ctx);
            return rc;
        }
        return ensure_image_buffers(ctx);
    }
    return C5_OK;
}

int c5_get_row_costs(c5_context* ctx, uint32_t* costs, int n_rows) {
    if (!ctx || !costs) return fail(ctx, C5_ERR_INVALID, "null argument");
    // (the option may have been switched off again since: the costs of the last frame that counted them stay readable
    // until the rows are laid out anew — a sweep probes one frame in many)
    if (!ctx->row_costs_collected) return fail(ctx, C5_ERR_STATE, "enable option \"row_costs\" before rendering");
    if (n_rows != ctx->im.n_local_rows) return fail(ctx, C5_ERR_INVALID, "expected %d rows", ctx->im.n_local_rows);
    int rc = c5_synchronize(ctx);
    if (rc) return rc;
    if (n_rows > 0)
        C5_HIP(ctx, hipMemcpy(costs, ctx->slots[ctx->row_cost_slot].row_cost.ptr, static_cast<size_t>(n_rows) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return C5_OK;
}

int c5_local_rows(const c5_context* ctx, int* n_rows) {
    if (!ctx || !n_rows) return C5_ERR_INVALID;
    *n_rows = ctx->have_image ? ctx->im.n_local_rows : 0;
    return C5_OK;
}

int c5_set_view(c5_context* ctx, const c5_rotation* rots, int n_rots) {
    if (!ctx) return fail(nullptr, C5_ERR_INVALID, "null context");
    return to_rotation_list(ctx, rots, n_rots, ctx->view);
}

int c5_set_solid_view(c5_context* ctx, int slot, const c5_rotation* rots, int n_rots) {
    if (!ctx) return fail(nullptr, C5_ERR_INVALID, "null context");
    if (slot < 0 || slot >= C5_MAX_SOLIDS) return fail(ctx, C5_ERR_INVALID, "solid slot %d out of range", slot);
    return to_rotation_list(ctx, rots, n_rots, ctx->solids[slot].rots);
}

int c5_set_alpha_limit(c5_context* ctx, double alpha_limit) {
    if (!ctx) return fail(nullptr, C5_ERR_INVALID, "null context");
    ctx->alpha_limit = alpha_limit;
    return C5_OK;
}

int c5_set_option(c5_context* ctx, const char* name, double value) {
    if (!ctx || !name) return fail(ctx, C5_ERR_INVALID, "null option");
    const std::string n(name);
    // whatever was built per view is stale ("view_cache") - except after the switches callers flip from frame to frame,
    // which the per-view data do not depend on
    if (n != "row_costs" && n != "stage_timing" && n != "walk_timing") ++ctx->setup_epoch;
    if (n == "tile") {
        if (value < 0 || value > 3) return fail(ctx, C5_ERR_INVALID, "tile must be 0, 1, 2 or 3");
        ctx->tile_shape = static_cast<int>(value);
    } else if (n == "transmittance_cutoff") {
        ctx->t_cutoff = value;
    } else if (n == "pipeline") {
        int rc = bind_device(ctx);
        if (rc) return rc;
        rc = drain(ctx);
        if (rc) return rc;
        if (ctx->n_cells > 0 || ctx->have_image)
            return fail(ctx, C5_ERR_STATE, "set \"pipeline\" before uploading the grid and setting the image");
        ctx->pipeline = static_cast<int>(value) != 0;
    } else if (n == "fuse_setup") {
        ctx->fuse_setup = static_cast<int>(value) != 0;
    } else if (n == "overlap_setup") {
        ctx->overlap_setup = static_cast<int>(value) != 0;
    } else if (n == "cell_order") {
        ctx->cell_order = static_cast<int>(value) != 0;
    } else if (n == "block_cull") {
        ctx->block_cull = static_cast<int>(value) != 0;
    } else if (n == "tile_flags") {
        ctx->tile_flags = static_cast<int>(value) != 0;
    } else if (n == "cost_order") {
        ctx->cost_order = static_cast<int>(value);  // (2: whatever the frame's size - experiments)
    } else if (n == "entry_key") {
        ctx->entry_key = static_cast<int>(value) != 0;
        ctx->overlap_seen = false;  // (with the testing value 0 an abutting entry can look like a skipped one: judge anew)
    } else if (n == "stage_slots") {
        if (value != 0 && value != 14 && value != 21) return fail(ctx, C5_ERR_INVALID, "stage_slots must be 0 (per frame), 14 or 21");
        ctx->stage_slots = static_cast<int>(value);
    } else if (n == "solid_interior_faces") {
        ctx->solid_interior_faces = static_cast<int>(value) != 0;
        forget_solid_masks(ctx);
    } else if (n == "view_cache") {
        ctx->view_cache = static_cast<int>(value) != 0;
    } else if (n == "batch_width") {
        if (value != 0 && value != 4 && value != 8) return fail(ctx, C5_ERR_INVALID, "batch_width must be 0 (by the batch), 4 or 8");
        ctx->deriv.batch_width = static_cast<int>(value);
    } else if (n == "vertex_merge") {
        ctx->deriv.vertex_merge = static_cast<int>(value) != 0;
    } else if (n == "adjoint_exact") {
        ctx->deriv.adjoint_exact = static_cast<int>(value) != 0;
    } else if (n == "exact_sums") {
        if (value != 0 && value != 1) return fail(ctx, C5_ERR_INVALID, "exact_sums must be 0 (fp64 atomics) or 1");
        ctx->deriv.exact_sums = static_cast<int>(value);
    } else if (n == "vertex_exact") {
        if (value != 0 && value != 1) return fail(ctx, C5_ERR_INVALID, "vertex_exact must be 0 (fp64 atomics) or 1");
        ctx->deriv.vertex_exact = static_cast<int>(value);
    } else if (n == "split_tilt_x" || n == "split_tilt_y") {  // testing: tilt of a forced split's planes
        if (!(std::fabs(value) < 64.0)) return fail(ctx, C5_ERR_INVALID, "split tilt out of range");
        (n == "split_tilt_x" ? ctx->split_tilt_x : ctx->split_tilt_y) = value;
    } else if (n == "entry_records") {
        ctx->entry_records = static_cast<int>(value) != 0;
    } else if (n == "depth_split") {
        if (value < 0 || value > c5::kMaxSlabs || value != std::floor(value))
            return fail(ctx, C5_ERR_INVALID, "depth_split must be 0 (per frame), 1 (never) or 2..%d slabs", c5::kMaxSlabs);
        ctx->depth_split = static_cast<int>(value);
    } else if (n == "solid_cache") {
        ctx->solid_cache = static_cast<int>(value) != 0;
        forget_solid_masks(ctx);
    } else if (n == "algorithm") {
        if (value != 0 && value != 1) return fail(ctx, C5_ERR_INVALID, "algorithm must be 0 (walk) or 1 (bin_sort_resolve)");
        ctx->algorithm = static_cast<int>(value);
    } else if (n == "lds_stage") {
        ctx->lds_stage = static_cast<int>(value) < 0 ? 0 : (static_cast<int>(value) > 2 ? 2 : static_cast<int>(value));
    } else if (n == "integration") {
        ctx->order = static_cast<int>(value) != 0;
    } else if (n == "entry_pool") {  // testing: (re)size the overflow pool of the entry lists, in records
        if (value < 1 || value > 16777214) return fail(ctx, C5_ERR_INVALID, "entry_pool out of range");
        int rc = drain(ctx);
        if (rc) return rc;
        for (FrameSlot& fs : ctx->slots) {
            fs.entry_capacity = static_cast<int64_t>(value);
            C5_HIP(ctx, fs.pool.ensure(static_cast<size_t>(fs.entry_capacity) * sizeof(c5::Entry)));
        }
    } else if (n == "band_rows") {  // tuning: image rows per XCD band of the walk (0: default 32)
        if (value < 0 || value > 4096) return fail(ctx, C5_ERR_INVALID, "band_rows out of range");
        ctx->band_rows = static_cast<int>(value);
    } else if (n == "lds_pad") {  // tuning: occupancy experiments (scripts/occupancy_sweep.py)
        if (value < 0 || value > 96 * 1024) return fail(ctx, C5_ERR_INVALID, "lds_pad out of range");
        ctx->lds_pad = static_cast<int>(value);
    } else if (n == "xcd_mode") {
        ctx->xcd_mode = static_cast<int>(value) < 0 ? 0 : (static_cast<int>(value) > 2 ? 2 : static_cast<int>(value));
    } else if (n == "row_costs") {
        ctx->row_costs = static_cast<int>(value) != 0;
    } else if (n == "stage_timing") {
        ctx->stage_timing = static_cast<int>(value) != 0;
    } else if (n == "walk_timing") {
        if (!(value >= 0.0 && value <= 1024.0)) return fail(ctx, C5_ERR_INVALID, "walk_timing: 0 (off) or every N-th launch, N <= 1024");
        ctx->walk_timing = static_cast<int>(value);
        ctx->walk_seq = 0;
    } else {
        return fail(ctx, C5_ERR_INVALID, "unknown option '%s'", name);
    }
    return C5_OK;
}

int c5_get_stats(c5_context* ctx, c5_stats* out) {
    if (!ctx || !out) return fail(ctx, C5_ERR_INVALID, "null argument");
    int rc = c5_synchronize(ctx);
    *out = ctx->last;
    return rc;
}

int c5_walk_kernel_ms(c5_context* ctx, int reset, double* avg_ms, int64_t* launches) {
    if (!ctx) return fail(nullptr, C5_ERR_INVALID, "null context");
    int rc = bind_device(ctx);
    if (rc) return rc;
    C5_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < ctx->walk_used; ++k) {
        float ms = 0.f;
        C5_HIP(ctx, hipEventElapsedTime(&ms, ctx->walk_a[k], ctx->walk_b[k]));
        ctx->walk_ms_sum += ms;
    }
    ctx->walk_launches += ctx->walk_used;
    ctx->walk_used = 0;
    if (avg_ms) *avg_ms = ctx->walk_launches ? ctx->walk_ms_sum / static_cast<double>(ctx->walk_launches) : 0.0;
    if (launches) *launches = ctx->walk_launches;
    if (reset) {
        ctx->walk_ms_sum = 0.0;
        ctx->walk_launches = 0;
    }
    return C5_OK;
}

int c5_face_adjacency(const int32_t* cell_vert, int64_t n_cells, int64_t n_pts, int32_t* adj,
                      int64_t* n_boundary_faces) {
    if (n_cells < 0 || n_pts < 0 || (n_cells > 0 && (!cell_vert || !adj)))
        return fail(nullptr, C5_ERR_INVALID, "bad adjacency arguments");
    std::vector<int32_t> a;
    std::vector<uint32_t> b;
    std::string err;
    if (!c5::build_face_adjacency(cell_vert, n_cells, n_pts, a, b, err))
        return fail(nullptr, err.find("range") != std::string::npos ? C5_ERR_INVALID : C5_ERR_MESH, "%s", err.c_str());
    if (n_cells > 0) std::memcpy(adj, a.data(), a.size() * sizeof(int32_t));
    if (n_boundary_faces) *n_boundary_faces = static_cast<int64_t>(b.size());
    return C5_OK;
}

int c5_weld_points(const double* xyz, int64_t n_pts, int32_t* rep, int64_t* n_merged) {
    if (n_pts < 0 || (n_pts > 0 && (!xyz || !rep))) return fail(nullptr, C5_ERR_INVALID, "bad weld arguments");
    for (int64_t i = 0; i < 3 * n_pts; ++i)
        if (!std::isfinite(xyz[i])) return fail(nullptr, C5_ERR_INVALID, "point %lld has a non-finite coordinate", static_cast<long long>(i / 3));
    std::vector<int32_t> r;
    const int64_t m = c5::weld_points(xyz, n_pts, r);
    if (n_pts > 0) std::memcpy(rep, r.data(), r.size() * sizeof(int32_t));
    if (n_merged) *n_merged = m;
    return C5_OK;
}

int c5_download_view_points(c5_context* ctx, double* xyz) {
    if (!ctx || !xyz) return fail(ctx, C5_ERR_INVALID, "null argument");
    const int frame_rc = c5_synchronize(ctx);
    if (frame_rc && frame_rc != C5_RETRY) return frame_rc;
    const size_t n = static_cast<size_t>(ctx->n_pts);
    std::vector<double> x(n), y(n), z(n);
    if (n) {
        C5_HIP(ctx, hipMemcpy(x.data(), ctx->slots[ctx->last_slot].vx.ptr, n * 8, hipMemcpyDeviceToHost));
        C5_HIP(ctx, hipMemcpy(y.data(), ctx->slots[ctx->last_slot].vy.ptr, n * 8, hipMemcpyDeviceToHost));
        C5_HIP(ctx, hipMemcpy(z.data(), ctx->slots[ctx->last_slot].vz.ptr, n * 8, hipMemcpyDeviceToHost));
    }
    for (size_t i = 0; i < n; ++i) {
        xyz[3 * i] = x[i];
        xyz[3 * i + 1] = y[i];
        xyz[3 * i + 2] = z[i];
    }
    return frame_rc;  // the points are valid either way; C5_RETRY says the frame they belong to is not
}

}  // extern "C"

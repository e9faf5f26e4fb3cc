// The persistent grid of the C ABI (include/course5_hip.h): c5_upload_grid and the scalar updates.
#include "context.hpp"

using namespace c5api;

namespace c5api __attribute__((visibility("hidden"))) {

int ensure_device_perm(c5_context* ctx) {
    if (!ctx->cell_perm.empty() && ctx->adj_perm_serial != ctx->grid_serial) {
        const size_t n_cells = static_cast<size_t>(ctx->n_cells);
        C5_HIP(ctx, ctx->adj_perm.ensure(n_cells * sizeof(int32_t)));
        C5_HIP(ctx, hipMemcpy(ctx->adj_perm.ptr, ctx->cell_perm.data(), n_cells * sizeof(int32_t), hipMemcpyHostToDevice));
        ctx->adj_perm_serial = ctx->grid_serial;
    }
    return C5_OK;
}

}  // namespace c5api

namespace {

// Coincident points are one point: the reference copies coordinates per cell (object3d_base.cpp:37-42)
// and never sees ids, so files with per-cell point copies or duplicated seam points must walk like any
// other grid (without this every face of such a file would be a boundary face).
// cell_vert: pointed at `welded`, the cells over the points' representatives, where any point was merged.
// rep: every point's representative where any was merged, else left empty.
void weld_cells(const double* xyz, int64_t n_pts, int64_t n_cells, const int32_t*& cell_vert, std::vector<int32_t>& welded,
                std::vector<int32_t>& rep) {
    if (c5::weld_points(xyz, n_pts, rep) <= 0) {
        rep.clear();
        return;
    }
    welded.resize(static_cast<size_t>(4 * n_cells));
    for (int64_t i = 0; i < 4 * n_cells; ++i) welded[static_cast<size_t>(i)] = rep[static_cast<size_t>(cell_vert[i])];
    cell_vert = welded.data();
}

// "cell_order" (round 4): the cells are kept in Morton order of their centroids, whatever order the caller has them in
// - 256 consecutive cells are then a compact lump of the grid, which is what lets build_records drop whole workgroups
// by a sphere about their cells (GridView::block_sphere) and keeps a boundary face's record near its neighbours'.
// Nothing of it shows outside: images are bit-equal (a cell's own arithmetic does not know its number), and
// c5_update_scalars takes its arrays in the caller's order.  Not for grids that go to bin_sort_resolve (c5_upload_grid).
// perm: new index -> the caller's, and cell_vert pointed at `ordered`, the cells in that order (both left alone where
// the caller's order is the Morton order already).
void morton_order_cells(const double* xyz, int64_t n_cells, const int32_t*& cell_vert, std::vector<int32_t>& perm,
                        std::vector<int32_t>& ordered) {
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    std::vector<double> cen(static_cast<size_t>(3 * n_cells));
    for (int64_t c = 0; c < n_cells; ++c)
        for (int k = 0; k < 3; ++k) {
            double m = 0.0;
            for (int a = 0; a < 4; ++a) m += xyz[3 * static_cast<int64_t>(cell_vert[4 * c + a]) + k];
            cen[static_cast<size_t>(3 * c + k)] = m;
            lo[k] = std::fmin(lo[k], m);
            hi[k] = std::fmax(hi[k], m);
        }
    auto spread = [](uint64_t v) {  // 10 bits -> every third bit
        v &= 0x3ffull;
        v = (v | (v << 16)) & 0x30000ffull;
        v = (v | (v << 8)) & 0x300f00full;
        v = (v | (v << 4)) & 0x30c30c3ull;
        v = (v | (v << 2)) & 0x9249249ull;
        return v;
    };
    std::vector<std::pair<uint64_t, int32_t>> keyed(static_cast<size_t>(n_cells));
    for (int64_t c = 0; c < n_cells; ++c) {
        uint64_t key = 0;
        for (int k = 0; k < 3; ++k) {
            const double span = hi[k] - lo[k];
            const double t = span > 0.0 ? (cen[static_cast<size_t>(3 * c + k)] - lo[k]) / span * 1024.0 : 0.0;
            key |= spread(static_cast<uint64_t>(std::fmin(std::fmax(t, 0.0), 1023.0))) << k;
        }
        keyed[static_cast<size_t>(c)] = {key, static_cast<int32_t>(c)};
    }
    std::sort(keyed.begin(), keyed.end());  // (ties by the caller's index: a total order, the same on every rank)
    bool identity = true;
    for (int64_t c = 0; c < n_cells && identity; ++c) identity = keyed[static_cast<size_t>(c)].second == c;
    if (identity) return;
    perm.resize(static_cast<size_t>(n_cells));
    ordered.resize(static_cast<size_t>(4 * n_cells));
    for (int64_t c = 0; c < n_cells; ++c) {
        const int32_t from = keyed[static_cast<size_t>(c)].second;
        perm[static_cast<size_t>(c)] = from;
        for (int a = 0; a < 4; ++a) ordered[static_cast<size_t>(4 * c + a)] = cell_vert[4 * static_cast<int64_t>(from) + a];
    }
    cell_vert = ordered.data();
}

// alpha and Q of n_cells > 0 cells, given in the caller's order, to the device in its own (perm: device index -> the
// caller's; empty: the same)
int upload_scalars(c5_context* ctx, const double* alpha, const double* q, int64_t n_cells, const std::vector<int32_t>& perm) {
    const size_t cb = static_cast<size_t>(n_cells);
    std::vector<double> a_dev, q_dev;
    const double *a_src = alpha, *q_src = q;
    if (!perm.empty()) {
        a_dev.resize(cb);
        q_dev.resize(cb);
        for (size_t c = 0; c < cb; ++c) a_dev[c] = alpha[perm[c]], q_dev[c] = q[perm[c]];
        a_src = a_dev.data(), q_src = q_dev.data();
    }
    C5_HIP(ctx, hipMemcpy(ctx->alpha.ptr, a_src, cb * 8, hipMemcpyHostToDevice));
    C5_HIP(ctx, hipMemcpy(ctx->q.ptr, q_src, cb * 8, hipMemcpyHostToDevice));
    return C5_OK;
}

// the largest alpha of the grid, and the smallest that is >= DBL_EPSILON (c5_context::alpha_top, alpha_floor)
void scan_alpha(c5_context* ctx, const double* alpha, int64_t n_cells) {
    ctx->alpha_top = 0.0;
    ctx->alpha_floor = INFINITY;
    for (int64_t c = 0; c < n_cells; ++c) {
        if (alpha[c] > ctx->alpha_top) ctx->alpha_top = alpha[c];  // (+inf counts: it is clamped to the limit; NaN never compares greater)
        if (alpha[c] >= DBL_EPSILON && alpha[c] < ctx->alpha_floor) ctx->alpha_floor = alpha[c];
        if (alpha[c] != alpha[c]) ctx->alpha_floor = 0.0;  // (a NaN alpha: no claim about conditioning)
    }
}

// The grid's arrays to the device, once the context's stream has drained: points (SoA), cells, adjacency, scalars,
// boundary faces; the frame slots' per-view buffers sized for them.
int upload_grid_arrays(c5_context* ctx, const double* xyz, int64_t n_pts, const int32_t* cell_vert, int64_t n_cells,
                       const std::vector<int32_t>& adj, const std::vector<uint32_t>& bfaces, const double* alpha, const double* q,
                       const std::vector<int32_t>& perm) {
    // SoA split of the points
    std::vector<double> sx(static_cast<size_t>(n_pts)), sy(static_cast<size_t>(n_pts)), sz(static_cast<size_t>(n_pts));
    for (int64_t i = 0; i < n_pts; ++i) {
        sx[static_cast<size_t>(i)] = xyz[3 * i];
        sy[static_cast<size_t>(i)] = xyz[3 * i + 1];
        sz[static_cast<size_t>(i)] = xyz[3 * i + 2];
    }
    const size_t pb = static_cast<size_t>(n_pts) * sizeof(double);
    const size_t cb = static_cast<size_t>(n_cells);
    C5_HIP(ctx, hipStreamSynchronize(ctx->stream));
    DeviceBuffer* pbufs[] = {&ctx->px, &ctx->py, &ctx->pz};
    for (DeviceBuffer* b : pbufs) C5_HIP(ctx, b->ensure(pb ? pb : 8));
    for (int k = 0; k < (ctx->pipeline ? kFrameSlots : 1); ++k) {
        FrameSlot& fs = ctx->slots[k];
        C5_HIP(ctx, fs.vx.ensure(pb ? pb : 8));
        C5_HIP(ctx, fs.vy.ensure(pb ? pb : 8));
        C5_HIP(ctx, fs.vz.ensure(pb ? pb : 8));
        // one 128-byte record per cell and view (ExitRecord)
        C5_HIP(ctx, fs.rec.ensure(cb * sizeof(c5::ExitRecord) + 256));
        // records of cells outside a context's row band are never rebuilt; keep whatever they hold a
        // valid record (neighbour ids inside the grid) from the start
        C5_HIP(ctx, hipMemset(fs.rec.ptr, 0, fs.rec.bytes));
    }
    C5_HIP(ctx, ctx->cell_vert.ensure(cb * 16 + 16));
    C5_HIP(ctx, ctx->cell_adj.ensure(cb * 16 + 16));
    C5_HIP(ctx, ctx->alpha.ensure(cb * 8 + 8));
    C5_HIP(ctx, ctx->q.ensure(cb * 8 + 8));
    C5_HIP(ctx, ctx->bface.ensure(bfaces.size() * 4 + 4));
    if (n_pts > 0) {
        C5_HIP(ctx, hipMemcpy(ctx->px.ptr, sx.data(), pb, hipMemcpyHostToDevice));
        C5_HIP(ctx, hipMemcpy(ctx->py.ptr, sy.data(), pb, hipMemcpyHostToDevice));
        C5_HIP(ctx, hipMemcpy(ctx->pz.ptr, sz.data(), pb, hipMemcpyHostToDevice));
    }
    if (n_cells > 0) {
        C5_HIP(ctx, hipMemcpy(ctx->cell_vert.ptr, cell_vert, cb * 16, hipMemcpyHostToDevice));
        // the device's copy names every boundary face by its index in the sorted boundary-face list: -(i + 2) where the
        // host API says -1 (build_records leaves the face's record in slot i: device_types.hpp: BFaceRecord)
        std::vector<int32_t> adj_dev(adj);
        for (size_t i = 0; i < bfaces.size(); ++i)
            adj_dev[static_cast<size_t>(bfaces[i] >> 2) * 4 + (bfaces[i] & 3u)] = -static_cast<int32_t>(i) - 2;
        C5_HIP(ctx, hipMemcpy(ctx->cell_adj.ptr, adj_dev.data(), cb * 16, hipMemcpyHostToDevice));
        int rc = upload_scalars(ctx, alpha, q, n_cells, perm);
        if (rc) return rc;
    }
    if (!bfaces.empty())
        C5_HIP(ctx, hipMemcpy(ctx->bface.ptr, bfaces.data(), bfaces.size() * 4, hipMemcpyHostToDevice));
    return C5_OK;
}

// What the frames need to know about the grid's size: its bounding box and diagonal, the largest |coordinate|, the
// longest edge of any cell (object space: no view changes them).
void measure_grid(c5_context* ctx, const double* xyz, int64_t n_pts, const int32_t* cell_vert, int64_t n_cells) {
    double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}, top = 0.0;
    for (int64_t i = 0; i < n_pts; ++i)
        for (int k = 0; k < 3; ++k) {
            const double v = xyz[3 * i + k];
            lo[k] = i ? std::fmin(lo[k], v) : v;
            hi[k] = i ? std::fmax(hi[k], v) : v;
            top = std::fmax(top, std::fabs(v));
        }
    for (int k = 0; k < 3; ++k) ctx->box_lo[k] = lo[k], ctx->box_hi[k] = hi[k];
    ctx->grid_diagonal = std::sqrt((hi[0] - lo[0]) * (hi[0] - lo[0]) + (hi[1] - lo[1]) * (hi[1] - lo[1]) + (hi[2] - lo[2]) * (hi[2] - lo[2]));
    // (the view rotates about x = x0 of each rotation: a point's distance from that axis, hence its depth, stays
    // within the largest |coordinate| + |x0|; the constant below has room for both)
    ctx->coord_max = top + 2.0;
    double edge2 = 0.0;
    for (int64_t c = 0; c < n_cells; ++c) {
        const int32_t* v = cell_vert + 4 * c;
        for (int a = 0; a < 4; ++a)
            for (int b = a + 1; b < 4; ++b) {
                const double* pa = xyz + 3 * static_cast<int64_t>(v[a]);
                const double* pb = xyz + 3 * static_cast<int64_t>(v[b]);
                const double d2 = (pa[0] - pb[0]) * (pa[0] - pb[0]) + (pa[1] - pb[1]) * (pa[1] - pb[1]) + (pa[2] - pb[2]) * (pa[2] - pb[2]);
                if (d2 > edge2) edge2 = d2;
            }
    }
    ctx->edge_max = std::sqrt(edge2) * (1.0 + 1e-9);  // (the rotations round: a hair of margin)
}

// a sphere about every 256 consecutive cells (one workgroup of build_records): kernels.hpp: GridView::block_sphere
int upload_block_spheres(c5_context* ctx, const double* xyz, const int32_t* cell_vert, int64_t n_cells) {
    const int64_t n_blocks = (n_cells + 255) / 256;
    std::vector<double> sph(static_cast<size_t>(4 * n_blocks), 0.0);
    for (int64_t b = 0; b < n_blocks; ++b) {
        double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int64_t c = 256 * b; c < std::min<int64_t>(n_cells, 256 * (b + 1)); ++c)
            for (int a = 0; a < 4; ++a) {
                const double* p = xyz + 3 * static_cast<int64_t>(cell_vert[4 * c + a]);
                for (int k = 0; k < 3; ++k) lo[k] = std::fmin(lo[k], p[k]), hi[k] = std::fmax(hi[k], p[k]);
            }
        double r2 = 0.0;
        for (int k = 0; k < 3; ++k) {
            sph[static_cast<size_t>(4 * b + k)] = 0.5 * (lo[k] + hi[k]);
            r2 += 0.25 * (hi[k] - lo[k]) * (hi[k] - lo[k]);
        }
        sph[static_cast<size_t>(4 * b + 3)] = std::sqrt(r2) * (1.0 + 1e-12);
    }
    C5_HIP(ctx, ctx->block_sphere.ensure(sph.size() * sizeof(double) + 32));
    if (!sph.empty()) C5_HIP(ctx, hipMemcpy(ctx->block_sphere.ptr, sph.data(), sph.size() * sizeof(double), hipMemcpyHostToDevice));
    return C5_OK;
}
}  // namespace

extern "C" {

int c5_upload_grid(c5_context* ctx, const double* xyz, int64_t n_pts, const int32_t* cell_vert,
                   int64_t n_cells, const double* alpha, const double* q) {
    if (!ctx) return fail(nullptr, C5_ERR_INVALID, "null context");
    ++ctx->setup_epoch;  // whatever was built per view is stale ("view_cache")
    if (n_pts < 0 || n_cells < 0) return fail(ctx, C5_ERR_INVALID, "negative size");
    if (n_cells > 0 && (!xyz || !cell_vert || !alpha || !q)) return fail(ctx, C5_ERR_INVALID, "null grid array");
    if (n_cells >= static_cast<int64_t>(c5::kNoCell))
        return fail(ctx, C5_ERR_INVALID, "cell count %lld does not fit 28 bits (line.hpp:71-79)",
                    static_cast<long long>(n_cells));
    for (int64_t i = 0; i < 3 * n_pts; ++i)
        if (!std::isfinite(xyz[i])) return fail(ctx, C5_ERR_INVALID, "point %lld has a non-finite coordinate", static_cast<long long>(i / 3));
    int rc = bind_device(ctx);
    if (rc) return rc;

    for (int64_t i = 0; i < 4 * n_cells; ++i)
        if (cell_vert[i] < 0 || cell_vert[i] >= n_pts)
            return fail(ctx, C5_ERR_INVALID, "cell %lld references a point id out of range", static_cast<long long>(i / 4));
    // the cells as the device gets them: over welded points, in Morton order
    std::vector<int32_t> welded, ordered;
    std::vector<int32_t> perm;  // new index -> the caller's
    std::vector<int32_t> rep;   // (empty: no point was merged)
    weld_cells(xyz, n_pts, n_cells, cell_vert, welded, rep);
    const int32_t* caller_cell_vert = cell_vert;
    if (ctx->cell_order && n_cells >= 4096) morton_order_cells(xyz, n_cells, cell_vert, perm, ordered);
    std::vector<int32_t> adj;
    std::vector<uint32_t> bfaces;
    std::string err;
    bool conforming = true;
    if (!c5::build_face_adjacency(cell_vert, n_cells, n_pts, adj, bfaces, err)) {
        cell_vert = caller_cell_vert;  // (bin_sort_resolve breaks ties of equal depths by the cells' order: the caller's stays)
        perm.clear();
        if (err.find("range") != std::string::npos) return fail(ctx, C5_ERR_INVALID, "%s", err.c_str());
        // a face shared by more than two cells: no walk possible, the reference's own algorithm will do
        conforming = false;
        adj.assign(static_cast<size_t>(4 * n_cells), -1);
        bfaces.clear();
    }

    rc = upload_grid_arrays(ctx, xyz, n_pts, cell_vert, n_cells, adj, bfaces, alpha, q, perm);
    if (rc) return rc;
    ctx->cell_perm = std::move(perm);
    ctx->host_cell_vert.assign(cell_vert, cell_vert + 4 * n_cells);  // (c5_update_points measures the grid again)
    ctx->point_rep = std::move(rep);
    ++ctx->grid_serial;
    ctx->deriv.vtx_inc.release();  // ("vertex_exact": the incidence table is the old connectivity's; the next exact call builds its own)
    ctx->deriv.vtx_inc_serial = ~uint64_t{0};
    ctx->shape.have_rest = false;  // (c5_shape_prior_*: the rest shape was the old grid's)
    measure_grid(ctx, xyz, n_pts, cell_vert, n_cells);
    scan_alpha(ctx, alpha, n_cells);
    ctx->split_auto_k = 1;
    ctx->ray_depth_known = false;
    ctx->fit_known = false;
    rc = upload_block_spheres(ctx, xyz, cell_vert, n_cells);
    if (rc) return rc;
    ctx->n_pts = n_pts;
    ctx->n_cells = n_cells;
    ctx->n_bfaces = static_cast<int64_t>(bfaces.size());
    ctx->grid_conforming = conforming;
    ctx->overlap_seen = false;
    return C5_OK;
}

int c5_update_scalars(c5_context* ctx, const double* alpha, const double* q, int64_t n_cells) {
    if (!ctx) return fail(nullptr, C5_ERR_INVALID, "null context");
    ++ctx->setup_epoch;  // whatever was built per view is stale ("view_cache")
    if (n_cells != ctx->n_cells) return fail(ctx, C5_ERR_INVALID, "scalar count differs from the uploaded grid");
    if (n_cells > 0 && (!alpha || !q)) return fail(ctx, C5_ERR_INVALID, "null scalar array");
    int rc = bind_device(ctx);
    if (rc) return rc;
    C5_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (n_cells > 0) {
        rc = upload_scalars(ctx, alpha, q, n_cells, ctx->cell_perm);  // (the device keeps the cells in its own order: "cell_order")
        if (rc) return rc;
    }
    scan_alpha(ctx, alpha, n_cells);
    return C5_OK;
}

int c5_update_points(c5_context* ctx, const double* xyz, int64_t n_pts) {
    if (!ctx) return fail(nullptr, C5_ERR_INVALID, "null context");
    if (n_pts != ctx->n_pts) return fail(ctx, C5_ERR_INVALID, "point count differs from the uploaded grid");
    if (n_pts > 0 && !xyz) return fail(ctx, C5_ERR_INVALID, "null point array");
    for (int64_t i = 0; i < 3 * n_pts; ++i)
        if (!std::isfinite(xyz[i])) return fail(ctx, C5_ERR_INVALID, "point %lld has a non-finite coordinate", static_cast<long long>(i / 3));
    ++ctx->setup_epoch;  // whatever was built per view is stale ("view_cache")
    ++ctx->points_serial;  // (c5_prior_*: the TPFA weights are the old points')
    int rc = bind_device(ctx);
    if (rc) return rc;
    rc = drain(ctx);  // (frames set up on the other streams read the points too)
    if (rc) return rc;
    // a point welded at upload keeps following its representative
    std::vector<double> moved;
    if (!ctx->point_rep.empty()) {
        moved.resize(static_cast<size_t>(3 * n_pts));
        for (int64_t i = 0; i < n_pts; ++i)
            for (int k = 0; k < 3; ++k) moved[static_cast<size_t>(3 * i + k)] = xyz[3 * static_cast<int64_t>(ctx->point_rep[static_cast<size_t>(i)]) + k];
        xyz = moved.data();
    }
    std::vector<double> soa(static_cast<size_t>(3 * n_pts));
    for (int64_t i = 0; i < n_pts; ++i)
        for (int k = 0; k < 3; ++k) soa[static_cast<size_t>(k * n_pts + i)] = xyz[3 * i + k];
    const size_t pb = static_cast<size_t>(n_pts) * sizeof(double);
    if (n_pts > 0) {
        C5_HIP(ctx, hipMemcpy(ctx->px.ptr, soa.data(), pb, hipMemcpyHostToDevice));
        C5_HIP(ctx, hipMemcpy(ctx->py.ptr, soa.data() + n_pts, pb, hipMemcpyHostToDevice));
        C5_HIP(ctx, hipMemcpy(ctx->pz.ptr, soa.data() + 2 * n_pts, pb, hipMemcpyHostToDevice));
    }
    // what c5_upload_grid derives from the coordinates, again
    const int32_t* cell_vert = ctx->host_cell_vert.data();
    measure_grid(ctx, xyz, n_pts, cell_vert, ctx->n_cells);
    ctx->split_auto_k = 1;
    ctx->ray_depth_known = false;
    ctx->fit_known = false;
    ctx->overlap_seen = false;  // (the first frame finds out again whether the components interpenetrate)
    return upload_block_spheres(ctx, xyz, cell_vert, ctx->n_cells);
}

int c5_update_scalars_device(c5_context* ctx, const void* alpha_dev, const void* q_dev, int64_t n_cells) {
    if (!ctx) return fail(nullptr, C5_ERR_INVALID, "null context");
    ++ctx->setup_epoch;  // whatever was built per view is stale ("view_cache")
    if (n_cells != ctx->n_cells) return fail(ctx, C5_ERR_INVALID, "scalar count differs from the uploaded grid");
    if (n_cells > 0 && (!alpha_dev || !q_dev)) return fail(ctx, C5_ERR_INVALID, "null scalar array");
    int rc = bind_device(ctx);
    if (rc) return rc;
    if (ctx->pipeline || ctx->overlap_setup) {  // (frames set up on the other streams read the scalars)
        rc = drain(ctx);
        if (rc) return rc;
    }
    double top = 0.0, floor = INFINITY;
    if (n_cells > 0) {
        rc = ensure_device_perm(ctx);
        if (rc) return rc;
        C5_HIP(ctx, ctx->scal_stats.ensure(4 * sizeof(unsigned long long)));
        if (!ctx->scal_host)
            C5_HIP(ctx, hipHostMalloc(reinterpret_cast<void**>(&ctx->scal_host), 4 * sizeof(unsigned long long), hipHostMallocDefault));
        unsigned long long* const stats = ctx->scal_stats.as<unsigned long long>();
        hipStream_t s = ctx->stream;
        C5_HIP(ctx, hipMemsetAsync(stats, 0, 3 * sizeof(unsigned long long), s));
        c5::launch_scalars_gather(s, static_cast<const double*>(alpha_dev), static_cast<const double*>(q_dev),
                                  ctx->cell_perm.empty() ? nullptr : ctx->adj_perm.as<int32_t>(), n_cells, ctx->alpha.as<double>(),
                                  ctx->q.as<double>(), stats);
        C5_HIP(ctx, hipGetLastError());
        C5_HIP(ctx, hipMemcpyAsync(ctx->scal_host, stats, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        C5_HIP(ctx, hipStreamSynchronize(s));
        unsigned long long bits = ctx->scal_host[0];
        std::memcpy(&top, &bits, sizeof top);
        if (ctx->scal_host[2]) {
            floor = 0.0;  // (a NaN alpha)
        } else if (ctx->scal_host[1]) {
            bits = ~ctx->scal_host[1];
            std::memcpy(&floor, &bits, sizeof floor);
        }
    }
    ctx->alpha_top = top;
    ctx->alpha_floor = floor;
    return C5_OK;
}

}  // extern "C"

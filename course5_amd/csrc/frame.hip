// The per-frame kernel sequence behind c5_render_device and every other render of the C ABI (include/course5_hip.h):
// enqueue_frame puts one frame's launches on the context's streams, wait_and_collect / finish_frame read its outcome.
#include "context.hpp"

namespace c5api __attribute__((visibility("hidden"))) {

// "depth_split": below this clamped alpha (and above DBL_EPSILON, where a cell stops taking part: line.cpp:220-224) the
// reference's recurrence I = (Q - (Q - alpha I) exp(-alpha dz)) / alpha is dominated by its own cancellation error
// (eps Q / alpha per step: golden fixture g4), which depends on the very bits of the I it is fed: partial integrals
// composed afterwards cannot reproduce it.  A grid with such a cell is walked whole unless the caller forces the split.
constexpr double kSplitAlphaFloor = 1e-6;

// (a9) solid mask of this frame into fs.mask; returns whether any solid exists
int enqueue_solids(c5_context* ctx, FrameSlot& fs, int slot_id, hipStream_t s, c5::SolidTable& table, bool& any_solid) {
    const c5::ImageParams& im = ctx->im;
    const int64_t padded = padded_pixels(im);
    any_solid = false;
    for (int k = 0; k < C5_MAX_SOLIDS; ++k) {
        table.colour[k] = ctx->solids[k].colour;
        if (ctx->solids[k].n_tets > 0) any_solid = true;
    }
    table.n_slots = C5_MAX_SOLIDS;
    if (any_solid) {
        C5_HIP(ctx, hipMemsetAsync(fs.mask.ptr, 0, static_cast<size_t>(padded) * sizeof(uint32_t), s));
        for (int k = 0; k < C5_MAX_SOLIDS; ++k) {
            Solid& so = ctx->solids[k];
            if (so.n_tets <= 0) continue;
            // unchanged since the frame before, and still on the same stream?
            const bool same = ctx->solid_cache && !ctx->pipeline && so.seen_stream == s && so.seen_generation == so.generation &&
                              same_rotations(so.seen_rots, so.rots) && same_image(so.seen_im, im);
            so.unchanged_frames = same ? so.unchanged_frames + 1 : 0;
            if (!same) {
                so.own_mask_ready = false;
                so.seen_rots = so.rots;
                so.seen_im = im;
                so.seen_generation = so.generation;
                so.seen_stream = s;
            }
            if (so.own_mask_ready) {
                c5::launch_mask_overlay(s, so.own_mask.as<uint32_t>(), fs.mask.as<uint32_t>(), padded);
                continue;
            }
            uint32_t* target = fs.mask.as<uint32_t>();
            if (so.unchanged_frames >= 1) {  // second frame in a row with this view: raster into the solid's own mask
                C5_HIP(ctx, so.own_mask.ensure(static_cast<size_t>(padded) * sizeof(uint32_t)));
                C5_HIP(ctx, hipMemsetAsync(so.own_mask.ptr, 0, static_cast<size_t>(padded) * sizeof(uint32_t), s));
                target = so.own_mask.as<uint32_t>();
            }
            c5::launch_transform_aos(s, so.raw.as<double>(), so.view[slot_id].as<double>(), so.n_points, so.rots);
            // Interior faces (a cell on either side: they cover no pixel the solid's other faces do not) are skipped -
            // where get_pixel_by_x/_y's clamp has no hand in their pixels (plane.cpp:194-212: what a face beyond a
            // border smears onto it is NOT the projection of anything).  A solid whose bounding sphere lies inside
            // the domain: none of them is even launched; one that reaches a border: each interior face decides for
            // itself (solid_mask_raster, only_across_border).
            int64_t skip = 0;
            const bool filter_interior = !ctx->solid_interior_faces && so.n_interior > 0 && so.n_interior < so.n_faces;
            if (filter_interior) {
                double c[3] = {so.centre[0], so.centre[1], so.centre[2]};
                rotate_host(so.rots, c);
                const double pad = so.radius * (1.0 + 1e-9) + 2.0 * std::fmax(std::fabs(im.step_x), std::fabs(im.step_y));
                const double x_a = im.x_min, x_b = im.x_min + im.step_x * (im.res_x - 1);
                const double y_a = im.y_min, y_b = im.y_min + im.step_y * (im.res_y - 1);
                if (c[0] - pad > std::fmin(x_a, x_b) && c[0] + pad < std::fmax(x_a, x_b) && c[1] - pad > std::fmin(y_a, y_b) &&
                    c[1] + pad < std::fmax(y_a, y_b))
                    skip = so.n_interior;
            }
            // lanes per face: about one per eight image rows of the group's tallest face, a power of two up to 64;
            // neighbouring groups that come to the same number share a launch
            int64_t run_begin = -1, run_count = 0;
            int run_lanes = 0;
            bool run_filtered = false;
            auto flush = [&]() {
                if (run_count > 0)
                    c5::launch_solid_mask_raster(s, so.view[slot_id].as<double>(), so.faces.as<int4>() + run_begin, run_count,
                                                 static_cast<uint32_t>(k) + 1u, ctx->ytab.as<double>(), im, target, run_lanes,
                                                 run_filtered);
                run_count = 0;
            };
            for (const Solid::FaceGroup& g : so.groups) {
                if (g.begin < skip) continue;  // an interior group of a solid inside the domain
                const bool filtered = filter_interior && g.begin < so.n_interior;
                // a lane per eight rows of the group's tallest face while the group alone does not fill the GPU, per
                // thirty-two once it does (every lane of a face repeats the face's set-up)
                const double rows = g.longest / std::fabs(im.step_y);
                int lanes = 1;
                while (lanes < 64 && rows > 8.0 * lanes && (g.count * lanes < (int64_t{1} << 18) || rows > 32.0 * lanes)) lanes *= 2;
                if (run_count > 0 && (lanes != run_lanes || filtered != run_filtered || g.begin != run_begin + run_count)) flush();
                if (run_count == 0) run_begin = g.begin, run_lanes = lanes, run_filtered = filtered;
                run_count += g.count;
            }
            flush();
            if (target != fs.mask.as<uint32_t>()) {
                so.own_mask_ready = true;
                c5::launch_mask_overlay(s, so.own_mask.as<uint32_t>(), fs.mask.as<uint32_t>(), padded);
            }
        }
    }
    return C5_OK;
}

// "algorithm" 1, a face in more than two cells, or interpenetrating components: the frame goes through bin_sort_resolve
bool uses_bin_sort(const c5_context* ctx) { return ctx->algorithm == 1 || !ctx->grid_conforming || ctx->overlap_seen; }

// the frame's uniform entry-key slack (walk_common.hpp: entry_key_slack): a fraction of the GRID's size — not of
// the image domain's: a slack larger than a whole ray would let a pixel that two boundary faces both claim (its
// centre exactly on their common edge) walk the same cells twice — plus the rounding of an absolute depth
double entry_key_slack(const c5_context* ctx) {
    return !ctx->entry_key ? -1.0 : c5::kEntryKeySlack * ctx->grid_diagonal + 0x1p-40 * ctx->coord_max;
}

// bin_sort_resolve's lists of the view in g (plane.cpp:184-192) into ctx->offs64 / ctx->segs.  Needs the segment total
// on the host between its two binning passes, so it synchronises.
int enqueue_bin_lists(c5_context* ctx, FrameSlot& fs, const c5::GridView& g, hipStream_t s, c5::FrameCounters* counters, int64_t& total) {
    const c5::ImageParams& im = ctx->im;
    const int64_t n_px = local_pixels(im), padded = padded_pixels(im);
    C5_HIP(ctx, ctx->offs64.ensure(static_cast<size_t>(padded + 1024) * sizeof(int64_t)));
    C5_HIP(ctx, ctx->scratch64.ensure(static_cast<size_t>(padded / 1024 + 1024) * sizeof(int64_t)));
    C5_HIP(ctx, hipMemsetAsync(fs.count.ptr, 0, static_cast<size_t>(padded + 1) * sizeof(int32_t), s));
    c5::launch_bin_count(s, g, ctx->xtab.as<double>(), ctx->ytab.as<double>(), im, fs.count.as<int32_t>(), &counters->odd_pixels);
    c5::launch_scan64(s, fs.count.as<int32_t>(), ctx->offs64.as<int64_t>(), n_px, ctx->scratch64.as<int64_t>());
    total = 0;
    C5_HIP(ctx, hipMemcpyAsync(&total, ctx->offs64.as<int64_t>() + n_px, sizeof total, hipMemcpyDeviceToHost, s));
    C5_HIP(ctx, hipStreamSynchronize(s));
    C5_HIP(ctx, ctx->segs.ensure(static_cast<size_t>(total + 16) * c5::segment_bytes()));
    c5::launch_bin_fill(s, g, ctx->xtab.as<double>(), ctx->ytab.as<double>(), im, fs.count.as<int32_t>(),
                        ctx->offs64.as<int64_t>(), ctx->segs.ptr);
    return C5_OK;
}

namespace {

// What the steps of one enqueue_frame share (it lives on that call's stack).
struct FrameJob {
    FrameSlot& fs;
    int slot_id;
    hipStream_t main_s;  // the walk's stream: the context's
    hipStream_t s;       // the setup's: the auxiliary stream with "pipeline", else the same
    int64_t padded;      // the pixels of the context's rows, rounded up to 1024
    bool timed;          // "stage_timing": an event between the stages
    c5::FrameCounters* counters;
    bool bin_sort;
    // the walk's per-row costs (sb_cost_buffer)
    uint32_t* sb = nullptr;
    int n_sb = 0;
    long long sb_key = -1;
    bool reuse = false;  // "view_cache": the slot's per-view data stand, the frame skips their setup (decide_view_cache)
    // what enqueue_view_setup leaves for the walk
    double key_slack = -1.0;
    c5::SolidTable table{};
    bool any_solid = false;
};

hipError_t mark(const FrameJob& f, int k, hipStream_t st) { return f.timed ? hipEventRecord(f.fs.ev[k], st) : hipSuccess; }

// the frame is in the streams: what wait_and_collect and the next enqueue_frame go by
void note_enqueued(c5_context* ctx, const FrameJob& f) {
    ctx->last_slot = f.slot_id;
    ctx->last_counters = f.counters;
    ctx->frame_index += 1;
    ctx->frame_pending = true;
    ctx->frame_timed = f.timed;
}

// bin_sort_resolve: the reference's algorithm (plane.cpp:184-192 + 144-172) on the GPU, behind the frame's transform.
int enqueue_bin_sort(c5_context* ctx, FrameJob& f, const c5::GridView& g, float2* out_dev) {
    FrameSlot& fs = f.fs;
    hipStream_t s = f.s;
    C5_HIP(ctx, mark(f, 2, s));
    int64_t total = 0;
    int rc = enqueue_bin_lists(ctx, fs, g, s, f.counters, total);
    if (rc) return rc;
    C5_HIP(ctx, mark(f, 3, s));
    rc = enqueue_solids(ctx, fs, f.slot_id, s, f.table, f.any_solid);
    if (rc) return rc;
    C5_HIP(ctx, mark(f, 4, s));
    c5::launch_resolve(s, g, ctx->im, ctx->offs64.as<int64_t>(), ctx->segs.ptr, f.any_solid ? fs.mask.as<uint32_t>() : nullptr,
                       f.table, ctx->alpha_limit, out_dev, f.counters);
    C5_HIP(ctx, mark(f, 5, s));
    C5_HIP(ctx, hipGetLastError());
    C5_HIP(ctx, hipMemcpyAsync(fs.host_counters, f.counters, kCountersBytes, hipMemcpyDeviceToHost, s));
    C5_HIP(ctx, hipMemcpyAsync(ctx->host_sticky, ctx->sticky.ptr, kStickyWords * sizeof(unsigned), hipMemcpyDeviceToHost, s));
    C5_HIP(ctx, hipStreamSynchronize(s));
    ctx->counters_on_host = true;
    fs.host_counters->seg_tiles = static_cast<unsigned long long>(total);  // (fewer than 2^40: they were all allocated)
    if (ctx->pipeline) {  // keep the two-stream bookkeeping consistent
        C5_HIP(ctx, hipEventRecord(fs.setup_done, s));
        C5_HIP(ctx, hipStreamWaitEvent(f.main_s, fs.setup_done, 0));
        C5_HIP(ctx, hipEventRecord(fs.walk_done, f.main_s));
        fs.walk_recorded = true;
    }
    note_enqueued(ctx, f);
    return C5_OK;
}

}  // namespace

// no cell and no solid with a tetrahedron (plane.cpp:269-271)
bool nothing_to_render(const c5_context* ctx) {
    if (ctx->n_cells > 0) return false;
    for (const Solid& s : ctx->solids)
        if (s.n_tets > 0) return false;
    return true;
}

// The grid as the kernels see it, with the per-view buffers of frame slot fs.
c5::GridView grid_view(const c5_context* ctx, const FrameSlot& fs) {
    const c5::ImageParams& im = ctx->im;
    c5::GridView g;
    g.n_pts = ctx->n_pts;
    g.n_cells = ctx->n_cells;
    g.n_bfaces = ctx->n_bfaces;
    g.px = ctx->px.as<double>();
    g.py = ctx->py.as<double>();
    g.pz = ctx->pz.as<double>();
    g.vx = fs.vx.as<double>();
    g.vy = fs.vy.as<double>();
    g.vz = fs.vz.as<double>();
    g.cell_vert = ctx->cell_vert.as<int4>();
    g.cell_adj = ctx->cell_adj.as<int4>();
    g.alpha = ctx->alpha.as<double>();
    g.q = ctx->q.as<double>();
    g.bface = ctx->bface.as<uint32_t>();
    g.xrec = fs.rec.as<c5::ExitRecord>();
    g.rot = ctx->view;
    // (whole workgroups of build_records judged by their cells' sphere: only where the rows are a part of the image)
    g.block_sphere = (ctx->block_cull && im.n_local_rows > 0 && im.n_local_rows < im.res_y && ctx->block_sphere.ptr) ? ctx->block_sphere.as<double4>() : nullptr;
    // y band of the rows this context renders (one pixel of slack on both sides)
    if (im.n_local_rows > 0) {
        const int first = c5::global_row_of(im, 0), last = c5::global_row_of(im, im.n_local_rows - 1);
        const double pad = std::fabs(im.step_y);
        const double ya = ctx->host_ytab[static_cast<size_t>(first)], yb = ctx->host_ytab[static_cast<size_t>(last)];
        g.cull_y_lo = std::fmin(ya, yb) - pad;
        g.cull_y_hi = std::fmax(ya, yb) + pad;
    } else {
        g.cull_y_lo = 1.0;
        g.cull_y_hi = -1.0;
    }
    return g;
}

namespace {

// The experimental switches, by what they change about a frame.  The steps below test these two where the conditions
// are the same and the single options where they are not (the per-row costs and the tile flags go with any LDS staging,
// not with "lds_stage" 2 alone; the boundary records and the tile flags ask about the side stream of THIS frame).

// One frame's setup is one chain of launches on the context's stream: no second frame slot ("pipeline"), no records and
// entry lists in one launch ("fuse_setup"), no side stream ("overlap_setup").
bool serial_setup(const c5_context* ctx) { return !ctx->pipeline && !ctx->fuse_setup && !ctx->overlap_setup; }

// The walk as it ships: 8x8 tiles, rows of super-blocks across the XCDs, the records staged in LDS with deferred misses,
// the reference's order of integration.
bool default_walk(const c5_context* ctx) {
    return ctx->tile_shape == 3 && ctx->xcd_mode == 2 && ctx->lds_stage == 2 && ctx->order == 0;
}

// (a2) + the walk's per-row costs, cleared by the transform's launch (what decides the order its rows of super-blocks
// start in, finish_frame): the slot's buffer for them, where the walk collects them.  Its first use clears it on f.s.
int sb_cost_buffer(c5_context* ctx, FrameJob& f) {
    const c5::ImageParams& im = ctx->im;
    FrameSlot& fs = f.fs;
    if (ctx->cost_order && ctx->xcd_mode == 2 && ctx->lds_stage && im.n_local_rows > 0) {
        const int sb_rows = c5::walk_sb_rows(ctx->tile_shape, ctx->band_rows);
        f.n_sb = (im.n_local_rows + sb_rows - 1) / sb_rows;
        if (f.n_sb <= c5::kMaxSbRows) {
            if (!fs.sb.ptr) {
                C5_HIP(ctx, fs.sb.ensure(c5::kMaxSbRows * sizeof(uint32_t)));
                C5_HIP(ctx, hipMemsetAsync(fs.sb.ptr, 0, fs.sb.bytes, f.s));
            }
            f.sb_key = (static_cast<long long>(im.n_local_rows) << 20) ^ (static_cast<long long>(sb_rows) << 4) ^ ctx->tile_shape;
            f.sb = fs.sb.as<uint32_t>();
        } else {
            f.n_sb = 0;
        }
    }
    fs.sb_key = f.sb_key;
    fs.sb_n = f.n_sb;
    return C5_OK;
}

// "depth_split" (device_types.hpp: SplitParams): how many slabs of depth a frame's rays are cut into, and where
struct SplitPlan {
    int k = 1;
    double w[c5::kMaxSlabs + 1] = {};
    double g[2] = {0.0, 0.0};  // the planes' common tilt
};

// the range of z - g[0] x - g[1] y over the corners of the grid's bounding box under the context's view
void box_depth_range(const c5_context* ctx, const double g[2], double& lo, double& hi) {
    lo = INFINITY, hi = -INFINITY;
    for (int corner = 0; corner < 8; ++corner) {
        double c[3] = {(corner & 1) ? ctx->box_hi[0] : ctx->box_lo[0], (corner & 2) ? ctx->box_hi[1] : ctx->box_lo[1],
                       (corner & 4) ? ctx->box_hi[2] : ctx->box_lo[2]};
        rotate_host(ctx->view, c);
        const double d = c[2] - g[0] * c[0] - g[1] * c[1];
        lo = std::fmin(lo, d);
        hi = std::fmax(hi, d);
    }
}

// The depth-split plan of this frame: host arithmetic on the context's state and its view.
SplitPlan plan_depth_split(const c5_context* ctx, bool bin_sort) {
    SplitPlan p;
    const bool able = !bin_sort && serial_setup(ctx) && default_walk(ctx) && ctx->n_cells > 0 &&
                      ctx->n_cells < (int64_t{1} << 25) && ctx->im.n_local_rows > 0;
    double a_floor = ctx->alpha_floor;  // the smallest clamped alpha >= DBL_EPSILON any cell can have
    if (ctx->alpha_limit < a_floor) a_floor = ctx->alpha_limit >= DBL_EPSILON ? ctx->alpha_limit : INFINITY;
    const bool well_conditioned = a_floor >= kSplitAlphaFloor;
    int want = 1;
    if (ctx->depth_split >= 2) want = ctx->depth_split;  // (forced: the caller answers for the conditioning)
    else if (ctx->depth_split == 0 && well_conditioned) want = ctx->split_auto_k;
    if (!able || want <= 1) return p;
    // the grid's depth range under this view, from the corners of its bounding box; planes at equal distances
    double z_lo, z_hi;
    box_depth_range(ctx, p.g, z_lo, z_hi);
    // (the rays of the last finished frame ran between narrower bounds: rows of a frame, a view from a corner)
    // (only when the library chooses the slabs itself: a forced count keeps planes that depend on the view alone, so
    // that renders of different rows of one frame stay bit-equal)
    if (ctx->depth_split == 0 && ctx->ray_depth_known && ctx->ray_depth_lo >= z_lo && ctx->ray_depth_hi <= z_hi)
        z_lo = ctx->ray_depth_lo, z_hi = ctx->ray_depth_hi;
    // Planes of constant depth cut the rays of an oblique view at different fractions (the cube of the benchmark seen
    // at -X 0.1 -Y 0.07: a ray's entry depth changes by 0.22 across the image, a fifth of its length - the longest
    // third of a ray cut in three had 83 of its 183 steps).  With the planes fitted through the last frame's entries
    // and ends at hand, the cutting planes take their mean tilt and divide the stretch between the two at the
    // sample's centre: parallel planes, in order everywhere.  Quantised (2^-16, 2^-20 of the grid's size), so that
    // the last bits of sums added in another order do not move them from frame to frame.
    if (ctx->depth_split == 0 && ctx->fit_known) {
        const double q_g = 0x1p-16, q_w = std::ldexp(std::fmax(ctx->grid_diagonal, 1e-300), -20);
        p.g[0] = std::round(ctx->fit_gx / q_g) * q_g;
        p.g[1] = std::round(ctx->fit_gy / q_g) * q_g;
        z_lo = std::round(ctx->fit_entry0 / q_w) * q_w;
        z_hi = std::round(ctx->fit_exit0 / q_w) * q_w;
    } else if (ctx->depth_split >= 2 && (ctx->split_tilt_x != 0.0 || ctx->split_tilt_y != 0.0)) {
        // (testing: a forced tilt; the bounding box's corners in the tilted coordinate)
        p.g[0] = ctx->split_tilt_x, p.g[1] = ctx->split_tilt_y;
        box_depth_range(ctx, p.g, z_lo, z_hi);
    }
    if (z_hi > z_lo && std::isfinite(z_hi - z_lo)) {
        p.k = std::min(want, c5::kMaxSlabs);
        p.w[0] = -DBL_MAX;
        p.w[p.k] = DBL_MAX;
        // (a hair off the k / K-th: structured grids have whole layers of nodes - and faces - at simple fractions of
        // their depth range, and a face lying IN a cutting plane to rounding makes which of its two cells starts the
        // job above a coin toss per pixel: harmless for the image, but the cell below is then counted by nobody)
        for (int k = 1; k < p.k; ++k) p.w[k] = z_lo + (z_hi - z_lo) * ((static_cast<double>(k) + 0.0309016994) / p.k);
    }
    return p;
}

// room for every cell at every plane in a shard of the straddle list: a shard can never overflow
int64_t straddle_capacity(int64_t n_cells, int split_k) {
    const int64_t waves = (n_cells + 63) / 64;
    return ((waves + c5::kStraddleShards - 1) / c5::kStraddleShards) * 64 * (split_k - 1);
}

// The slot's depth-split buffers, laid out anew when the slab count, the image or the grid changed since they were:
// waits for f.s, then clears them on it.
int layout_split_buffers(c5_context* ctx, FrameJob& f, const SplitPlan& p) {
    FrameSlot& fs = f.fs;
    const int64_t tiles = c5::walk_tiles(ctx->im);
    if (fs.split_k == p.k && fs.split_px == f.padded && fs.split_tiles == tiles && fs.split_cells == ctx->n_cells) return C5_OK;
    // (re)lay out: plane cells [K - 1][pixels], the sharded list of cells that straddle a plane (room for every
    // cell at every plane: a shard can never overflow), two halves of shard counters (build_records fills one while
    // the other, cleared by the plane raster of the frame before, waits for the next frame), partial results
    // [K][tiles * 64] x (tau, tauc, b: fp64; segments: u32), arrivals [tiles]
    const int64_t cap = straddle_capacity(ctx->n_cells, p.k);
    C5_HIP(ctx, hipStreamSynchronize(f.s));
    C5_HIP(ctx, fs.plane_cell.ensure(static_cast<size_t>(p.k - 1) * f.padded * sizeof(uint32_t)));
    C5_HIP(ctx, fs.straddle.ensure(static_cast<size_t>(c5::kStraddleShards) * cap * sizeof(uint32_t)));
    C5_HIP(ctx, fs.straddle_count.ensure(2 * c5::kStraddleShards * c5::kStraddleCounterStride * sizeof(uint32_t)));
    C5_HIP(ctx, fs.partials.ensure(static_cast<size_t>(p.k) * tiles * 64 * 28));
    C5_HIP(ctx, fs.arrivals.ensure(static_cast<size_t>(tiles) * sizeof(uint32_t)));
    C5_HIP(ctx, hipMemsetAsync(fs.plane_cell.ptr, 0, fs.plane_cell.bytes, f.s));
    C5_HIP(ctx, hipMemsetAsync(fs.straddle_count.ptr, 0, fs.straddle_count.bytes, f.s));
    C5_HIP(ctx, hipMemsetAsync(fs.arrivals.ptr, 0, fs.arrivals.bytes, f.s));
    fs.split_k = p.k;
    fs.split_px = f.padded;
    fs.split_tiles = tiles;
    fs.split_cells = ctx->n_cells;
    fs.split_seq = 0;
    fs.setup_epoch = 0;  // whatever plane cells the slot held are gone
    return C5_OK;
}

// "view_cache" (the persistent device grid of a -D sweep: only the donor turns, main.cpp:112-116): transformed
// vertices, records and entry lists depend on the grid, the image, the view, the alpha limit and the order - a frame
// that has all of them in common with the frame before reuses them.  The walk normally hands the entry heads back
// cleared, so it takes TWO frames with the same view in a row before there is something to reuse: the second one
// builds everything once more and tells its walk to leave the heads alone; the third and later ones skip the
// per-view setup.  A sweep whose view changes every frame never pays for any of this.
// Returns whether this frame reuses the slot's per-view data, and notes in the slot what they are now built for.
bool decide_view_cache(const c5_context* ctx, FrameSlot& fs, bool bin_sort, const SplitPlan& p) {
    const bool cacheable = ctx->view_cache && serial_setup(ctx) && !bin_sort && ctx->n_cells > 0;
    const bool same_view = cacheable && fs.setup_epoch == ctx->setup_epoch && same_rotations(fs.setup_view, ctx->view) &&
                           fs.setup_limit == ctx->alpha_limit && fs.setup_order == ctx->order && fs.setup_split == p.k &&
                           std::memcmp(fs.setup_w, p.w, sizeof p.w) == 0 && std::memcmp(fs.setup_g, p.g, sizeof p.g) == 0;
    const bool reuse = same_view && fs.setup_kept;
    fs.setup_reused = reuse;
    fs.setup_epoch = cacheable ? ctx->setup_epoch : 0;
    fs.setup_view = ctx->view;
    fs.setup_limit = ctx->alpha_limit;
    fs.setup_order = ctx->order;
    fs.setup_kept = same_view;  // (this frame's walk leaves the heads in place)
    fs.setup_split = p.k;
    std::memcpy(fs.setup_w, p.w, sizeof p.w);
    std::memcpy(fs.setup_g, p.g, sizeof p.g);
    return reuse;
}

// SplitParams of this frame over the slot's buffers; a frame that builds its plane cells anew takes a new stamp (and
// clears the plane cells on f.s when the stamps come round).
int fill_split_params(c5_context* ctx, FrameJob& f, const SplitPlan& p, c5::SplitParams& sp) {
    FrameSlot& fs = f.fs;
    sp = c5::SplitParams{};
    if (p.k <= 1) return C5_OK;
    if (!f.reuse) {
        fs.split_seq += 1;  // a new set of plane cells: a new stamp (the words of the 15 frames before it stay behind, invalid)
        if (fs.split_seq % 15 == 0) C5_HIP(ctx, hipMemsetAsync(fs.plane_cell.ptr, 0, fs.plane_cell.bytes, f.s));  // stamps come round
    }
    sp.n_slabs = p.k;
    sp.stamp = static_cast<uint32_t>(fs.split_seq % 15) + 1u;
    std::memcpy(sp.w, p.w, sizeof p.w);
    sp.gx = p.g[0];
    sp.gy = p.g[1];
    sp.plane_cell = fs.plane_cell.as<uint32_t>();
    sp.plane_stride = f.padded;
    sp.straddle = fs.straddle.as<uint32_t>();
    const size_t half = static_cast<size_t>(c5::kStraddleShards) * c5::kStraddleCounterStride;
    sp.straddle_count = fs.straddle_count.as<uint32_t>() + (fs.split_seq & 1u) * half;
    sp.straddle_count_next = fs.straddle_count.as<uint32_t>() + ((fs.split_seq + 1u) & 1u) * half;
    sp.straddle_capacity = static_cast<uint32_t>(straddle_capacity(ctx->n_cells, p.k));
    sp.part_stride = fs.split_tiles * 64;
    char* const base = static_cast<char*>(fs.partials.ptr);
    const size_t n = static_cast<size_t>(p.k) * sp.part_stride;
    sp.part_tau = reinterpret_cast<double*>(base);
    sp.part_tauc = reinterpret_cast<double*>(base + n * 8);
    sp.part_b = reinterpret_cast<double*>(base + n * 16);
    sp.part_nseg = reinterpret_cast<uint32_t*>(base + n * 24);
    sp.arrivals = fs.arrivals.as<uint32_t>();
    return C5_OK;
}

// build_records leaves a 96-byte record per boundary face a ray can enter through (entry_raster_rec): the slot's buffer
// for them and this frame's stamp, into g
int boundary_records(c5_context* ctx, FrameJob& f, c5::GridView& g) {
    FrameSlot& fs = f.fs;
    if (fs.bfrec.bytes < static_cast<size_t>(g.n_bfaces) * sizeof(c5::BFaceRecord)) {
        C5_HIP(ctx, fs.bfrec.ensure(static_cast<size_t>(g.n_bfaces) * sizeof(c5::BFaceRecord)));
        C5_HIP(ctx, hipMemsetAsync(fs.bfrec.ptr, 0, fs.bfrec.bytes, f.s));
        fs.bf_seq = 0;
    }
    fs.bf_seq += 1;
    if (fs.bf_seq == 0) {  // (4 billion frames on: no stale record may look current)
        C5_HIP(ctx, hipMemsetAsync(fs.bfrec.ptr, 0, fs.bfrec.bytes, f.s));
        fs.bf_seq = 1;
    }
    g.bfrec = fs.bfrec.as<c5::BFaceRecord>();
    g.bf_seq = fs.bf_seq;
    g.bf_want_upper = ctx->order != 0;
    g.bf_key_slack = f.key_slack;
    return C5_OK;
}

// ... and a mark on every 8x8 tile that holds an entry ("tile_flags"; the default tile shape's tiling; not with
// "fuse_setup"): the slot's words for them and this raster run's stamp (cleared on stream e when laid out anew)
int tile_flag_buffer(c5_context* ctx, FrameJob& f, const c5::GridView& g, bool fused, hipStream_t e, uint32_t*& tile_flag) {
    FrameSlot& fs = f.fs;
    fs.flags_valid = false;
    if (!(ctx->tile_flags && ctx->tile_shape == 3 && ctx->lds_stage && !fused && g.n_cells > 0 && g.n_bfaces > 0)) return C5_OK;
    const int64_t tiles = c5::walk_tiles(ctx->im);
    if (fs.flag_tiles != tiles || !fs.tile_flag.ptr) {
        C5_HIP(ctx, fs.tile_flag.ensure(static_cast<size_t>(tiles) * sizeof(uint32_t)));
        C5_HIP(ctx, hipMemsetAsync(fs.tile_flag.ptr, 0, static_cast<size_t>(tiles) * sizeof(uint32_t), e));
        fs.flag_tiles = tiles;
        fs.flag_seq = 0;
    }
    fs.flag_seq += 1;
    if (fs.flag_seq == 0) {  // (4 billion raster runs on: no old mark may look current)
        C5_HIP(ctx, hipMemsetAsync(fs.tile_flag.ptr, 0, static_cast<size_t>(tiles) * sizeof(uint32_t), e));
        fs.flag_seq = 1;
    }
    tile_flag = fs.tile_flag.as<uint32_t>();
    fs.flags_valid = true;
    return C5_OK;
}

// (a1, a10, a13 constants) per-cell records on the setup stream; the boundary entry lists and the
// solid mask need only the transformed vertices, so they run beside it on a side stream (they are
// small, latency-bound launches).  With stage timing on, everything stays in one stream so that
// the per-stage times mean something.
int enqueue_view_setup(c5_context* ctx, FrameJob& f, c5::GridView& g) {
    FrameSlot& fs = f.fs;
    const c5::ImageParams& im = ctx->im;
    hipStream_t s = f.s;
    const bool side = ctx->overlap_setup && !f.timed;
    hipStream_t e = side ? ctx->side_stream : s;
    if (side) {
        C5_HIP(ctx, hipEventRecord(ctx->fork_ev, s));
        C5_HIP(ctx, hipStreamWaitEvent(e, ctx->fork_ev, 0));
    }
    f.key_slack = entry_key_slack(ctx);
    const bool fused = ctx->fuse_setup && !side && g.n_cells > 0;
    if (!fused && !f.reuse) {
        if (ctx->entry_records && !ctx->fuse_setup && !side && g.n_bfaces > 0) {  // (the raster must run BEHIND build_records)
            int rc = boundary_records(ctx, f, g);
            if (rc) return rc;
        }
        // (a cell's optics ride in its record since round 3 — one line per cell and step — and are rewritten with it)
        c5::launch_build_records(s, g, ctx->alpha_limit, ctx->order);
        c5::launch_plane_raster(s, g, ctx->xtab.as<double>(), ctx->ytab.as<double>(), im);  // ("depth_split"; nothing otherwise)
    }
    if (!fused) C5_HIP(ctx, mark(f, 2, s));
    // boundary entries: one raster pass (per-pixel count + first entry + overflow chain)
    if (!fs.head_clean && !f.reuse) C5_HIP(ctx, hipMemsetAsync(fs.head.ptr, 0, static_cast<size_t>(f.padded) * sizeof(c5::EntryHead), e));
    fs.head_clean = false;
    uint32_t* tile_flag = nullptr;
    if (!f.reuse) {
        int rc = tile_flag_buffer(ctx, f, g, fused, e, tile_flag);
        if (rc) return rc;
    }
    if (fused) {
        // records and entry lists as ONE launch of interleaved workgroups ("fuse_setup"; ms_records then holds the
        // time of both and ms_entries is zero)
        c5::launch_setup_fused(s, g, ctx->alpha_limit, ctx->order, ctx->xtab.as<double>(), ctx->ytab.as<double>(), im,
                               fs.head.as<c5::EntryHead>(), fs.first.as<c5::Entry>(), fs.pool.as<c5::Entry>(), fs.entry_capacity,
                               f.counters, ctx->sticky.as<unsigned>(), ctx->order != 0, f.key_slack);
        C5_HIP(ctx, mark(f, 2, s));
    } else if (g.n_cells > 0 && !f.reuse) {
        c5::launch_entry_lists(e, g, ctx->xtab.as<double>(), ctx->ytab.as<double>(), im, fs.head.as<c5::EntryHead>(),
                               fs.first.as<c5::Entry>(), fs.pool.as<c5::Entry>(), fs.entry_capacity, f.counters,
                               ctx->sticky.as<unsigned>(), ctx->order != 0, f.key_slack, tile_flag, fs.flag_seq);
    }
    C5_HIP(ctx, mark(f, 3, e));
    // (a9) solids
    int rc = enqueue_solids(ctx, fs, f.slot_id, e, f.table, f.any_solid);
    if (rc) return rc;
    C5_HIP(ctx, mark(f, 4, e));
    if (side) {
        C5_HIP(ctx, hipEventRecord(ctx->join_ev, e));
        C5_HIP(ctx, hipStreamWaitEvent(s, ctx->join_ev, 0));
    }
    return C5_OK;
}

// (a11-a14) the walk's parameters over the slot's per-view data (the per-row segment counts are enqueue_frame's to add)
void fill_walk_params(const c5_context* ctx, const FrameJob& f, const c5::GridView& g, float2* out_dev, c5::WalkParams& wp) {
    const FrameSlot& fs = f.fs;
    wp.xrec = g.xrec;
    wp.entry_head = fs.head.as<c5::EntryHead>();
    wp.entry_first = fs.first.as<c5::Entry>();
    wp.entry_pool = fs.pool.as<c5::Entry>();
    wp.pool_capacity = fs.entry_capacity;
    wp.key_slack = f.key_slack > 0.0 ? f.key_slack : 0.0;
    wp.mask = f.any_solid ? fs.mask.as<uint32_t>() : nullptr;
    wp.solids = f.table;
    wp.Xtab = ctx->xtab.as<double>();
    wp.Ytab = ctx->ytab.as<double>();
    wp.out = out_dev;
    wp.im = ctx->im;
    wp.t_cutoff = ctx->t_cutoff;
    wp.max_steps = static_cast<uint32_t>(ctx->n_cells + 64);
    wp.xcd_mode = ctx->xcd_mode;
    wp.lds_pad = ctx->lds_pad;
    wp.stage_slots = ctx->stage_slots ? ctx->stage_slots : (ctx->rays_per_cell > 0.0 && ctx->rays_per_cell < 120.0 ? 21 : 14);
    wp.band_rows = ctx->band_rows;
    wp.order = ctx->order;
    // walk_composite_lds addresses the records by 32-bit byte offsets: n_cells * 128 must fit
    wp.lds_stage = (ctx->lds_stage && ctx->n_cells < (int64_t{1} << 25)) ? ctx->lds_stage : 0;
    wp.counters = f.counters;
    // (a pixel a solid covers is written by its wavefront whether or not the grid is there: with solids every tile is read)
    wp.tile_flag = (fs.flags_valid && !f.any_solid && ctx->tile_flags) ? fs.tile_flag.as<uint32_t>() : nullptr;
    wp.tile_stamp = fs.flag_seq;
    {   // every exp argument of this grid within (-1/8, 0]?  alpha_c <= min(limit, largest alpha), chord <= longest edge
        double a_max = std::fmin(ctx->alpha_top, ctx->alpha_limit);
        if (!(a_max >= 0.0)) a_max = ctx->alpha_top;  // (a NaN limit clamps nothing: line.cpp:216-218)
        wp.small_exp_only = (a_max * ctx->edge_max < 0.125) ? 1 : 0;
    }
    wp.keep_entries = fs.setup_kept ? 1 : 0;
    wp.split = g.split;
    wp.row_cost = nullptr;
    wp.sb_cost = f.sb;
    wp.n_sb_rows = 0;
    if (f.sb && ctx->sb_order_key == f.sb_key && ctx->sb_order_n == f.n_sb) {  // an order worked out for this very tiling
        wp.n_sb_rows = f.n_sb;
        std::memcpy(wp.sb_order, ctx->sb_order, sizeof wp.sb_order);
    }
    wp.sticky = ctx->sticky.as<unsigned>();
}

// ("walk_timing" N: events around every N-th launch - two events cost 6 us of a 0.53-ms frame when frames follow one another)
// The event before the walk, on its stream; ev_slot: the pair's place in the pool, or -1 for a launch that is not timed.
int begin_walk_timing(c5_context* ctx, hipStream_t main_s, int& ev_slot) {
    ev_slot = -1;
    if (!ctx->walk_timing || (ctx->walk_seq++ % static_cast<unsigned>(ctx->walk_timing)) != 0u) return C5_OK;
    if (ctx->walk_used == kWalkEventPool) {  // fold the pool before reusing it
        for (int k = 0; k < kWalkEventPool; ++k) {
            C5_HIP(ctx, hipEventSynchronize(ctx->walk_b[k]));
            float ms = 0.f;
            C5_HIP(ctx, hipEventElapsedTime(&ms, ctx->walk_a[k], ctx->walk_b[k]));
            ctx->walk_ms_sum += ms;
        }
        ctx->walk_launches += kWalkEventPool;
        ctx->walk_used = 0;
    }
    ev_slot = ctx->walk_used++;
    C5_HIP(ctx, hipEventRecord(ctx->walk_a[ev_slot], main_s));
    return C5_OK;
}

}  // namespace

// Enqueue one frame; the image goes to out_dev.  The per-view setup runs on the auxiliary stream
// into frame slot (frame_index & 1), the walk on the main stream once that setup is done, so the
// setup of the next frame overlaps this frame's walk.
// own_counters: the frame's statistics go to these FrameCounters[kCounterShards] instead of the slot's (frames delivered to
// host memory: each frame of the ring keeps its own, c5_render_host_async).
int enqueue_frame(c5_context* ctx, float2* out_dev, c5::FrameCounters* own_counters) {
    if (nothing_to_render(ctx)) return fail(ctx, C5_ERR_STATE, "plane initializer. empty set of objects to render");  // plane.cpp:269-271
    if (!ctx->have_image) return fail(ctx, C5_ERR_STATE, "critical error. empty plane");  // plane.cpp:151-153
    int rc = bind_device(ctx);
    if (rc) return rc;

    const int slot_id = ctx->pipeline ? static_cast<int>(ctx->frame_index & 1) : 0;
    FrameSlot& fs = ctx->slots[slot_id];
    FrameJob f{fs, slot_id, ctx->stream, ctx->pipeline ? ctx->aux_stream : ctx->stream, padded_pixels(ctx->im), ctx->stage_timing != 0,
               own_counters ? own_counters : fs.counters.as<c5::FrameCounters>(), uses_bin_sort(ctx)};
    hipStream_t main_s = f.main_s, s = f.s;

    // the slot's buffers are free once the walk that last read them has finished
    if (ctx->pipeline && fs.walk_recorded) C5_HIP(ctx, hipStreamWaitEvent(s, fs.walk_done, 0));
    C5_HIP(ctx, mark(f, 0, s));

    // what this frame builds per view, and into which buffers (memsets on s where a buffer is laid out anew)
    c5::GridView g = grid_view(ctx, fs);
    rc = sb_cost_buffer(ctx, f);
    if (rc) return rc;
    const SplitPlan plan = plan_depth_split(ctx, f.bin_sort);
    if (plan.k > 1) {
        rc = layout_split_buffers(ctx, f, plan);
        if (rc) return rc;
    }
    f.reuse = decide_view_cache(ctx, fs, f.bin_sort, plan);
    rc = fill_split_params(ctx, f, plan, g.split);
    if (rc) return rc;

    // (a2) view transform + the frame's statistics and the walk's per-row costs cleared by the same launch
    if (f.reuse) {
        c5::launch_clear_walk_counters(s, f.counters, f.sb, f.n_sb, fs.raster_counters);
    } else {
        c5::launch_transform_soa(s, g.px, g.py, g.pz, g.vx, g.vy, g.vz, g.n_pts, ctx->view, f.counters, f.sb, f.n_sb);
        fs.raster_counters = f.counters;  // (this frame's raster adds its pool demand / overflow here)
    }
    C5_HIP(ctx, mark(f, 1, s));
    if (f.bin_sort) return enqueue_bin_sort(ctx, f, g, out_dev);
    rc = enqueue_view_setup(ctx, f, g);
    if (rc) return rc;

    // (a11-a14) walk on the main stream, after this slot's setup
    c5::WalkParams wp{};
    fill_walk_params(ctx, f, g, out_dev, wp);
    if (ctx->row_costs && ctx->im.n_local_rows > 0) {
        wp.row_cost = fs.row_cost.as<uint32_t>();
        C5_HIP(ctx, hipMemsetAsync(fs.row_cost.ptr, 0, static_cast<size_t>(ctx->im.n_local_rows) * sizeof(uint32_t), s));
        ctx->row_costs_collected = true;
        ctx->row_cost_slot = slot_id;  // ("pipeline" alternates the slots: the costs stay in the slot of the frame that counted them)
    }
    if (ctx->pipeline) {
        C5_HIP(ctx, hipEventRecord(fs.setup_done, s));
        C5_HIP(ctx, hipStreamWaitEvent(main_s, fs.setup_done, 0));
    }
    int ev_slot = -1;
    rc = begin_walk_timing(ctx, main_s, ev_slot);
    if (rc) return rc;
    c5::launch_walk(main_s, wp, ctx->tile_shape);
    fs.head_clean = !wp.keep_entries;  // stream order: every pixel's head is zero again once the walk has run
    if (ev_slot >= 0) C5_HIP(ctx, hipEventRecord(ctx->walk_b[ev_slot], main_s));
    C5_HIP(ctx, mark(f, 5, main_s));
    C5_HIP(ctx, hipGetLastError());
    // the statistics of the last frame and the sticky failure words are fetched when somebody waits for
    // the stream (wait_and_collect), not once per frame: two API calls and two small copies less per frame
    ctx->counters_on_host = false;
    if (ctx->pipeline) {
        C5_HIP(ctx, hipEventRecord(fs.walk_done, main_s));
        fs.walk_recorded = true;
    }
    note_enqueued(ctx, f);
    return C5_OK;
}

namespace {

// A frame's counters: the shards' sums, the packed pairs taken apart (device_types.hpp: FrameCounters)
struct FrameTotals {
    unsigned long long segments = 0, steps = 0, covered = 0, solid_pixels = 0, entries = 0, ray_tiles = 0, exit_max_key = 0, entry_min_key = 0;
    unsigned walk_overflow = 0, entry_overflow = 0, odd_pixels = 0, pool_used = 0, seg_max = 0;
};

FrameTotals sum_counters(const c5::FrameCounters* shards) {
    FrameTotals hc;
    for (int k = 0; k < c5::kCounterShards; ++k) {
        const c5::FrameCounters& p = shards[k];
        hc.segments += p.seg_tiles & c5::kCounterLowMask;
        hc.ray_tiles += p.seg_tiles >> c5::kCounterHighShift;
        hc.steps += p.steps_cov & c5::kCounterLowMask;
        hc.covered += p.steps_cov >> c5::kCounterHighShift;
        hc.entries += p.ent_solid & c5::kCounterLowMask;
        hc.solid_pixels += p.ent_solid >> c5::kCounterHighShift;
        hc.walk_overflow += p.walk_overflow;
        hc.entry_overflow += p.entry_overflow;
        hc.odd_pixels += p.odd_pixels;
        hc.pool_used += p.pool_used;
        hc.seg_max = std::max(hc.seg_max, p.seg_max);
        hc.exit_max_key = std::max(hc.exit_max_key, p.exit_max_key);
        hc.entry_min_key = std::max(hc.entry_min_key, p.entry_min_key);
    }
    return hc;
}

// The order the next frames' rows of super-blocks start in.  A frame with fewer wavefronts of rays than about two
// rounds of the GPU's wavefront slots lasts as long as its longest wavefronts plus the time the dispatcher takes
// to reach them behind thousands of empty or short tiles, and ends on whatever started last: such frames start
// the rows with the LONGEST RAYS first (by this frame's longest ray per row - of one tile per super-block - in eight
// classes of the longest of all, so that rows of about the same length keep their image order).  Round 4 (profiles/
// experiments.md): the key used to be the row's SUM of segments, which sent a cut-off row of full-length rays at the
// lower edge of a share to the very end (the upper half of the C3 frame: 0.318 -> 0.347 ms with the order, 0.301 with
// this one; an eighth of the 4800x3600 frame at the image's edge 0.307 -> 0.247).  Larger frames (several rounds of
// wavefronts) lose a little (C3 frame 0.534 -> 0.542 ms) and stay in image order; so do frames of a few hundred
// wavefronts (C2 ball at 600x450: 0.106 -> 0.112).
void update_sb_order(c5_context* ctx, const FrameSlot& fs, unsigned long long covered) {
    ctx->sb_order_key = -1;
    ctx->sb_order_n = 0;
    constexpr unsigned long long kSmallFrameRays = 2ull * 256 * 32 * 64;  // two rounds of 8 wavefronts per SIMD
    constexpr unsigned long long kTinyFrameRays = 100000;                  // ~1 500 wavefronts
    if (!(fs.sb_key >= 0 && ctx->host_sb && fs.sb_n > 1 && fs.sb_n <= c5::kMaxSbRows &&
          ((covered >= kTinyFrameRays && covered < kSmallFrameRays) || (covered > 0 && ctx->cost_order == 2))))
        return;
    const int n = fs.sb_n;
    uint32_t top = 0;
    for (int j = 0; j < n; ++j) top = std::max(top, ctx->host_sb[j]);
    const uint32_t unit = top / 8u + 1u;
    int order[c5::kMaxSbRows];
    for (int j = 0; j < n; ++j) order[j] = j;
    std::stable_sort(order, order + n, [&](int a, int b) { return ctx->host_sb[a] / unit > ctx->host_sb[b] / unit; });
    for (int j = 0; j < n; ++j) ctx->sb_order[j] = static_cast<uint8_t>(order[j]);
    ctx->sb_order_key = fs.sb_key;
    ctx->sb_order_n = n;
}

// "depth_split" 0: how many slabs the next frames' rays are cut into.  K jobs per tile of a K-th of a ray's steps each:
// worth it while the jobs do not fill the wavefront slots (a frame of one round lasts as long as ONE ray, however
// few rays it has) and the rays are long enough to be worth cutting.
// Measured (profiles/r04_split_probe.md): K jobs per tile pay while K x (tiles with rays) still fit the slots in ONE
// round — the 124-row share of the C3 frame that one of 8 GPUs renders: walk 0.19 -> 0.13 (2 slabs); 4 slabs, 8 640
// jobs on 7 168 slots, are two rounds and no faster than 2 — and a slab is worth its plane raster and its jobs'
// start and end (~40 segments per ray and slab: the C2 ball's 70-segment rays are left whole).
// What a frame lasts is set by its LONGEST rays (seg_max), and they are cut evenly only if the planes divide THEIR
// depth range: the next frame's planes go between the shallowest entry and the deepest exit this frame's rays had
// (one GPU's rows of a frame see a part of the grid's depth range only; no earlier frame: the grid's bounding box).
int next_split_count(const FrameTotals& hc) {
    if (!(hc.covered > 0 && hc.segments > 0 && hc.ray_tiles > 0)) return 1;
    // jobs that really walk: a tile's rays span about K x (their length / the longest ray's) slabs, + 1/2 for the
    // plane they straddle; the other jobs of the tile find nothing to do and leave their slot at once
    const double slots = 0.98 * 256.0 * 4.0 * 7.0;  // the split walk runs 7 wavefronts per SIMD
    const double mean_over_max = std::fmin(1.0, static_cast<double>(hc.segments) / static_cast<double>(hc.covered) / static_cast<double>(hc.seg_max ? hc.seg_max : 1u));
    int k = 1;
    for (int t = 2; t <= 4; ++t)
        if (static_cast<double>(hc.ray_tiles) * (t * mean_over_max + 0.5) <= slots) k = t;
    k = std::min(k, static_cast<int>(static_cast<double>(hc.seg_max) / 56.0));
    return std::max(1, k);
}

// The planes through the sampled rays' entries and ends: z ~ a + b x + c y by least squares, each; then the mean
// tilt (gx, gy), and what is left of either plane's depth at the origin once that tilt is taken out of its sample.
struct PlaneFit {
    bool known = false;
    double gx = 0.0, gy = 0.0, entry0 = 0.0, exit0 = 0.0;
};

PlaneFit fit_depth_planes(const c5::DepthSamples& smp, const c5::ImageParams& im) {
    struct { double entry[9], exit_[9]; } fit{};  // n, Sx, Sy, Sxx, Sxy, Syy, Sz, Sxz, Syz
    const int n_slots = std::min<int64_t>(c5::kFitSlots, static_cast<int64_t>(im.fit_cols) * ((im.res_y >> im.fit_shift) + 1));
    const int mid = ((1 << im.fit_shift) - 1) >> 1;
    for (int slot = 0; slot < n_slots; ++slot) {
        if (smp.entry_key[slot] == 0ull || smp.exit_key[slot] == 0ull) continue;
        const double x = im.x_min + im.step_x * (((slot % im.fit_cols) << im.fit_shift) + mid);
        const double y = im.y_min + im.step_y * (((slot / im.fit_cols) << im.fit_shift) + mid);
        const double z[2] = {c5::depth_of_key(smp.entry_key[slot]), c5::depth_of_key(smp.exit_key[slot])};
        double* const sums[2] = {fit.entry, fit.exit_};
        for (int t = 0; t < 2; ++t) {
            const double v[9] = {1.0, x, y, x * x, x * y, y * y, z[t], x * z[t], y * z[t]};
            for (int j = 0; j < 9; ++j) sums[t][j] += v[j];
        }
    }
    auto solve = [](const double* m, double out[3]) {  // normal equations, Cramer (3 x 3, well scaled: x, y ~ 1)
        const double n = m[0], sx = m[1], sy = m[2], sxx = m[3], sxy = m[4], syy = m[5], sz = m[6], sxz = m[7], syz = m[8];
        const double det = n * (sxx * syy - sxy * sxy) - sx * (sx * syy - sxy * sy) + sy * (sx * sxy - sxx * sy);
        if (!(std::fabs(det) > 1e-12 * std::fabs(n * sxx * syy) && n >= 12.0)) return false;
        out[0] = (sz * (sxx * syy - sxy * sxy) - sx * (sxz * syy - sxy * syz) + sy * (sxz * sxy - sxx * syz)) / det;
        out[1] = (n * (sxz * syy - syz * sxy) - sz * (sx * syy - sxy * sy) + sy * (sx * syz - sxz * sy)) / det;
        out[2] = (n * (sxx * syz - sxy * sxz) - sx * (sx * syz - sxz * sy) + sz * (sx * sxy - sxx * sy)) / det;
        return std::isfinite(out[0]) && std::isfinite(out[1]) && std::isfinite(out[2]);
    };
    PlaneFit r;
    double pe[3], px[3];
    if (solve(fit.entry, pe) && solve(fit.exit_, px)) {
        const double gx = 0.5 * (pe[1] + px[1]), gy = 0.5 * (pe[2] + px[2]);
        const double e0 = (fit.entry[6] - gx * fit.entry[1] - gy * fit.entry[2]) / fit.entry[0];
        const double x0 = (fit.exit_[6] - gx * fit.exit_[1] - gy * fit.exit_[2]) / fit.exit_[0];
        if (x0 > e0 && std::fabs(gx) < 64.0 && std::fabs(gy) < 64.0) {
            r.known = true;
            r.gx = gx, r.gy = gy, r.entry0 = e0, r.exit0 = x0;
        }
    }
    return r;
}

// What the frame tells the next ones about their depth split ("depth_split" 0): the planes fitted through its rays'
// entries and ends, the depths its rays ran between, and the slab count it suggests.
void update_split_state(c5_context* ctx, const FrameSlot& fs, const FrameTotals& hc) {
    // (the samples lie behind the counter shards; c5_set_image drains the ring before it changes the image)
    const PlaneFit fit = fit_depth_planes(*reinterpret_cast<const c5::DepthSamples*>(fs.host_counters + c5::kCounterShards), ctx->im);
    ctx->fit_known = fit.known;
    if (fit.known) ctx->fit_gx = fit.gx, ctx->fit_gy = fit.gy, ctx->fit_entry0 = fit.entry0, ctx->fit_exit0 = fit.exit0;
    ctx->ray_depth_known = hc.exit_max_key != 0 && hc.entry_min_key != 0;
    if (ctx->ray_depth_known) {
        ctx->ray_depth_lo = -c5::depth_of_key(hc.entry_min_key);
        ctx->ray_depth_hi = c5::depth_of_key(hc.exit_max_key);
        ctx->ray_depth_known = ctx->ray_depth_hi > ctx->ray_depth_lo;
    }
    if (!uses_bin_sort(ctx)) ctx->split_auto_k = next_split_count(hc);
}

// c5_stats of the frame (ctx->last), the stage times of a timed frame among them.
int fill_stats(c5_context* ctx, const FrameSlot& fs, const FrameTotals& hc) {
    c5_stats& st = ctx->last;
    st.segments = static_cast<int64_t>(hc.segments);
    st.covered_pixels = static_cast<int64_t>(hc.covered);
    st.solid_pixels = static_cast<int64_t>(hc.solid_pixels);
    st.entries = static_cast<int64_t>(hc.entries);
    st.boundary_faces = ctx->n_bfaces;
    st.steps = static_cast<int64_t>(hc.steps);
    st.walk_overflow = static_cast<int32_t>(hc.walk_overflow);
    st.entry_overflow = hc.entry_overflow > 0 ? 1 : 0;  // THIS frame; the sticky words cover every frame in flight
    st.odd_pixels = static_cast<int64_t>(hc.odd_pixels);
    if (ctx->frame_timed) {
        float* dst[5] = {&st.ms_transform, &st.ms_records, &st.ms_entries, &st.ms_solids, &st.ms_walk};
        for (int k = 0; k < 5; ++k) C5_HIP(ctx, hipEventElapsedTime(dst[k], fs.ev[k], fs.ev[k + 1]));
        C5_HIP(ctx, hipEventElapsedTime(&st.ms_total, fs.ev[0], fs.ev[5]));
        // a frame that reused the per-view data of the frames before it ("view_cache") ran none of the three: exactly 0
        if (fs.setup_reused) st.ms_transform = st.ms_records = st.ms_entries = 0.0f;
    }
    // overflow entries this frame needed: handed out (a shard hands out min(asked, its part)) + refused
    int64_t handed = 0;
    for (int k = 0; k < c5::kCounterShards; ++k) {
        const int64_t part = (static_cast<int64_t>(k + 1) * fs.entry_capacity) / c5::kCounterShards -
                             (static_cast<int64_t>(k) * fs.entry_capacity) / c5::kCounterShards;
        handed += std::min<int64_t>(static_cast<int64_t>(fs.host_counters[k].pool_used), part);
    }
    st.pool_entries = handed + static_cast<int64_t>(hc.entry_overflow);
    st.pool_capacity = fs.entry_capacity;
    return C5_OK;
}

// Some frame since the last look failed: wait for everything of the context and clear the sticky words.
int clear_sticky_words(c5_context* ctx, bool frames_incomplete) {
    int rc = drain(ctx);
    if (rc) return rc;
    // Frames delivered to host memory that are still outstanding were all enqueued before this moment, i.e.
    // rendered with the buffers that were too small: their waits must say so whatever their status snapshots
    // read (a snapshot is copied on the copy stream and may run after the words are cleared here) — also when
    // it is c5_get_stats / c5_get_row_costs / c5_synchronize, not c5_render_host_wait, that notices first.
    if (frames_incomplete) ctx->hr_retry_left = ctx->hr_count;
    if (ctx->copy_stream && ctx->hr_count) C5_HIP(ctx, hipStreamSynchronize(ctx->copy_stream));
    // cleared IN the stream the kernels that add to it run on, and waited for: nothing rests on how the NULL stream
    // is ordered against this context's non-blocking streams
    C5_HIP(ctx, hipMemsetAsync(ctx->sticky.ptr, 0, kStickyWords * sizeof(unsigned), ctx->stream));
    C5_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < kStickyWords; ++k) ctx->host_sticky[k] = 0;
    return C5_OK;
}

// Keep the pool at twice the demand just seen (plus a margin): the demand is a smooth function of the
// view, so in a sweep the pool grows ahead of it, between frames, without a frame ever being lost.
int size_entry_pool(c5_context* ctx, const FrameSlot& fs, int64_t refused) {
    const int64_t demand = ctx->last.pool_entries;
    int64_t want = 0;
    if (refused > 0) want = 2 * (std::max(demand, fs.entry_capacity) + refused) + 8192;
    else if (2 * demand + 4096 > fs.entry_capacity) want = 2 * demand + 8192;
    if (want > kMaxEntryPool) want = kMaxEntryPool;
    if (want <= fs.entry_capacity) return C5_OK;
    int rc = drain(ctx);
    if (rc) return rc;
    return grow_entry_pools(ctx, want);
}

// the failure the sticky words stand for, as the caller hears of it
int report_failures(c5_context* ctx, int64_t refused, unsigned lost_rays, unsigned overlap_rays) {
    if (refused > 0) {
        return fail(ctx, C5_RETRY,
                    "%lld boundary entries found no room in the overflow pool (now %lld records): every frame "
                    "since the last c5_synchronize is incomplete, render again",
                    static_cast<long long>(refused), static_cast<long long>(ctx->slots[0].entry_capacity));
    }
    if (lost_rays)
        return fail(ctx, C5_ERR_WALK, "%u rays exceeded the walk step bound (malformed grid?)", lost_rays);
    if (overlap_rays) {
        // Cells of two components that share no face interpenetrate (walk_common.hpp: next_entry): the reference bins and
        // sorts such a soup (plane.cpp:184-192, line.cpp:138), a walk cannot render it.  From here on this grid goes
        // through bin_sort_resolve, like a grid with a face in more than two cells (c5_upload_grid).
        ctx->overlap_seen = true;
        ++ctx->setup_epoch;
        return fail(ctx, C5_RETRY,
                    "%u rays met a boundary entry inside a stretch of cells they had walked: components of the grid interpenetrate; "
                    "every frame since the last c5_synchronize is wrong, render again (bin_sort_resolve from now on)", overlap_rays);
    }
    return C5_OK;
}

// After the stream drained: collect counters/timings; grow the entry buffer if it overflowed.
int finish_frame(c5_context* ctx) {
    if (!ctx->frame_pending) return C5_OK;
    ctx->frame_pending = false;
    const FrameSlot& fs = ctx->slots[ctx->last_slot];
    const FrameTotals hc = sum_counters(fs.host_counters);
    update_sb_order(ctx, fs, hc.covered);
    // How coarse the pixels are against the cells decides how many distinct cells an 8x8 tile meets per step, and
    // with it how many staging slots the next frame's walk gets (walk_plan.hpp: walk_plan, 14 or 21): rays per cell of the
    // WHOLE frame, this context's share scaled up by the number of row shards.
    if (ctx->n_cells > 0 && hc.segments > 0)
        ctx->rays_per_cell = static_cast<double>(hc.segments) * static_cast<double>(ctx->im.world > 0 ? ctx->im.world : 1) *
                             (static_cast<double>(ctx->im.res_y) / static_cast<double>(ctx->im.row_count > 0 ? ctx->im.row_count : ctx->im.res_y)) /
                             static_cast<double>(ctx->n_cells);
    update_split_state(ctx, fs, hc);
    int rc = fill_stats(ctx, fs, hc);
    if (rc) return rc;
    // failures of ANY frame since the last look (several frames may have been in flight)
    const int64_t refused = static_cast<int64_t>(ctx->host_sticky[0]);  // entries that found no slot, all those frames
    const unsigned lost_rays = ctx->host_sticky[1];
    const unsigned overlap_rays = ctx->host_sticky[2];
    if (refused > 0 || lost_rays || overlap_rays) {
        rc = clear_sticky_words(ctx, refused > 0 || overlap_rays);
        if (rc) return rc;
    }
    rc = size_entry_pool(ctx, fs, refused);
    if (rc) return rc;
    return report_failures(ctx, refused, lost_rays, overlap_rays);
}

}  // namespace

// Wait for the context's stream and collect the last frame's outcome.
int wait_and_collect(c5_context* ctx) {
    if (ctx->frame_pending && !ctx->counters_on_host) {
        FrameSlot& fs = ctx->slots[ctx->last_slot];
        C5_HIP(ctx, hipMemcpyAsync(fs.host_counters, ctx->last_counters ? ctx->last_counters : fs.counters.ptr, kCountersBytes, hipMemcpyDeviceToHost, ctx->stream));
        C5_HIP(ctx, hipMemcpyAsync(ctx->host_sticky, ctx->sticky.ptr, kStickyWords * sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
        if (fs.sb_key >= 0 && fs.sb.ptr && ctx->host_sb)
            C5_HIP(ctx, hipMemcpyAsync(ctx->host_sb, fs.sb.ptr, c5::kMaxSbRows * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        ctx->counters_on_host = true;
    }
    C5_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const int rc = finish_frame(ctx);
    const int rc_adj = finish_adjoint(ctx);
    return rc ? rc : rc_adj;
}

}  // namespace c5api

using namespace c5api;

extern "C" {

int c5_render_device(c5_context* ctx, void* out_device) {
    if (!ctx) return fail(nullptr, C5_ERR_INVALID, "null context");
    if (!out_device) return fail(ctx, C5_ERR_INVALID, "null output pointer");
    return enqueue_frame(ctx, static_cast<float2*>(out_device));
}

int c5_synchronize(c5_context* ctx) {
    if (!ctx) return fail(nullptr, C5_ERR_INVALID, "null context");
    int rc = bind_device(ctx);
    if (rc) return rc;
    return wait_and_collect(ctx);
}

}  // extern "C"

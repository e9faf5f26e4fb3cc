// The context behind the C ABI (include/course5_hip.h) and what the files that implement it share: device buffers, the
// frame slots, the solids, failure reporting.  Private to the library: everything here but c5_context itself lives in
// c5api, whose symbols stay out of the dynamic symbol table (the attribute goes on every body of the namespace: it
// holds for the declarations and definitions inside that one body).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/course5_hip.h"
#include "adjacency.hpp"
#include "adjoint.hpp"
#include "device_types.hpp"
#include "kernels.hpp"

namespace c5api __attribute__((visibility("hidden"))) {

struct DeviceBuffer {
    void* ptr = nullptr;
    size_t bytes = 0;
    hipError_t ensure(size_t want) {
        if (want <= bytes && ptr) return hipSuccess;
        if (ptr) {
            hipError_t e = hipFree(ptr);
            ptr = nullptr;
            bytes = 0;
            if (e != hipSuccess) return e;
        }
        if (want == 0) return hipSuccess;
        hipError_t e = hipMalloc(&ptr, want);
        if (e == hipSuccess) bytes = want;
        return e;
    }
    void release() {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        bytes = 0;
    }
    template <class T>
    T* as() const {
        return static_cast<T*>(ptr);
    }
};

struct Solid {
    int64_t n_tets = 0;      // as given
    int64_t n_points = 0;    // unique points
    int64_t n_faces = 0;     // unique faces
    int64_t n_interior = 0;  // of them, at the head of the list: faces with a cell on either side (adjacency.hpp)
    double colour = 0.0;
    // The faces in groups of about the same size (binary exponent of the longest edge, longest first; the interior faces'
    // groups before the others'): solid_mask_raster gives a face as many lanes as its rows ask for, and what a launch
    // lasts is the longest chain of rows ONE lane walks - the 130 000 surface triangles of the Roche lobe are a few pixels
    // each, its few hundred closing faces (object3d_base.cpp:171-174) span the whole solid.
    struct FaceGroup {
        int64_t begin, count;
        double longest;  // edge, object units (no rotation makes a face taller)
    };
    std::vector<FaceGroup> groups;
    double centre[3] = {0, 0, 0};        // bounding sphere of the points (object space)
    double radius = 0.0;
    DeviceBuffer raw;        // unique points [m][3]
    DeviceBuffer faces;      // unique faces, int4 (a, b, c, 0)
    DeviceBuffer view[2];    // transformed points, one per frame slot
    c5::RotationList rots{};
    // A solid whose view and image did not change since the frame before (the accretor sphere never rotates,
    // main.cpp:116; in a -D sweep only the lobe moves) is rastered ONCE into a mask of its own, which later
    // frames lay over theirs (one pass over the image instead of a transform and a raster of 10^5-10^6 faces).
    DeviceBuffer own_mask;
    c5::RotationList seen_rots{};
    c5::ImageParams seen_im{};
    uint64_t generation = 0, seen_generation = ~uint64_t{0};
    hipStream_t seen_stream = nullptr;  // the own mask is written and read in the order of ONE stream
    int unchanged_frames = 0;
    bool own_mask_ready = false;
};

inline bool same_rotations(const c5::RotationList& a, const c5::RotationList& b) {
    if (a.n != b.n) return false;
    for (int k = 0; k < a.n; ++k)
        if (a.axis[k] != b.axis[k] || a.cosv[k] != b.cosv[k] || a.sinv[k] != b.sinv[k] || a.x0[k] != b.x0[k]) return false;
    return true;
}
inline bool same_image(const c5::ImageParams& a, const c5::ImageParams& b) {
    return a.res_x == b.res_x && a.res_y == b.res_y && a.n_local_rows == b.n_local_rows && a.tile_rows == b.tile_rows &&
           a.rank == b.rank && a.world == b.world && a.row_begin == b.row_begin && a.row_count == b.row_count &&
           a.x_min == b.x_min && a.y_min == b.y_min && a.step_x == b.step_x && a.step_y == b.step_y;
}

constexpr int kWalkEventPool = 512;
constexpr size_t kStageChunk = size_t{4} << 20;  // pinned staging for pageable destinations, two of these
constexpr int kFrameSlots = 2;
constexpr int kStickyWords = 3;   // entries without a pool slot, rays over the step bound, rays that skipped an entry
constexpr int kStatusWords = 3;   // a frame's own walk_overflow, entry_overflow, overlap_rays (FrameCounters, shard 0)
constexpr int64_t kMaxEntryPool = int64_t{16777214} * 64;  // entries of an overflow pool at the most: slot + 1 must fit 31 bits
constexpr size_t kCountersBytes = sizeof(c5::FrameCounters) * c5::kCounterLines;  // the shards + DepthFitSums (device_types.hpp)

// Everything one frame writes before its image: two slots, so that the per-view setup of frame
// k + 1 (HBM-bound: transform, records, entry lists, solid mask) can run on the auxiliary stream
// while walk_composite of frame k (VALU / address-path bound) runs on the main stream.
struct FrameSlot {
    DeviceBuffer vx, vy, vz, rec, count, head, first, pool, mask, counters, row_cost;
    DeviceBuffer sb;        // cost of the walk's rows of super-blocks in the last frame (WalkParams::sb_cost)
    long long sb_key = -1;  // the tiling they belong to (-1: not collected)
    int sb_n = 0;
    // "view_cache": the per-view data in this slot (transformed vertices, records, entry lists) were built for ...
    uint64_t setup_epoch = 0;     // ... this state of the context (c5_context::setup_epoch; 0: nothing built)
    c5::RotationList setup_view{};
    double setup_limit = 0.0;
    int setup_order = 0;
    bool setup_kept = false;      // ... and the walk that used them left the entry heads in place
    bool setup_reused = false;    // the last frame enqueued into this slot skipped the per-view setup
    const c5::FrameCounters* raster_counters = nullptr;  // device: counters of the frame whose raster built the slot's entry lists
    // "depth_split" (device_types.hpp: SplitParams)
    DeviceBuffer plane_cell, straddle, straddle_count, partials, arrivals;
    DeviceBuffer bfrec;          // BFaceRecord per boundary face (build_records -> entry_raster_rec), stamped with ...
    uint32_t bf_seq = 0;         // ... the number of the frame that wrote it
    int split_k = 0;             // slabs the buffers above are laid out for (0: none)
    int64_t split_px = 0, split_tiles = 0, split_cells = 0;
    uint64_t split_seq = 0;      // raster frames so far: stamp = seq % 15 + 1, counter half = seq & 1
    int setup_split = 1;         // slabs the slot's per-view data (plane cells) were built for ("view_cache")
    double setup_w[c5::kMaxSlabs + 1] = {};
    double setup_g[2] = {0.0, 0.0};
    int64_t entry_capacity = 0;
    // which 8x8 tiles hold an entry (walk_common.hpp: RasterArgs::tile_flag): a word per tile = the number of the raster run
    // that found one there
    DeviceBuffer tile_flag;
    uint32_t flag_seq = 0;
    int64_t flag_tiles = 0;
    bool flags_valid = false;  // the slot's entry lists were built by a raster that kept them
    bool head_clean = false;  // the per-pixel entry heads are all zero (the walk kernels leave them so)
    c5::FrameCounters* host_counters = nullptr;  // pinned
    hipEvent_t setup_done = nullptr, walk_done = nullptr;
    bool walk_recorded = false;
    hipEvent_t ev[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
};

// Everything the derivative renders keep on the context (derivative_host.hpp and the files over it): buffers, options,
// and the status of the last call.
struct DerivativeState {
    // adjoint render (c5_render_adjoint*): nothing of it is allocated before the first adjoint call
    DeviceBuffer adj_lambda;    // [n_local_px] fp64: pass 1 -> pass 2 (scalar_derivative_kernels.hip)
    DeviceBuffer adj_counters;  // the adjoint's own FrameCounters: a frame's statistics and failure words stay the frame's
    DeviceBuffer adj_sticky;    // the entry raster's failure words for the adjoint (never the frames' sticky words)
    DeviceBuffer adj_grad;      // [2][n_cells] fp64, device order
    unsigned* adj_status = nullptr;  // pinned: walk_overflow, entry_overflow, overlap_rays of the last adjoint or tangent,
                                     // rows a ray matrix fill found changed, contributions an exact sum found beyond their exponent
    bool adjoint_pending = false;    // its status has not been looked at yet
    const char* adj_what = "adjoint";  // which of the two it was (finish_adjoint's messages)

    // exact adjoint sums ("adjoint_exact", c5_render_adjoint_exact_*): allocated at the first exact call only
    int adjoint_exact = 0;           // "adjoint_exact": c5_render_adjoint* and its batch return the exact sums (exact_sum.hpp)
    int exact_sums = 0;              // "exact_sums": the adjoint, c5_render_gn_* and c5_render_hvp* return the exact sums
    DeviceBuffer adj_exact;   // [n_cells][4] int64 words, [n_cells] int2 exponents (device order), then the misfit word

    // tangent render (c5_render_tangent*): shares the adjoint's counters, sticky and status words; nothing of
    // it is allocated before the first tangent call
    DeviceBuffer tan_dir;  // [n_cells] {dalpha, dQ} fp64, device order (scalar_derivative_kernels.hip: tangent_gather)

    // batches (c5_render_tangent_batch*, c5_render_adjoint_batch*): nothing of it is allocated before the first batch call
    int batch_width = 0;    // "batch_width": directions or upstream images per walk (0: 4 for batches of up to 4, else 8)
    DeviceBuffer bat_dirs;  // [n_cells][width] {dalpha, dQ} fp64, device order (scalar_derivative_kernels.hip: tangent_gather_batch)
    DeviceBuffer bat_grad;  // [n_cells][2 width] fp64, device order (adjoint_walk_batch)
    // Gauss-Newton renders (c5_render_gn_product*, c5_render_gn_diagonal*): nothing of it is allocated before the first call
    DeviceBuffer gn_g;      // [width][n_local_px] float2: pass A's w * J v, pass B's upstream images (a chunk's)
    DeviceBuffer gn_spare;  // [width][n_cells] fp64: where the block of H v goes that the caller did not ask for
    // Hessian-vector render (c5_render_hvp*): shares adj_lambda, adj_grad and tan_dir; allocated at the first call only
    DeviceBuffer hvp_lambda_dot;  // [n_local_px] fp64: pass 1 -> pass 2 (scalar_derivative_kernels.hip: hvp_walk)
    // vertex adjoint (c5_render_vertex_adjoint*): nothing of it is allocated before the first call (it shares adj_lambda)
    DeviceBuffer vtx_face;  // [n_cells][4][3] fp64, device order: the chords' weights per face and vertex of the face
    DeviceBuffer vtx_grad;  // [n_pts][3] fp64: the gradient in view space
    int vertex_merge = 1;          // "vertex_merge": vertex_walk sums the lanes of a wavefront in one cell before its atomics
                                   // (measured on the C3 frame: 5.7 ms against 58 ms for the walk; profiles/vertex_adjoint_probe.md)
    // batched vertex adjoint (c5_render_vertex_adjoint_batch*): allocated at the first batched call only
    DeviceBuffer vtx_bat_face;  // [n_cells][width][4][3] fp64, device order: vtx_face per image of a chunk
    DeviceBuffer vtx_bat_grad;  // [n_pts][3][width] fp64: vtx_grad per image of a chunk, the images of a component side by side
    // exact vertex adjoint sums ("vertex_exact", c5_render_vertex_exact_*): allocated at the first exact vertex call only
    int vertex_exact = 0;              // "vertex_exact": c5_render_vertex_adjoint* and its batch return the exact sums
    DeviceBuffer vtx_exact;     // [n_cells][12][2] int64 words, [n_cells][12] int32 exponents (device order), the misfit word
    DeviceBuffer vtx_triples;   // [n_cells][4][3] fp64, device order: a cell's share of its four vertices' view-space gradient
    DeviceBuffer vtx_inc;       // point -> (cell, vertex) incidence, CSR: int32 [n_pts + 1] offsets, int32 [4 n_cells] entries
    uint64_t vtx_inc_serial = ~uint64_t{0};  // ... for the grid of this upload (c5_context::grid_serial; kept across c5_update_points)
    // vertex tangent (c5_render_vertex_tangent*): allocated at the first call only
    DeviceBuffer vtx_vel;   // [n_pts][width][3] fp64: the points' view-space velocities (vertex_velocity)
    // ray matrix (c5_ray_matrix_*): allocated at the first call only (the scan's scratch is bin_sort_resolve's scratch64)
    DeviceBuffer rm_count;  // [padded local px] int32 segments per pixel, then one word: rows the fill found changed
    // the host-pointer forms of all derivative renders: what the caller hands in and what goes back (run_staged)
    DeviceBuffer io;

    // Frees everything above that is owned: every buffer, and the pinned status words.
    void release() {
        DeviceBuffer* const owned[] = {&adj_lambda, &adj_counters, &adj_sticky, &adj_grad, &adj_exact, &tan_dir, &bat_dirs, &bat_grad,
                                       &gn_g, &gn_spare, &hvp_lambda_dot, &vtx_face, &vtx_grad, &vtx_bat_face, &vtx_bat_grad,
                                       &vtx_exact, &vtx_triples, &vtx_inc, &vtx_vel, &rm_count, &io};
        for (DeviceBuffer* b : owned) b->release();
        if (adj_status) (void)hipHostFree(adj_status);
        adj_status = nullptr;
    }
};

// The smoothness prior (c5_prior_*, prior.hip): nothing of it is allocated before the first call.
struct PriorState {
    DeviceBuffer w[2];  // [n_cells][4] fp64 face weights, device order, per weighting (C5_PRIOR_UNIT, C5_PRIOR_TPFA)
    uint64_t w_grid[2] = {~uint64_t{0}, ~uint64_t{0}};    // ... for the grid of this upload (c5_context::grid_serial)
    uint64_t w_points[2] = {~uint64_t{0}, ~uint64_t{0}};  // ... and these points (c5_context::points_serial; TPFA alone looks)
    int64_t n_interior[2] = {0, 0}, n_degenerate[2] = {0, 0};
    DeviceBuffer counts;    // two words the weights' build counts into
    DeviceBuffer partials;  // [2][blocks] fp64: the value's per-block sums
    DeviceBuffer io;        // the host-pointer forms' staging
    void release() {
        DeviceBuffer* const owned[] = {&w[0], &w[1], &counts, &partials, &io};
        for (DeviceBuffer* b : owned) b->release();
    }
};

// The shape prior (c5_shape_prior_*, shape_prior.hip): nothing of it is allocated before the first call.
struct ShapeState {
    DeviceBuffer binv, vol;  // the rest data, device order: B = Dm^-1 [n_cells][3][3] and V0 [n_cells] (zeros: a degenerate cell)
    bool have_rest = false;  // ... set by c5_shape_prior_rest, dropped by c5_upload_grid, kept across c5_update_points
    int64_t n_degenerate = 0;
    DeviceBuffer shares;     // [n_cells][4][3] fp64, device order: the cell launch -> the point launch
    DeviceBuffer partials;   // [blocks] fp64 then [blocks] int64: the value's and the inverted count's per-block sums
    DeviceBuffer counts;     // two words the rest's build counts into (non-finite coordinates, degenerate cells)
    DeviceBuffer io;         // the host-pointer forms' staging
    void release() {
        DeviceBuffer* const owned[] = {&binv, &vol, &shares, &partials, &counts, &io};
        for (DeviceBuffer* b : owned) b->release();
        have_rest = false;
    }
};

}  // namespace c5api

struct c5_context {
    int device = 0;
    hipStream_t stream = nullptr;      // stream in use
    hipStream_t own_stream = nullptr;  // created by c5_create
    std::string error;

    // persistent grid
    int64_t n_pts = 0, n_cells = 0, n_bfaces = 0;
    hipStream_t aux_stream = nullptr;  // per-view setup of the next frame
    hipStream_t side_stream = nullptr; // entry lists + solid mask beside build_records
    hipEvent_t fork_ev = nullptr, join_ev = nullptr;
    int fuse_setup = 0;     // build_records + entry_raster as one launch of interleaved workgroups: measured 0.119 ms against
                            // 0.047 + 0.047 ms for the two launches on the C3 frame (the raster inherits the records' 49 KB of LDS)
    int cell_order = 1;     // "cell_order": c5_upload_grid keeps the cells in Morton order of their centroids (set BEFORE the upload)
    std::vector<int32_t> cell_perm;  // device index -> the caller's (empty: the same)
    int block_cull = 1;     // "block_cull": build_records judges whole workgroups by a sphere about their cells (a part of the rows only)
    int tile_flags = 1;     // "tile_flags": the raster marks the tiles that hold an entry, the walk looks there first (enqueue_frame)
    int cost_order = 1;     // "cost_order": rows of super-blocks start dearest first (by the last frame the host waited for)
    uint8_t sb_order[128] = {};
    long long sb_order_key = -1;
    int sb_order_n = 0;
    uint32_t* host_sb = nullptr;  // pinned: the last frame's per-row costs
    int entry_key = 1;      // "entry_key": 1 = entries keyed a slack behind their face (hanging-node interfaces), 0 = at the face (testing)
    int stage_slots = 0;    // "stage_slots": 0 = chosen per frame from rays_per_cell, or 14 / 21
    double rays_per_cell = 0.0;  // of the last finished frame (0: none yet)
    int solid_cache = 1;    // a solid unchanged since the frame before is not rastered again (enqueue_solids)
    int view_cache = 1;     // "view_cache": a frame with the view of the two before it reuses their per-view data (enqueue_frame)
    uint64_t setup_epoch = 1;  // bumped by everything but the view, the alpha limit and the solids that the per-view data depend on
    int solid_interior_faces = 0;  // 1: interior faces are rastered too (they cover nothing the others do not; testing)
    int depth_split = 0;    // "depth_split": 0 = chosen per frame (split_auto_k), 1 = never, 2..8 = that many slabs
    int entry_records = 1;  // "entry_records": build_records leaves a record per boundary face for the entry raster (0: the raster gathers)
    int split_auto_k = 1;   // what the last finished frame suggests (finish_frame)
    bool ray_depth_known = false;  // ... and the depths its rays ran between (walk coordinate)
    double ray_depth_lo = 0.0, ray_depth_hi = 0.0;
    // ... and the planes fitted through where its (sampled) rays entered the grid and where they ended (DepthFitSums):
    // common tilt (fit_gx, fit_gy) and the two planes' depths at x = y = 0 once that tilt is taken out
    bool fit_known = false;
    double fit_gx = 0.0, fit_gy = 0.0, fit_entry0 = 0.0, fit_exit0 = 0.0;
    double split_tilt_x = 0.0, split_tilt_y = 0.0;  // "split_tilt_x" / "_y" (testing): the tilt of a FORCED split's planes
    double box_lo[3] = {0, 0, 0}, box_hi[3] = {0, 0, 0};  // the grid's bounding box in object space
    double alpha_floor = 0.0;  // smallest alpha of the grid that is >= DBL_EPSILON (+inf: none)
    int overlap_setup = 0;  // measured: 1.27 vs 1.26 ms/frame, the side stream buys nothing
    c5api::DeviceBuffer px, py, pz, cell_vert, cell_adj, alpha, q, bface, block_sphere;
    double alpha_top = 0.0;      // largest alpha of the grid (c5_upload_grid / c5_update_scalars)
    double edge_max = 0.0;       // longest edge of any cell: no view makes a cell longer along a ray
    double grid_diagonal = 0.0;  // of the grid's bounding box in object space: no rotation makes the grid longer along a ray
    double coord_max = 0.0;      // largest |coordinate| (what the rounding of an absolute depth scales with)
    c5api::FrameSlot slots[c5api::kFrameSlots];
    int64_t frame_index = 0;
    int last_slot = 0;
    void* last_counters = nullptr;  // device: the counters the last enqueued frame adds to (the slot's, or a host-ring frame's own)
    int row_cost_slot = 0;          // the slot whose row_cost[] holds the segments per row of the last frame that counted them
    int algorithm = 0;        // 0: walk, 1: bin_sort_resolve
    bool grid_conforming = true;   // no face in more than two cells (c5_upload_grid)
    bool overlap_seen = false;     // a frame's walk met interpenetrating components (finish_frame): bin_sort_resolve until the next upload
    c5api::DeviceBuffer offs64, scratch64, segs;  // bin_sort_resolve
    int pipeline = 0;  // measured at the end of round 1: 0.689 ms per C3 frame with it, 0.702 without
    c5::RotationList view{};
    c5api::Solid solids[C5_MAX_SOLIDS];

    // image
    bool have_image = false;
    double bounds[4] = {0, 0, 0, 0};
    c5::ImageParams im{};
    int cfg_tile_rows = 0, cfg_rank = 0, cfg_world = 1;
    int cfg_row_begin = 0, cfg_row_count = -1;  // -1: all rows
    c5api::DeviceBuffer xtab, ytab, out, sticky;  // sticky: kStickyWords x u32 failure words that persist across frames (kernels.hpp: WalkParams::sticky)
    unsigned* host_sticky = nullptr;       // pinned copy, refreshed at the end of every frame
    std::vector<double> host_ytab;
    int row_costs = 0;
    bool row_costs_collected = false;  // some frame since the rows were last laid out counted its segments per row

    // options
    double alpha_limit = 2.5;
    double t_cutoff = 1e-12;
    int tile_shape = 3;  // 8x8 pixels per wavefront (fewest distinct cells per step), one wavefront per workgroup
    int xcd_mode = 2;
    int lds_pad = 0;
    int band_rows = 0;
    int order = 0;
    int lds_stage = 2;
    // instruments, off unless asked for: the six stage events cost 21-25 us of a 0.52-ms frame when frames follow one another
    // without a wait, the two around the walk 6 (profiles/experiments.md)
    int stage_timing = 0;
    int walk_timing = 0;
    unsigned walk_seq = 0;

    // events
    hipEvent_t walk_a[c5api::kWalkEventPool];
    hipEvent_t walk_b[c5api::kWalkEventPool];
    int walk_used = 0;
    double walk_ms_sum = 0.0;
    int64_t walk_launches = 0;

    // frames delivered to host memory (c5_render_host_async / _wait, c5_render)
    struct HostFrame {
        c5api::DeviceBuffer img;
        // statistics of THIS frame (FrameCounters[kCounterShards]): frames in flight never share them, so the frame's own
        // failure words can be read behind it whatever the frames after it are doing
        c5api::DeviceBuffer counters;
        hipEvent_t rendered = nullptr, copied = nullptr;
        unsigned* status = nullptr;  // pinned: {rays over the step bound, entries without a pool slot} of THIS frame
    };
    hipStream_t copy_stream = nullptr;
    HostFrame hring[C5_HOST_RING];
    int hr_head = 0, hr_count = 0, hr_next = 0;
    int hr_retry_left = 0;  // outstanding frames that were enqueued before an overflow was noticed
    void* stage[2] = {nullptr, nullptr};  // pinned staging chunks for pageable destinations
    hipEvent_t stage_ev[2] = {nullptr, nullptr};

    bool using_caller_stream = false;
    bool frame_pending = false;
    bool counters_on_host = true;  // the last frame's counters / sticky words have been copied to the host
    bool frame_timed = false;
    c5_stats last{};

    c5api::DerivativeState deriv;      // the derivative renders' buffers, options and status (derivative_host.hpp)
    c5api::DeviceBuffer adj_perm;      // cell_perm on the device, for the grid of upload adj_perm_serial (grid.hip: ensure_device_perm)
    uint64_t grid_serial = 0, adj_perm_serial = ~uint64_t{0};
    uint64_t points_serial = 0;        // bumped by c5_update_points: what is derived from the coordinates on demand is stale
    c5api::PriorState prior;           // the smoothness prior's weights and scratch (prior.hip)
    c5api::ShapeState shape;           // the shape prior's rest data and scratch (shape_prior.hip)
    // c5_update_points: the cells as the device has them (welded, in its order) and, where c5_upload_grid welded points,
    // every point's representative (empty: none welded) - what measure_grid and upload_block_spheres are run again with
    std::vector<int32_t> host_cell_vert, point_rep;
    // c5_update_scalars_device: the three statistics of the scalars on the device, and their pinned copy
    c5api::DeviceBuffer scal_stats;
    unsigned long long* scal_host = nullptr;
};

namespace c5api __attribute__((visibility("hidden"))) {

// ---- context.hip
int fail(c5_context* ctx, int code, const char* fmt, ...);

#define C5_HIP(ctx, expr)                                                                        \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return fail((ctx), C5_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                                     \
    } while (0)

int bind_device(c5_context* ctx);
int to_rotation_list(c5_context* ctx, const c5_rotation* rots, int n, c5::RotationList& out);
// tetra.cpp:44-62 on the host (what rotate_point does on the device), for bounding boxes and centres
void rotate_host(const c5::RotationList& R, double c[3]);
// Wait until nothing of this context is running (all its streams).
int drain(c5_context* ctx);
// every frame slot in use gets an overflow pool of at least `want` entries (the caller has drained the context)
int grow_entry_pools(c5_context* ctx, int64_t want);

// ---- grid.hip
// cell_perm on the device (adj_perm), for the derivatives' and c5_update_scalars_device's gathers and permutations
int ensure_device_perm(c5_context* ctx);

// ---- frame.hip
// pixels of the context's rows, and the same rounded up to the scan's 1024
inline int64_t local_pixels(const c5::ImageParams& im) { return static_cast<int64_t>(im.n_local_rows) * im.res_x; }
inline int64_t padded_pixels(const c5::ImageParams& im) { return ((local_pixels(im) + 1023) / 1024) * 1024; }
// bytes of the image of the context's rows: (tau, I) in fp32 per pixel
inline size_t image_bytes(const c5_context* ctx) { return static_cast<size_t>(local_pixels(ctx->im)) * 2 * sizeof(float); }
bool nothing_to_render(const c5_context* ctx);
bool uses_bin_sort(const c5_context* ctx);
double entry_key_slack(const c5_context* ctx);
c5::GridView grid_view(const c5_context* ctx, const FrameSlot& fs);
int enqueue_bin_lists(c5_context* ctx, FrameSlot& fs, const c5::GridView& g, hipStream_t s, c5::FrameCounters* counters, int64_t& total);
int enqueue_solids(c5_context* ctx, FrameSlot& fs, int slot_id, hipStream_t s, c5::SolidTable& table, bool& any_solid);
int enqueue_frame(c5_context* ctx, float2* out_dev, c5::FrameCounters* own_counters = nullptr);
int wait_and_collect(c5_context* ctx);

// ---- derivative_setup.hip (derivative_host.hpp: what the derivative renders' files share)
int finish_adjoint(c5_context* ctx);

// ---- geometry_derivatives.hip
// the point -> (cell, local vertex) incidence table of the uploaded grid on the device (adjoint.hpp: VertexIncidence), built
// at first use after an upload: shared by the exact vertex sums and the shape prior
int vertex_incidence(c5_context* ctx, c5::VertexIncidence& inc);

}  // namespace c5api

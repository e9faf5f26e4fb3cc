/*
 * course5_hip.h — C ABI of the MI355X (gfx950) render path for mlozhechko/course5.
 *
 * The reference has no FFI: its seam is three C++ calls made once per frame from
 * project/src/main.cpp:127-129,
 *
 *     plane base_plane{res_x, res_y, {acc_disk, roche_lobe, acc_sphere}, domain};   // plane.cpp:260-315
 *     base_plane.find_intersections();                                              // plane.cpp:184-192
 *     object2d result = base_plane.trace_rays(tetra_value::alpha, tetra_value::Q);  // plane.cpp:144-172
 *
 * preceded by the view transform object3d_base::rotate_around_{x,y}_axis
 * (object3d_base.cpp:202-219, main.cpp:105-107,112-114).  This header is what a maintainer
 * binds in their place (INTEGRATION.md shows the edit).  Everything is extern "C" with plain
 * pointers and sizes; no C++ types, no exceptions and no torch types cross it.
 *
 * Conventions
 *   - every function returns an int status (C5_OK == 0); c5_last_error() gives the message
 *     (the reference throws std::runtime_error instead: plane.cpp:40,152,263,270, line.cpp:45);
 *   - a context is used by one host thread at a time and drives one GPU;
 *   - caller keeps ownership of every host array; the library copies what it needs;
 *   - image layout is out[row][col][2] fp32, col fastest, channel innermost — the order
 *     object2d::export_to_vti writes (object2d.cpp:17-21); channel 0 = tau
 *     (line.cpp:176-193), channel 1 = I (line.cpp:195-227).
 */
#ifndef COURSE5_HIP_H
#define COURSE5_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define C5_ABI_VERSION 2

enum {
    C5_OK = 0,
    C5_ERR_INVALID = 1,     /* bad argument (null pointer, size, id range) */
    C5_ERR_STATE = 2,       /* call order: render before grid/image were set */
    C5_ERR_HIP = 3,         /* HIP runtime failure (message carries hipGetErrorString) */
    C5_ERR_MESH = 4,        /* c5_face_adjacency: a face is shared by more than two cells */
    C5_ERR_NO_DEVICE = 5,   /* no usable GPU */
    C5_ERR_WALK = 6,        /* a ray exceeded the step bound (malformed grid) */
    C5_RETRY = 7            /* EVERY frame enqueued since the last call that waited for the stream is incomplete or
                               wrong and must not be used; call c5_render_device again.  Two causes, both settled by the
                               library before it says so: an internal buffer was too small and has been grown; or the
                               walk met rays that had to SKIP a boundary entry inside a stretch of cells they had walked
                               - components of the grid that share no face interpenetrate, which the reference simply
                               bins and sorts (plane.cpp:184-192, line.cpp:138) - and the grid is rendered with
                               "algorithm" 1 from now on.  Reported by every call that waits for the stream
                               (c5_synchronize, c5_get_stats, c5_set_stream, c5_get_row_costs,
                               c5_download_view_points, c5_render_host_wait); c5_render retries by itself. */
};

#define C5_MAX_ROTATIONS 8
#define C5_MAX_SOLIDS 8

typedef struct c5_context c5_context;

/* One elementary in-place rotation, applied in list order to every vertex.
 * axis 0: tetra::point_rotate_around_x_axis (tetra.cpp:44-48);
 * axis 1: tetra::point_rotate_around_y_axis about the line x = x0, z = 0 (tetra.cpp:51-62).
 * The host evaluates cos/sin (libm, like the reference); the device applies them with
 * separately rounded multiplies and adds, so transformed vertices equal the reference's. */
typedef struct c5_rotation {
    int32_t axis;
    int32_t reserved;
    double angle; /* radians */
    double x0;
} c5_rotation;

typedef struct c5_stats {
    int64_t segments;        /* ray-tet segments with dz > 0 == plane::count_all_intersections (plane.cpp:3-12) */
    int64_t covered_pixels;  /* pixels with at least one segment */
    int64_t solid_pixels;    /* pixels overwritten by a solid colour (line.cpp:246-249) */
    int64_t entries;         /* boundary entry records produced by the entry raster */
    int64_t boundary_faces;  /* static: faces with no neighbour */
    int64_t steps;           /* walk steps taken (>= segments) */
    int32_t walk_overflow;   /* rays that hit the step bound */
    int32_t entry_overflow;  /* the overflow pool was too small for this frame (C5_RETRY) */
    /* GPU time of the last frame per stage, milliseconds (HIP events on the context stream) */
    float ms_transform;      /* view transform                     (a2); this and the next two are exactly 0 for a frame that
                              * reused the per-view data of the frames before it (option "view_cache") */
    float ms_records;        /* per-cell walk records              (a1, a10) */
    float ms_entries;        /* boundary entry raster, one pass    (a6/a7 for boundary faces) */
    float ms_solids;         /* solid mask raster                  (a6, a9) */
    float ms_walk;           /* walk_composite                     (a11-a14) */
    float ms_total;          /* first kernel start -> image complete in HBM */
    int64_t odd_pixels;      /* bin_sort_resolve only: (pixel, cell) pairs covered by an odd number of the
                                cell's faces, i.e. exactly degenerate alignment; the reference mis-pairs or
                                aborts there (plane.cpp:39-41, line.cpp:40-47), here they are skipped */
    int64_t pool_entries;    /* second and further entries of rays this frame needed room for (sum over the
                                pixels of entries - 1): a property of grid, view and image alone */
    int64_t pool_capacity;   /* room there was; the frame is complete iff pool_entries <= pool_capacity */
} c5_stats;

/* --- lifetime ----------------------------------------------------------------------------- */
int c5_abi_version(void);
int c5_device_count(int* count);
int c5_create(int device_ordinal, c5_context** out_ctx);
void c5_destroy(c5_context* ctx);
/* Message of the last failure on ctx (or of the last c5_create failure when ctx == NULL). */
const char* c5_last_error(const c5_context* ctx);

/* Run the context's work on a caller-owned HIP stream (hipStream_t passed as void*), e.g. the
 * stream of the framework that owns the output buffer, so that ordering with the caller's own
 * kernels and collectives needs no host synchronisation.  NULL restores the context's own stream. */
int c5_set_stream(c5_context* ctx, void* hip_stream);  /* waits for the old stream first: may return C5_RETRY */

/* --- scene (persistent across frames) ------------------------------------------------------ */
/* Volume grid: replaces object3d_base::read_vtk_file's per-cell copies (object3d_base.cpp:13-53)
 * and the tetra AoS (tetra.hpp:12-46).  xyz[n_pts][3] raw (untransformed) points,
 * cell_vert[n_cells][4] point ids, alpha/q[n_cells] = AbsorpCoef / radEnLooseRate
 * (object3d_accretion_disk.cpp:4).  Points with equal coordinates are welded (c5_weld_points), then the
 * face adjacency is built; n_cells must be < 2^28 (line.hpp:71-79).  A grid in which some face belongs to more than two cells cannot be walked:
 * it is accepted and rendered with "algorithm" 1 (see c5_set_option); so is, from the first frame that shows it, a grid
 * whose components share no face but interpenetrate (C5_RETRY once, see above). */
int c5_upload_grid(c5_context* ctx, const double* xyz, int64_t n_pts, const int32_t* cell_vert,
                   int64_t n_cells, const double* alpha, const double* q);
/* Replace only the cell scalars of the uploaded grid. */
int c5_update_scalars(c5_context* ctx, const double* alpha, const double* q, int64_t n_cells);
/* The same from device memory (hipMalloc'ed by anyone in this process, the caller's cell order): gathered into the
 * library's order on the context's stream, which sees the caller's work before it when it is the caller's own stream
 * (c5_set_stream).  The host needs the largest and the smallest alpha (the walk's choices, "depth_split"): the call reads
 * them back and WAITS for the stream.  A render after it returns the same bits as after c5_update_scalars. */
int c5_update_scalars_device(c5_context* ctx, const void* alpha_dev, const void* q_dev, int64_t n_cells);
/* Replace only the point coordinates of the uploaded grid (xyz[n_pts][3], the order of c5_upload_grid): what a fit of the
 * grid's SHAPE calls between its iterations.  Connectivity, weld groups, face adjacency, the cells' order and scalars stay;
 * what c5_upload_grid derives from the coordinates (bounding box, longest edge, the spheres of "block_cull") is made again,
 * and the per-view data are stale ("view_cache"), as after c5_update_scalars.  Waits for the stream.  n_pts must be the
 * uploaded grid's, every coordinate finite: else C5_ERR_INVALID and the grid is untouched.
 * Points welded at upload STAY welded: such a point takes its representative's new coordinates, its own are ignored.
 * Contract: a render after it returns, bit for bit, what a fresh context returns that was uploaded with the new
 * coordinates - whenever the new coordinates create no NEW coincident points (those a fresh upload would weld and this
 * call does not), and points welded before still coincide. */
int c5_update_points(c5_context* ctx, const double* xyz, int64_t n_pts);
/* Solid object `slot` (0..C5_MAX_SOLIDS-1): tets[n][4][3] raw vertex copies, one colour.
 * Replaces the solid part of the tetra vector (main.cpp:110-116,127; plane.cpp:130-131).
 * n == 0 removes the object.  Higher slots / higher tet index win ties, like serial -j1. */
int c5_set_solid(c5_context* ctx, int slot, const double* tets, int64_t n_tets, double colour);

/* --- per-frame parameters -------------------------------------------------------------------- */
/* plane::plane(res_x, res_y, ..., bounds) (plane.cpp:260-315); bounds4 in the reference's order
 * {x_max, x_min, y_max, y_min} (main.cpp:83). */
int c5_set_image(c5_context* ctx, int res_x, int res_y, const double* bounds4);
/* Row sharding for multi-GPU: rows are grouped in tiles of tile_rows; tile t belongs to
 * rank t % world.  Default (1 tile of res_y rows, world 1) renders the whole image.  The local
 * strip holds this rank's rows in ascending global order. */
int c5_set_row_tiles(c5_context* ctx, int tile_rows, int rank, int world);
/* Restrict rendering to the contiguous rows [row_begin, row_begin + row_count) (row_count -1 = to the
 * end); tiles of c5_set_row_tiles are then counted from row_begin.  A context only builds the
 * per-view records of cells its rows can reach, so contiguous blocks also shard the per-view
 * setup.  Default: the whole image. */
int c5_set_row_range(c5_context* ctx, int row_begin, int row_count);
int c5_local_rows(const c5_context* ctx, int* n_rows);
/* Segments per local row of the last frame rendered with option "row_costs" = 1 (the option may be off again since):
 * the cost estimate for balancing row blocks across GPUs. */
int c5_get_row_costs(c5_context* ctx, uint32_t* costs, int n_rows);
/* View transform of the volume grid (main.cpp:105-107) and of each solid (main.cpp:112-114,
 * object3d_roche_lobe.cpp:48). */
int c5_set_view(c5_context* ctx, const c5_rotation* rots, int n_rots);
int c5_set_solid_view(c5_context* ctx, int slot, const c5_rotation* rots, int n_rots);
/* app::config.limit_alpha_value (config.hpp:25, line.cpp:204,216-218); default 2.5. */
int c5_set_alpha_limit(c5_context* ctx, double alpha_limit);
/* Knobs:
 *   "integration"  0 (default): rays are walked from -z to +z and ch1 is integrated back to front
 *                  with the reference's own recurrence and rounding (line.cpp:206-225);
 *                  1: front to back from the viewer, I = sum T_k S_k, with the wavefront early-out
 *                  once the transmittance T falls below "transmittance_cutoff" (default 1e-12,
 *                  0 disables).  Both agree to rounding wherever the reference's recurrence is
 *                  well conditioned (it is not for DBL_EPSILON <= alpha < ~1e-8).
 *   "depth_split"  0 (default): a frame whose rays do not fill the GPU's wavefront slots - a small image, one GPU's rows of
 *                  a frame - and are long enough is rendered with every ray cut at K - 1 parallel planes of depth (K <= 4,
 *                  chosen from the statistics of the frame before, the planes tilted so that an oblique view's rays are cut
 *                  at equal fractions: fitted to where a sample of that frame's rays entered the grid and where they
 *                  ended): K jobs per 8x8 pixel tile walk the K parts at once and
 *                  the partial integrals are composed in depth order (tau = sum; I <- exp(-tauc_s) I + b_s: the recurrence
 *                  of line.cpp:206-225 is affine in I).  Same segment counts; I differs from the whole-ray walk in its
 *                  rounding ORDER only (~1e-16) - which is why a grid with a clamped alpha in [DBL_EPSILON, 1e-6), where
 *                  the reference's recurrence is dominated by its own cancellation error, is never cut.  1: never.
 *                  2..8: always that many slabs, with planes of constant depth that depend on the view alone (renders of
 *                  different rows of one frame are bit-equal only at the same slab count; "split_tilt_x" / "split_tilt_y",
 *                  testing: the planes' tilt, depth - tx x - ty y = const).  Default tile shape, "lds_stage" 2,
 *                  "integration" 0 and "xcd_mode" 2 only; whole rays otherwise.  DESIGN.md section 4.3.
 *   "algorithm"    0 (default for conforming grids): face-adjacency walk.  1: bin_sort_resolve, the
 *                  reference's own algorithm on the GPU (every face of every cell scan-converted onto
 *                  the pixels, per-pixel sort by z, integrate) — handles tet soups, overlapping and
 *                  non-conforming cells like the reference does; c5_upload_grid selects it by itself
 *                  when a face is shared by more than two cells.  Needs ~24 B per ray-cell segment
 *                  and synchronises inside c5_render_device.
 *   "lds_stage"    2 (default): walk_composite_lds with LDS-DMA staging — per step a wavefront loads each distinct
 *                  cell record once, straight into LDS (global_load_lds_dwordx4), and its rays read it from there;
 *                  1: the same staged through vector registers (global_load + ds_write_b128; also what 2 falls
 *                  back to beyond 2^24 cells); 0: every lane loads its own record.  Same results, bit for bit.
 *   "cost_order"   1 (default): frames with fewer rays than about two rounds of the GPU's wavefront slots (and more than ~1 500
 *                  wavefronts) start the rows of their image that hold the LONGEST rays first (by the last frame the caller
 *                  waited for) instead of top to bottom: a launch ends on whatever started last; 0: always top to bottom;
 *                  2: that order whatever the frame's size (experiments).  Same results.
 *   "cell_order"   1 (default; read by c5_upload_grid: set it BEFORE the upload): the library keeps the cells in Morton order of
 *                  their centroids, whatever order the caller has them in (grids of 4 096 cells and more that go to the
 *                  walk); c5_update_scalars still takes its arrays in the caller's order.  Same results, bit for bit.
 *   "block_cull"   1 (default): a context that renders a part of the image's rows judges every 256 consecutive cells by a
 *                  sphere about them before it builds their per-view records; 0: cell by cell only.  Same results.
 *   "tile_flags"   1 (default): the entry raster marks the 8x8 pixel tiles a boundary face's box meets, and a wavefront of the
 *                  walk looks at its tile's mark before anything else (default tile shape, no solids); 0: every wavefront
 *                  reads its pixels' entry heads.  Same results.
 *   "stage_slots"  "lds_stage" 1 / 2: distinct cells staged per wavefront and step (LDS-DMA passes of seven).  0 (default): 21
 *                  when the frame before had fewer than 120 ray-cell segments per cell (pixels coarse against the cells:
 *                  more distinct cells per 8x8 tile), else 14 (one more wavefront per SIMD); 14 / 21: fixed.  Same results
 *                  either way.
 *   "tile"         wavefront tile: 0 = 64x1 row tile, 1 = 16x4, 2 = 8x8 pixels, four wavefronts per workgroup; 3 (default):
 *                  8x8 pixels, one wavefront per workgroup (its slot is free again when ITS rays are done).
 *   "xcd_mode"     how workgroups map to the 8 XCDs (blocks b and b + 8 share an L2): 2 (default): square
 *                  super-blocks of workgroups dealt round-robin; 1: bands of image rows; 0: row-major tiles.
 *   "band_rows"    tuning: rows per super-block ("xcd_mode" 2, 0 = default 32) or band (1, default 16).
 *   "fuse_setup"   1: the per-cell records and the boundary entry lists are built by ONE launch of interleaved
 *                  workgroups; 0 (default): two launches.  Same results; measured slower fused.
 *   "solid_cache"  1 (default): a solid whose view and image are the same as in the frame before (the accretor sphere
 *                  never rotates, main.cpp:116; in a -D sweep only the lobe moves) is rastered once into a mask of its
 *                  own, which later frames lay over theirs; 0: every solid is transformed and rastered every frame.
 *                  Same masks either way.
 *   "solid_interior_faces"  0 (default): a face of a solid with a cell of non-zero volume on either side is not rastered: the
 *                  mask is the union over all faces (plane.cpp:130-131 -> line.cpp:246-249), and a ray through such a face
 *                  also meets a face with nothing behind it — the three fan faces of every cell of the reference's
 *                  centre-fan solids (object3d_base.cpp:152-193).  Only where get_pixel_by_x/_y's clamp (plane.cpp:194-212)
 *                  has no hand in the face's pixels: an interior face within a pixel of a border, or beyond it, is kept.
 *                  1 (testing): every unique face is rastered.  Same masks, bit for bit.
 *   "view_cache"   1 (default): a frame whose grid, scalars, image, rows, view, alpha limit and order are those of the TWO frames
 *                  before it reuses their per-view data — transformed vertices, cell records, boundary entry lists — instead
 *                  of building them again: the persistent device grid of a donor sweep (main.cpp:112-116: only the lobe
 *                  turns).  The second frame of such a run builds everything once more and tells its walk to leave the
 *                  per-pixel entry heads in place (the walk normally hands them back cleared); the third and later ones
 *                  skip the three setup launches (c5_stats: their ms_transform / ms_records / ms_entries are exactly 0).
 *                  Anything the data depend on makes them stale: c5_upload_grid, c5_update_scalars, c5_update_points, c5_set_image, the row
 *                  setters, c5_set_stream, any option but "row_costs" / "stage_timing" / "walk_timing", a grown entry pool.
 *                  A sweep whose view changes every frame never pays for it.  0: every frame builds its own.  Same results.
 *   "batch_width"  tuning: directions or upstream images one walk of c5_render_tangent_batch* / c5_render_adjoint_batch*
 *                  carries: 4 or 8; 0 (default): 4 for batches of up to 4, else 8.  Same results (the adjoint's to rounding).
 *                  c5_render_vertex_adjoint_batch* chunks its upstream images by it in the same way (96 x "batch_width" bytes
 *                  per cell and 24 x "batch_width" per point), its results the same to the atomics' rounding.
 *   "vertex_merge" tuning: 1 (default): c5_render_vertex_adjoint* sums the lanes of a wavefront that share a cell (in LDS)
 *                  before its atomics; 0: every lane adds its own six values (measured 10 x slower on the C3 frame).  Same
 *                  results, to the atomics' rounding.  c5_render_vertex_adjoint_batch* ignores it for more than one image:
 *                  it always merges.
 *   "adjoint_exact" 1: c5_render_adjoint, c5_render_adjoint_device and their batch forms return the exact adjoint sums
 *                  (the section below c5_render_adjoint_batch): bit-reproducible from run to run and additive over rows.
 *                  Default 0: fp64 atomics, every kernel, code path and bit as before.  The Gauss-Newton, Hessian-vector
 *                  and vertex adjoint calls ignore it (the vertex adjoint has "vertex_exact").  40 more bytes per cell,
 *                  allocated at the first exact call.
 *   "exact_sums"   1: c5_render_adjoint* as under "adjoint_exact" 1, and c5_render_gn_diagonal*, c5_render_gn_product* and
 *                  c5_render_hvp* return exact sums too (the section below c5_render_hvp): every operator of a fit of
 *                  (alpha, Q) bit-reproducible and additive over rows.  Default 0: as before.  The vertex adjoint ignores it
 *                  (its own option: "vertex_exact").
 *   "vertex_exact" 1: c5_render_vertex_adjoint, c5_render_vertex_adjoint_device and their batch forms return the exact
 *                  vertex adjoint sums (the section below c5_render_vertex_adjoint_batch): bit-reproducible from run to run,
 *                  whatever "cell_order" and the walk's options, and additive over rows.  0 (default): fp64 atomics, every
 *                  kernel, code path and bit as before.  Anything else: C5_ERR_INVALID.  "vertex_merge" is ignored under it.
 *                  336 more bytes per cell and 4 (n_pts + 1) + 16 n_cells bytes of incidence table, allocated at the first
 *                  exact vertex call.
 *   "overlap_setup" 1: entry lists and solid mask are built on a side stream while build_records
 *                  runs (only when "stage_timing" is 0).  Default 0: measured no faster.
 *   "pipeline"     1: two frame slots; the per-view setup of frame k + 1 runs on a second stream while
 *                  frame k is walked (set before c5_upload_grid / c5_set_image).  Default 0; measured
 *                  2 % faster on the C3 frame at the end of round 1 (a second set of per-view records).
 *   "entry_pool"   testing: size of the overflow pool of the per-pixel entry lists, in records (it holds
 *                  the second and further entries of a ray).  A frame is complete iff its total demand
 *                  (c5_stats.pool_entries) fits; the library keeps the pool at twice the demand of the
 *                  last frame it looked at and reports C5_RETRY for frames that did not fit.
 *   "lds_pad"      tuning: extra dynamic LDS per workgroup in bytes, to cap the resident wavefronts.
 *   "row_costs"    1: walk_composite also accumulates segments per image row (c5_get_row_costs).  May be switched per
 *                  frame: the costs of the last frame that counted them stay readable until the rows are laid out
 *                  anew (a sweep probes one frame in many).
 *   "entry_key"    1 (default): a boundary entry is keyed a slack behind its face, the same slack for every face of the
 *                  frame (+ more for faces steep against the rays), so that a ray leaving through a face that has no
 *                  partner with the same three points — hanging nodes: a coarse face against several fine ones — is
 *                  picked up by the abutting cell (the reference never looks at connectivity, object3d_base.cpp:37-42;
 *                  DESIGN.md section 5).  0 (testing): keyed at the face's own depth, as before round 3.
 *   "stage_timing" / "walk_timing"  record HIP events per stage (0 / 1; c5_stats::ms_* are those of the last frame rendered
 *                  with it on) / around walk_composite ("walk_timing" N: around every N-th launch, for c5_walk_kernel_ms).
 *                  Both default to 0: the six stage events cost 21-25 us of a 0.52-ms frame when frames follow one another
 *                  without a wait, the two around the walk 6. */
int c5_set_option(c5_context* ctx, const char* name, double value);

/* --- render ---------------------------------------------------------------------------------- */
/* find_intersections + trace_rays for the local rows.  out_host[local_rows][res_x][2].  Synchronous; retries
 * by itself on C5_RETRY.  A pinned out_host (c5_host_alloc) receives the image by one direct copy; a pageable
 * one through pinned staging chunks, copied out on the host threads while the next chunk is in flight. */
int c5_render(c5_context* ctx, float* out_host);
/* Same, asynchronous on the context's stream, into device memory (hipMalloc'ed by anyone in
 * this process).  Pair with c5_synchronize. */
int c5_render_device(c5_context* ctx, void* out_device);
int c5_synchronize(c5_context* ctx);

/* --- adjoint render ----------------------------------------------------------------------------
 * Gradients of the frame c5_render would produce NOW (same grid, scalars, solids, image, rows, view and alpha limit; no
 * render needs to come first) with respect to every cell's AbsorpCoef (alpha) and radEnLooseRate (Q), weighted by an
 * upstream image grad_out[local_rows][res_x][2] fp32 in the output's own layout (channel 0: the weight of tau, channel 1:
 * the weight of I):
 *     grad_alpha[c] = sum over the pixels p and the segments of cell c on p's ray of g_tau(p) dtau/dalpha_c + g_I(p) dI/dalpha_c
 *     grad_q[c]     = sum of g_I(p) dI/dQ_c
 * The derivative of the reference's integral as written (line.cpp:176-227): the alpha limit clamps (a clamped alpha has
 * dI/dalpha = 0; tau takes the raw alpha), a cell with clamped alpha < DBL_EPSILON neither absorbs nor emits (dI/d. = 0),
 * solid-marked pixels contribute nothing, whatever "integration", "depth_split", "lds_stage" or "tile" say.
 * grad_alpha / grad_q: n_cells fp64 each, in the caller's cell order (c5_upload_grid's), overwritten.
 * The sums are fp64 atomics added in arrival order: the results are NOT bit-reproducible from run to run (relative
 * differences of ~1e-15).  Option "adjoint_exact" 1 makes these two calls and the batch forms return the exact adjoint
 * sums instead (below: "exact adjoint sums"): the same bits every run, for any split of the rows.
 * Side effects: none on the options, the statistics or the images — a c5_render after an adjoint returns bit for bit
 * what it would have returned without it (the per-view data it reused are rebuilt: "view_cache").  The first call
 * allocates what the adjoint needs (8 bytes per local pixel, 16 per cell, the status words); a context that never
 * calls it uses no more memory than before.
 * c5_render_adjoint: synchronous, host arrays; retries by itself on C5_RETRY, like c5_render.
 * c5_render_adjoint_device: asynchronous on the context's stream, device arrays; its status (C5_RETRY included: run it
 * again) is reported by the next call that waits for the stream, like c5_render_device's. */
int c5_render_adjoint(c5_context* ctx, const float* grad_out_host, double* grad_alpha_host, double* grad_q_host);
int c5_render_adjoint_device(c5_context* ctx, const void* grad_out_device, void* grad_alpha_device, void* grad_q_device);

/* --- tangent render ----------------------------------------------------------------------------
 * The forward-mode twin of the adjoint: the change of the same frame (the one c5_render would produce NOW; no render needs
 * to come first) for a change (d_alpha, d_q) of the cells' AbsorpCoef and radEnLooseRate, i.e. J v where the adjoint
 * gives J^T g:
 *     out[p] = (sum over the cells c on p's ray of dtau/dalpha_c d_alpha[c],  sum of dI/dalpha_c d_alpha[c] + dI/dQ_c d_q[c])
 * with the adjoint's conventions: the alpha limit clamps (a clamped alpha does not move I), a cell with clamped alpha <
 * DBL_EPSILON neither absorbs nor emits, solid-marked and uncovered pixels are 0 in both channels, whole rays in the
 * reference's order whatever "integration", "depth_split", "lds_stage" or "tile" say.
 * d_alpha / d_q: n_cells fp64 each in the caller's cell order (c5_upload_grid's); either may be NULL (a zero direction).
 * out: [local_rows][res_x][2] fp32, the output's own layout (row range and row tiles as for a frame).
 * One walk per ray, no atomics: the result IS bit-reproducible from run to run, and <g, J v> = <J^T g, v> holds with
 * c5_render_adjoint to rounding.
 * Side effects: as the adjoint's (it shares the adjoint's counters and status words, never a frame's); the first call
 * allocates 16 bytes per cell (c5_render_tangent: 16 more, and one image); a context that never calls it uses no more
 * memory than before.
 * c5_render_tangent: synchronous, host arrays; retries by itself on C5_RETRY, like c5_render.
 * c5_render_tangent_device: asynchronous on the context's stream, device arrays; its status (C5_RETRY included: run it
 * again) is reported by the next call that waits for the stream.  Both refuse while c5_render_host_async frames are
 * outstanding. */
int c5_render_tangent(c5_context* ctx, const double* d_alpha_host, const double* d_q_host, float* out_host);
int c5_render_tangent_device(c5_context* ctx, const void* d_alpha_dev, const void* d_q_dev, void* out_device);

/* --- batched derivative renders -----------------------------------------------------------------
 * n tangents or n adjoints of the same frame in one call: what a Jacobian against a few parameters, several losses at
 * once or a block of Gauss-Newton / CG directions asks for.  The per-view setup is built once and every ray is walked
 * once for up to "batch_width" directions or upstream images at a time; the adjoint's first pass (the ray's optical
 * depths) runs once for all n.
 * c5_render_tangent_batch: d_alpha / d_q [n_dirs][n_cells] fp64 in the caller's cell order, either may be NULL (zero);
 * out [n_dirs][local_rows][res_x][2] fp32.  Every slice is bit for bit what c5_render_tangent returns for that direction
 * alone, whatever the batch size or "batch_width" (on "algorithm" 1, a pixel whose list holds segments of equal depth
 * takes them in the order the lists were filled in, which may change from call to call: for the single call too).
 * c5_render_adjoint_batch: grad_out [n_imgs][local_rows][res_x][2] fp32; grad_alpha / grad_q [n_imgs][n_cells] fp64 in
 * the caller's order, overwritten.  Every slice is c5_render_adjoint's for that image alone to rounding: fp64 atomics
 * added in arrival order, NOT bit-reproducible from run to run (as the single adjoint).
 * n < 1 or a null output: C5_ERR_INVALID.  Side effects, status and retries: as the single calls' (their counters and
 * status words, never a frame's; a c5_render after them returns what it would have without them); the first call
 * allocates 16 x "batch_width" bytes per cell (the adjoint twice that); the synchronous forms, room for the caller's
 * arrays besides.  The _device forms are asynchronous on the context's stream with device arrays; their status
 * (C5_RETRY included: run them again) is reported by the next call that waits for the stream.  All four refuse while
 * c5_render_host_async frames are outstanding. */
int c5_render_tangent_batch(c5_context* ctx, int n_dirs, const double* d_alpha_host, const double* d_q_host, float* out_host);
int c5_render_tangent_batch_device(c5_context* ctx, int n_dirs, const void* d_alpha_dev, const void* d_q_dev, void* out_dev);
int c5_render_adjoint_batch(c5_context* ctx, int n_imgs, const float* grad_out_host, double* grad_alpha_host, double* grad_q_host);
int c5_render_adjoint_batch_device(c5_context* ctx, int n_imgs, const void* grad_out_dev, void* grad_alpha_dev, void* grad_q_dev);

/* --- exact adjoint sums --------------------------------------------------------------------------
 * The adjoint's per-cell sums in integers.  Float adds do not commute, integer adds do: every contribution (one per
 * segment of a cell on a ray: the terms of c5_render_adjoint, computed as there) is rounded ONCE onto a fixed-point grid
 * of its cell, and everything after that - the sum inside a wavefront, the atomic in memory, the combination of ranks -
 * is a 64-bit integer add.  The grid of a cell follows from the largest exponent among its contributions, itself an
 * order-free reduction (an integer max).  The format, for an image of res_x x res_y pixels - the WHOLE image of
 * c5_set_image, not a rank's rows - and per cell for each of the two sums (grad_alpha, grad_q):
 *     h = ceil(log2(res_x res_y)) + 1     headroom: a ray crosses a cell at most once, so a cell has at most res_x res_y contributions
 *     m = 62 - h                          bits per word (images beyond 2^39 pixels are refused)
 *     e (int32)   the largest ilogb(|x|) over the cell's non-zero finite contributions x; INT32_MIN: no contribution;
 *                 INT32_MAX: some contribution was not finite, and the result is NaN
 *     for |x| < 2^(e+1):  y = x 2^(m-e-1),  k1 = rint(y),  k0 = rint((y - k1) 2^m)   (ties to even; nothing else rounds)
 *     words  s1 = sum k1,  s0 = sum k0   (int64; |s1| <= 2^61, |s0| <= 2^60: they cannot overflow)
 *     value  (s1 2^m + s0) 2^(e+1-2m), rounded once to fp64 with ties to even, subnormals included; INT32_MIN gives +0.0
 * Each contribution is off by at most 2^(e-2m); for 2400 x 1800 pixels (h = 24, m = 38) the whole sum of a cell is within
 * 2^(e-53) of the exact sum of its fp64 contributions, before the one final rounding.
 *
 * With option "adjoint_exact" 1, c5_render_adjoint, c5_render_adjoint_device, c5_render_adjoint_batch and
 * c5_render_adjoint_batch_device return these sums, finished to fp64, through four passes inside the one call: the
 * adjoint's pass 1, pass E (the exponents), pass S (the words) and the finish.  The batch forms then run that single
 * path image after image (the host loop that "algorithm" 1 uses for its batches; pass 1 runs once).  Results are
 * bit-reproducible from run to run, whatever "cell_order", the walk's options or the rows' split.  On "algorithm" 1 that
 * is promised only as far as the tangent's is: a pixel whose list holds segments of equal depth takes them in an order that
 * may change from call to call.  c5_render_gn_*, c5_render_hvp* and c5_render_vertex_adjoint* ignore the option
 * (the first two have "exact_sums").
 * Memory: 40 more bytes per cell, allocated at the first exact call.
 *
 * For callers who split an image (row ranges, row tiles, several GPUs), the two intermediate results:
 * c5_render_adjoint_exact_bounds: pass 1 and pass E over the context's rows; exp_alpha / exp_q: int32 [n_cells] in the
 * caller's cell order, overwritten.
 * c5_render_adjoint_exact_sums: pass 1 and pass S against the GIVEN exponents (int32 [n_cells] each); sums_alpha / sums_q:
 * int64 [n_cells][2] = (s1, s0) in the caller's order, overwritten.  A contribution with |x| >= 2^(e+1) - the exponent
 * given is too small - is never wrapped: it is added nowhere and counted, and the call (its _device form: the next call
 * that waits for the stream) reports C5_ERR_INVALID with a c5_last_error text.  Cells marked INT32_MAX take nothing.
 * c5_exact_sums_finish: a pure host function (no context, no GPU): out_fp64[i] = the value of (exp[i], sums[i][0],
 * sums[i][1]) for i < n with the m of a res_x x res_y image.
 * The contract: take the exponents of any set of row ranges (or row tiles) combined by elementwise max, and the words -
 * every part's computed against those combined exponents - combined by elementwise integer add; finished, they are bit
 * for bit what one call over the union of the rows gives.  The "adjoint_exact" single call is exactly that composition.
 * Status, retries, side effects: as c5_render_adjoint's; the _device forms are asynchronous on the context's stream with
 * device arrays, and all four refuse while c5_render_host_async frames are outstanding. */
int c5_render_adjoint_exact_bounds(c5_context* ctx, const float* grad_out_host, int32_t* exp_alpha_host, int32_t* exp_q_host);
int c5_render_adjoint_exact_bounds_device(c5_context* ctx, const void* grad_out_device, void* exp_alpha_device, void* exp_q_device);
int c5_render_adjoint_exact_sums(c5_context* ctx, const float* grad_out_host, const int32_t* exp_alpha_host, const int32_t* exp_q_host,
                                 int64_t* sums_alpha_host, int64_t* sums_q_host);
int c5_render_adjoint_exact_sums_device(c5_context* ctx, const void* grad_out_device, const void* exp_alpha_device,
                                        const void* exp_q_device, void* sums_alpha_device, void* sums_q_device);
int c5_exact_sums_finish(const int32_t* exp, const int64_t* sums, int64_t n, int res_x, int res_y, double* out_fp64);
/* Testing: (k1, k0) of every x[i], i < n, against the exponent `exp` with the m of a res_x x res_y image, into
 * words[n][2]; C5_ERR_INVALID if some x does not fit (|x| >= 2^(exp+1) or not finite).  No context, no GPU. */
int c5_exact_quantise(const double* x, int64_t n, int32_t exp, int res_x, int res_y, int64_t* words);

/* --- Gauss-Newton renders ---------------------------------------------------------------------------
 * With J the Jacobian of the frame c5_render would produce now with respect to the cells' (alpha, Q) - the map of
 * c5_render_tangent, its transpose the map of c5_render_adjoint - and W a diagonal matrix of per-pixel, per-channel
 * weights:
 * c5_render_gn_product: H v = J^T W J v for n_dirs directions v = (d_alpha, d_q), the normal-equation product of a
 * Gauss-Newton / CG fit of the cell field to observed images.  d_alpha / d_q [n_dirs][n_cells] fp64 in the caller's cell
 * order, either may be NULL (a zero direction; the matching output block is still written: the off-diagonal block's
 * action).  weight [local_rows][res_x][2] fp32 (channel 0 weighs tau, 1 weighs I), NULL = all ones; one weight image for
 * all directions.  h_alpha / h_q [n_dirs][n_cells] fp64, overwritten; either may be NULL when only the other field is
 * fitted, not both.  jv_out [n_dirs][local_rows][res_x][2] fp32 or NULL: J v, bit for bit c5_render_tangent_batch's image.
 * It is ONE call for what otherwise takes c5_render_tangent_batch, a multiply and c5_render_adjoint_batch: one per-view
 * setup, and the tangent walk leaves the adjoint's first pass behind.  The intermediate image is fp32 on purpose: the
 * result is that of c5_render_adjoint_batch on grad_out = weight * (fp32 image of c5_render_tangent_batch), one fp32
 * multiply per channel, up to the order of the adjoint's atomics.  So H is symmetric positive semidefinite for weights
 * >= 0 up to that fp32 rounding (6e-8 relative per pixel), and the results are NOT bit-reproducible from run to run, as
 * the adjoint's.
 * c5_render_gn_diagonal: diag(J^T W J), split as diag_alpha / diag_q [n_cells] fp64 in the caller's order, overwritten:
 * the Jacobi preconditioner of that CG, the scaling of Levenberg-Marquardt, and a measure of how strongly the frame
 * constrains each cell (0: no walked ray crosses it).  A ray crosses a cell in at most one segment, so it is the per-cell
 * sum of weight * (the adjoint's per-segment term)^2, in fp64 throughout; not bit-reproducible either.
 * n_dirs < 1 or no output: C5_ERR_INVALID.  Row ranges and row tiles, side effects, status and retries: as the batch
 * calls' (the adjoint's counters and status words, never a frame's; a c5_render afterwards returns the bits it would
 * have returned without them; the synchronous forms retry by themselves on C5_RETRY, the _device forms are asynchronous
 * on the context's stream and report through the next call that waits for it).  Memory is allocated at the first call
 * only: the batch calls' buffers, "batch_width" images, and for a NULL h_alpha or h_q 8 x "batch_width" bytes per cell.
 * All four refuse while c5_render_host_async frames are outstanding. */
int c5_render_gn_product(c5_context* ctx, int n_dirs, const double* d_alpha_host, const double* d_q_host,
                         const float* weight_host, double* h_alpha_host, double* h_q_host, float* jv_out_host);
int c5_render_gn_product_device(c5_context* ctx, int n_dirs, const void* d_alpha_dev, const void* d_q_dev,
                                const void* weight_dev, void* h_alpha_dev, void* h_q_dev, void* jv_out_dev);
int c5_render_gn_diagonal(c5_context* ctx, const float* weight_host, double* diag_alpha_host, double* diag_q_host);
int c5_render_gn_diagonal_device(c5_context* ctx, const void* weight_dev, void* diag_alpha_dev, void* diag_q_dev);

/* --- Hessian-vector render ---------------------------------------------------------------------------
 * The exact second derivative of the frame c5_render would produce now in the cells' (alpha, Q), applied to one
 * direction: with phi = sum over the pixels of g_tau tau + g_I I for an upstream image grad_out = (g_tau, g_I),
 *     (h_alpha, h_q) = Hess(phi) (d_alpha, d_q),
 * the residual-weighted curvature sum_p g_p Hess(I_p) v that the Gauss-Newton product leaves out: c5_render_gn_product
 * (weight W) plus this call on grad_out = W r is the exact Hessian product of 1/2 sum w r^2, r the residual image.
 * tau is linear in alpha: channel 0 of grad_out is read and has no effect, and a pixel with g_I == 0 is not walked.
 * With the adjoint's numbering and conventions (segments k = 1..n, deepest first; a_k = min(alpha_k, limit); E_k =
 * exp(-a_k dz_k); T_k the transmittance to the viewer; Lambda_k = sum_{j <= k} a_j dz_j), lambda_k = g_I T_k,
 *     S_k    = (1 - E_k) / a_k,   S_a = dz E / a - (1 - E) / a^2,   S_aa = 2 (1 - E) / a^3 - 2 dz E / a^2 - dz^2 E / a
 * (S_a and S_aa by their series below a dz = 1/8), G_k = Q_k S_a,k - dz_k E_k I_{k-1}, and for the direction
 *     a_dot_k = d_alpha[cell_k] where the cell is active and its alpha not clamped, else 0 (a clamped alpha does not
 *               move: no row and no column, as in c5_render_adjoint);   Q_dot_k = d_q[cell_k];
 *     I_dot_k = E_k I_dot_{k-1} - dz_k E_k a_dot_k I_{k-1} + Q_dot_k S_k + Q_k S_a,k a_dot_k     (c5_render_tangent's I_dot)
 *     Lambda_dot_k = sum_{j <= k} a_dot_j dz_j,   lambda_dot_k = -lambda_k (Lambda_dot_n - Lambda_dot_k)
 * every segment adds to its cell
 *     h_q     += lambda_dot_k S_k + lambda_k S_a,k a_dot_k
 *     h_alpha += lambda_dot_k G_k + lambda_k (Q_dot_k S_a,k + Q_k S_aa,k a_dot_k + dz_k^2 E_k a_dot_k I_{k-1} - dz_k E_k I_dot_{k-1})
 * (h_alpha only where alpha is not clamped).  Inactive cells and solid-marked pixels add nothing.  The operator is
 * symmetric, in general indefinite, and its Q-Q block is zero (I is linear in Q).
 * d_alpha / d_q [n_cells] fp64 in the caller's cell order; either may be NULL (zero), both NULL is C5_ERR_INVALID.
 * grad_out [local_rows][res_x][2] fp32, required.  h_alpha / h_q [n_cells] fp64 in the caller's order, overwritten;
 * either may be NULL, not both.  The sums are fp64 atomics in arrival order: NOT bit-reproducible from run to run (the
 * last bits move), as the adjoint's.  Row ranges and row tiles, side effects, status and retries as the adjoint's (its
 * counters and status words, never a frame's; a c5_render afterwards returns the bits it would have returned without
 * the call): c5_render_hvp is synchronous and retries by itself on C5_RETRY; the _device form is asynchronous on the
 * context's stream with device arrays and reports through the next call that waits for it.  Memory is allocated at the
 * first call only: the adjoint's and the tangent's buffers and 8 bytes more per local pixel.  Both refuse while
 * c5_render_host_async frames are outstanding. */
int c5_render_hvp(c5_context* ctx, const double* d_alpha_host, const double* d_q_host, const float* grad_out_host,
                  double* h_alpha_host, double* h_q_host);
int c5_render_hvp_device(c5_context* ctx, const void* d_alpha_dev, const void* d_q_dev, const void* grad_out_dev,
                         void* h_alpha_dev, void* h_q_dev);

/* --- exact sums for the Gauss-Newton and Hessian-vector renders --------------------------------------
 * Option "exact_sums" 1 gives every per-cell sum a fit of (alpha, Q) runs on the number format of "exact adjoint sums"
 * above - the same h, m, exponents, words and finish; in all three operators below a ray adds to a cell at most once,
 * each segment to its own cell, so the headroom argument carries over as it is:
 *   c5_render_adjoint* and its batch    behave as under "adjoint_exact" 1.
 *   c5_render_gn_diagonal*              pass 1, pass E on the SQUARED terms w (term)^2 as c5_render_gn_diagonal forms them
 *                                       (the exponents of the unsquared adjoint say nothing about them), pass S, the finish.
 *   c5_render_hvp*                      pass 1 (Lambda and Lambda_dot per pixel) once, then pass E, pass S and the finish
 *                                       on the per-segment (h_alpha, h_q) terms of c5_render_hvp.
 *   c5_render_gn_product*               per chunk of "batch_width" directions the tangent walk as it is (J v, g = weight *
 *                                       fp32(J v) with one fp32 multiply per channel, and Lambda); then every direction's g
 *                                       goes through pass E, pass S and the finish, one direction after the other.  The
 *                                       result is DEFINED as, and is bit for bit, what c5_render_adjoint under
 *                                       "adjoint_exact" 1 returns for grad_out = weight * (fp32 image of
 *                                       c5_render_tangent_batch); jv_out keeps its bits; every slice of a batch is the
 *                                       single call's, whatever "batch_width".
 * All results are finished to fp64 inside the one call and are bit-reproducible from run to run, whatever "cell_order",
 * the walk's options or the rows' split (on "algorithm" 1 as far as the tangent's is: lists with segments of equal depth).
 * Where a NULL output or direction is legal without the option it stays legal.  "adjoint_exact" keeps its meaning: the
 * adjoint only.  c5_render_vertex_adjoint* ignores both options (its per-point finish is another reduction; its own
 * option is "vertex_exact", the section below c5_render_vertex_adjoint_batch).  Default 0:
 * fp64 atomics, every kernel, code path and bit as before.  Memory: the exact adjoint's 40 bytes per cell, the same buffer.
 *
 * For callers who split an image, the two intermediate results of every kind of sum, one generic pair:
 *   what = C5_EXACT_ADJOINT      image: the upstream image grad_out, required.  d_alpha / d_q: must be NULL.  Exactly
 *                                c5_render_adjoint_exact_bounds / _sums, which are this kind by another name.
 *   what = C5_EXACT_GN_DIAGONAL  image: the weight image, NULL = all ones.  d_alpha / d_q: must be NULL.
 *   what = C5_EXACT_HVP          image: the upstream image grad_out, required.  d_alpha / d_q [n_cells] fp64 in the
 *                                caller's order: either may be NULL (zero), not both.
 * A direction given to another kind than C5_EXACT_HVP, a missing image, or an unknown `what`: C5_ERR_INVALID.
 * c5_render_exact_bounds: pass 1 and pass E over the context's rows; exp_alpha / exp_q int32 [n_cells] in the caller's
 * order, overwritten.  c5_render_exact_sums: pass 1 and pass S against the GIVEN exponents; sums_alpha / sums_q int64
 * [n_cells][2] = (s1, s0), overwritten.  The contract is the exact adjoint's: exponents over any row ranges or row tiles
 * combine by elementwise max, the words - every part's computed against the combined exponents - by elementwise integer
 * add, and c5_exact_sums_finish then gives bit for bit what the single "exact_sums" call over the union of the rows
 * gives.  The split Gauss-Newton product needs no kind of its own: it is a tangent render on the part's rows, the fp32
 * multiply by the part's weights, then C5_EXACT_ADJOINT on that image.
 * The mechanisms are the exact adjoint's too: a contribution beyond its cell's exponent is counted and reported, never
 * wrapped (C5_ERR_INVALID with a c5_last_error text; the _device forms: by the next call that waits for the stream);
 * INT32_MAX marks a non-finite contribution and finishes to NaN; the host forms retry by themselves on C5_RETRY; status
 * and counters are the adjoint's own, never a frame's; the _device forms are asynchronous on the context's stream with
 * device arrays; all four refuse while c5_render_host_async frames are outstanding. */
enum { C5_EXACT_ADJOINT = 0, C5_EXACT_GN_DIAGONAL = 1, C5_EXACT_HVP = 2 };
int c5_render_exact_bounds(c5_context* ctx, int what, const double* d_alpha_host, const double* d_q_host, const float* image_host,
                           int32_t* exp_alpha_host, int32_t* exp_q_host);
int c5_render_exact_bounds_device(c5_context* ctx, int what, const void* d_alpha_dev, const void* d_q_dev, const void* image_dev,
                                  void* exp_alpha_dev, void* exp_q_dev);
int c5_render_exact_sums(c5_context* ctx, int what, const double* d_alpha_host, const double* d_q_host, const float* image_host,
                         const int32_t* exp_alpha_host, const int32_t* exp_q_host, int64_t* sums_alpha_host, int64_t* sums_q_host);
int c5_render_exact_sums_device(c5_context* ctx, int what, const void* d_alpha_dev, const void* d_q_dev, const void* image_dev,
                                const void* exp_alpha_dev, const void* exp_q_dev, void* sums_alpha_dev, void* sums_q_dev);

/* --- motion tangent render ---------------------------------------------------------------------------
 * The frame c5_render would produce NOW differentiated with respect to the GEOMETRY, the cells' scalars held: the grid
 * moves in view space with an affine velocity field u(p) = A p + b, and out is the change of every pixel per unit of that
 * motion.  A change of a view angle is one such field (c5_rotation_motion), so is a shift or a stretch of the grid.
 * The rays are parallel to z and a face is a plane w = c + gx x + gy y: its depth at the pixel (x, y) changes by
 *     dw = u_z(P) - gx u_x(P) - gy u_y(P),   P = (x, y, w) the point the ray hits,
 * a segment's chord by ddz_k = dw_exit,k - dw_entry,k, and with the adjoint's numbering and conventions
 *     tau_dot = sum_k alpha_k ddz_k                                   (raw alpha, every segment)
 *     I_dot_k = E_k I_dot_{k-1} + E_k (Q_k - a_k I_{k-1}) ddz_k       (active segments)
 * A clamped alpha still moves with its chord (the clamp is on alpha); a cell with clamped alpha < DBL_EPSILON adds nothing
 * to I_dot; solid-marked and uncovered pixels are 0 in both channels (a solid's own motion is not differentiated); whole
 * rays in the reference's order whatever "integration", "depth_split", "lds_stage" or "tile" say.
 * Pixels that GAIN OR LOSE coverage under the motion - silhouettes, a ray that crosses an edge into another list of
 * cells - are not differentiated: the result is the derivative of the smooth piece the pixel is on (the image is
 * piecewise smooth in the pose; the jumps are of the size of one chord).
 * fields: [n_dirs][12] fp64 in HOST memory in both forms (they travel as kernel arguments): A row-major, then b, in view
 * space (x, y the image's axes, z towards the viewer's depth).  out: [n_dirs][local_rows][res_x][2] fp32, the output's own
 * layout (row range and row tiles as for a frame).  More than "batch_width" fields run as chunks over one per-view setup;
 * every slice is bit for bit what the call returns for that field alone.  One walk per ray, no atomics: bit-reproducible.
 * Status, retries, side effects and the refusal while c5_render_host_async frames are outstanding: as
 * c5_render_tangent_batch's (the adjoint's counters and status words, never a frame's; a c5_render afterwards returns the
 * bits it would have returned without it).  c5_render_motion_tangent is synchronous into host memory and retries by
 * itself; the _device form is asynchronous on the context's stream into device memory.
 * c5_rotation_motion: host only, no context, no GPU.  field[12] = the view-space velocity field of d / d(rots[index].angle)
 * (what 0) or d / d(rots[index].x0) (what 1; zero for axis 0) of the view c5_set_view(rots, n_rots) sets. */
int c5_render_motion_tangent(c5_context* ctx, int n_dirs, const double* fields_host, float* out_host);
int c5_render_motion_tangent_device(c5_context* ctx, int n_dirs, const double* fields_host, void* out_dev);
int c5_rotation_motion(const c5_rotation* rots, int n_rots, int index, int what, double field[12]);

/* --- vertex adjoint render ---------------------------------------------------------------------------
 * The reverse mode of the motion tangent: the gradient of the frame c5_render would produce NOW with respect to the
 * coordinates of every grid point, the cells' scalars held, weighted by an upstream image grad_out[local_rows][res_x][2]
 * fp32 (channel 0: the weight of tau, 1: of I) as for c5_render_adjoint.  One adjoint-style pass for all points, where
 * finite differences take 3 n_pts renders.
 * With the adjoint's numbering, segment k of pixel p has d loss / d dz_k =
 *     G_k = g_tau alpha_k + g_I T_k E_k (Q_k - a_k I_{k-1})           (raw alpha; the second term for active segments)
 * (the clamp is on alpha, not on the chord).  The chord is dz_k = w_exit - w_entry, and a face with view-space vertices
 * P_0, P_1, P_2 has the depth w = sum_i lambda_i z_i at the pixel, lambda the barycentric coordinates of (x, y) in the
 * projected triangle: dw / d(x_i, y_i, z_i) = lambda_i (-gx, -gy, 1) with the face's slopes (gx, gy) - the motion
 * tangent's dw = u_z - gx u_x - gy u_y for u(P) = sum lambda_i u_i.  So in view space
 *     grad_view[v] = sum over pixels, segments and the segment's two faces holding v of
 *                    (+G_k lambda_v at the exit face, -G_k lambda_v at the entry face) (-gx, -gy, 1)
 * and the result is given in the coordinates c5_upload_grid took: grad_xyz[v] = M^T grad_view[v], M the linear part of
 * the view (the rotations are rigid; their centres drop out).  For any affine field, sum_v grad_view[v] . (A p_v + b) =
 * <grad_out, c5_render_motion_tangent's image> up to that image's fp32 rounding.
 * Conventions: the other derivative renders'.  Solid-marked and uncovered pixels contribute nothing; a cell with clamped
 * alpha < DBL_EPSILON contributes through tau only; faces edge-on to the rays contribute nothing; whole rays in the
 * reference's order whatever "integration", "depth_split", "lds_stage" or "tile" say; pixels that gain or lose coverage
 * when a point moves are not differentiated (the derivative of the smooth piece the pixel is on).
 * WELDED POINTS: a point c5_upload_grid welded to another (c5_weld_points: rep[i] != i) receives 0; its representative
 * receives the sum of the group.
 * grad_xyz: [n_pts][3] fp64 in the caller's point order, overwritten.  Row ranges and row tiles as for a frame (the
 * gradients of the parts sum to the whole frame's).  fp64 atomics added in arrival order: NOT bit-reproducible from run
 * to run, as the adjoint - unless option "vertex_exact" is 1 (exact vertex adjoint sums, below).
 * Status, retries, side effects: as c5_render_adjoint's (the adjoint's counters and status words, never a frame's; a
 * c5_render afterwards returns the bits it would have returned without it).  The first call allocates the adjoint's 8
 * bytes per local pixel, 96 bytes per cell and 24 per point; a context that never calls it uses no more memory than
 * before.  c5_render_vertex_adjoint is synchronous with host arrays and retries by itself on C5_RETRY; the _device form
 * is asynchronous on the context's stream with device arrays, its status (C5_RETRY included: run it again) reported by the
 * next call that waits for the stream.  A null pointer: C5_ERR_INVALID.  Both refuse while c5_render_host_async frames
 * are outstanding (C5_ERR_STATE). */
int c5_render_vertex_adjoint(c5_context* ctx, const float* grad_out_host, double* grad_xyz_host);
int c5_render_vertex_adjoint_device(c5_context* ctx, const void* grad_out_dev, void* grad_xyz_dev);

/* The batch: n_imgs upstream images grad_out[n_imgs][local_rows][res_x][2] fp32 -> grad_xyz[n_imgs][n_pts][3] fp64 in the
 * caller's point order, overwritten.  Every ray is walked once for up to "batch_width" images at a time, and the adjoint's
 * first pass (Lambda: it does not depend on the weights) runs once for all of them: of a segment only g_tau and g_I
 * differ from image to image.  Every slice is c5_render_vertex_adjoint's for that image alone up to the order of the fp64
 * additions - each contribution is the same product of the same two doubles - and like it NOT bit-reproducible from run
 * to run.  An image of zeros gives a slice of exact zeros, and welded non-representatives receive exact zeros in every
 * slice.  n_imgs == 1 is the single call.  On "algorithm" 1, and after a C5_RETRY onto its lists, the images run one
 * after the other over one per-view setup.  "vertex_merge" is ignored for n_imgs > 1 (the batch always merges), as are
 * "adjoint_exact" and "exact_sums".  Under "vertex_exact" 1 the first pass runs once and every image then goes through the
 * single exact path, one after the other: every slice is bit for bit the single exact call's, whatever "batch_width".
 * Status, counters, retries and side effects: the single call's.  The first batched call allocates 96 x "batch_width"
 * bytes per cell and 24 x "batch_width" per point beside the single call's buffers; a context that never calls it uses
 * no more memory than before.  c5_render_vertex_adjoint_batch is synchronous with host arrays and retries by itself on
 * C5_RETRY; the _device form is asynchronous on the context's stream with device arrays.  n_imgs < 1 or a null pointer:
 * C5_ERR_INVALID.  Both refuse while c5_render_host_async frames are outstanding (C5_ERR_STATE). */
int c5_render_vertex_adjoint_batch(c5_context* ctx, int n_imgs, const float* grad_out_host, double* grad_xyz_host);
int c5_render_vertex_adjoint_batch_device(c5_context* ctx, int n_imgs, const void* grad_out_dev, void* grad_xyz_dev);

/* --- exact vertex adjoint sums -------------------------------------------------------------------------
 * Option "vertex_exact" 1 makes c5_render_vertex_adjoint* and its batch return grad_xyz DEFINED by four steps, none of
 * which depends on an order of arrival:
 *   1. Per cell and slot, an exact sum.  A segment adds six doubles, the ones the atomic mode adds: +G_k lambda to the
 *      three slots of its exit face, -G_k lambda to those of its entry face, one rounding each.  The slots are a cell's
 *      [4 faces][3 vertices of the face] (faces 0:(0,1,2) 1:(0,1,3) 2:(0,2,3) 3:(1,2,3) of the cell's four points).  They
 *      are summed per (cell, slot) in the number format of "exact adjoint sums" above: exponent e = the largest ilogb over
 *      the slot's contributions (INT32_MIN: none, INT32_MAX: one that is not finite), two int64 words (s1, s0), h and m of
 *      the WHOLE image.  A ray crosses a cell at most once and its two faces differ, so a slot receives at most one
 *      contribution per ray and the headroom argument carries over.  face_w[cell][slot] = the words finished: one rounding.
 *   2. Per cell, fixed arithmetic.  For each of the cell's four vertices the triple (sum -gx_f w, sum -gy_f w, sum w) over
 *      the faces f holding the vertex, in ascending f, (gx, gy) the face's slopes; edge-on faces and zero weights are
 *      skipped; every product and every sum is rounded by itself (no contraction).
 *   3. Per point, a gather in a fixed order: grad_view[point] = the sum of the triples of its (cell, vertex) incidences in
 *      ascending order of the CALLER's cell index (not the device's: the result does not depend on "cell_order"), from
 *      +0.0.  Points welded to another have no incidences and receive exact +0.0, as does every point of an all-zero sum.
 *   4. grad_xyz[point] = M^T grad_view[point], as in the atomic mode.
 * Bit-reproducible from run to run, whatever "cell_order", "vertex_merge", "batch_width" and the walk's options (on
 * "algorithm" 1, and after a C5_RETRY onto its lists, as far as the list order is: segments of equal depth).  Against
 * the atomic mode it is one more valid order of the same terms.  "adjoint_exact" and "exact_sums" have no say here.
 *
 * For callers who split an image, the intermediate results:
 *   c5_render_vertex_exact_bounds  the adjoint's first pass and pass E over the context's rows.  exps: int32 [n_cells][12]
 *                                  in the caller's cell order, overwritten.
 *   c5_render_vertex_exact_sums    the first pass and pass S against the GIVEN exponents.  sums: int64 [n_cells][12][2] =
 *                                  (s1, s0) per slot, the word order of c5_render_exact_sums, overwritten.
 *   c5_vertex_exact_finish         steps 1 (the finish of the words) to 4 for the given exponents and words into grad_xyz
 *                                  [n_pts][3] fp64.  It needs the context - the faces' slopes in the current view, the
 *                                  grid's incidences, the view - and runs a per-view setup of its own; no ray is walked.
 * SPLIT CONTRACT.  Exponents over any row ranges or row tiles combine by elementwise max; the words - every part's taken
 * against the combined exponents - by elementwise integer add; c5_vertex_exact_finish on ANY ONE of the contexts (same
 * grid, points and view) then gives bit for bit what the single "vertex_exact" call over the union of the rows gives.
 * The mechanisms are the exact adjoint's: a contribution beyond its slot's exponent is added nowhere, counted and reported
 * (C5_ERR_INVALID with a c5_last_error text; the _device forms: by the next call that waits for the stream); the host forms
 * are synchronous and retry by themselves on C5_RETRY; the _device forms are asynchronous on the context's stream with
 * device arrays; status and counters are the adjoint's own, never a frame's, and a c5_render afterwards returns the bits
 * it would have returned without them; a null pointer: C5_ERR_INVALID; all six refuse while c5_render_host_async frames
 * are outstanding (C5_ERR_STATE).  A scene without cells: nothing is written to exps / sums (they are empty), grad_xyz is
 * zeros.  The incidence table is built by the host at the first exact vertex call after c5_upload_grid and kept across
 * c5_update_points. */
int c5_render_vertex_exact_bounds(c5_context* ctx, const float* grad_out_host, int32_t* exps_host);
int c5_render_vertex_exact_bounds_device(c5_context* ctx, const void* grad_out_dev, void* exps_dev);
int c5_render_vertex_exact_sums(c5_context* ctx, const float* grad_out_host, const int32_t* exps_host, int64_t* sums_host);
int c5_render_vertex_exact_sums_device(c5_context* ctx, const void* grad_out_dev, const void* exps_dev, void* sums_dev);
int c5_vertex_exact_finish(c5_context* ctx, const int32_t* exps_host, const int64_t* sums_host, double* grad_xyz_host);
int c5_vertex_exact_finish_device(c5_context* ctx, const void* exps_dev, const void* sums_dev, void* grad_xyz_dev);

/* --- vertex tangent render ---------------------------------------------------------------------------
 * The forward mode of the shape: how the frame c5_render would produce NOW changes when every grid point v moves with
 * the velocity d_xyz[v], the cells' scalars held - the motion tangent with a velocity per point instead of an affine
 * field.  d_xyz is given in the coordinates c5_upload_grid took; in view space u_v = M d_xyz[v], M the linear part of the
 * view.  A face with slopes (gx, gy) and the pixel's barycentric coordinates lambda in its projected triangle moves at
 * the pixel by
 *     dw = sum_{i<3} lambda_i (u_z - gx u_x - gy u_y)[vertex i of the face],
 * a segment's chord by ddz_k = dw_exit,k - dw_entry,k, and
 *     tau_dot = sum_k alpha_k ddz_k                                   (raw alpha, every segment)
 *     I_dot_k = E_k I_dot_{k-1} + E_k (Q_k - a_k I_{k-1}) ddz_k       (active segments)
 * as for the motion tangent.  Both faces of a segment are found from its cell's own vertices, as the vertex adjoint finds
 * them.  For d_xyz[v] = M^T (A p_v + b), p_v the point in view space, the result is c5_render_motion_tangent's for (A, b).
 * Conventions: the motion tangent's and the vertex adjoint's.  The clamp is on alpha, not on the chord; a cell with
 * clamped alpha < DBL_EPSILON moves tau only; solid-marked and uncovered pixels are 0; faces edge-on to the rays move
 * nothing; whole rays in the reference's order whatever "integration", "depth_split", "lds_stage" or "tile" say; pixels
 * that gain or lose coverage when the points move are not differentiated.
 * WELDED POINTS: the cells name the representative of a group of welded points (c5_weld_points: rep[i] != i), so the row
 * of a welded non-representative is never read: the group moves with its representative's row.  (The vertex adjoint
 * writes exact zeros to those rows.)
 * DUALITY: this is the operator c5_render_vertex_adjoint is the transpose of.  For any upstream image g and any d_xyz,
 * <g, out> = <grad_xyz, d_xyz> up to the fp32 rounding of out and the adjoint's order of summation.
 * d_xyz: [n_dirs][n_pts][3] fp64 in the caller's point order.  out: [n_dirs][local_rows][res_x][2] fp32, the motion
 * tangent's layout (row range and row tiles as for a frame).  More than "batch_width" fields run as chunks over one
 * per-view setup; every slice is bit for bit what the call returns for that field alone.  One walk per ray, no atomics:
 * bit-reproducible.
 * Status, retries, side effects and the refusal while c5_render_host_async frames are outstanding: as
 * c5_render_tangent_batch's (C5_ERR_INVALID for a null pointer or n_dirs < 1; the adjoint's counters and status words,
 * never a frame's; a c5_render afterwards returns the bits it would have returned without it).  The first call allocates
 * 24 bytes per point and field of a chunk; a context that never calls it uses no more memory than before.
 * c5_render_vertex_tangent is synchronous with host arrays and retries by itself on C5_RETRY; the _device form is
 * asynchronous on the context's stream with device arrays. */
int c5_render_vertex_tangent(c5_context* ctx, int n_dirs, const double* d_xyz_host, float* out_host);
int c5_render_vertex_tangent_device(c5_context* ctx, int n_dirs, const void* d_xyz_dev, void* out_dev);

/* --- vertex Gauss-Newton product -----------------------------------------------------------------------
 * With J the Jacobian of the frame c5_render would produce now with respect to the coordinates of the grid's points - the
 * map of c5_render_vertex_tangent, its transpose the map of c5_render_vertex_adjoint - and W a diagonal matrix of
 * per-pixel, per-channel weights:
 * c5_render_vertex_gn_product: H v = J^T W J v for n_dirs per-point fields v, the normal-equation product of a
 * Gauss-Newton / CG fit of the SHAPE to observed images.  d_xyz [n_dirs][n_pts][3] fp64 with c5_render_vertex_tangent's
 * conventions (the caller's point order, the coordinates of the upload; rows of welded non-representatives are never
 * read).  weight [local_rows][res_x][2] fp32 (channel 0 weighs tau, 1 weighs I), NULL = all ones; one weight image for all
 * fields.  h_xyz [n_dirs][n_pts][3] fp64, overwritten, with c5_render_vertex_adjoint's conventions (welded
 * non-representatives receive exact zeros).  jv_out [n_dirs][local_rows][res_x][2] fp32 or NULL: J v, bit for bit
 * c5_render_vertex_tangent's image.
 * It is ONE call for what otherwise takes c5_render_vertex_tangent, a multiply and c5_render_vertex_adjoint_batch: one
 * per-view setup, and the tangent walk leaves the adjoint's first pass (Lambda) behind - that pass is never launched.  The
 * intermediate image is fp32 on purpose: the result is that of c5_render_vertex_adjoint_batch on grad_out = weight * (fp32
 * image of c5_render_vertex_tangent), one fp32 multiply per channel (rounded by itself, no fma) -
 *   "vertex_exact" 0: up to the order of the fp64 additions, and like the vertex adjoint NOT bit-reproducible from run to
 *                     run.  One field takes the single vertex adjoint's second pass ("vertex_merge" has its say), several
 *                     take the batch's.
 *   "vertex_exact" 1: bit for bit; every field's weighted image goes through the single exact path, one after the other.
 * So H is symmetric positive semidefinite for weights >= 0 up to that fp32 rounding.  On "algorithm" 1, and after a
 * C5_RETRY onto its lists, the fields run one after the other over one per-view setup.
 * n_dirs < 1, a NULL d_xyz or a NULL h_xyz: C5_ERR_INVALID.  A scene without cells: zeros in h_xyz and jv_out.  Row ranges
 * and row tiles (the products of the parts sum to the whole frame's), status words, counters, retries and side effects:
 * the batch calls' (the adjoint's counters and status words, never a frame's; a c5_render afterwards returns the bits it
 * would have returned without it).  Memory is allocated at the first call only: the buffers of the vertex tangent, of the
 * vertex adjoint (its batch's for n_dirs > 1, the exact sums' under "vertex_exact") and "batch_width" images.
 * c5_render_vertex_gn_product is synchronous with host arrays and retries by itself on C5_RETRY; the _device form is
 * asynchronous on the context's stream with device arrays, its status reported by the next call that waits for the
 * stream.  Both refuse while c5_render_host_async frames are outstanding (C5_ERR_STATE). */
int c5_render_vertex_gn_product(c5_context* ctx, int n_dirs, const double* d_xyz_host, const float* weight_host,
                                double* h_xyz_host, float* jv_out_host);
int c5_render_vertex_gn_product_device(c5_context* ctx, int n_dirs, const void* d_xyz_dev, const void* weight_dev,
                                       void* h_xyz_dev, void* jv_out_dev);

/* --- ray matrix --------------------------------------------------------------------------------------
 * The operator every derivative render applies, handed out: for each pixel the cells its ray crosses and the chord dz of
 * each crossing, as a CSR matrix A with A[pixel][cell] = dz.  Channel 0 of the image is linear in the cells' alpha:
 * tau = A alpha (raw alpha, line.cpp:189), and A^T g is c5_render_adjoint's grad_alpha for the upstream image (g, 0).
 * Channel 1 (I) is not linear in alpha: its derivatives per segment are c5_ray_jacobian_fill's, below.
 * The matrix belongs to the frame c5_render would produce NOW: grid, solids, image, row range and row tiles, view.  No
 * render needs to come first; the cells' scalars and the alpha limit do not enter.
 * Rows: the context's local pixels, lrow * res_x + col, the output image's order.  Columns: cells in the CALLER's order
 * (c5_upload_grid's), whatever "cell_order" does inside.  Within a row the segments come in the order of the reference's
 * recurrence (line.cpp:206): deepest first, z ascending.  The entries are exactly the segments the frame sums: dz > 0 and
 * finite.  Solid-marked and uncovered pixels have empty rows; a solids-only scene gives all-empty rows (its fill writes
 * nothing, waits for the stream and returns C5_ERR_STATE itself for a row_ptr whose total is not 0).  A ray crosses a
 * cell at most once: (row, column) pairs are unique.
 * Two calls, count and fill:
 * c5_ray_matrix_rows: row_ptr[local_px + 1] int64, the exclusive prefix sums of the rows' lengths; row_ptr[local_px] ==
 * *nnz.  Waits for the stream: *nnz (host memory in both forms) is valid on return.  The host form retries by itself on
 * C5_RETRY; the _device form returns C5_RETRY (run it again).
 * c5_ray_matrix_fill: row_ptr is what c5_ray_matrix_rows returned for this frame (input).  col[capacity] int32,
 * dz[capacity] fp64, z_exit[capacity] fp64 or NULL: the segment's far end in view space (the reference's z_hi; its near
 * end is z_exit - dz).  The host form is synchronous and retries by itself; the _device form is asynchronous on the
 * context's stream and reports at the next call that waits for it.
 * The fill is stateless and guarded: element k of row p goes to i = row_ptr[p] + k only where 0 <= i < capacity and
 * k < row_ptr[p + 1] - row_ptr[p]; nothing outside [0, capacity) is ever written, whatever row_ptr holds.  A row whose
 * length differs from row_ptr's, or that found no room below capacity, is counted, and the next wait returns C5_ERR_STATE
 * ("the frame changed between c5_ray_matrix_rows and c5_ray_matrix_fill").  row_ptr[local_px] > capacity in the host
 * form: C5_ERR_INVALID with the size needed, nothing written.
 * No atomics, every lane owns its row: bit-reproducible from run to run, and the rows of a row range or of row tiles
 * are bit for bit those rows of the whole frame's matrix.
 * Status, retries, side effects: the other derivative renders' (each call makes a per-view setup of its own; the adjoint's
 * counters and status words, never a frame's; a c5_render afterwards returns the bits it would have returned without
 * them; C5_ERR_WALK; C5_RETRY for a grown entry pool or interpenetrating components).  A null pointer (z_exit excepted):
 * C5_ERR_INVALID.  All four refuse while c5_render_host_async frames are outstanding (C5_ERR_STATE).  The first call
 * allocates 4 bytes per local pixel and the scan's scratch; a context that never calls them uses no more memory than
 * before.  The arrays take nnz x 12 bytes, 20 with z_exit. */
int c5_ray_matrix_rows(c5_context* ctx, int64_t* row_ptr_host, int64_t* nnz);
int c5_ray_matrix_rows_device(c5_context* ctx, void* row_ptr_dev, int64_t* nnz);
int c5_ray_matrix_fill(c5_context* ctx, const int64_t* row_ptr_host, int64_t capacity, int32_t* col_host, double* dz_host,
                       double* z_exit_host);
int c5_ray_matrix_fill_device(c5_context* ctx, const void* row_ptr_dev, int64_t capacity, void* col_dev, void* dz_dev,
                              void* z_exit_dev);

/* --- ray Jacobian ------------------------------------------------------------------------------------
 * The Jacobian J = d(tau, I) / d(alpha, Q) the derivative renders apply, handed out per segment: three CSR matrices over
 * the ray matrix's structure.  For pixel p and the k-th cell c its ray crosses (the notation of c5_render_adjoint: a_k =
 * min(alpha_k, limit), E_k = exp(-a_k dz_k), T_k the transmittance from segment k to the viewer, I_{k-1} the intensity
 * behind it):
 *   dz[k]        = d tau_p / d alpha_c                                                    (raw alpha, every segment)
 *   dI_dalpha[k] = d I_p / d alpha_c = T_k [Q_k (dz_k E_k / a_k - (1 - E_k) / a_k^2) - dz_k E_k I_{k-1}]
 *   dI_dq[k]     = d I_p / d Q_c     = T_k (1 - E_k) / a_k
 * An inactive segment (a_k < DBL_EPSILON) stores explicit zeros in dI_dalpha and dI_dq; a clamped alpha (alpha_k > limit)
 * stores 0 in dI_dalpha and the value in dI_dq.  The values are the doubles c5_render_adjoint adds to its sums:
 * c5_render_adjoint for an upstream image that is (0, 1) at pixel p and zero elsewhere returns row p of dI_dalpha /
 * dI_dq scattered by col, bit for bit, and for (1, 0) row p of dz (an element of -0 reads +0 there).
 * Inputs: row_ptr is c5_ray_matrix_rows' output for the same frame.  The Jacobian belongs to the frame c5_render would
 * produce NOW; unlike the ray matrix it includes the cells' scalars (c5_update_scalars(_device)) and c5_set_alpha_limit.
 * The STRUCTURE never depends on them: rows, the column convention (the caller's cell order), the entries (dz > 0 and
 * finite) and the order within a row (deepest first) are exactly c5_ray_matrix_fill's, col and dz its arrays bit for bit;
 * solid-marked and uncovered pixels give empty rows.
 * col and dz may be NULL (a caller who has them from c5_ray_matrix_fill); one of dI_dalpha and dI_dq may be NULL, both:
 * C5_ERR_INVALID.  A NULL row_ptr, a negative capacity: C5_ERR_INVALID.
 * Guard and status are the ray matrix fill's: nothing outside [0, capacity) is ever written, whatever row_ptr holds; rows
 * whose length differs from row_ptr's, or that found no room below capacity, are counted, and the next wait returns
 * C5_ERR_STATE; row_ptr[local_px] > capacity in the host form: C5_ERR_INVALID with the size needed, nothing written; a
 * solids-only scene writes nothing and returns C5_ERR_STATE itself for a row_ptr whose total is not 0.  C5_RETRY and
 * C5_ERR_WALK as for every derivative; the host form is synchronous and retries by itself, the _device form is asynchronous
 * on the context's stream and reports at the next call that waits for it.  Both refuse while c5_render_host_async frames
 * are outstanding (C5_ERR_STATE), and a context without a grid or an image as c5_render_adjoint does.
 * The options "integration", "depth_split", "lds_stage", "tile", "adjoint_exact", "exact_sums" and "vertex_exact" change
 * nothing: whole rays, the reference's order.  No atomics, every lane owns its row: bit-reproducible, and the rows of a
 * row range or of row tiles are bit for bit those rows of the whole frame's.  A c5_render afterwards returns the bits it
 * would have returned without the call (the slot's per-view data are marked stale, as by the adjoint).
 * Memory: the arrays are the caller's, nnz x 28 bytes for all four.  The library allocates the adjoint's 8 bytes per local
 * pixel (Lambda) and the ray matrix's 4; a context that never calls it allocates nothing. */
int c5_ray_jacobian_fill(c5_context* ctx, const int64_t* row_ptr_host, int64_t capacity, int32_t* col_host, double* dz_host,
                         double* dI_dalpha_host, double* dI_dq_host);
int c5_ray_jacobian_fill_device(c5_context* ctx, const void* row_ptr_dev, int64_t capacity, void* col_dev, void* dz_dev,
                                void* dI_dalpha_dev, void* dI_dq_dev);

/* --- ray shape Jacobian ------------------------------------------------------------------------------
 * The Jacobian J = d(tau, I) / d xyz the vertex renders apply (c5_render_vertex_tangent forwards, c5_render_vertex_adjoint
 * transposed), handed out per segment over the ray matrix's structure, in two parts.
 * c5_ray_shape_jacobian_fill: for pixel p and the k-th cell c its ray crosses (the notation of c5_render_vertex_adjoint:
 * the chord is dz_k = w_exit - w_entry, a face's depth at the pixel w = sum_i lambda_i z_i)
 *   dI_ddz[k]  = d I_p / d dz_k = T_k E_k (Q_k - a_k I_{k-1})              (an inactive segment, a_k < DBL_EPSILON: explicit 0;
 *                the clamp is on alpha, not on the chord: a clamped alpha stores the value.)  d tau_p / d dz_k is the cell's
 *                raw alpha, which the caller holds: there is no array for it.  The double is the g_I factor of the G_k
 *                c5_render_vertex_adjoint forms.
 *   faces[k]   = bits 0-1: the exit face's index in the cell (c5_face_adjacency's numbering: face f lacks vertex 3 - f),
 *                bits 2-3: the entry face's; bit 4: the exit face contributes, bit 5: the entry face does.  Where the cell's
 *                two faces are not found at the pixel (a face edge-on to the rays is never a candidate) neither contributes, as
 *                in the vertex adjoint: the byte is 0.
 *   bary[k][0][.], bary[k][1][.] = the pixel's barycentric coordinates in the projected exit and entry face, for the
 *                face's three vertices in the order of face_points below; exact zeros where the face's bit is clear.
 * c5_face_gradients: per cell c (the CALLER's order) and face f, from grid, points and view alone:
 *   face_points[c][f][i] int32 = the point (the caller's order; the representative where points were welded) of vertex i of
 *                face f: {0,1,2}, {0,1,3}, {0,2,3}, {1,2,3} of the cell's four;
 *   dw_dxyz[c][f][.] = M^T (-gx, -gy, 1): the change of the face's depth at a pixel per unit of barycentric weight and unit
 *                motion of a vertex, (gx, gy) the face's slopes in view space, M the linear part of the view; exact zeros
 *                for a face edge-on to the rays.
 * From these, with col and dz of c5_ray_matrix_fill (c = col[k]),
 *   d I_p / d xyz[v]   = sum_k dI_ddz[k] sum_{side, i: face_points[c][f_side][i] == v} (+-bary[k][side][i]) dw_dxyz[c][f_side]
 * with + at the exit face (side 0) and - at the entry face (side 1), and d tau_p / d xyz[v] the same sum with alpha[c] in
 * place of dI_ddz[k].  Row p of it is c5_render_vertex_adjoint's gradient for the upstream image that is (0, 1) / (1, 0) at
 * p and zero elsewhere, up to the order of its sums; J d is c5_render_vertex_tangent's image.  Pixels that gain or lose
 * coverage are not differentiated, as there.
 * Structure: rows, entries (dz > 0 and finite) and the order within a row (deepest first) are c5_ray_matrix_fill's for
 * c5_ray_matrix_rows' row_ptr of the same frame; the values include the cells' scalars and c5_set_alpha_limit, the
 * structure never does.  Any one of dI_ddz, faces and bary may be NULL; all three: C5_ERR_INVALID.  A NULL row_ptr, a
 * negative capacity, a NULL face_points or dw_dxyz: C5_ERR_INVALID.
 * Guard and status are c5_ray_jacobian_fill's: nothing outside [0, capacity) (elements; 6 doubles each in bary) is ever
 * written, whatever row_ptr holds; rows whose length differs from row_ptr's, or that found no room below capacity, are
 * counted, and the next wait returns C5_ERR_STATE; row_ptr[local_px] > capacity in the host form: C5_ERR_INVALID with the
 * size needed, nothing written; a solids-only scene writes nothing and returns C5_ERR_STATE itself for a row_ptr whose
 * total is not 0 (c5_face_gradients: writes nothing, C5_OK).  C5_RETRY and C5_ERR_WALK as for every derivative; the host
 * forms are synchronous and retry by themselves, the _device forms are asynchronous on the context's stream and report at
 * the next call that waits for it.  All four refuse while c5_render_host_async frames are outstanding (C5_ERR_STATE), and a
 * context without a grid or an image as c5_render_adjoint does.
 * The options "integration", "depth_split", "lds_stage", "tile", "adjoint_exact", "exact_sums", "vertex_exact" and
 * "vertex_merge" change nothing.  No atomics, every lane owns its row: bit-reproducible, and the rows of a row range or of
 * row tiles are bit for bit those rows of the whole frame's.  A c5_render afterwards returns the bits it would have
 * returned without the calls (the slot's per-view data are marked stale, as by the adjoint).
 * Memory: the arrays are the caller's, nnz x 57 bytes for all three and n_cells x 144 for the faces.  The library
 * allocates the adjoint's 8 bytes per local pixel (Lambda) and the ray matrix's 4; a context that never calls them
 * allocates nothing. */
int c5_ray_shape_jacobian_fill(c5_context* ctx, const int64_t* row_ptr_host, int64_t capacity, double* dI_ddz_host,
                               uint8_t* faces_host, double* bary_host);
int c5_ray_shape_jacobian_fill_device(c5_context* ctx, const void* row_ptr_dev, int64_t capacity, void* dI_ddz_dev,
                                      void* faces_dev, void* bary_dev);
int c5_face_gradients(c5_context* ctx, int32_t* face_points_host, double* dw_dxyz_host);
int c5_face_gradients_device(c5_context* ctx, void* face_points_dev, void* dw_dxyz_dev);

/* --- cell-field smoothness prior ---------------------------------------------------------------------
 * What makes a fit of (alpha, Q) well-posed where the rays say nothing: a penalty on the difference of a field across
 * every interior face of the grid, with its gradient, its Hessian product and the Hessian's diagonal.  The calls need a
 * grid and nothing else (no image, view, rows or options); the fields are ARGUMENTS, in the caller's cell order - the
 * prior may be taken at any field, not only at the context's scalars.
 *
 * Interior face: a pair of cells (c, n) joined by face f of c (c5_face_adjacency's numbering) in the adjacency
 * c5_upload_grid built - over welded points, so cells joined only through coincident point copies are neighbours.  Faces
 * without a partner couple nothing: boundary faces, faces at hanging nodes, the two sides of a non-conforming interface.
 *
 * Weight w of a face.  0 on a face that is not interior.  On an interior face
 *   C5_PRIOR_UNIT   w = 1
 *   C5_PRIOR_TPFA   w = A / |x_n - x_c|: A the face's area, x a cell's centroid (the mean of its four points), both from
 *                   the object-space coordinates as the device holds them now (after welding, after the last
 *                   c5_update_points; no view enters).  In fp64, no contraction: with the face's three welded point ids
 *                   ascending, t0 < t1 < t2, e1 = P[t1] - P[t0], e2 = P[t2] - P[t0], c = e1 x e2 (cx = e1y e2z - e1z e2y,
 *                   ...), A = 0.5 sqrt((cx^2 + cy^2) + cz^2); the two cells share the face's points, so x_n - x_c is
 *                   (a_n - a_c) / 4 for their remaining points a: g = a_n - a_c, |x_n - x_c| = 0.25 sqrt((gx^2 + gy^2) +
 *                   gz^2); w = A / |x_n - x_c|.  A weight that is not finite and positive (zero area, coincident
 *                   centroids) is stored as 0 and counted.
 * w is a function of the UNORDERED pair: every operand above is the same whichever cell asks (g only changes sign, and is
 * squared), so w[c][f] and its partner's w[n][f'] are the same bits, under "cell_order" 0 and 1 alike.
 *
 * Penalty psi of a difference d = x_c - x_n, per field with its own delta:
 *   C5_PRIOR_QUADRATIC     psi = d^2 / 2, psi' = d, psi'' = 1
 *   C5_PRIOR_PSEUDO_HUBER  with u = d / delta, t = u u, s = sqrt(1 + t):
 *                          psi = delta^2 t / (1 + s), formed as (d d) / (1 + s)   (never s - 1, which is 0 below |u| = 1e-8;
 *                          d d is delta^2 t without delta^2 leaving the format), psi' = d / s, psi'' = 1 / ((1 + t) s)
 *                          Range: every finite d and delta > 0.  t leaves the format at |u| = 2^512 (and u itself may be inf),
 *                          where the forms above would give psi' = 0 and psi = inf / inf; so from |u| >= 2^256 on - where
 *                          s = |u| to the last bit - the linear tail is taken in closed form: psi = delta (|d| - delta),
 *                          psi' = copysign(delta, d), psi'' = ((1 / |u|) / |u|) / |u|, which underflows gradually to 0.
 *                          Below that, where d d is inf, psi = |d| (|d| / (1 + s)).  Below |u| = 2^256 a finite result of the plain
 *                          forms is returned as it is.  A psi beyond the format is +inf; a NaN comes from a NaN only.
 * Operators, per field x (alpha or Q) with its own lambda >= 0, the sums over the faces f of cell c that have a neighbour n:
 *   R(x)            = lambda sum over interior faces, each once, of w psi(d)
 *   (grad R)_c      = lambda sum_f w_f psi'(x_c - x_n)
 *   (hess R(x) p)_c = lambda sum_f (w_f psi''(x_c - x_n)) (p_c - p_n)
 *   diag_c          = lambda sum_f w_f psi''(x_c - x_n)
 * Order of operations: a cell's sum runs over f = 0, 1, 2, 3 as (((0 + t0) + t1) + t2) + t3, a face without a neighbour
 * adding nothing; each term by plain multiplies as bracketed above, no fused multiply-add; lambda multiplies the finished
 * sum.  So a numpy restatement reproduces the quadratic operators bit for bit from c5_prior_weights' output, no vector
 * depends on the cells' device order ("cell_order"), and the quadratic gradient at x IS the product applied to x.
 * The value: cell c's half h_c = 0.5 (((0 + w_0 psi_0) + w_1 psi_1) + ...), summed over the cells of the device's order in
 * a fixed tree (wavefront, block, then one block over the blocks' partials) and multiplied by lambda: no atomics, the same
 * bits from call to call, on a fresh context and between the host and _device forms.
 *
 * c5_prior_weights: w[n_cells][4] in the caller's cell and face order (may be NULL), the number of interior faces and of
 * those stored as 0 (either may be NULL; always host pointers).  The weights are kept on the device per weighting, built
 * at first use and again after c5_upload_grid and (TPFA) c5_update_points; that build waits for the context's stream once.
 * c5_prior_gradient: value[2] = (R(alpha), R(q)) where value is not NULL, and the two gradients.
 * c5_prior_product: the point (alpha, q) is ignored and may be NULL for C5_PRIOR_QUADRATIC, as in c5_prior_diagonal.
 * A field whose lambda is 0 is left out: its value is 0, its output array, where given, is zeros, all its pointers may be
 * NULL.  A field with lambda > 0 needs its arrays: C5_ERR_INVALID.  An unknown penalty or weighting, a negative or
 * non-finite lambda, a delta that is not finite and positive where the penalty is C5_PRIOR_PSEUDO_HUBER and the field's
 * lambda > 0: C5_ERR_INVALID, nothing written.  A grid uploaded as non-conforming (a face in more than two cells) holds no
 * adjacency: C5_ERR_MESH.  A context without cells answers as the derivative renders do: C5_ERR_STATE where there is
 * nothing at all, C5_OK with nothing written but value = (0, 0) where there are only solids.
 * The host forms are synchronous.  The _device forms take device pointers (value: a device double[2]), are enqueued on
 * the context's stream and do not wait (but for a pending build of the weights).  One lane per cell, no atomics:
 * bit-reproducible.  Memory: 32 bytes per cell and weighting used, 16 bytes per 256 cells for the value. */
enum { C5_PRIOR_QUADRATIC = 0, C5_PRIOR_PSEUDO_HUBER = 1 };
enum { C5_PRIOR_UNIT = 0, C5_PRIOR_TPFA = 1 };
typedef struct c5_prior {
    int32_t penalty;                /* C5_PRIOR_QUADRATIC | C5_PRIOR_PSEUDO_HUBER */
    int32_t weighting;              /* C5_PRIOR_UNIT | C5_PRIOR_TPFA */
    double lambda_alpha, lambda_q;  /* >= 0, finite; 0 leaves the field out */
    double delta_alpha, delta_q;    /* > 0, finite where the penalty uses them */
} c5_prior;
int c5_prior_weights(c5_context* ctx, int weighting, double* w_host, int64_t* n_interior_faces, int64_t* n_degenerate);
int c5_prior_weights_device(c5_context* ctx, int weighting, void* w_dev, int64_t* n_interior_faces, int64_t* n_degenerate);
int c5_prior_gradient(c5_context* ctx, const c5_prior* prior, const double* alpha_host, const double* q_host, double value_host[2],
                      double* grad_alpha_host, double* grad_q_host);
int c5_prior_gradient_device(c5_context* ctx, const c5_prior* prior, const void* alpha_dev, const void* q_dev, void* value_dev,
                             void* grad_alpha_dev, void* grad_q_dev);
int c5_prior_product(c5_context* ctx, const c5_prior* prior, const double* alpha_host, const double* q_host, const double* v_alpha_host,
                     const double* v_q_host, double* h_alpha_host, double* h_q_host);
int c5_prior_product_device(c5_context* ctx, const c5_prior* prior, const void* alpha_dev, const void* q_dev, const void* v_alpha_dev,
                            const void* v_q_dev, void* h_alpha_dev, void* h_q_dev);
int c5_prior_diagonal(c5_context* ctx, const c5_prior* prior, const double* alpha_host, const double* q_host, double* diag_alpha_host,
                      double* diag_q_host);
int c5_prior_diagonal_device(c5_context* ctx, const c5_prior* prior, const void* alpha_dev, const void* q_dev, void* diag_alpha_dev,
                             void* diag_q_dev);

/* --- shape prior ---------------------------------------------------------------------------------------
 * What makes a fit of the grid's SHAPE (c5_update_points, c5_render_vertex_adjoint, c5_render_vertex_gn_product)
 * well-posed where the rays say nothing, and what tells a caller that a trial step turns a cell inside out: an elastic
 * energy of the points relative to a rest shape, with its gradient, its Hessian product, the Hessian's diagonal and the
 * cells' volume ratios.  The calls need a grid and nothing else (no image, view, rows or options, and no face adjacency:
 * a grid uploaded as non-conforming is served like any other); the coordinates are ARGUMENTS, [n_pts][3] fp64 in the order
 * of c5_upload_grid - a line search evaluates trial points without moving the grid.
 *
 * Rest shape.  Coordinates X[n_pts][3], taken once by c5_shape_prior_rest, give per cell with points (X0..X3) - in the
 * order the device holds the cell's four ids, a point welded at upload replaced by its representative -
 *   Dm = [X1 - X0, X2 - X0, X3 - X0] (columns), B = Dm^-1, V0 = |det Dm| / 6,
 * in fp64 without contraction: with the cofactors C00 = D11 D22 - D12 D21, C01 = D12 D20 - D10 D22, C02 = D10 D21 - D11 D20,
 * C10 = D02 D21 - D01 D22, C11 = D00 D22 - D02 D20, C12 = D01 D20 - D00 D21, C20 = D01 D12 - D02 D11, C21 = D02 D10 - D00 D12,
 * C22 = D00 D11 - D01 D10: det = (D00 C00 + D01 C01) + D02 C02 and B[r][c] = C[c][r] / det (the adjugate over the
 * determinant).  A cell whose V0 or B is not finite, or whose V0 is not positive, is DEGENERATE: it is stored with V0 = 0
 * and B = 0, contributes nothing anywhere (its ratio below is 0 and it is never counted as inverted), and is counted in
 * n_degenerate.
 *
 * Deformation at coordinates x: Ds = [x1 - x0, x2 - x0, x3 - x0], F = Ds B with F[r][c] = (Ds[r][0] B[0][c] + Ds[r][1]
 * B[1][c]) + Ds[r][2] B[2][c], J = det F by the cofactor formula above.
 *
 * Energy R(x) = lambda sum over the cells of V0 psi(F):
 *   C5_SHAPE_DIRICHLET    psi = 1/2 |F - I|^2, P = F - I, dP = dF.  Quadratic: the Hessian is constant, the point x is
 *                         ignored by product and diagonal.  Invariant under translation, not under rotation.
 *   C5_SHAPE_NEO_HOOKEAN  psi = 1/2 (|F|^2 - 3) - ln J + (kappa / 2) (ln J)^2, kappa >= 0: invariant under rotation, zero with
 *                         zero gradient at rest, +inf as J -> 0+.  With F^-T = cofactors(F) / J:
 *                         P  = F + (kappa ln J - 1) F^-T
 *                         dP = (dF + (1 - kappa ln J) (F^-T dF^T F^-T)) + (kappa tr(F^-1 dF)) F^-T
 *                         the exact Hessian, which can be indefinite.
 * |A|^2 is the sum of the squares of A's entries, row by row from the first; tr(F^-1 dF) the sum of F^-T[r][c] dF[r][c] in
 * the same order; every 3-term inner product is (a0 b0 + a1 b1) + a2 b2.
 *
 * A cell's shares.  G = V0 (P B^T): G[r][i] = V0 ((P[r][0] B[i][0] + P[r][1] B[i][1]) + P[r][2] B[i][2]); the gradient at
 * x_i (i = 1..3) is column i - 1 of G, at x_0 it is -((G[r][0] + G[r][1]) + G[r][2]).  The product: the same with dP of
 * dF = [v1 - v0, v2 - v0, v3 - v0] B.  The diagonal: entry (point k, coordinate r) of the product applied to the unit
 * vector of (k, r), by the same operations - it IS the product on unit vectors.
 *
 * Inverted cells.  A non-degenerate cell with J <= 0 or J not finite at x is INVERTED: counted in n_inverted under both
 * energies; under C5_SHAPE_NEO_HOOKEAN it makes the value +inf and contributes nothing to gradient, product and
 * diagonal, whose outputs stay finite - a caller can back off.
 *
 * Per-point sums.  A point's result is the sum of its incident cells' shares in ascending order of the CALLER's cell
 * index, left to right from 0, then multiplied by lambda: bit-reproducible and independent of "cell_order".  A point
 * welded to another receives 0, its representative the group's sum, and the welded point's own input coordinates are
 * ignored (c5_update_points' and c5_render_vertex_adjoint's conventions).  So a numpy restatement reproduces the Dirichlet
 * operators bit for bit from c5_shape_prior_rest_data's output.  The value: the cells' V0 psi summed over the device's cell
 * order in a fixed tree (wavefront, block, one block over the blocks' partials), multiplied by lambda: no atomics, the
 * same bits from call to call and between the host and _device forms.
 *
 * c5_shape_prior_rest: xyz[n_pts][3], or NULL for the points the context holds now (after the last c5_update_points);
 *   n_degenerate may be NULL (always a host pointer; both forms wait for the stream).  The rest data live on the context:
 *   c5_upload_grid drops them, c5_update_points does not touch them.  A wrong n_pts or a non-finite coordinate:
 *   C5_ERR_INVALID, and the rest shape set before stays.  Every other call returns C5_ERR_STATE before a rest shape is set.
 * c5_shape_prior_rest_data: B [n_cells][3][3] (row-major), V0 [n_cells] and the four representatives int32 [n_cells][4] in
 *   the order the arithmetic uses, all in the CALLER's cell order; every output may be NULL.
 * c5_shape_prior_gradient: value[1] and n_inverted[1] (either may be NULL) and the gradient.
 * c5_shape_prior_product / _diagonal: xyz may be NULL under C5_SHAPE_DIRICHLET.
 * c5_shape_prior_quality: ratio[n_cells] = J in the caller's cell order (may be NULL) and n_inverted (may be NULL); it is
 *   the operators' cell launch with a store of J.
 * Any other NULL array, an unknown energy, a lambda or kappa that is negative or not finite, reserved != 0:
 * C5_ERR_INVALID, nothing written.  A context without cells answers as the c5_prior_* calls do; all calls refuse while
 * c5_render_host_async frames are outstanding (C5_ERR_STATE).  The host forms are synchronous.  The _device forms take
 * device pointers (value: a device double, n_inverted: a device int64, read them after the next wait), are enqueued on the
 * context's stream and do not wait - but for c5_shape_prior_rest and, once per upload, the build of the point-to-cell
 * incidence table that "vertex_exact" shares.  Memory: 80 bytes per cell of rest data, 96 of shares. */
enum { C5_SHAPE_DIRICHLET = 0, C5_SHAPE_NEO_HOOKEAN = 1 };
typedef struct c5_shape_prior {
    int32_t energy;    /* C5_SHAPE_DIRICHLET | C5_SHAPE_NEO_HOOKEAN */
    int32_t reserved;  /* 0 */
    double lambda;     /* >= 0, finite */
    double kappa;      /* >= 0, finite (C5_SHAPE_NEO_HOOKEAN's volume term) */
} c5_shape_prior;
int c5_shape_prior_rest(c5_context* ctx, const double* xyz_host, int64_t n_pts, int64_t* n_degenerate);
int c5_shape_prior_rest_device(c5_context* ctx, const void* xyz_dev, int64_t n_pts, int64_t* n_degenerate);
int c5_shape_prior_rest_data(c5_context* ctx, double* binv_host, double* vol_host, int32_t* vert_host);
int c5_shape_prior_rest_data_device(c5_context* ctx, void* binv_dev, void* vol_dev, void* vert_dev);
int c5_shape_prior_gradient(c5_context* ctx, const c5_shape_prior* prior, const double* xyz_host, double* value_host, int64_t* n_inverted,
                            double* grad_xyz_host);
int c5_shape_prior_gradient_device(c5_context* ctx, const c5_shape_prior* prior, const void* xyz_dev, void* value_dev, void* n_inverted_dev,
                                   void* grad_xyz_dev);
int c5_shape_prior_product(c5_context* ctx, const c5_shape_prior* prior, const double* xyz_host, const double* v_xyz_host, double* h_xyz_host);
int c5_shape_prior_product_device(c5_context* ctx, const c5_shape_prior* prior, const void* xyz_dev, const void* v_xyz_dev, void* h_xyz_dev);
int c5_shape_prior_diagonal(c5_context* ctx, const c5_shape_prior* prior, const double* xyz_host, double* diag_xyz_host);
int c5_shape_prior_diagonal_device(c5_context* ctx, const c5_shape_prior* prior, const void* xyz_dev, void* diag_xyz_dev);
int c5_shape_prior_quality(c5_context* ctx, const double* xyz_host, double* ratio_host, int64_t* n_inverted);
int c5_shape_prior_quality_device(c5_context* ctx, const void* xyz_dev, void* ratio_dev, void* n_inverted_dev);

/* --- frames delivered to host memory, pipelined ----------------------------------------------------
 * plane::trace_rays hands back HOST pixels (plane.cpp:144-172); over PCIe Gen5 a 2400x1800 image is
 * 0.65 ms of transfer beside 0.7 ms of rendering, so the two are overlapped: c5_render_host_async renders
 * frame k into one of C5_HOST_RING internal device images and copies it to out_host on a copy stream of
 * its own while frame k + 1 is already being rendered.  out_host should be pinned (c5_host_alloc): a
 * pageable buffer makes the copy synchronous.  At most C5_HOST_RING frames may be outstanding; every
 * c5_render_host_async is paired, in order, with one c5_render_host_wait, which returns when THAT frame's
 * pixels are in out_host.  C5_RETRY from the wait: that frame and every frame enqueued after it are
 * incomplete (an internal buffer was too small and has been grown, or the grid turned out to need "algorithm" 1) —
 * wait for the rest, discard, render again.  A frame's status is read from ITS OWN counters (every frame of the ring
 * keeps its statistics apart: no frame in flight can add to another's).  Whichever call notices a failure first
 * (c5_get_stats, c5_get_row_costs, c5_synchronize between an async and its wait included) settles it and returns
 * C5_RETRY once; the waits of every frame outstanding at that moment return C5_RETRY as well, whatever their own
 * status words read; c5_last_error names the words. */
#define C5_HOST_RING 3
int c5_render_host_async(c5_context* ctx, float* out_host);
int c5_render_host_wait(c5_context* ctx);
/* The same, but frame_host is the FULL res_y x res_x image shared by all the contexts that render it
 * (c5_set_row_tiles / c5_set_row_range, one context per GPU): this context's rows are copied straight to
 * their final places in it — one strided copy over the context's own PCIe link, no exchange between GPUs and
 * no reassembly (the "N direct copies" of SURVEY.md section 8(e); with 8 GPUs, 8 links instead of the root's one).
 * Paired with c5_render_host_wait like c5_render_host_async. */
int c5_render_frame_rows_async(c5_context* ctx, float* frame_host);
/* Pinned host memory for images (hipHostMalloc with hipHostMallocPortable: several contexts — one per GPU — may copy
 * their rows into the same frame, c5_render_frame_rows_async / hipHostFree). */
int c5_host_alloc(c5_context* ctx, size_t bytes, void** out_ptr);
int c5_host_free(c5_context* ctx, void* ptr);

/* Statistics of the last completed frame (synchronizes). */
int c5_get_stats(c5_context* ctx, c5_stats* out);
/* Average duration (ms) of the walk kernel over the launches since the last call with
 * reset != 0; measured with HIP events on the context's stream. */
int c5_walk_kernel_ms(c5_context* ctx, int reset, double* avg_ms, int64_t* launches);

/* Host-only helper (no GPU needed): face adjacency of a conforming tetrahedral grid, the table
 * c5_upload_grid builds internally.  adj[n_cells][4] = neighbour across face f or -1, with the
 * reference's face numbering 0:(0,1,2) 1:(0,1,3) 2:(0,2,3) 3:(1,2,3) (plane.cpp:16-21).
 * Returns C5_ERR_MESH when a face is shared by more than two cells. */
int c5_face_adjacency(const int32_t* cell_vert, int64_t n_cells, int64_t n_pts, int32_t* adj,
                      int64_t* n_boundary_faces);

/* Host-only helper (no GPU needed): the point welding c5_upload_grid applies before it builds the
 * adjacency.  rep[i] = smallest point id whose coordinates equal point i's (rep[i] == i where nothing
 * coincides).  The reference copies four points per cell and ignores ids (object3d_base.cpp:37-42), so
 * coincident points are one point there by construction. */
int c5_weld_points(const double* xyz, int64_t n_pts, int32_t* rep, int64_t* n_merged);

/* Debug/inspection: transformed grid vertices of the last frame, xyz[n_pts][3]. */
int c5_download_view_points(c5_context* ctx, double* xyz);

#ifdef __cplusplus
}
#endif
#endif /* COURSE5_HIP_H */

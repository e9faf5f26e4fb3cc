// Host-callable launchers of the derivative renders.  scalar_derivative_kernels.hip: the adjoint (gradients of the image
// with respect to the cells' alpha and Q), the tangent (the image's change for a change of them), their batches and the
// Gauss-Newton renders; geometry_derivative_kernels.hip: the motion tangent, the vertex adjoint and the vertex tangent;
// ray_matrix_kernels.hip: the ray matrix (the ray Jacobian's kernels run the adjoint's bodies: scalar_derivative_kernels.hip).
// All launches are asynchronous on the given stream.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "device_types.hpp"
#include "kernels.hpp"

namespace c5 {

// What every *_resolve kernel reads ("algorithm" 1): bin_sort_resolve's per-pixel segment lists of launch_bin_fill, which
// the kernel sorts in place, over the view's grid and image.
struct ResolveParams {
    GridView g;
    ImageParams im;
    const double *Xtab, *Ytab;  // the pixels' view-space coordinates (the kernels that look faces up)
    const int64_t* offs;        // [n_local_px + 1] a pixel's list: segs[offs[p] .. offs[p + 1])
    void* segs;
    const uint32_t* mask;       // solid-marked pixels, or nullptr
    double alpha_limit;
};

struct AdjointParams {
    // the walk's inputs, as walk_composite reads them (records built with "integration" 0: the reference's order)
    WalkParams w;
    const float2* grad_out;  // [n_local_rows][res_x] upstream weights (g_tau, g_I)
    double* lambda;          // [n_local_px] pass 1 -> pass 2: sum of a dz over the ray's active segments
    double* grad_a;          // [n_cells] device order, accumulated by pass 2
    double* grad_q;
};

// pass 1 (pass == 1): Lambda per pixel; leaves the entry heads in place and counts rays over the step bound and rays that
// skipped an entry in w.counters (shard 0: walk_overflow, overlap_rays).  pass 2: the scatter; hands the heads back cleared.
void launch_adjoint_walk(hipStream_t s, const AdjointParams& a, int pass);

// bin_sort_resolve's twin: the per-pixel segment lists of launch_bin_fill -> grad_a / grad_q (device order)
void launch_adjoint_resolve(hipStream_t s, const ResolveParams& r, const float2* grad_out, double* grad_a, double* grad_q);

// out[perm[i]] = dev[i] for both arrays (perm nullptr: the identity)
void launch_adjoint_permute(hipStream_t s, const double* ga_dev, const double* gq_dev, const int32_t* perm, int64_t n,
                            double* ga_out, double* gq_out);

// ---- exact adjoint sums ("adjoint_exact", c5_render_adjoint_exact_*): the fixed-point format of exact_sum.hpp.  40
// bytes per cell and one word, in device order.
struct ExactSums {
    int2* exps;            // [n_cells] {exponent of grad_alpha's contributions, of grad_q's}: pass E's atomicMax
    long long* words;      // [n_cells][4] {alpha s1, alpha s0, q s1, q s0}: pass S's integer atomicAdd
    unsigned* misfits;     // += contributions pass S found beyond their cell's exponent (added nowhere)
    int32_t word_bits;     // m of the WHOLE image (c5_set_image), not of the context's rows
    int32_t keep_entries;  // pass S, the walk: 1 leaves the entry heads in place (another image follows); 0 hands them back cleared
};

// exps to "no contribution", words to zero and / or *misfits to zero
void launch_exact_clear(hipStream_t s, const ExactSums& x, int64_t n, bool exps, bool words, bool misfits);
// pass E (sums false: leaves the entry heads in place) or pass S of the walk; both need launch_adjoint_walk(.., 1) first
// and read a.w, a.grad_out and a.lambda only
void launch_adjoint_exact_walk(hipStream_t s, const AdjointParams& a, const ExactSums& x, bool sums);
// the same over bin_sort_resolve's lists (sorts them in place, as launch_adjoint_resolve)
void launch_adjoint_exact_resolve(hipStream_t s, const ResolveParams& r, const float2* grad_out, const ExactSums& x, bool sums);
// x.exps[i] = {exp_a[perm[i]], exp_q[perm[i]]} (perm nullptr: the identity), and back; the words back; the words as fp64
void launch_exact_gather_exps(hipStream_t s, const int32_t* exp_a, const int32_t* exp_q, const int32_t* perm, int64_t n, const ExactSums& x);
void launch_exact_emit_exps(hipStream_t s, const ExactSums& x, const int32_t* perm, int64_t n, int32_t* exp_a, int32_t* exp_q);
void launch_exact_emit_words(hipStream_t s, const ExactSums& x, const int32_t* perm, int64_t n, int64_t* sums_a, int64_t* sums_q);
// (ga_out or gq_out null: that block is not written)
void launch_exact_finish(hipStream_t s, const ExactSums& x, const int32_t* perm, int64_t n, double* ga_out, double* gq_out);

struct TangentParams {
    // the walk's inputs, as for the adjoint (records of "integration" 0)
    WalkParams w;
    const double2* dir;  // [n_cells] device order: {dalpha, dQ} (launch_tangent_gather)
    float2* out;         // [n_local_rows][res_x] (tau_dot, I_dot)
};

// dir[i] = {d_alpha[perm[i]], d_q[perm[i]]}: the caller's order -> the device's (perm nullptr: the identity); a null
// d_alpha or d_q stands for zeros
void launch_tangent_gather(hipStream_t s, const double* d_alpha, const double* d_q, const int32_t* perm, int64_t n,
                           double2* dir);

// the step of adjoint_walk<1> once per ray: (tau_dot, I_dot) per pixel (0 on solid-marked and uncovered pixels); counts
// as pass 1 does and hands the entry heads back cleared
void launch_tangent_walk(hipStream_t s, const TangentParams& t);

// the tangent over bin_sort_resolve's lists (sorts them in place, as launch_adjoint_resolve)
void launch_tangent_resolve(hipStream_t s, const ResolveParams& r, const double2* dir, float2* out);

// bytes of one segment of the bin-sort lists as the *_resolve kernels read them (deriv_lists.hpp: AdjSegment;
// derivatives.hip checks it against segment_bytes())
size_t adjoint_segment_bytes();

// ---- batches (c5_render_tangent_batch*, c5_render_adjoint_batch*): one walk per ray for up to kc directions or upstream
// images (kc: the chunk width, 4 or 8); a call with more runs several chunks over the same per-view setup.

// dirs[i][j] = {d_alpha[k0 + j][perm[i]], d_q[k0 + j][perm[i]]} for j < n_used, zero for n_used <= j < kc: the caller's
// [K][n] directions -> kc interleaved pairs per cell in device order (a null d_alpha or d_q stands for zeros)
void launch_tangent_gather_batch(hipStream_t s, int kc, const double* d_alpha, const double* d_q, const int32_t* perm, int64_t n,
                                 int k0, int n_used, double2* dirs);

struct TangentBatchParams {
    WalkParams w;          // as TangentParams
    const double2* dirs;   // [n_cells][kc] device order (launch_tangent_gather_batch)
    float2* out;           // [n_used][n_local_rows][res_x] (tau_dot, I_dot): the chunk's first image
    int64_t image_px;      // pixels per image (n_local_rows * res_x)
    int32_t n_used;        // directions of the chunk (<= kc)
    int32_t keep_entries;  // 1: leave the entry heads in place for a later chunk; 0: hand them back cleared
};

// tangent_walk's step once per ray for kc directions: every image bit for bit what launch_tangent_walk gives for its
// direction alone; counts as tangent_walk does
void launch_tangent_walk_batch(hipStream_t s, int kc, const TangentBatchParams& t);

struct AdjointBatchParams {
    WalkParams w;              // as AdjointParams (the heads left in place by pass 1)
    const float2* grad_out;    // [n_used][n_local_rows][res_x] upstream weights: the chunk's first image
    int64_t image_px;          // pixels per image
    const double* lambda;      // pass 1's Lambda per pixel (launch_adjoint_walk(.., 1), once for every chunk)
    double* grad;              // [n_cells][2 kc] device order, accumulated: {ga_0 .. ga_kc-1, gq_0 .. gq_kc-1} per cell
    int32_t n_used;            // images of the chunk (<= kc)
    int32_t keep_entries;      // as TangentBatchParams
};

// adjoint_walk<2> for kc upstream images at once (needs pass 1 first)
void launch_adjoint_walk_batch(hipStream_t s, int kc, const AdjointBatchParams& a);

// ga_out[(k0 + j) n + perm[i]] = grad[i][j], gq_out[...] = grad[i][kc + j] for j < n_used (perm nullptr: the identity)
void launch_adjoint_permute_batch(hipStream_t s, int kc, const double* grad, const int32_t* perm, int64_t n, int k0, int n_used,
                                  double* ga_out, double* gq_out);

// ---- Gauss-Newton renders (c5_render_gn_product*, c5_render_gn_diagonal*)

struct GnWalkParams {
    WalkParams w;          // as TangentParams
    const double2* dirs;   // [n_cells][kc] device order (launch_tangent_gather_batch)
    const float2* weight;  // [n_local_rows][res_x] (w_tau, w_I), or nullptr: ones
    double* lambda;        // [n_local_px] out: pass 1's Lambda
    float2* g;             // [n_used][n_local_rows][res_x] out: w * (float)(tau_dot, I_dot), one fp32 multiply per channel
    float2* jv_out;        // the same shape, out: (tau_dot, I_dot) as launch_tangent_walk_batch stores them; or nullptr
    int64_t image_px;      // pixels per image
    int32_t n_used;        // directions of the chunk (<= kc)
};

// tangent_walk_batch's walk that is also pass 1 of the adjoint: leaves the entry heads in place and counts as pass 1 does
void launch_gn_walk_a(hipStream_t s, int kc, const GnWalkParams& a);

// adjoint_walk<2> with the segment terms squared (needs pass 1 first): a.grad_out holds the weights (nullptr: ones),
// a.grad_a / a.grad_q accumulate diag(J^T W J); hands the heads back cleared
void launch_gn_diag_walk(hipStream_t s, const AdjointParams& a);

// g[j][p] = w[p] * t[j][p] per channel in fp32 (w nullptr: ones), n_imgs images of n_px pixels
void launch_gn_weight(hipStream_t s, const float2* t, const float2* w, int64_t n_px, int n_imgs, float2* g);

// launch_adjoint_resolve's twin for the diagonal
void launch_gn_diag_resolve(hipStream_t s, const ResolveParams& r, const float2* weight, double* diag_a, double* diag_q);

// "exact_sums": pass E (sums false) or pass S of the diagonal - launch_adjoint_exact_walk / _resolve with the segment
// terms squared, pass E on the squares themselves; a.grad_out / weight: the weights (nullptr: ones)
void launch_gn_diag_exact_walk(hipStream_t s, const AdjointParams& a, const ExactSums& x, bool sums);
void launch_gn_diag_exact_resolve(hipStream_t s, const ResolveParams& r, const float2* weight, const ExactSums& x, bool sums);

// ---- Hessian-vector render (c5_render_hvp*): the second derivative of sum_p g_I I_p in the cells' (alpha, Q), applied to
// one direction

struct HvpParams {
    WalkParams w;            // as AdjointParams
    const double2* dir;      // [n_cells] device order: {dalpha, dQ} (launch_tangent_gather)
    const float2* grad_out;  // [n_local_rows][res_x] upstream weights; channel 0 has no effect (pass 2)
    double* lambda;          // [n_local_px] pass 1 -> pass 2: Lambda, as AdjointParams
    double* lambda_dot;      // [n_local_px] pass 1 -> pass 2: sum of dalpha dz over the active, unclamped segments
    double* h_a;             // [n_cells] device order, accumulated by pass 2
    double* h_q;
};

// pass 1: Lambda and Lambda_dot per pixel; leaves the entry heads in place and counts as launch_adjoint_walk(.., 1) does.
// pass 2: the scatter of (h_alpha, h_q); hands the heads back cleared.
void launch_hvp_walk(hipStream_t s, const HvpParams& h, int pass);

// the same over bin_sort_resolve's lists (sorts them in place, as launch_adjoint_resolve)
void launch_hvp_resolve(hipStream_t s, const ResolveParams& r, const double2* dir, const float2* grad_out, double* h_a, double* h_q);

// "exact_sums": pass E (sums false: leaves the entry heads in place) or pass S of launch_hvp_walk(.., 2)'s walk, after
// launch_hvp_walk(.., 1); reads h.w, h.dir, h.grad_out, h.lambda and h.lambda_dot only.  And the same over
// bin_sort_resolve's lists.
void launch_hvp_exact_walk(hipStream_t s, const HvpParams& h, const ExactSums& x, bool sums);
void launch_hvp_exact_resolve(hipStream_t s, const ResolveParams& r, const double2* dir, const float2* grad_out, const ExactSums& x,
                              bool sums);

// launch_adjoint_permute with either output null (that block is not written)
void launch_hvp_permute(hipStream_t s, const double* ha_dev, const double* hq_dev, const int32_t* perm, int64_t n, double* ha_out,
                        double* hq_out);

// ---- motion tangent (c5_render_motion_tangent*): the frame differentiated with respect to an affine motion of the grid in
// view space, u(p) = A p + b

constexpr int kMotionWidth = 8;  // fields one walk carries at most (the widest "batch_width")
struct MotionField {
    double f[12];  // A row-major, then b, in the walk coordinate (records of "integration" 0: w = view z)
};
// what finds a cell's faces where the walk has no plane for them: the cell's vertices in view space (device order)
struct MotionGeometry {
    const int4* cell_vert;
    const double *vx, *vy, *vz;
};
struct MotionParams {
    WalkParams w;          // as TangentParams
    MotionGeometry geo;
    float2* out;           // [n_used][n_local_rows][res_x] (tau_dot, I_dot): the chunk's first image
    int64_t image_px;      // pixels per image
    int32_t n_used;        // fields of the chunk (<= kc)
    int32_t keep_entries;  // as TangentBatchParams
    double field[kMotionWidth][12];  // the chunk's fields (zero beyond n_used): read by uniform loads
};

// tangent_walk's walk for kc (4 or 8) velocity fields; every image bit for bit that of its field alone at either width;
// counts as tangent_walk does
void launch_motion_walk(hipStream_t s, int kc, const MotionParams& m);

// the same over bin_sort_resolve's lists, one field (sorts them in place, as launch_tangent_resolve)
void launch_motion_resolve(hipStream_t s, const ResolveParams& r, const MotionField& field, float2* out);

// ---- vertex adjoint (c5_render_vertex_adjoint*): the gradient of the frame with respect to the grid's points.  With
// G_k = d loss / d dz_k of a segment and lambda the barycentric coordinates of the pixel in the two faces the chord runs
// between, the face's three vertices receive +-G_k lambda (exit +, entry -); a face's slopes then turn that weight into
// the view-space gradient (-gx, -gy, 1) per vertex, and the view's linear part M into the caller's coordinates.

struct VertexParams {
    WalkParams w;            // as AdjointParams (the heads left in place by pass 1)
    MotionGeometry geo;
    const float2* grad_out;  // [n_local_rows][res_x] upstream weights (g_tau, g_I)
    const double* lambda;    // pass 1's Lambda per pixel (launch_adjoint_walk(.., 1))
    double* face_w;          // [n_cells][4][3] device order, accumulated: face f, its three vertices in face_plane's order
};

// adjoint_walk<2>'s walk with the chords' weights scattered to face_w (needs pass 1 first); hands the heads back cleared.
// merge: the lanes of a wavefront in one cell are summed in LDS first ("vertex_merge"); else every lane adds its own
void launch_vertex_walk(hipStream_t s, const VertexParams& v, bool merge);

// the same over bin_sort_resolve's lists (sorts them in place, as launch_adjoint_resolve)
void launch_vertex_resolve(hipStream_t s, const ResolveParams& r, const float2* grad_out, double* face_w);

// face_w -> grad_view[n_pts][3] (zeroed by the caller; accumulated per cell and face, edge-on faces skipped), then
// grad_xyz[v] = M^T grad_view[v] for every point, M the linear part of the view R
void launch_vertex_finish(hipStream_t s, const MotionGeometry& geo, int64_t n_cells, const double* face_w, double* grad_view,
                          int64_t n_pts, const RotationList& R, double* grad_xyz);

// ---- exact vertex adjoint sums ("vertex_exact", c5_render_vertex_exact_*): face_w's twelve slots per cell in the
// fixed-point format of exact_sum.hpp, then fixed arithmetic per cell and a gather per point in a fixed order.  240 bytes
// per cell for exponents and words, 96 for the per-cell triples, in device order.
struct VertexExactSums {
    int32_t* exps;         // [n_cells][12] the exponent of every slot's contributions: pass E's atomicMax
    long long* words;      // [n_cells][12][2] {s1, s0} per slot: pass S's integer atomicAdd
    unsigned* misfits;     // += contributions pass S found beyond their slot's exponent (added nowhere)
    int32_t word_bits;     // m of the WHOLE image (c5_set_image), not of the context's rows
    int32_t keep_entries;  // pass S, the walk: 1 leaves the entry heads in place (another image follows); 0 hands them back cleared
};

// exps to "no contribution", words to zero and / or *misfits to zero
void launch_vertex_exact_clear(hipStream_t s, const VertexExactSums& x, int64_t n_cells, bool exps, bool words, bool misfits);
// pass E (sums false: leaves the entry heads in place) or pass S of vertex_walk's walk; both need launch_adjoint_walk(.., 1)
// first and read v.w, v.geo, v.grad_out and v.lambda only
void launch_vertex_exact_walk(hipStream_t s, const VertexParams& v, const VertexExactSums& x, bool sums);
// the same over bin_sort_resolve's lists (sorts them in place, as launch_vertex_resolve)
void launch_vertex_exact_resolve(hipStream_t s, const ResolveParams& r, const float2* grad_out, const VertexExactSums& x, bool sums);
// the caller's cell order -> the device's: x.exps[i][.] = exps[perm[i]][.] and x.words[i][.] = sums[perm[i]][.] (perm
// nullptr: the identity; exps or sums null: that block stays), and back
void launch_vertex_exact_gather(hipStream_t s, const int32_t* exps, const int64_t* sums, const int32_t* perm, int64_t n_cells,
                                const VertexExactSums& x);
void launch_vertex_exact_emit(hipStream_t s, const VertexExactSums& x, const int32_t* perm, int64_t n_cells, int32_t* exps, int64_t* sums);
// the point -> (cell, local vertex) incidence as CSR: inc_idx[inc_ptr[v] .. inc_ptr[v + 1]) = 4 * (device cell) + (vertex),
// ascending in the CALLER's cell index
struct VertexIncidence {
    const int32_t* ptr;  // [n_pts + 1]
    const int32_t* idx;  // [4 n_cells]
};
// words -> face_w (device order, one rounding per slot), face_w -> cell_triples [n_cells][4][3] (plain stores; separately
// rounded products and sums, a vertex's faces in ascending order), then per point the triples of its incidence list added
// in the list's order and grad_xyz[v] = M^T of that sum (a point of no cell, and a sum of zeros: exact +0.0)
void launch_vertex_exact_finish(hipStream_t s, const VertexExactSums& x, const MotionGeometry& geo, int64_t n_cells, double* face_w,
                                double* cell_triples, const VertexIncidence& inc, int64_t n_pts, const RotationList& R, double* grad_xyz);

// ---- batched vertex adjoint (c5_render_vertex_adjoint_batch*): one walk per ray for up to kc upstream images (kc: the
// chunk width, 4 or 8), after ONE pass 1

struct VertexBatchParams {
    WalkParams w;            // as VertexParams (the heads left in place by pass 1)
    MotionGeometry geo;
    const float2* grad_out;  // [n_used][n_local_rows][res_x] upstream weights: the chunk's first image
    int64_t image_px;        // pixels per image
    const double* lambda;    // pass 1's Lambda per pixel (launch_adjoint_walk(.., 1), once for every chunk)
    double* face_w;          // [n_cells][kc][4][3] device order, accumulated: VertexParams' face_w per image
    int32_t n_used;          // images of the chunk (<= kc)
    int32_t keep_entries;    // as TangentBatchParams
};

// vertex_walk (merged) for kc upstream images at once (needs pass 1 first): every contribution the double the single
// walk adds for that image alone, added in another order
void launch_vertex_walk_batch(hipStream_t s, int kc, const VertexBatchParams& v);

// launch_vertex_finish per image: face_w [n_cells][kc][12] -> grad_view[n_pts][3][kc] (zeroed by the caller; a point's
// components apart, the images of one component side by side), then grad_xyz[k0 + j][v] = M^T grad_view[v][.][j] for
// j < n_used
void launch_vertex_finish_batch(hipStream_t s, int kc, const MotionGeometry& geo, int64_t n_cells, const double* face_w, double* grad_view,
                                int64_t n_pts, const RotationList& R, int k0, int n_used, double* grad_xyz);

// ---- vertex tangent (c5_render_vertex_tangent*): the frame differentiated along a displacement per grid point, the
// operator launch_vertex_walk + launch_vertex_finish are the transpose of.  A face's depth at the pixel moves by
// dw = sum_i lambda_i (u_z - gx u_x - gy u_y)[vertex i], u = M d_xyz the points' view-space velocities.

// u_view[pt][j][3] = M d_xyz[k0 + j][pt] for j < n_used, zero for n_used <= j < kc: the caller's [K][n_pts][3]
// displacements -> kc view-space velocities per point (24 kc bytes, contiguous); M the linear part of the view R
void launch_vertex_velocity(hipStream_t s, int kc, const double* d_xyz, int64_t n_pts, int k0, int n_used, const RotationList& R,
                            double* u_view);

struct VertexTangentParams {
    WalkParams w;          // as TangentParams
    MotionGeometry geo;
    const double* u_view;  // [n_pts][kc][3] (launch_vertex_velocity)
    float2* out;           // [n_used][n_local_rows][res_x] (tau_dot, I_dot): the chunk's first image
    int64_t image_px;      // pixels per image
    int32_t n_used;        // fields of the chunk (<= kc)
    int32_t keep_entries;  // as TangentBatchParams
};

// motion_walk's walk for kc (4 or 8) per-point fields, both faces of every segment from the cell's vertices; every image
// bit for bit that of its field alone at either width; counts as tangent_walk does
void launch_vertex_tangent_walk(hipStream_t s, int kc, const VertexTangentParams& v);

// the same over bin_sort_resolve's lists for field j of u_view [n_pts][kc][3] (sorts them in place, as launch_tangent_resolve)
void launch_vertex_tangent_resolve(hipStream_t s, const ResolveParams& r, const double* u_view, int kc, int j, float2* out);

// ---- vertex Gauss-Newton product (c5_render_vertex_gn_product*): J^T W J v for per-point fields, J the vertex tangent's map

struct VertexGnWalkParams {
    WalkParams w;          // as VertexTangentParams
    MotionGeometry geo;
    const double* u_view;  // [n_pts][kc][3] (launch_vertex_velocity)
    const float2* weight;  // [n_local_rows][res_x] (w_tau, w_I), or nullptr: ones
    double* lambda;        // [n_local_px] out: pass 1's Lambda
    float2* g;             // [n_used][n_local_rows][res_x] out: w * (float)(tau_dot, I_dot), one fp32 multiply per channel
    float2* jv_out;        // the same shape, out: (tau_dot, I_dot) as launch_vertex_tangent_walk stores them; or nullptr
    int64_t image_px;      // pixels per image
    int32_t n_used;        // fields of the chunk (<= kc)
};

// vertex_tangent_walk's walk that is also pass 1 of the adjoint: leaves the entry heads in place and counts as pass 1 does
void launch_vertex_gn_walk_a(hipStream_t s, int kc, const VertexGnWalkParams& a);

// ---- ray matrix (c5_ray_matrix_*): per pixel the cells its ray crosses and the chord of each crossing, as CSR arrays

struct RayMatrixParams {
    WalkParams w;             // as TangentParams (unused by the *_resolve twins)
    int32_t* count;           // pass 1 out: [n_local_px] segments per pixel
    // pass 2: row p's element k goes to row_ptr[p] + k where that lies in [0, capacity) and k < row_ptr[p + 1] - row_ptr[p]
    const int64_t* row_ptr;   // [n_local_px + 1]
    int64_t capacity;
    const int32_t* perm;      // device order -> the caller's (nullptr: the identity)
    int32_t* col;             // [capacity] the cell, the caller's order
    double* dz;               // [capacity] the chord
    double* z_exit;           // [capacity] the segment's far end in view space, or nullptr
    unsigned* changed_rows;   // += rows whose length is not row_ptr's or that found no room below capacity
};

// pass 1: the count; leaves the entry heads in place and counts rays over the step bound and rays that skipped an entry as
// launch_adjoint_walk(.., 1) does.  pass 2 (after a per-view setup of its own): the fill, in the order the walk runs -
// deepest first; counts as pass 1 and hands the heads back cleared.  The step is adj::ray_step: the other derivatives' chords.
void launch_segment_walk(hipStream_t s, const RayMatrixParams& m, int pass);

// the same over bin_sort_resolve's lists: the count, and the fill (sorts them in place, as launch_adjoint_resolve)
void launch_segment_count_resolve(hipStream_t s, const ResolveParams& r, int32_t* count);
void launch_segment_fill_resolve(hipStream_t s, const ResolveParams& r, const RayMatrixParams& m);

// ---- ray Jacobian (c5_ray_jacobian_fill*): the ray matrix's structure with the adjoint's per-segment terms as values -
// per pixel and crossed cell d tau / d alpha = dz, d I / d alpha and d I / d Q, what adjoint_walk<2> adds to the cells' sums

struct JacobianRows {
    // row p's element k goes where RayMatrixParams says; any array may be null (not written)
    const int64_t* row_ptr;   // [n_local_px + 1]
    int64_t capacity;
    const int32_t* perm;      // device order -> the caller's (nullptr: the identity)
    int32_t* col;             // [capacity] the cell, the caller's order
    double* dz;               // [capacity] the chord: d tau / d alpha
    double* dI_da;            // [capacity] 0 for an inactive segment and for a clamped alpha
    double* dI_dq;            // [capacity] 0 for an inactive segment
    unsigned* changed_rows;   // += rows whose length is not row_ptr's or that found no room below capacity
};

// adjoint_walk<2>'s walk (after launch_adjoint_walk(.., 1): a.w and a.lambda are read) for the upstream image (0, 1) of
// every pixel, each lane's terms stored to its own row in the order the walk runs, deepest first; hands the heads back cleared
void launch_jacobian_walk(hipStream_t s, const AdjointParams& a, const JacobianRows& j);
// the same over bin_sort_resolve's lists: adjoint_resolve's arithmetic, segment_fill_resolve's rows
void launch_jacobian_fill_resolve(hipStream_t s, const ResolveParams& r, const JacobianRows& j);

// ---- shape Jacobian (c5_ray_shape_jacobian_fill*, c5_face_gradients*): the ray matrix's structure with the vertex adjoint's
// per-segment terms as values - d I / d dz, the chord's two faces and the pixel's barycentric coordinates in them - and, per
// cell and face, what turns a face's depth into its three points' coordinates

struct ShapeRows {
    // row p's element k goes where RayMatrixParams says; any array may be null (not written)
    const int64_t* row_ptr;   // [n_local_px + 1]
    int64_t capacity;
    double* dI_ddz;           // [capacity] T E (Q - a I_prev): the g_I factor of vertex_walk's G_k; 0 for an inactive segment
    uint8_t* faces;           // [capacity] exit face | entry face << 2 | 0x10 (exit contributes) | 0x20 (entry contributes)
    double* bary;             // [capacity][2][3] cell_faces_bary's (l0, l1, l2) of the exit face, then of the entry face
    unsigned* changed_rows;   // += rows whose length is not row_ptr's or that found no room below capacity
};

// vertex_walk's walk (after launch_adjoint_walk(.., 1): v.w, v.geo and v.lambda are read) for the upstream image (0, 1) of
// every pixel, each lane's terms stored to its own row in the order the walk runs, deepest first; hands the heads back cleared
void launch_shape_jacobian_walk(hipStream_t s, const VertexParams& v, const ShapeRows& j);
// the same over bin_sort_resolve's lists: vertex_resolve's arithmetic, segment_fill_resolve's rows
void launch_shape_jacobian_resolve(hipStream_t s, const ResolveParams& r, const ShapeRows& j);
// per cell (the caller's order through perm; nullptr: the identity) and face: the three points in face_plane's order and
// M^T (-gx, -gy, 1), zeros for an edge-on face; either array may be null
void launch_face_gradients(hipStream_t s, const MotionGeometry& geo, int64_t n_cells, const int32_t* perm, const RotationList& R,
                           int32_t* face_points, double* dw_dxyz);

// c5_update_scalars_device: alpha[i] = alpha_src[perm[i]], q[i] = q_src[perm[i]] (perm nullptr: the identity), and into
// stats[3] (zeroed by the caller): the bits of the largest alpha > 0, the complemented bits of the smallest alpha >=
// DBL_EPSILON, and 1 if some alpha is NaN (the host loop of c5_update_scalars, as an order-free max / min / or)
void launch_scalars_gather(hipStream_t s, const double* alpha_src, const double* q_src, const int32_t* perm, int64_t n, double* alpha,
                           double* q, unsigned long long* stats);

}  // namespace c5

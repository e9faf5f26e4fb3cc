// gfx950 kernels of the geometry derivatives: the frame differentiated with respect to where the grid is.  They walk as the
// scalar derivatives do (deriv_ray.hpp) and look a chord's two faces up by one rule (deriv_faces.hpp).
//
// The motion tangent (c5_render_motion_tangent*): the change of every pixel when the grid moves rigidly or affinely in
// view space with the velocity field u(p) = A p + b (a change of a view angle is one such field, c5_rotation_motion),
// the cells' scalars held.  The rays are parallel to z, and a face is a plane w = c + gx x + gy y: its depth at the
// pixel (x, y) changes by dw = u_z(P) - gx u_x(P) - gy u_y(P), P = (x, y, w) the point hit.  With ddz_k = dw_exit,k -
// dw_entry,k the change of the k-th chord,
//     tau_dot = sum_k alpha_k ddz_k                                              (raw alpha, every segment)
//     I_dot_k = E_k I_dot_{k-1} + E_k (Q_k - a_k I_{k-1}) ddz_k                  (active segments; dI_k / ddz_k)
// (a clamped alpha still moves with its chord: the clamp is on alpha).  Pixels that gain or lose coverage - silhouettes,
// a ray that crosses an edge into another list of cells - are not differentiated: the result is the derivative of the
// smooth piece the pixel is on.
//   motion_walk<KC>   tangent_walk's frame for KC fields: I, and per field I_dot, tau_dot and the dw of the face the ray
//                     entered its cell through.  An interior step hands the exit face's dw on; a boundary entry (the
//                     ray's start, a re-entry, a pick-up across a hanging-node interface) has no plane in the record of
//                     the cell entered and finds the face from the cell's four vertices (cell_slopes).  The fields are
//                     kernel arguments: uniform loads.
//   motion_resolve    the same over bin_sort_resolve's lists: both faces of every segment from the cell's vertices.
// No atomics, no pre-pass: bit-reproducible, like the tangent.
//
// The vertex adjoint (c5_render_vertex_adjoint*), the motion tangent's reverse mode per grid point, its batch over K
// upstream images (c5_render_vertex_adjoint_batch*) and the vertex tangent (c5_render_vertex_tangent*), the operator it is
// the transpose of, and the vertex Gauss-Newton product (c5_render_vertex_gn_product*: the vertex tangent's walk that is
// also the adjoint's first pass): their blocks further down.  The vertex adjoint's sums, single and batched, are fp64 atomics
// (global_atomic_add_f64: -munsafe-fp-atomics, build.py), added in arrival order: NOT bit-reproducible - unless
// "vertex_exact" is on: then the exact vertex adjoint sums' kernels run instead (their block below the vertex adjoint's).
// The shape Jacobian (c5_ray_shape_jacobian_fill*, c5_face_gradients*): the vertex adjoint's per-segment terms stored to
// the ray matrix's rows instead of summed, no atomics at all: its block at the end.
#include <type_traits>

#include "deriv_faces.hpp"
#include "deriv_lists.hpp"
#include "exact_sum.hpp"

namespace c5 {

// ---- motion tangent (c5_render_motion_tangent*) ---------------------------------------------------------------------------

// tangent_walk's frame for KC velocity fields.  Nothing is shared between the lanes: a lane leaves when its ray ends.
template <int KC>
__global__ __launch_bounds__(64) void motion_walk(MotionParams A) {
    using namespace adj;
    const WalkParams& P = A.w;
    Ray r;
    double I = 0.0, I_dot[KC], tau_dot[KC], dw_carry[KC];  // dw_carry: of the face the ray entered its cell through
#pragma unroll
    for (int j = 0; j < KC; ++j) I_dot[j] = tau_dot[j] = dw_carry[j] = 0.0;

    const EntryHead ent = ray_begin(r, P);

    // a boundary entry into `cell`: the entry face from the cell's vertices (rare: a few times per ray)
    auto enter = [&](int cell) {
        const CellSlopes cf = cell_slopes(A.geo, cell, r.x, r.y);
#pragma unroll
        for (int j = 0; j < KC; ++j) dw_carry[j] = cf.found ? face_dw(A.field[j], cf.in.gx, cf.in.gy, r.x, r.y, cf.in.w) : 0.0;
    };

    CellRegs cur;
    if (r.cell >= 0) {
        load_cell(cur, P.xrec, r.cell);
        enter(r.cell);
    }

    while (r.cell >= 0) {
        const SlopedExit se = step_geometry_sloped(cur, r.x, r.y);  // (ray_step's own geometry: the same operations, once)
        double dz, carry_next;
        const int nb = ray_step(r, P, ent, cur, dz, carry_next);
        CellRegs nxt;
        if (nb >= 0) load_cell(nxt, P.xrec, nb);

        const bool has_exit = se.w_exit < INFINITY;
        // nb, if any, lies behind the exit face (else it is a boundary entry)
        const bool through_face = has_exit && (se.w_out & kIdMask) != kNoCell;
        double dw_exit[KC];
#pragma unroll
        for (int j = 0; j < KC; ++j) dw_exit[j] = has_exit ? face_dw(A.field[j], se.gx, se.gy, r.x, r.y, se.w_exit) : 0.0;

        if (is_segment(dz)) {
            const double a_raw = cur.r6.a, a = cur.r6.b, q = cur.r7.b;  // a: clamped, 0 = inactive (cell_optics)
            double ddz[KC];
#pragma unroll
            for (int j = 0; j < KC; ++j) {
                ddz[j] = dw_exit[j] - dw_carry[j];
                tau_dot[j] = fma(a_raw, ddz[j], tau_dot[j]);  // d tau / d dz (raw alpha)
            }
            if (a != 0.0) {
                const double E = exp_nonpositive(-a * dz);
                const double dI_ddz = chord_dI(a, q, E, I);
#pragma unroll
                for (int j = 0; j < KC; ++j) I_dot[j] = fma(E, I_dot[j], dI_ddz * ddz[j]);
                I = segment_terms(a, q, dz, E, 1.0, I).I_next;
            }
        }
        if (nb >= 0) {
            if (through_face) {
#pragma unroll
                for (int j = 0; j < KC; ++j) dw_carry[j] = dw_exit[j];
            } else {
                enter(nb);
            }
        }
        ray_advance(r, nb, carry_next);
        cur = nxt;
    }

    if (r.in_image) {
#pragma unroll
        for (int j = 0; j < KC; ++j)
            if (j < A.n_used)
                A.out[static_cast<size_t>(j) * A.image_px + r.lp] = make_float2(static_cast<float>(tau_dot[j]), static_cast<float>(I_dot[j]));
    }
    if (!A.keep_entries) ray_clear_head(r, P);
    ray_count(r, P);
}

// tangent_resolve's frame: the same sort, the same back-to-front order; both faces of a segment from its cell's vertices.
__global__ __launch_bounds__(256) void motion_resolve(ResolveParams R, MotionField field, float2* __restrict__ out) {
    using namespace adj;
    const ListFrame f = list_frame<true>(R);
    if (!f.in_image) return;
    const GridView& g = R.g;
    const MotionGeometry geo{g.cell_vert, g.vx, g.vy, g.vz};
    double I = 0.0, I_dot = 0.0, tau_dot = 0.0;
    for (int i = f.n - 1; i >= 0; --i) {
        const int c = static_cast<int>(f.list[i].cell);
        const double dz = f.list[i].dz, q = g.q[c], a_raw = g.alpha[c];
        const ClampedAlpha ca = clamp_alpha(a_raw, R.alpha_limit);
        const CellSlopes cf = cell_slopes(geo, c, f.x, f.y);
        const double ddz = cf.found ? face_dw(field.f, cf.out.gx, cf.out.gy, f.x, f.y, cf.out.w) -
                                          face_dw(field.f, cf.in.gx, cf.in.gy, f.x, f.y, cf.in.w)
                                    : 0.0;
        tau_dot = fma(a_raw, ddz, tau_dot);
        if (ca.active) {
            const double E = exp(-ca.a * dz);
            I_dot = fma(E, I_dot, chord_dI(ca.a, q, E, I) * ddz);
            I = segment_terms(ca.a, q, dz, E, 1.0, I).I_next;
        }
    }
    out[f.lp] = make_float2(static_cast<float>(tau_dot), static_cast<float>(I_dot));
}

// ---- vertex adjoint (c5_render_vertex_adjoint*) ---------------------------------------------------------------------------
// The gradient of the frame with respect to the grid's points, the reverse mode of the motion tangent.  A segment's chord is
// dz_k = w_exit - w_entry and d loss / d dz_k = G_k = g_tau alpha_k + g_I T_k E_k (Q_k - a_k I_{k-1}) (the second term for
// active segments; T_k as the adjoint's pass 2 forms it).  A face's depth at the pixel is w = sum_i lambda_i z_i, lambda the
// barycentric coordinates of (x, y) in the projected triangle, and dw / d(x_i, y_i, z_i) = lambda_i (-gx, -gy, 1).
//   adjoint_walk<1>   Lambda per pixel, as for the adjoint.
//   vertex_walk       adjoint_walk<2>'s walk; per segment the two faces from the cell's vertices (cell_faces_bary) and
//                     +-G_k lambda added to face_w[cell][face][vertex of the face]: six atomics per segment, no slopes.
//   vertex_resolve    the same over bin_sort_resolve's lists: adj::vertex_resolve_body, the ONE list body of the vertex
//                     adjoint, with the sink LaneAtomics (the exact sums run it with LaneExact<SUMS>: their block below).
//                     The body finds a segment's (cell, G, two faces); the sink, per lane, says what they become.
//   vertex_finish     per cell: the four faces' slopes again, face_w times (-gx, -gy, 1) added to grad_view[point]; per
//                     point: M^T grad_view, M the linear part of the view, into the caller's array.
// Cells name the representatives of welded points, so a group's sum lands on its representative and the others stay 0.

namespace adj {

// +G lambda to the exit face's three vertices, -G lambda to the entry face's: six atomics
__device__ __forceinline__ void scatter_faces(double* __restrict__ face_w, int cell, double G, const CellFacesBary& cf) {
    double* const fw = face_w + static_cast<size_t>(cell) * 12;
    double* const o = fw + 3 * cf.out.f;
    double* const i = fw + 3 * cf.in.f;
    atomicAdd(o, G * cf.out.l0);
    atomicAdd(o + 1, G * cf.out.l1);
    atomicAdd(o + 2, G * cf.out.l2);
    atomicAdd(i, -G * cf.in.l0);
    atomicAdd(i + 1, -G * cf.in.l1);
    atomicAdd(i + 2, -G * cf.in.l2);
}

}  // namespace adj

// adjoint_walk<2>'s frame.  The cell's vertex ids are loaded beside its record, the vertices at the top of its step.
// MERGE false ("vertex_merge" 0): nothing is shared between the lanes, a lane leaves when its ray ends and adds its six
// values by itself - ten times slower on the C3 frame (neighbouring rays are in the same cells: the atomics of a step
// queue up on a few addresses).  MERGE true (the default): adjoint_walk_batch's reduction (deriv_ray.hpp: reduce_rows) - the
// loop is wave-uniform and every lane stages its cell's twelve values (six of them zero) in a row of LDS.
template <bool MERGE>
__global__ __launch_bounds__(64) void vertex_walk(VertexParams A) {
    using namespace adj;
    constexpr int kV = 12;
    __shared__ double stage[MERGE ? RowStage<kV>::kDoubles : 1];
    const WalkParams& P = A.w;
    Ray r;
    const int lane = r.lane;
    if (MERGE) stage_begin<kV>(stage, lane);
    double lam = 0.0, lam_total = 0.0, I = 0.0, g_tau = 0.0, g_I = 0.0;

    const EntryHead ent = ray_begin(r, P, [&] {
        const float2 g = A.grad_out[r.lp];
        g_tau = g.x;
        g_I = g.y;
        lam_total = A.lambda[r.lp];
        return g_tau != 0.0 || g_I != 0.0;
    });

    CellRegs cur;
    int4 cv = make_int4(0, 0, 0, 0);
    if (r.cell >= 0) {
        load_cell(cur, P.xrec, r.cell);
        cv = A.geo.cell_vert[r.cell];
    }

    for (;;) {
        const bool live = r.cell >= 0;
        if (MERGE ? __builtin_amdgcn_ballot_w64(live) == 0ull : !live) break;
        const int here = r.cell;
        bool emit = false;
        if (live) {
            double p[4][3];
            load_vertices(A.geo, cv, p);
            double dz, carry_next;
            const int nb = ray_step(r, P, ent, cur, dz, carry_next);
            CellRegs nxt;
            int4 cv_nxt = cv;
            if (nb >= 0) {
                load_cell(nxt, P.xrec, nb);
                cv_nxt = A.geo.cell_vert[nb];
            }

            if (is_segment(dz)) {
                const double a_raw = cur.r6.a, a = cur.r6.b, q = cur.r7.b;  // a: clamped, 0 = inactive (cell_optics)
                double G = g_tau * a_raw;                                  // d tau / d dz (raw alpha, every segment)
                if (a != 0.0) {
                    lam = lambda_add(lam, a, dz);  // (as in pass 1: Lambda_n == Lambda bit for bit, Lambda - Lambda_k >= 0)
                    const double T = exp_nonpositive(fmin(lam - lam_total, 0.0));
                    const double E = exp_nonpositive(-a * dz);
                    G = fma(g_I * T, chord_dI(a, q, E, I), G);  // G_k
                    I = segment_terms(a, q, dz, E, 1.0, I).I_next;
                }
                if (G != 0.0) {
                    const CellFacesBary cf = cell_faces_bary(p, r.x, r.y);
                    if (cf.found) {
                        if (!MERGE) {
                            scatter_faces(A.face_w, here, G, cf);
                        } else {
                            emit = true;
                            double* const row = stage_row<kV>(stage, lane);
#pragma unroll
                            for (int v = 0; v < kV; ++v) row[v] = 0.0;
                            row[3 * cf.out.f] = G * cf.out.l0;
                            row[3 * cf.out.f + 1] = G * cf.out.l1;
                            row[3 * cf.out.f + 2] = G * cf.out.l2;
                            row[3 * cf.in.f] = -G * cf.in.l0;
                            row[3 * cf.in.f + 1] = -G * cf.in.l1;
                            row[3 * cf.in.f + 2] = -G * cf.in.l2;
                        }
                    }
                }
            }
            ray_advance(r, nb, carry_next);
            cur = nxt;
            cv = cv_nxt;
        }
        if (MERGE) reduce_rows<kV>(stage, emit, here, lane, A.face_w);
    }

    ray_clear_head(r, P);
}

namespace adj {

// The list body of the vertex adjoint: adjoint_resolve's frame - the same sort, the same back-to-front order - with both
// faces of a segment from its cell's vertices.  The sink, per lane, says what a segment's (cell, G, two faces) becomes
// (segment) and what is left to do behind the list (finish): LaneAtomics here, LaneExact<SUMS> for the exact sums below.
template <class Sink>
__device__ __forceinline__ void vertex_resolve_body(const ResolveParams& R, const float2* __restrict__ grad_out, Sink sk) {
    constexpr bool kRows = Sink::kRows;  // (the shape Jacobian's rows: the upstream image is (0, 1) everywhere, grad_out is not read)
    double g_tau = 0.0, g_I = 0.0;
    const ListFrame f = list_frame<true>(R, [&](int64_t lp) {
        if constexpr (kRows) return true;
        const float2 gw = grad_out[lp];
        g_tau = gw.x;
        g_I = gw.y;
        return !(g_tau == 0.0 && g_I == 0.0);
    });
    if constexpr (kRows) sk.begin(f.in_image, static_cast<size_t>(f.lp));
    const GridView& g = R.g;
    const MotionGeometry geo{g.cell_vert, g.vx, g.vy, g.vz};
    const double lam_total = lambda_total(f.list, f.n, g, R.alpha_limit);
    double lam = 0.0, I = 0.0;
    for (int i = f.n - 1; i >= 0; --i) {
        const int c = static_cast<int>(f.list[i].cell);
        const double dz = f.list[i].dz, q = g.q[c], a_raw = g.alpha[c];
        const ClampedAlpha ca = clamp_alpha(a_raw, R.alpha_limit);
        double G = kRows ? 0.0 : g_tau * a_raw;  // (kRows: an inactive segment stores +0.0, whatever its raw alpha)
        if (ca.active) {
            lam = lambda_add(lam, ca.a, dz);
            const double T = exp(fmin(lam - lam_total, 0.0));
            const double E = exp(-ca.a * dz);
            if constexpr (kRows) G = T * chord_dI(ca.a, q, E, I);  // (G_k's g_I factor: d I / d dz_k)
            else G = fma(g_I * T, chord_dI(ca.a, q, E, I), G);
            I = segment_terms(ca.a, q, dz, E, 1.0, I).I_next;
        }
        if constexpr (kRows) {  // (the rows hold the segments the frame sums, as segment_fill_resolve's)
            if (is_segment(dz)) {
                double p[4][3];
                load_vertices(geo, g.cell_vert[c], p);
                sk.segment(c, G, cell_faces_bary(p, f.x, f.y));
            }
        } else if (G != 0.0) {
            double p[4][3];
            load_vertices(geo, g.cell_vert[c], p);
            const CellFacesBary cf = cell_faces_bary(p, f.x, f.y);
            if (cf.found) sk.segment(c, G, cf);
        }
    }
    sk.finish();
}

// the lane adds its six values by itself, fp64 atomics in arrival order
struct LaneAtomics {
    static constexpr bool kRows = false;
    double* __restrict__ face_w;
    __device__ __forceinline__ void segment(int cell, double G, const CellFacesBary& cf) const { scatter_faces(face_w, cell, G, cf); }
    __device__ __forceinline__ void finish() const {}
};

}  // namespace adj

__global__ __launch_bounds__(256) void vertex_resolve(ResolveParams R, const float2* __restrict__ grad_out, double* __restrict__ face_w) {
    adj::vertex_resolve_body(R, grad_out, adj::LaneAtomics{face_w});
}

namespace adj {

// d w / d (x, y, z) of a vertex of the face fp that holds the weight wk of the face's depth: wk (-gx, -gy, 1), view space
// (vertex_finish_cells adds it; face_gradients_kernel hands it out for wk = 1)
__device__ __forceinline__ void face_weight_gradient(const FacePlane& fp, double wk, double (&g)[3]) {
    g[0] = -fp.gx * wk;
    g[1] = -fp.gy * wk;
    g[2] = wk;
}

}  // namespace adj

// vertex_finish, per cell: the weights of its faces' vertices times (-gx, -gy, 1) to the points
__global__ __launch_bounds__(256) void vertex_finish_cells(MotionGeometry G, int64_t n_cells, const double* __restrict__ face_w,
                                                           double* __restrict__ grad_view) {
    const int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (i >= n_cells) return;
    double w[12];
    bool any = false;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        w[k] = face_w[i * 12 + k];
        any = any || w[k] != 0.0;
    }
    if (!any) return;
    const int4 cv = G.cell_vert[i];
    const int vid[4] = {cv.x, cv.y, cv.z, cv.w};
    double p[4][3];
    adj::load_vertices(G, cv, p);
#pragma unroll
    for (int f = 0; f < 4; ++f) {
        const FacePlane fp = face_plane(p, f);
        if (fp.kind == 0) continue;  // (edge-on: no ray crosses it, and it has no slopes)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double wk = w[3 * f + k];
            if (wk != 0.0) {
                double* const gv = grad_view + 3 * static_cast<int64_t>(vid[adj::face_vertex(f, k)]);
                double g[3];
                adj::face_weight_gradient(fp, wk, g);
                atomicAdd(gv, g[0]);
                atomicAdd(gv + 1, g[1]);
                atomicAdd(gv + 2, g[2]);
            }
        }
    }
}

// vertex_finish, per point: grad_xyz = M^T grad_view, the view's rotations transposed in reverse order (their centres
// drop out of the linear part)
__global__ __launch_bounds__(256) void vertex_finish_points(const double* __restrict__ grad_view, int64_t n_pts, RotationList R,
                                                            double* __restrict__ grad_xyz) {
    const int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (i >= n_pts) return;
    double gx = grad_view[3 * i], gy = grad_view[3 * i + 1], gz = grad_view[3 * i + 2];
    adj::rotate_linear<true>(R, gx, gy, gz);
    grad_xyz[3 * i] = gx;
    grad_xyz[3 * i + 1] = gy;
    grad_xyz[3 * i + 2] = gz;
}

// ---- exact vertex adjoint sums ("vertex_exact", c5_render_vertex_exact_*) --------------------------------------------------
// The vertex adjoint with no step that depends on an order of arrival.  A segment's six contributions are the doubles
// vertex_walk stages (+G lambda to the exit face's slots, -G lambda to the entry face's: the same G, the same
// cell_faces_bary, one rounding each); they are summed per (cell, slot) in the fixed-point format of exact_sum.hpp - a ray
// crosses a cell at most once and its two faces differ, so a slot receives at most one contribution per ray and the
// format's headroom holds as it does for the scalar sums.
//   adjoint_walk<1>             Lambda per pixel, as for the adjoint.
//   vertex_exact_walk<false>    pass E: vertex_walk<true>'s frame; per step a lane stages the exponents of its twelve values
//                               (kNone for the six slots it does not touch), reduce_rows_max takes the max per cell and
//                               slot into exps[cell][12].  Leaves the entry heads in place.
//   vertex_exact_walk<true>     pass S: the same walk again.  A lane loads the exponents of its six slots, rounds its six
//                               values onto their grids (exact::quantise: the only rounding) before any cross-lane work
//                               and stages 24 int64 words;
//                               reduce_rows_words adds them per cell into words[cell][12][2].  A value beyond its slot's
//                               exponent is added nowhere and counted in *misfits.
//   vertex_exact_resolve<.>     the same two over bin_sort_resolve's lists: vertex_resolve_body with the sink LaneExact<SUMS>,
//                               six atomicMax or twelve integer adds per segment.
//   vertex_exact_face_w         face_w[cell][slot] = exact::finish of the slot's words: one rounding.
//   vertex_exact_cells          per cell and local vertex the triple (sum -gx w, sum -gy w, sum w) over the faces holding
//                               the vertex, in ascending order of the face; products and sums rounded separately; plain
//                               stores into [n_cells][4][3].  Edge-on faces and zero weights are skipped, as in
//                               vertex_finish_cells.
//   vertex_exact_points         per point the triples of its (cell, vertex) incidences added in the list's order -
//                               ascending in the caller's cell index (derivatives.hip builds the list) - then M^T.
//   vertex_exact_clear / _gather / _emit   the staged calls' traffic between the caller's cell order and the device's.

namespace adj {

// a product and a sum that round by themselves, whatever stands around them (__dmul_rn / __dadd_rn are plain operators in
// a header compiled with contraction on: the pragma takes the permission away from these two)
__device__ __forceinline__ double mul_alone(double a, double b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ double add_alone(double a, double b) {
#pragma clang fp contract(off)
    return a + b;
}

// one face's three values against the exact sums, by the lane itself (the resolve twins): pass E's atomicMax or pass S's
// integer adds
template <bool SUMS>
__device__ __forceinline__ void exact_scatter_face(const VertexExactSums& X, int cell, double g, const FaceBary& fb, unsigned& bad) {
    const double l[3] = {fb.l0, fb.l1, fb.l2};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double v = mul_alone(g, l[k]);
        const size_t slot = 12 * static_cast<size_t>(cell) + 3 * fb.f + k;
        if (!SUMS) {
            const int32_t e = exact::exponent_of(v);
            if (e != exact::kNone) atomicMax(X.exps + slot, e);
        } else {
            const int32_t e = X.exps[slot];
            if (e == exact::kNotFinite) continue;  // (the slot stays NaN whatever is added: its words are not looked at)
            int64_t k1, k0;
            if (!exact::quantise(v, e, X.word_bits, k1, k0)) {
                ++bad;
                continue;
            }
            unsigned long long* const w = reinterpret_cast<unsigned long long*>(X.words) + 2 * slot;
            if (k1) atomicAdd(w, static_cast<unsigned long long>(k1));
            if (k0) atomicAdd(w + 1, static_cast<unsigned long long>(k0));
        }
    }
}

// vertex_resolve_body's sink for the exact sums: pass E (SUMS false) or pass S; misfits counted per lane, added once
template <bool SUMS>
struct LaneExact {
    static constexpr bool kRows = false;
    const VertexExactSums& X;
    unsigned bad = 0;
    __device__ __forceinline__ void segment(int cell, double G, const CellFacesBary& cf) {
        exact_scatter_face<SUMS>(X, cell, G, cf.out, bad);
        exact_scatter_face<SUMS>(X, cell, -G, cf.in, bad);
    }
    __device__ __forceinline__ void finish() const {
        if (SUMS && bad) atomicAdd(X.misfits, bad);
    }
};

}  // namespace adj

// vertex_walk<true>'s frame.  SUMS false: pass E; true: pass S.
template <bool SUMS>
__global__ __launch_bounds__(64) void vertex_exact_walk(VertexParams A, VertexExactSums X) {
    using namespace adj;
    using Word = typename std::conditional<SUMS, long long, int>::type;
    constexpr int kV = SUMS ? 24 : 12;
    __shared__ Word stage[WordStage<Word, kV>::kWords];
    const WalkParams& P = A.w;
    Ray r;
    const int lane = r.lane;
    word_stage_begin<Word, kV>(stage, lane, SUMS ? Word(0) : Word(exact::kNone));
    double lam = 0.0, lam_total = 0.0, I = 0.0, g_tau = 0.0, g_I = 0.0;
    unsigned bad = 0;

    const EntryHead ent = ray_begin(r, P, [&] {
        const float2 g = A.grad_out[r.lp];
        g_tau = g.x;
        g_I = g.y;
        lam_total = A.lambda[r.lp];
        return g_tau != 0.0 || g_I != 0.0;
    });

    CellRegs cur;
    int4 cv = make_int4(0, 0, 0, 0);
    if (r.cell >= 0) {
        load_cell(cur, P.xrec, r.cell);
        cv = A.geo.cell_vert[r.cell];
    }

    // wave-uniform loop (the reduction wants every lane): a lane whose ray has ended takes part with nothing to add
    for (;;) {
        const bool live = r.cell >= 0;
        if (__builtin_amdgcn_ballot_w64(live) == 0ull) break;
        const int here = r.cell;
        bool emit = false;
        if (live) {
            double p[4][3];
            load_vertices(A.geo, cv, p);
            double dz, carry_next;
            const int nb = ray_step(r, P, ent, cur, dz, carry_next);
            CellRegs nxt;
            int4 cv_nxt = cv;
            if (nb >= 0) {
                load_cell(nxt, P.xrec, nb);
                cv_nxt = A.geo.cell_vert[nb];
            }

            if (is_segment(dz)) {
                const double a_raw = cur.r6.a, a = cur.r6.b, q = cur.r7.b;  // a: clamped, 0 = inactive (cell_optics)
                double G = g_tau * a_raw;                                  // d tau / d dz (raw alpha, every segment)
                if (a != 0.0) {
                    lam = lambda_add(lam, a, dz);  // (as in pass 1: Lambda_n == Lambda bit for bit, Lambda - Lambda_k >= 0)
                    const double T = exp_nonpositive(fmin(lam - lam_total, 0.0));
                    const double E = exp_nonpositive(-a * dz);
                    G = fma(g_I * T, chord_dI(a, q, E, I), G);  // G_k
                    I = segment_terms(a, q, dz, E, 1.0, I).I_next;
                }
                if (G != 0.0) {
                    const CellFacesBary cf = cell_faces_bary(p, r.x, r.y);
                    if (cf.found) {
                        emit = true;
                        // vertex_walk's six doubles: exit +, entry -, each rounded once
                        Word* const row = word_stage_row<Word, kV>(stage, lane);
#pragma unroll
                        for (int v = 0; v < kV; ++v) row[v] = SUMS ? Word(0) : Word(exact::kNone);
                        const int so = 3 * cf.out.f, si = 3 * cf.in.f;
                        if constexpr (!SUMS) {
                            row[so] = exact::exponent_of(mul_alone(G, cf.out.l0));
                            row[so + 1] = exact::exponent_of(mul_alone(G, cf.out.l1));
                            row[so + 2] = exact::exponent_of(mul_alone(G, cf.out.l2));
                            row[si] = exact::exponent_of(mul_alone(-G, cf.in.l0));
                            row[si + 1] = exact::exponent_of(mul_alone(-G, cf.in.l1));
                            row[si + 2] = exact::exponent_of(mul_alone(-G, cf.in.l2));
                        } else {
                            // (a slot marked not finite stays NaN whatever is added: its words are not looked at)
                            auto put = [&](int slot, double v, int e) {
                                if (e == exact::kNotFinite) return;
                                int64_t k1, k0;
                                if (!exact::quantise(v, e, X.word_bits, k1, k0)) ++bad;
                                row[2 * slot] = k1;
                                row[2 * slot + 1] = k0;
                            };
                            // the two faces' exponents, loaded here: held in registers from the step before (twelve per
                            // cell, beside the next cell's record) the choice of a face's three compiled to a table in
                            // scratch, 52 to 112 bytes per lane (profiles/experiments.md)
                            const int32_t* const ex = X.exps + 12 * static_cast<size_t>(here);
                            const int eo0 = ex[so], eo1 = ex[so + 1], eo2 = ex[so + 2], ei0 = ex[si], ei1 = ex[si + 1], ei2 = ex[si + 2];
                            put(so, mul_alone(G, cf.out.l0), eo0);
                            put(so + 1, mul_alone(G, cf.out.l1), eo1);
                            put(so + 2, mul_alone(G, cf.out.l2), eo2);
                            put(si, mul_alone(-G, cf.in.l0), ei0);
                            put(si + 1, mul_alone(-G, cf.in.l1), ei1);
                            put(si + 2, mul_alone(-G, cf.in.l2), ei2);
                        }
                    }
                }
            }
            ray_advance(r, nb, carry_next);
            cur = nxt;
            cv = cv_nxt;
        }
        if constexpr (SUMS) reduce_rows_words(stage, emit, here, lane, X.words);
        else reduce_rows_max(stage, emit, here, lane, exact::kNone, X.exps);
    }

    if (SUMS) {
        if (bad) atomicAdd(X.misfits, bad);
        if (!X.keep_entries) ray_clear_head(r, P);
    }
}

// vertex_resolve_body with the exact sink: pass E (SUMS false) or pass S.  Reproducible as far as the list order is
// (segments of equal depth).
template <bool SUMS>
__global__ __launch_bounds__(256) void vertex_exact_resolve(ResolveParams R, const float2* __restrict__ grad_out, VertexExactSums X) {
    adj::vertex_resolve_body(R, grad_out, adj::LaneExact<SUMS>{X});
}

// one thread per (cell, slot)
__global__ __launch_bounds__(256) void vertex_exact_clear(VertexExactSums X, int64_t n_slots, int exps, int words, int misfits) {
    const int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (misfits && i == 0) *X.misfits = 0u;
    if (i >= n_slots) return;
    if (exps) X.exps[i] = exact::kNone;
    if (words) X.words[2 * i] = X.words[2 * i + 1] = 0ll;
}

// the caller's cell order -> the device's (TO_DEVICE) or back; one thread per (cell, slot); a null array stays out of it
template <bool TO_DEVICE>
__global__ __launch_bounds__(256) void vertex_exact_permute(VertexExactSums X, const int32_t* __restrict__ perm, int64_t n_cells,
                                                            int32_t* __restrict__ exps, long long* __restrict__ sums) {
    const int64_t t = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (t >= 12 * n_cells) return;
    const int64_t i = t / 12, k = t - 12 * i;
    const int64_t c = 12 * (perm ? static_cast<int64_t>(perm[i]) : i) + k;  // the caller's slot
    if (exps) {
        if (TO_DEVICE) X.exps[t] = exps[c];
        else exps[c] = X.exps[t];
    }
    if (sums) {
        if (TO_DEVICE) X.words[2 * t] = sums[2 * c], X.words[2 * t + 1] = sums[2 * c + 1];
        else sums[2 * c] = X.words[2 * t], sums[2 * c + 1] = X.words[2 * t + 1];
    }
}

__global__ __launch_bounds__(256) void vertex_exact_face_w(VertexExactSums X, int64_t n_slots, double* __restrict__ face_w) {
    const int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (i >= n_slots) return;
    face_w[i] = exact::finish(X.exps[i], X.words[2 * i], X.words[2 * i + 1], X.word_bits);
}

// per cell: the four vertices' triples.  Nothing here may be contracted: every product and every sum rounds by itself.
__global__ __launch_bounds__(256) void vertex_exact_cells(MotionGeometry G, int64_t n_cells, const double* __restrict__ face_w,
                                                          double* __restrict__ triples) {
    const int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (i >= n_cells) return;
    double w[12], t[4][3];
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        w[k] = face_w[i * 12 + k];
        t[k / 3][k % 3] = 0.0;
    }
    double p[4][3];
    adj::load_vertices(G, G.cell_vert[i], p);
#pragma unroll
    for (int f = 0; f < 4; ++f) {  // (ascending: a vertex's faces are added in this order)
        const FacePlane fp = face_plane(p, f);
        if (fp.kind == 0) continue;  // (edge-on: no ray crosses it, and it has no slopes)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double wk = w[3 * f + k];
            if (wk != 0.0) {
                double* const tv = t[adj::face_vertex(f, k)];
                tv[0] = adj::add_alone(tv[0], adj::mul_alone(-fp.gx, wk));
                tv[1] = adj::add_alone(tv[1], adj::mul_alone(-fp.gy, wk));
                tv[2] = adj::add_alone(tv[2], wk);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) triples[i * 12 + k] = t[k / 3][k % 3];
}

// per point: its incidences' triples in the list's order, then grad_xyz = M^T grad_view (vertex_finish_points' rotation).
// A point of no cell (a welded non-representative) and a sum of zeros give exact +0.0.
__global__ __launch_bounds__(256) void vertex_exact_points(VertexIncidence inc, const double* __restrict__ triples, int64_t n_pts,
                                                           RotationList R, double* __restrict__ grad_xyz) {
    const int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (i >= n_pts) return;
    double gx = 0.0, gy = 0.0, gz = 0.0;
    for (int32_t j = inc.ptr[i]; j < inc.ptr[i + 1]; ++j) {
        const double* const t = triples + 3 * static_cast<int64_t>(inc.idx[j]);
        gx = adj::add_alone(gx, t[0]);
        gy = adj::add_alone(gy, t[1]);
        gz = adj::add_alone(gz, t[2]);
    }
    if (gx == 0.0 && gy == 0.0 && gz == 0.0) gx = gy = gz = 0.0;  // (+0.0, whatever the signs of the zeros and of the view's cosines)
    else adj::rotate_linear<true>(R, gx, gy, gz);
    grad_xyz[3 * i] = gx;
    grad_xyz[3 * i + 1] = gy;
    grad_xyz[3 * i + 2] = gz;
}

// ---- batched vertex adjoint (c5_render_vertex_adjoint_batch*) --------------------------------------------------------------
// KC upstream images per walk.  Of a segment only g_tau and g_I differ from image to image: Lambda, T, E, chord_dI, the I
// recurrence and the two faces' lambda are the ray's.  With G_j = fma(g_I,j T, chord_dI, g_tau,j a_raw) an image costs two
// multiplies and one fma per segment and its share of the scatter.
//   vertex_walk_batch<KC>          vertex_walk<true>'s frame; per step a lane stages its twelve signed lambda and its KC
//                                  values G_j, and reduce_faces (deriv_ray.hpp) adds the cells' sums of lambda_v G_j to
//                                  face_w[cell][j][face][vertex of the face].  Every contribution is the double
//                                  vertex_walk stages for image j alone - the same two factors, rounded once - so a slice
//                                  differs from the single call in the order of the additions only.
//   vertex_finish_cells_batch<KC>  vertex_finish_cells per (cell, image), into grad_view[point][3][KC].
//   vertex_finish_points_batch<KC> vertex_finish_points per (point, image), into the caller's [K][n_pts][3].
// On bin_sort_resolve's lists the host runs vertex_resolve and vertex_finish per image.

// The images: float2 g[KC] in registers at KC = 4 (168 VGPRs, the third wave per SIMD), in LDS ([KC][64], one 8-byte
// column per lane) at KC = 8 - in registers the 8-wide kernel takes 186 VGPRs and loses that wave; from LDS it takes 154,
// its 15 024 bytes of LDS per workgroup still let ten waves onto a CU, and the K = 8 batch on the C3 frame ran in 26.6 ms
// against 27.5 (profiles/vertex_adjoint_batch_probe.md).
template <int KC>
__global__ __launch_bounds__(64) void vertex_walk_batch(VertexBatchParams A) {
    using namespace adj;
    using Stage = FaceStage<KC>;
    constexpr bool G_LDS = KC > 4;
    __shared__ double stage[Stage::kDoubles];
    __shared__ float2 gs[G_LDS ? 64 * KC : 1];
    const WalkParams& P = A.w;
    Ray r;
    const int lane = r.lane;
    face_stage_begin<KC>(stage, lane);
    double lam = 0.0, lam_total = 0.0, I = 0.0;
    float2 g[G_LDS ? 1 : KC];
    auto g_set = [&](int j, float2 v) {
        if constexpr (G_LDS) gs[j * 64 + lane] = v;
        else g[j] = v;
    };
    auto g_of = [&](int j) {
        if constexpr (G_LDS) return gs[j * 64 + lane];
        else return g[j];
    };
#pragma unroll
    for (int j = 0; j < KC; ++j) g_set(j, make_float2(0.0f, 0.0f));

    const EntryHead ent = ray_begin(r, P, [&] {
        bool any = false;
#pragma unroll
        for (int j = 0; j < KC; ++j)
            if (j < A.n_used) {
                const float2 gj = A.grad_out[static_cast<size_t>(j) * A.image_px + r.lp];
                g_set(j, gj);
                any = any || gj.x != 0.0f || gj.y != 0.0f;
            }
        lam_total = A.lambda[r.lp];
        return any;
    });

    CellRegs cur;
    int4 cv = make_int4(0, 0, 0, 0);
    if (r.cell >= 0) {
        load_cell(cur, P.xrec, r.cell);
        cv = A.geo.cell_vert[r.cell];
    }

    // wave-uniform loop (the reduction wants every lane): a lane whose ray has ended takes part with nothing to add
    for (;;) {
        const bool live = r.cell >= 0;
        if (__builtin_amdgcn_ballot_w64(live) == 0ull) break;
        const int here = r.cell;
        bool emit = false;
        if (live) {
            double p[4][3];
            load_vertices(A.geo, cv, p);
            double dz, carry_next;
            const int nb = ray_step(r, P, ent, cur, dz, carry_next);
            CellRegs nxt;
            int4 cv_nxt = cv;
            if (nb >= 0) {
                load_cell(nxt, P.xrec, nb);
                cv_nxt = A.geo.cell_vert[nb];
            }

            if (is_segment(dz)) {
                const double a_raw = cur.r6.a, a = cur.r6.b, q = cur.r7.b;  // a: clamped, 0 = inactive (cell_optics)
                double* const row = face_stage_row<KC>(stage, lane);
                bool any = false;
                if (a != 0.0) {
                    lam = lambda_add(lam, a, dz);  // (as in pass 1: Lambda_n == Lambda bit for bit, Lambda - Lambda_k >= 0)
                    const double T = exp_nonpositive(fmin(lam - lam_total, 0.0));
                    const double E = exp_nonpositive(-a * dz);
                    const double dI = chord_dI(a, q, E, I);
#pragma unroll
                    for (int j = 0; j < KC; ++j) {  // G_j, vertex_walk's operations
                        const float2 gj = g_of(j);
                        const double g_tau = gj.x, g_I = gj.y;
                        const double G = fma(g_I * T, dI, g_tau * a_raw);
                        row[Stage::kG + j] = G;
                        any = any || G != 0.0;
                    }
                    I = segment_terms(a, q, dz, E, 1.0, I).I_next;
                } else {
#pragma unroll
                    for (int j = 0; j < KC; ++j) {
                        const double g_tau = g_of(j).x;
                        const double G = g_tau * a_raw;  // d tau / d dz (raw alpha, every segment)
                        row[Stage::kG + j] = G;
                        any = any || G != 0.0;
                    }
                }
                if (any) {
                    const CellFacesBary cf = cell_faces_bary(p, r.x, r.y);
                    if (cf.found) {
                        emit = true;
#pragma unroll
                        for (int v = 0; v < 12; ++v) row[v] = 0.0;
                        row[3 * cf.out.f] = cf.out.l0;  // exit +, entry -: (-lambda) G is -(lambda G) to the bit
                        row[3 * cf.out.f + 1] = cf.out.l1;
                        row[3 * cf.out.f + 2] = cf.out.l2;
                        row[3 * cf.in.f] = -cf.in.l0;
                        row[3 * cf.in.f + 1] = -cf.in.l1;
                        row[3 * cf.in.f + 2] = -cf.in.l2;
                    }
                }
            }
            ray_advance(r, nb, carry_next);
            cur = nxt;
            cv = cv_nxt;
        }
        reduce_faces<KC>(stage, emit, here, lane, A.face_w);
    }

    if (!A.keep_entries) ray_clear_head(r, P);
}

// vertex_finish_cells for KC images: face_w[cell][KC][12] -> grad_view[point][3][KC].  One thread per (cell, image), each
// running vertex_finish_cells' atomics (the same products) for its image; the slopes are found per thread (the loads of a
// cell's KC threads are one).  The KC lanes of a cell add to KC neighbouring doubles - one component of one point - which is
// why grad_view keeps a point's components apart, [3][KC], not [KC][3].  Measured on the C3 frame at KC = 8 (profiles/
// vertex_adjoint_batch_probe.md): 2.28 ms, 1.45 single finishes.  One thread per cell with the slopes found once - its
// 36 KC atomics in turn, every lane of an instruction on another point - took 14.3 ms, more than eight single finishes
// (12.5), and the K = 8 batch 26.6 ms instead of 14.5; threads per (cell, image) into [KC][3], 18.9 ms.
template <int KC>
__global__ __launch_bounds__(256) void vertex_finish_cells_batch(MotionGeometry G, int64_t n_cells, int n_used,
                                                                 const double* __restrict__ face_w, double* __restrict__ grad_view) {
    const int64_t t = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (t >= n_cells * KC) return;
    const int64_t i = t / KC;
    const int j = static_cast<int>(t - i * KC);
    if (j >= n_used) return;
    double w[12];
    bool any = false;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        w[k] = face_w[t * 12 + k];
        any = any || w[k] != 0.0;
    }
    if (!any) return;
    const int4 cv = G.cell_vert[i];
    const int vid[4] = {cv.x, cv.y, cv.z, cv.w};
    double p[4][3];
    adj::load_vertices(G, cv, p);
#pragma unroll
    for (int f = 0; f < 4; ++f) {
        const FacePlane fp = face_plane(p, f);
        if (fp.kind == 0) continue;  // (edge-on: no ray crosses it, and it has no slopes)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double wk = w[3 * f + k];
            if (wk != 0.0) {
                double* const gv = grad_view + static_cast<int64_t>(vid[adj::face_vertex(f, k)]) * (3 * KC) + j;
                atomicAdd(gv, -fp.gx * wk);
                atomicAdd(gv + KC, -fp.gy * wk);
                atomicAdd(gv + 2 * KC, wk);
            }
        }
    }
}

// vertex_finish_points for KC images: grad_xyz[k0 + j][point] = M^T grad_view[point][.][j] for j < n_used.  One thread per
// (point, image).
template <int KC>
__global__ __launch_bounds__(256) void vertex_finish_points_batch(const double* __restrict__ grad_view, int64_t n_pts, int k0, int n_used,
                                                                  RotationList R, double* __restrict__ grad_xyz) {
    const int64_t t = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (t >= n_pts * KC) return;
    const int64_t i = t / KC;
    const int j = static_cast<int>(t - i * KC);
    if (j >= n_used) return;
    const double* const gv = grad_view + i * (3 * KC) + j;
    double gx = gv[0], gy = gv[KC], gz = gv[2 * KC];
    adj::rotate_linear<true>(R, gx, gy, gz);
    double* const out = grad_xyz + 3 * (static_cast<int64_t>(k0 + j) * n_pts + i);
    out[0] = gx;
    out[1] = gy;
    out[2] = gz;
}

// ---- vertex tangent (c5_render_vertex_tangent*) ---------------------------------------------------------------------------
// The forward mode of the vertex adjoint: the motion tangent with the velocity u(P) = sum_i lambda_i u_i interpolated from
// the face's three vertices instead of an affine field.  With u_v = M d_xyz[v] (M the linear part of the view) a face's
// depth at the pixel moves by dw = sum_i lambda_i (u_z - gx u_x - gy u_y)[vertex i], the chord by ddz = dw_exit - dw_entry,
// and the sums are the motion tangent's.
//   vertex_velocity<KC>        per point and field: u_view[pt][j] = M d_xyz[k0 + j][pt] (vertex_finish_points run forward).
//   vertex_tangent_walk<KC>    motion_walk's frame; per segment both faces from the cell's own vertices
//                              (cell_faces: cell_faces_bary's rule, with the slopes) - nothing is carried from the previous cell, as
//                              in vertex_walk, so the two are transposes of each other term by term.
//   vertex_tangent_resolve     the same over bin_sort_resolve's lists, one field per launch.
// No atomics, no LDS, no pre-pass: bit-reproducible, and a field's image does not depend on the width or on its place in
// the chunk (its arithmetic is vertex_ddz, the same for every field).

// u_view[pt][j] = M d_xyz[k0 + j][pt] for j < n_used, zero beyond: the view's rotations in forward order, linear part only
// (vertex_finish_points the other way).  One thread per point and field; a point's KC fields are contiguous.
template <int KC>
__global__ __launch_bounds__(256) void vertex_velocity(const double* __restrict__ d_xyz, int64_t n_pts, int k0, int n_used,
                                                       RotationList R, double* __restrict__ u_view) {
    const int64_t t = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (t >= n_pts * KC) return;
    const int64_t i = t / KC;
    const int j = static_cast<int>(t - i * KC);
    double ux = 0.0, uy = 0.0, uz = 0.0;
    if (j < n_used) {
        const double* const d = d_xyz + 3 * (static_cast<int64_t>(k0 + j) * n_pts + i);
        ux = d[0], uy = d[1], uz = d[2];
        adj::rotate_linear<false>(R, ux, uy, uz);
    }
    u_view[3 * t] = ux;
    u_view[3 * t + 1] = uy;
    u_view[3 * t + 2] = uz;
}

// motion_walk's frame over the per-point velocities.  The next record and the next cell's vertex ids are loaded before the
// arithmetic, the vertices at the top of the step (vertex_walk's order).  Nothing is shared between the lanes.  Params:
// VertexTangentParams, or VertexGnWalkParams for the walk that is also adjoint_walk<1> (vertex_gn_walk_a below).
template <int KC, class Params>
__device__ __forceinline__ void vertex_tangent_body(const Params& A) {
    using namespace adj;
    constexpr bool kGn = std::is_same<Params, VertexGnWalkParams>::value;
    const WalkParams& P = A.w;
    Ray r;
    double lam = 0.0;  // (kGn) Lambda, summed as adjoint_walk<1> sums it
    double I = 0.0, I_dot[KC], tau_dot[KC];
#pragma unroll
    for (int j = 0; j < KC; ++j) I_dot[j] = tau_dot[j] = 0.0;

    const EntryHead ent = ray_begin(r, P);

    CellRegs cur;
    int4 cv = make_int4(0, 0, 0, 0);
    if (r.cell >= 0) {
        load_cell(cur, P.xrec, r.cell);
        cv = A.geo.cell_vert[r.cell];
    }

    while (r.cell >= 0) {
        double p[4][3];
        load_vertices(A.geo, cv, p);
        double dz, carry_next;
        const int nb = ray_step(r, P, ent, cur, dz, carry_next);
        CellRegs nxt;
        int4 cv_nxt = cv;
        if (nb >= 0) {
            load_cell(nxt, P.xrec, nb);
            cv_nxt = A.geo.cell_vert[nb];
        }

        if (is_segment(dz)) {
            const double a_raw = cur.r6.a, a = cur.r6.b, q = cur.r7.b;  // a: clamped, 0 = inactive (cell_optics)
            const CellFaces cf = cell_faces(p, r.x, r.y);
            int vo[3], vi[3];
            face_points(cv, cf.b.out.f, vo);
            face_points(cv, cf.b.in.f, vi);
            double ddz[KC];
#pragma unroll
            for (int j = 0; j < KC; ++j) {
                ddz[j] = cf.b.found ? vertex_ddz(A.u_view + 3 * j, 3 * KC, vo, vi, cf) : 0.0;  // (faces not found: 0)
                tau_dot[j] = fma(a_raw, ddz[j], tau_dot[j]);                                         // d tau / d dz (raw alpha)
            }
            if (a != 0.0) {
                if (kGn) lam = lambda_add(lam, a, dz);  // (adjoint_walk<1>: pass B's running Lambda_k ends on this to the bit)
                const double E = exp_nonpositive(-a * dz);
                const double dI_ddz = chord_dI(a, q, E, I);
#pragma unroll
                for (int j = 0; j < KC; ++j) I_dot[j] = fma(E, I_dot[j], dI_ddz * ddz[j]);
                I = segment_terms(a, q, dz, E, 1.0, I).I_next;
            }
        }
        ray_advance(r, nb, carry_next);
        cur = nxt;
        cv = cv_nxt;
    }

    if constexpr (kGn) {
        if (r.in_image) {
            A.lambda[r.lp] = lam;
            const float2 w = A.weight ? A.weight[r.lp] : make_float2(1.0f, 1.0f);  // (loaded here, not held across the loop)
#pragma unroll
            for (int j = 0; j < KC; ++j)
                if (j < A.n_used) {
                    const float2 t = make_float2(static_cast<float>(tau_dot[j]), static_cast<float>(I_dot[j]));
                    if (A.jv_out) A.jv_out[static_cast<size_t>(j) * A.image_px + r.lp] = t;
                    A.g[static_cast<size_t>(j) * A.image_px + r.lp] = make_float2(__fmul_rn(w.x, t.x), __fmul_rn(w.y, t.y));
                }
            // (the entry heads stay in place for pass B)
        }
    } else {
        if (r.in_image) {
#pragma unroll
            for (int j = 0; j < KC; ++j)
                if (j < A.n_used)
                    A.out[static_cast<size_t>(j) * A.image_px + r.lp] = make_float2(static_cast<float>(tau_dot[j]), static_cast<float>(I_dot[j]));
        }
        if (!A.keep_entries) ray_clear_head(r, P);
    }
    ray_count(r, P);
}

template <int KC>
__global__ __launch_bounds__(64) void vertex_tangent_walk(VertexTangentParams A) {
    vertex_tangent_body<KC>(A);
}

// ---- vertex Gauss-Newton product (c5_render_vertex_gn_product*) -------------------------------------------------------------
// H v = J^T W J v, J the Jacobian of the image with respect to the grid's points (the vertex tangent's map, its transpose
// the vertex adjoint's), W a per-pixel, per-channel weight image.
//   vertex_gn_walk_a<KC>   vertex_tangent_walk<KC>'s walk that is also adjoint_walk<1>: per pixel Lambda, and per field
//                          g = w * (float)(tau_dot, I_dot), ONE fp32 multiply per channel - the bits a caller would get who
//                          multiplied render_vertex_tangent's image by the weights in fp32 and handed it to
//                          render_vertex_adjoint_batch.  A field's arithmetic is vertex_tangent_walk's: jv_out is its image
//                          to the bit.  Leaves the entry heads in place.
//   pass B                 vertex_walk / vertex_walk_batch<KC> / vertex_exact_walk as they are, on g and Lambda.
// On bin_sort_resolve's lists: vertex_tangent_resolve -> gn_weight (scalar_derivative_kernels.hip) -> the vertex adjoint's
// resolve per field.
template <int KC>
__global__ __launch_bounds__(64) void vertex_gn_walk_a(VertexGnWalkParams A) {
    vertex_tangent_body<KC>(A);
}

// motion_resolve's frame over a velocity per point.  u: field `j`'s first double of point 0 in a velocity buffer of `pitch`
// doubles per point.
__global__ __launch_bounds__(256) void vertex_tangent_resolve(ResolveParams R, const double* __restrict__ u, int pitch,
                                                              float2* __restrict__ out) {
    using namespace adj;
    const ListFrame f = list_frame<true>(R);
    if (!f.in_image) return;
    const GridView& g = R.g;
    const MotionGeometry geo{g.cell_vert, g.vx, g.vy, g.vz};
    double I = 0.0, I_dot = 0.0, tau_dot = 0.0;
    for (int i = f.n - 1; i >= 0; --i) {
        const int c = static_cast<int>(f.list[i].cell);
        const double dz = f.list[i].dz, q = g.q[c], a_raw = g.alpha[c];
        const ClampedAlpha ca = clamp_alpha(a_raw, R.alpha_limit);
        const int4 cv = g.cell_vert[c];
        double p[4][3];
        load_vertices(geo, cv, p);
        const CellFaces cf = cell_faces(p, f.x, f.y);
        double ddz = 0.0;
        if (cf.b.found) {
            int vo[3], vi[3];
            face_points(cv, cf.b.out.f, vo);
            face_points(cv, cf.b.in.f, vi);
            ddz = vertex_ddz(u, static_cast<size_t>(pitch), vo, vi, cf);
        }
        tau_dot = fma(a_raw, ddz, tau_dot);
        if (ca.active) {
            const double E = exp(-ca.a * dz);
            I_dot = fma(E, I_dot, chord_dI(ca.a, q, E, I) * ddz);
            I = segment_terms(ca.a, q, dz, E, 1.0, I).I_next;
        }
    }
    out[f.lp] = make_float2(static_cast<float>(tau_dot), static_cast<float>(I_dot));
}

// ---- shape Jacobian (c5_ray_shape_jacobian_fill*, c5_face_gradients*) --------------------------------------------------------
// The vertex adjoint's per-segment terms handed out instead of summed, over the ray matrix's rows: per segment
// d I / d dz_k (the g_I factor of vertex_walk's G_k; d tau / d dz_k is the cell's raw alpha, which the caller holds), the two
// faces the chord runs between and the pixel's barycentric coordinates in them (cell_faces_bary, to the bit).  What turns
// a face's depth into its vertices' coordinates depends on grid and view alone: face_gradients_kernel, per cell and face.
//   adjoint_walk<1>          Lambda per pixel, as for the adjoint.
//   shape_jacobian_walk      vertex_walk<false>'s frame for the upstream image (0, 1) at every pixel: nothing is shared between
//                            the lanes, a lane leaves when its ray ends.  EVERY segment is a row's element (the rows are
//                            segment_walk<2>'s), whatever its G_k: each lane appends to its own row with plain stores.
//   shape_jacobian_resolve   vertex_resolve_body with the sink ShapeRowStore, over bin_sort_resolve's lists.
//   face_gradients_kernel    one lane per cell of the device's order, stored through perm into the caller's.
// No atomics, no LDS, every lane owns its row: bit-reproducible.

namespace adj {

// The shape Jacobian's sink: a lane's row (RowCursor: inside [0, capacity) whatever row_ptr holds) and what it stores there.
struct ShapeRowStore {
    static constexpr bool kRows = true;
    ShapeRows J;
    RowCursor row;
    __device__ explicit ShapeRowStore(const ShapeRows& j) : J(j) {}
    __device__ __forceinline__ void begin(bool in_image, size_t lp) { row.begin(in_image, J.row_ptr, lp, J.capacity); }
    // faces: bits 0-1 the exit face, 2-3 the entry face, 4 / 5: the exit / entry face contributes (found: both or neither)
    __device__ __forceinline__ void segment(int, double dI_ddz, const CellFacesBary& cf) {
        row.put([&](long long at) {  // (plain stores, as store_segment's: ray_matrix_kernels.hip)
            if (J.dI_ddz) J.dI_ddz[at] = dI_ddz;
            if (J.faces) J.faces[at] = cf.found ? static_cast<uint8_t>(cf.out.f | (cf.in.f << 2) | 0x30) : static_cast<uint8_t>(0);
            if (J.bary) {
                double* const b = J.bary + 6 * at;
                b[0] = cf.found ? cf.out.l0 : 0.0;
                b[1] = cf.found ? cf.out.l1 : 0.0;
                b[2] = cf.found ? cf.out.l2 : 0.0;
                b[3] = cf.found ? cf.in.l0 : 0.0;
                b[4] = cf.found ? cf.in.l1 : 0.0;
                b[5] = cf.found ? cf.in.l2 : 0.0;
            }
        });
    }
    // by every lane of the wavefront, after its loop
    __device__ __forceinline__ void finish() const { row.finish(J.changed_rows); }
};

}  // namespace adj

// vertex_walk<false>'s frame (A.grad_out and A.face_w are not read).  The next record and the next cell's vertex ids are
// loaded before the arithmetic, the vertices at the top of the step.
__global__ __launch_bounds__(64) void shape_jacobian_walk(VertexParams A, ShapeRows J) {
    using namespace adj;
    const WalkParams& P = A.w;
    Ray r;
    ShapeRowStore sk(J);
    double lam = 0.0, lam_total = 0.0, I = 0.0;

    const EntryHead ent = ray_begin(r, P, [&] {
        lam_total = A.lambda[r.lp];
        return true;
    });
    sk.begin(r.in_image, r.lp);

    CellRegs cur;
    int4 cv = make_int4(0, 0, 0, 0);
    if (r.cell >= 0) {
        load_cell(cur, P.xrec, r.cell);
        cv = A.geo.cell_vert[r.cell];
    }

    while (r.cell >= 0) {
        double p[4][3];
        load_vertices(A.geo, cv, p);
        double dz, carry_next;
        const int nb = ray_step(r, P, ent, cur, dz, carry_next);
        CellRegs nxt;
        int4 cv_nxt = cv;
        if (nb >= 0) {
            load_cell(nxt, P.xrec, nb);
            cv_nxt = A.geo.cell_vert[nb];
        }

        if (is_segment(dz)) {
            const double a = cur.r6.b, q = cur.r7.b;  // a: clamped, 0 = inactive (cell_optics)
            double dI_ddz = 0.0;
            if (a != 0.0) {
                lam = lambda_add(lam, a, dz);  // (as in pass 1: Lambda_n == Lambda bit for bit, Lambda - Lambda_k >= 0)
                const double T = exp_nonpositive(fmin(lam - lam_total, 0.0));
                const double E = exp_nonpositive(-a * dz);
                dI_ddz = T * chord_dI(a, q, E, I);  // (G_k's g_I factor)
                I = segment_terms(a, q, dz, E, 1.0, I).I_next;
            }
            sk.segment(r.cell, dI_ddz, cell_faces_bary(p, r.x, r.y));
        }
        ray_advance(r, nb, carry_next);
        cur = nxt;
        cv = cv_nxt;
    }

    sk.finish();
    ray_clear_head(r, P);
}

__global__ __launch_bounds__(256) void shape_jacobian_resolve(ResolveParams R, ShapeRows J) {
    adj::vertex_resolve_body(R, nullptr, adj::ShapeRowStore(J));
}

// Per cell i of the device's order, into cell c = perm[i] of the caller's: face_points[c][f][k] the point of vertex k of face
// f (face_plane's order; cells name the representatives of welded points) and dw_dxyz[c][f] = M^T (-gx, -gy, 1), the face's
// slopes as vertex_finish_cells forms them (face_weight_gradient at weight 1), M the linear part of the view; an edge-on
// face (kind 0: no ray crosses it, and it has no slopes): exact zeros.  Either array may be null.
__global__ __launch_bounds__(256) void face_gradients_kernel(MotionGeometry G, int64_t n_cells, const int32_t* __restrict__ perm,
                                                             RotationList R, int32_t* __restrict__ face_points,
                                                             double* __restrict__ dw_dxyz) {
    const int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (i >= n_cells) return;
    const int64_t c = perm ? static_cast<int64_t>(perm[i]) : i;
    const int4 cv = G.cell_vert[i];
    double p[4][3];
    adj::load_vertices(G, cv, p);
#pragma unroll
    for (int f = 0; f < 4; ++f) {
        if (face_points) {
            int v[3];
            adj::face_points(cv, f, v);
#pragma unroll
            for (int k = 0; k < 3; ++k) face_points[12 * c + 3 * f + k] = v[k];
        }
        if (dw_dxyz) {
            const FacePlane fp = face_plane(p, f);
            double g[3] = {0.0, 0.0, 0.0};
            if (fp.kind != 0) {
                adj::face_weight_gradient(fp, 1.0, g);
                adj::rotate_linear<true>(R, g[0], g[1], g[2]);
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) dw_dxyz[12 * c + 3 * f + k] = g[k];
        }
    }
}

void launch_shape_jacobian_walk(hipStream_t s, const VertexParams& v, const ShapeRows& j) {
    if (const unsigned blocks = tile_blocks(v.w.im)) hipLaunchKernelGGL(shape_jacobian_walk, dim3(blocks), dim3(64), 0, s, v, j);
}

void launch_shape_jacobian_resolve(hipStream_t s, const ResolveParams& r, const ShapeRows& j) {
    if (const unsigned blocks = pixel_blocks(r.im)) hipLaunchKernelGGL(shape_jacobian_resolve, dim3(blocks), dim3(256), 0, s, r, j);
}

void launch_face_gradients(hipStream_t s, const MotionGeometry& geo, int64_t n_cells, const int32_t* perm, const RotationList& R,
                           int32_t* face_points, double* dw_dxyz) {
    if (n_cells > 0)
        hipLaunchKernelGGL(face_gradients_kernel, dim3(item_blocks(n_cells)), dim3(256), 0, s, geo, n_cells, perm, R, face_points, dw_dxyz);
}

void launch_motion_walk(hipStream_t s, int kc, const MotionParams& m) {
    if (const unsigned blocks = tile_blocks(m.w.im)) C5_LAUNCH_KC(motion_walk, kc, blocks, 64, s, m);
}

void launch_motion_resolve(hipStream_t s, const ResolveParams& r, const MotionField& field, float2* out) {
    if (const unsigned blocks = pixel_blocks(r.im)) hipLaunchKernelGGL(motion_resolve, dim3(blocks), dim3(256), 0, s, r, field, out);
}

void launch_vertex_walk(hipStream_t s, const VertexParams& v, bool merge) {
    const unsigned blocks = tile_blocks(v.w.im);
    if (!blocks) return;
    if (merge) hipLaunchKernelGGL(vertex_walk<true>, dim3(blocks), dim3(64), 0, s, v);
    else hipLaunchKernelGGL(vertex_walk<false>, dim3(blocks), dim3(64), 0, s, v);
}

void launch_vertex_resolve(hipStream_t s, const ResolveParams& r, const float2* grad_out, double* face_w) {
    if (const unsigned blocks = pixel_blocks(r.im)) hipLaunchKernelGGL(vertex_resolve, dim3(blocks), dim3(256), 0, s, r, grad_out, face_w);
}

void launch_vertex_finish(hipStream_t s, const MotionGeometry& geo, int64_t n_cells, const double* face_w, double* grad_view,
                          int64_t n_pts, const RotationList& R, double* grad_xyz) {
    if (n_cells > 0) hipLaunchKernelGGL(vertex_finish_cells, dim3(item_blocks(n_cells)), dim3(256), 0, s, geo, n_cells, face_w, grad_view);
    if (n_pts > 0) hipLaunchKernelGGL(vertex_finish_points, dim3(item_blocks(n_pts)), dim3(256), 0, s, grad_view, n_pts, R, grad_xyz);
}

void launch_vertex_exact_clear(hipStream_t s, const VertexExactSums& x, int64_t n_cells, bool exps, bool words, bool misfits) {
    hipLaunchKernelGGL(vertex_exact_clear, dim3(std::max(1u, item_blocks(12 * n_cells))), dim3(256), 0, s, x, 12 * n_cells, exps ? 1 : 0,
                       words ? 1 : 0, misfits ? 1 : 0);
}

void launch_vertex_exact_walk(hipStream_t s, const VertexParams& v, const VertexExactSums& x, bool sums) {
    const unsigned blocks = tile_blocks(v.w.im);
    if (!blocks) return;
    if (sums) hipLaunchKernelGGL(vertex_exact_walk<true>, dim3(blocks), dim3(64), 0, s, v, x);
    else hipLaunchKernelGGL(vertex_exact_walk<false>, dim3(blocks), dim3(64), 0, s, v, x);
}

void launch_vertex_exact_resolve(hipStream_t s, const ResolveParams& r, const float2* grad_out, const VertexExactSums& x, bool sums) {
    const unsigned blocks = pixel_blocks(r.im);
    if (!blocks) return;
    if (sums) hipLaunchKernelGGL(vertex_exact_resolve<true>, dim3(blocks), dim3(256), 0, s, r, grad_out, x);
    else hipLaunchKernelGGL(vertex_exact_resolve<false>, dim3(blocks), dim3(256), 0, s, r, grad_out, x);
}

void launch_vertex_exact_gather(hipStream_t s, const int32_t* exps, const int64_t* sums, const int32_t* perm, int64_t n_cells,
                                const VertexExactSums& x) {
    if (n_cells > 0)
        hipLaunchKernelGGL(vertex_exact_permute<true>, dim3(item_blocks(12 * n_cells)), dim3(256), 0, s, x, perm, n_cells,
                           const_cast<int32_t*>(exps), reinterpret_cast<long long*>(const_cast<int64_t*>(sums)));
}

void launch_vertex_exact_emit(hipStream_t s, const VertexExactSums& x, const int32_t* perm, int64_t n_cells, int32_t* exps, int64_t* sums) {
    if (n_cells > 0)
        hipLaunchKernelGGL(vertex_exact_permute<false>, dim3(item_blocks(12 * n_cells)), dim3(256), 0, s, x, perm, n_cells, exps,
                           reinterpret_cast<long long*>(sums));
}

void launch_vertex_exact_finish(hipStream_t s, const VertexExactSums& x, const MotionGeometry& geo, int64_t n_cells, double* face_w,
                                double* cell_triples, const VertexIncidence& inc, int64_t n_pts, const RotationList& R, double* grad_xyz) {
    if (n_cells > 0) {
        hipLaunchKernelGGL(vertex_exact_face_w, dim3(item_blocks(12 * n_cells)), dim3(256), 0, s, x, 12 * n_cells, face_w);
        hipLaunchKernelGGL(vertex_exact_cells, dim3(item_blocks(n_cells)), dim3(256), 0, s, geo, n_cells, face_w, cell_triples);
    }
    if (n_pts > 0) hipLaunchKernelGGL(vertex_exact_points, dim3(item_blocks(n_pts)), dim3(256), 0, s, inc, cell_triples, n_pts, R, grad_xyz);
}

void launch_vertex_walk_batch(hipStream_t s, int kc, const VertexBatchParams& v) {
    if (const unsigned blocks = tile_blocks(v.w.im)) C5_LAUNCH_KC(vertex_walk_batch, kc, blocks, 64, s, v);
}

void launch_vertex_finish_batch(hipStream_t s, int kc, const MotionGeometry& geo, int64_t n_cells, const double* face_w, double* grad_view,
                                int64_t n_pts, const RotationList& R, int k0, int n_used, double* grad_xyz) {
    if (n_cells > 0) C5_LAUNCH_KC(vertex_finish_cells_batch, kc, item_blocks(n_cells * kc), 256, s, geo, n_cells, n_used, face_w, grad_view);
    if (n_pts > 0) C5_LAUNCH_KC(vertex_finish_points_batch, kc, item_blocks(n_pts * kc), 256, s, grad_view, n_pts, k0, n_used, R, grad_xyz);
}

void launch_vertex_velocity(hipStream_t s, int kc, const double* d_xyz, int64_t n_pts, int k0, int n_used, const RotationList& R,
                            double* u_view) {
    if (n_pts <= 0) return;
    C5_LAUNCH_KC(vertex_velocity, kc, item_blocks(n_pts * kc), 256, s, d_xyz, n_pts, k0, n_used, R, u_view);
}

void launch_vertex_tangent_walk(hipStream_t s, int kc, const VertexTangentParams& v) {
    if (const unsigned blocks = tile_blocks(v.w.im)) C5_LAUNCH_KC(vertex_tangent_walk, kc, blocks, 64, s, v);
}

void launch_vertex_gn_walk_a(hipStream_t s, int kc, const VertexGnWalkParams& a) {
    if (const unsigned blocks = tile_blocks(a.w.im)) C5_LAUNCH_KC(vertex_gn_walk_a, kc, blocks, 64, s, a);
}

void launch_vertex_tangent_resolve(hipStream_t s, const ResolveParams& r, const double* u_view, int kc, int j, float2* out) {
    if (const unsigned blocks = pixel_blocks(r.im)) hipLaunchKernelGGL(vertex_tangent_resolve, dim3(blocks), dim3(256), 0, s, r, u_view + 3 * j, 3 * kc, out);
}

}  // namespace c5

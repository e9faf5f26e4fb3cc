// gfx950 kernels of the adjoint render: d(image)/d(alpha) and d(image)/d(Q) per cell, weighted by an upstream image.
//
// For one pixel, number its segments k = 1..n in the order line::integrate_ray_value_by_i processes them (line.cpp:206:
// from the deepest, z ascending; segment n is the one nearest the viewer), a_k = min(alpha_k, limit), active_k =
// !(a_k < DBL_EPSILON), E_k = exp(-a_k dz_k), I_k = E_k I_{k-1} + Q_k (1 - E_k) / a_k (inactive: I_k = I_{k-1}), and
// T_k = prod_{j > k} E_j = exp(-(Lambda - Lambda_k)), Lambda_k = sum_{j <= k} a_j dz_j over the active segments.  Then
//     d tau / d alpha_k = dz_k                                                 (raw alpha, every segment)
//     d I / d Q_k       = T_k (1 - E_k) / a_k                                  (active)
//     d I / d alpha_k   = T_k [Q_k (dz_k E_k / a_k - (1 - E_k) / a_k^2) - dz_k E_k I_{k-1}]   (active, alpha_k <= limit)
// and grad_alpha[c] = sum over the segments of c of g_tau dz + g_I dI/dalpha, grad_q[c] = sum of g_I dI/dQ, with the
// upstream weights (g_tau, g_I) of the segment's pixel.  Solid-marked pixels contribute nothing.
//
//   adjoint_walk<1>   the forward walk (walk_kernels.hip: walk_composite, "integration" 0: -z -> +z, the reference's
//                     order) once: Lambda per pixel.  Leaves the entry lists in place for ...
//   adjoint_walk<2>   ... the same walk again over exactly the same segments: I_{k-1} runs along, T_k from Lambda - Lambda_k,
//                     and the per-segment terms go to per-cell fp64 arrays (device order).  Lanes of a wavefront in the
//                     same cell at the same step are summed first: one pair of atomics per distinct cell and step.
//   adjoint_resolve   the same for the per-pixel sorted segment lists of bin_sort_resolve ("algorithm" 1).
//   adjoint_permute   device order -> the caller's (c5_upload_grid, "cell_order").
//
// The tangent (forward mode, c5_render_tangent*): the change (tau_dot, I_dot) of every pixel for a change (dalpha, dQ) of
// the cells' scalars, the same terms carried forward along the ray instead of scattered back:
//     tau_dot = sum_k dz_k dalpha_k                                              (raw alpha, every segment)
//     I_dot_k = E_k I_dot_{k-1} + dQ_k (1 - E_k) / a_k + dalpha'_k [Q_k (dz_k E_k / a_k - (1 - E_k) / a_k^2) - dz_k E_k I_{k-1}]
// (active segments; inactive: I_dot_k = I_dot_{k-1}; dalpha'_k = 0 where alpha_k is clamped), i.e. segment_terms with
// T = 1.  It is exactly the transpose of the adjoint: <g, J v> = <J^T g, v>.
//   tangent_gather    the caller's (dalpha, dQ) -> one 16-byte {dalpha, dQ} per cell in device order.
//   tangent_walk      the step of adjoint_walk<1> once, I, I_dot and tau_dot in registers: (tau_dot, I_dot) per pixel.
//   tangent_resolve   the same over the per-pixel sorted segment lists of bin_sort_resolve ("algorithm" 1).
// No atomics and no pre-pass: every pixel's sum runs in the reference's order on one lane, so the tangent IS
// bit-reproducible from run to run.
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
//                     the cell entered and finds the face from the cell's four vertices (cell_faces).  The fields are
//                     kernel arguments: uniform loads.
//   motion_resolve    the same over bin_sort_resolve's lists: both faces of every segment from the cell's vertices.
// No atomics, no pre-pass: bit-reproducible, like the tangent.
//
// The vertex adjoint (c5_render_vertex_adjoint*): the motion tangent's reverse mode, per grid point instead of per affine
// field - adjoint_walk<1>, then vertex_walk / vertex_resolve and vertex_finish (their block further down).
//
// The vertex tangent (c5_render_vertex_tangent*): the operator the vertex adjoint is the transpose of - the image's change
// for a displacement per grid point: vertex_velocity, then vertex_tangent_walk / vertex_tangent_resolve (their block
// further down).
//
// The ray matrix (c5_ray_matrix_*): the segments every render above sums over, themselves: segment_walk<1> counts them per
// pixel, segment_walk<2> stores (cell, dz, z_exit) per segment into CSR arrays; segment_count_resolve / segment_fill_resolve
// over bin_sort_resolve's lists (their block further down).
//
// Every walk kernel here (the batched and Gauss-Newton ones further down included) takes its rays through adj::Ray: ONE
// definition of the walk's step, of how a ray begins and of what it leaves behind.  The kernels differ in what they
// accumulate along the ray, and those that differ in nothing else share a body with a compile-time parameter
// (adjoint_walk_body: gn_diag_walk is pass 2 with squares; tangent_batch_body: gn_walk_a is tangent_walk_batch plus
// Lambda and the weighted store).  The *_resolve kernels share the reference's sort and its clamp of alpha.
//
// The sums are fp64 atomics, added in arrival order: the gradients are NOT bit-reproducible from run to run (the last bits
// move).  This file is compiled with -munsafe-fp-atomics (build.py): the adds are global_atomic_add_f64, no
// compare-and-swap loop.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <type_traits>

#include "adjoint.hpp"
#include "device_types.hpp"
#include "kernels.hpp"
#include "walk_common.hpp"

namespace c5 {
namespace adj {

// The walk's per-step helpers, as walk_kernels.hip has them (CellRegs, load_cell, step_geometry): that file stays as it is.
struct CellRegs {
    D2 r0, r1, r2, r3, r4, r5, r6, r7;  // ExitRecord: r0-r4 planes (+ nbr[0..1] in r4.b), r5.a = nbr[2] | flags, r6 / r7 optics
};

__device__ __forceinline__ void load_cell(CellRegs& c, const ExitRecord* rec, int cell) {
    const D2* rp = reinterpret_cast<const D2*>(rec + cell);
    c.r0 = rp[0];
    c.r1 = rp[1];
    c.r2 = rp[2];
    c.r3 = rp[3];
    c.r4 = rp[4];
    c.r5 = rp[5];
    c.r6 = rp[6];
    c.r7 = rp[7];
}

struct StepGeometry {
    double w_exit;   // +inf: the ray cannot leave (flat cell, edge-on faces): it ends here
    uint32_t w_out;  // neighbour word of the exit face
};

__device__ __forceinline__ StepGeometry step_geometry(const CellRegs& cur, double x, double y) {
    const double w0 = fma(cur.r0.b, x, fma(cur.r1.a, y, cur.r0.a));
    const double w1 = fma(cur.r2.a, x, fma(cur.r2.b, y, cur.r1.b));
    const double w2 = fma(cur.r3.b, x, fma(cur.r4.a, y, cur.r3.a));
    const unsigned long long n01 = __double_as_longlong(cur.r4.b);
    const uint32_t n0 = static_cast<uint32_t>(n01), n1 = static_cast<uint32_t>(n01 >> 32);
    const uint32_t n2 = static_cast<uint32_t>(__double_as_longlong(cur.r5.a));
    StepGeometry g;
    g.w_exit = fmin(w0, fmin(w1, w2));  // (never NaN: a candidate is a finite depth or +inf)
    g.w_out = (w0 == g.w_exit) ? n0 : (w1 == g.w_exit) ? n1 : n2;
    return g;
}

// step_geometry, and the exit face's slopes beside it (the motion tangent: how the face's depth moves)
struct SlopedExit {
    double w_exit;
    uint32_t w_out;
    double gx, gy;
};
__device__ __forceinline__ SlopedExit step_geometry_sloped(const CellRegs& cur, double x, double y) {
    const StepGeometry g = step_geometry(cur, x, y);
    const double w0 = fma(cur.r0.b, x, fma(cur.r1.a, y, cur.r0.a));
    const double w1 = fma(cur.r2.a, x, fma(cur.r2.b, y, cur.r1.b));
    SlopedExit s;
    s.w_exit = g.w_exit;
    s.w_out = g.w_out;
    s.gx = (w0 == g.w_exit) ? cur.r0.b : (w1 == g.w_exit) ? cur.r2.a : cur.r3.b;
    s.gy = (w0 == g.w_exit) ? cur.r1.a : (w1 == g.w_exit) ? cur.r2.b : cur.r4.a;
    return s;
}

// (1 - e^-x) / x = sum_m (-x)^m / (m + 1)!  for 0 <= x < 1/8 (truncation below 1e-19)
__device__ __forceinline__ double one_minus_exp_over_x(double x) {
    double p = 1.0 / 39916800.0;
    p = fma(p, -x, 1.0 / 3628800.0);
    p = fma(p, -x, 1.0 / 362880.0);
    p = fma(p, -x, 1.0 / 40320.0);
    p = fma(p, -x, 1.0 / 5040.0);
    p = fma(p, -x, 1.0 / 720.0);
    p = fma(p, -x, 1.0 / 120.0);
    p = fma(p, -x, 1.0 / 24.0);
    p = fma(p, -x, 1.0 / 6.0);
    p = fma(p, -x, 0.5);
    return fma(p, -x, 1.0);
}

// (x e^-x - (1 - e^-x)) / x^2 = sum_m (-1)^(m+1) (m + 1) / (m + 2)! x^m = -1/2 + x/3 - x^2/8 + ...  for 0 <= x < 1/8: the
// bracket of d I / d alpha divided by Q dz^2, which cancels to nothing when evaluated as written for small a dz
__device__ __forceinline__ double dalpha_bracket_series(double x) {
    double p = -1.0 / 43545600.0;
    p = fma(p, x, 1.0 / 3991680.0);
    p = fma(p, x, -1.0 / 403200.0);
    p = fma(p, x, 1.0 / 45360.0);
    p = fma(p, x, -1.0 / 5760.0);
    p = fma(p, x, 1.0 / 840.0);
    p = fma(p, x, -1.0 / 144.0);
    p = fma(p, x, 1.0 / 30.0);
    p = fma(p, x, -1.0 / 8.0);
    p = fma(p, x, 1.0 / 3.0);
    return fma(p, x, -0.5);
}

// Lambda's running sum, the same in every kernel that sums or re-sums it (pass 1 and pass 2 must agree to the bit).  A
// segment of optical depth beyond kLambdaCap counts as kLambdaCap: T = exp(-(Lambda - Lambda_k)) is 0 behind such a
// segment either way (exp_nonpositive is 0 below -746), and Lambda keeps the size of what can still be seen.  With
// alpha = 1e9 a single chord is worth 1e7, and Lambda - Lambda_k carried Lambda's rounding - 1e7 x 2^-53 per term, 2e-8
// of T and of every gradient seen through it - into the segments in front of that cell (tests/derivative_fuzz.py).
constexpr double kLambdaCap = 1024.0;
__device__ __forceinline__ double lambda_add(double lam, double a, double dz) {
    // (rounding is monotone: below the cap this is the fused sum to the bit; a NaN alpha stays a NaN)
    const double sum = fma(a, dz, lam), capped = lam + kLambdaCap;
    return capped < sum ? capped : sum;
}

// The terms of one active segment: d I / d Q and (unclamped) d I / d alpha, and I_k from I_{k-1}.  T: transmittance to the
// viewer; E: exp(-a dz).
struct SegmentTerms {
    double dI_dq, dI_da, I_next;
};
__device__ __forceinline__ SegmentTerms segment_terms(double a, double q, double dz, double E, double T, double I_prev) {
    const double x = a * dz;
    double s_over_q, bracket;  // (1 - E) / a;  Q (dz E / a - (1 - E) / a^2)
    if (x < -kSmallExpArg) {
        s_over_q = dz * one_minus_exp_over_x(x);
        bracket = q * dz * dz * dalpha_bracket_series(x);
    } else {
        s_over_q = (1.0 - E) / a;
        bracket = q * (dz * E - s_over_q) / a;
    }
    SegmentTerms t;
    t.dI_dq = T * s_over_q;
    t.dI_da = T * (bracket - dz * E * I_prev);
    t.I_next = fma(E, I_prev, q * s_over_q);
    return t;
}

// Adds (ga, gq) of every lane with `pending` set to grad_a / grad_q [its cell]: the lanes in one cell are summed across
// the wavefront first, and one lane adds the sums (one pair of atomics per distinct cell).  Every lane of the wavefront
// must be active.
__device__ __forceinline__ void scatter_wave(bool pending, int cell, double ga, double gq, double* __restrict__ grad_a,
                                             double* __restrict__ grad_q) {
    const int lane = static_cast<int>(threadIdx.x & 63);
    unsigned long long m = __builtin_amdgcn_ballot_w64(pending);
    while (m != 0ull) {
        const int leader = __builtin_ctzll(m);
        const int lc = __builtin_amdgcn_readlane(cell, leader);
        const bool mine = pending && cell == lc;
        double sa = mine ? ga : 0.0, sq = mine ? gq : 0.0;
        const unsigned long long mine_mask = __builtin_amdgcn_ballot_w64(mine);
        if (mine_mask != (1ull << leader)) {  // (wave-uniform) more than one lane in this cell
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                sa += __shfl_xor(sa, d);
                sq += __shfl_xor(sq, d);
            }
        }
        if (lane == leader) {
            atomicAdd(grad_a + lc, sa);
            atomicAdd(grad_q + lc, sq);
        }
        pending = pending && !mine;
        m &= ~mine_mask;
    }
}

// One ray of a walk kernel: one wavefront per 8x8 pixel tile, one lane per pixel (the walk's default tiling: neighbouring
// rays share cells, which is what the per-wave sums before the atomics live on).  Every walk kernel of this file takes its
// steps through this struct, and the step is that of walk_composite<*, 0> (walk_kernels.hip) operation for operation: the
// same segments, to the bit.  What a kernel accumulates along the ray stays in its own body.
//
// Three things a step needs are deliberately NOT members but locals of the kernel: the cell's record `cur`, the next
// one's `nxt` with the step's results (nb, dz, carry_next), and the pixel's EntryHead, handed over by value.  As members
// they end up on the stack, and next_entry's chain hop then reads through a pointer that is the stack or global memory
// (walk_common.hpp: next_entry).  The compiler's register count is sensitive to the shape of these helpers: check
// -Rpass-analysis=kernel-resource-usage after touching them (gn_walk_a<8> sits on its occupancy step, 168 VGPRs).
struct Ray {
    int lane = static_cast<int>(threadIdx.x);
    bool in_image = false;
    size_t lp = 0;  // the pixel among the context's rows
    double x = 0.0, y = 0.0;
    int cell = -1;  // the cell the ray is in; < 0: it has ended (or never began)
    double w_cur = -DBL_MAX, carry = 0.0, key_taken = -DBL_MAX;
    unsigned n_step = 0, overflow = 0;
    bool skipped = false;
};

// The lane's pixel, its entry head and the ray's first cell.  Where there is a ray - the pixel is in the image and not
// solid-marked (such a pixel shows the solid: line.cpp:177-179, nothing of the grid) - the kernel's `wanted` loads what
// else it needs of the pixel (r.lp) and says whether the ray is to be walked at all.
template <class Wanted>
__device__ __forceinline__ EntryHead ray_begin(Ray& r, const WalkParams& P, Wanted wanted) {
    const ImageParams& im = P.im;
    const int tiles_x = (im.res_x + 7) / 8;
    const int ty = static_cast<int>(blockIdx.x) / tiles_x, tx = static_cast<int>(blockIdx.x) - ty * tiles_x;
    const int col = tx * 8 + (r.lane & 7), lrow = ty * 8 + (r.lane >> 3);
    r.in_image = (col < im.res_x) && (lrow < im.n_local_rows);
    EntryHead ent{0, 0};
    if (r.in_image) {
        r.lp = static_cast<size_t>(lrow) * im.res_x + col;
        const uint32_t mv = P.mask ? P.mask[r.lp] : 0u;
        if (!mv) {
            r.x = P.Xtab[col];
            r.y = P.Ytab[global_row_of(im, lrow)];
            ent = load_entry_head(P.entry_head + r.lp);
            if (wanted() && ent.count > 0) r.cell = next_entry<true>(P, r.lp, ent, r.w_cur, r.carry, -DBL_MAX, -DBL_MAX, r.skipped);
            r.key_taken = r.w_cur;
        }
    }
    return ent;
}
__device__ __forceinline__ EntryHead ray_begin(Ray& r, const WalkParams& P) {
    return ray_begin(r, P, [] { return true; });
}

// One step up to the next cell's id (or -1): the exit, the step bound, the re-entry.  dz: the chord through the cell the
// ray is in.  The kernel then issues the next record's load (load_cell(nxt, P.xrec, nb)) BEFORE the segment's arithmetic
// and ends the step with ray_advance and cur = nxt.
__device__ __forceinline__ int ray_step(Ray& r, const WalkParams& P, EntryHead ent, const CellRegs& cur, double& dz, double& carry_next) {
    const StepGeometry sg = step_geometry(cur, r.x, r.y);
    ++r.n_step;
    const bool has_exit = sg.w_exit < INFINITY;
    dz = sg.w_exit - r.carry;
    int nb = -1;
    carry_next = r.carry;
    if (has_exit) {
        carry_next = sg.w_exit;
        r.w_cur = fmax(r.w_cur, sg.w_exit);
        const uint32_t id = sg.w_out & kIdMask;
        if (id != kNoCell) nb = static_cast<int>(id);
    }
    if (nb >= 0 && r.n_step >= P.max_steps) {
        r.overflow = 1;
        nb = -1;
    } else if (nb < 0 && !r.overflow) {
        nb = next_entry<true>(P, r.lp, ent, r.w_cur, carry_next, r.key_taken, has_exit ? sg.w_exit : -DBL_MAX, r.skipped);
        r.key_taken = r.w_cur;
    }
    return nb;
}

// a chord that is a segment of the pixel's sum
__device__ __forceinline__ bool is_segment(double dz) { return dz > 0.0 && dz < INFINITY; }

__device__ __forceinline__ void ray_advance(Ray& r, int nb, double carry_next) {
    r.cell = nb;
    r.carry = carry_next;
}

// the pixel's entry head cleared, as the walk leaves them (the last kernel over a view's entry lists)
__device__ __forceinline__ void ray_clear_head(const Ray& r, const WalkParams& P) {
    if (r.in_image) __builtin_nontemporal_store(0ll, reinterpret_cast<long long*>(P.entry_head + r.lp));
}

// rays over the step bound and rays that skipped an entry, counted once per view (the first kernel over its entry lists)
__device__ __forceinline__ void ray_count(const Ray& r, const WalkParams& P) {
    const unsigned s_ovf = static_cast<unsigned>(__popcll(__builtin_amdgcn_ballot_w64(r.overflow != 0u)));
    const unsigned s_skip = static_cast<unsigned>(__popcll(__builtin_amdgcn_ballot_w64(r.skipped)));
    if (r.lane == 0) {
        if (s_ovf) atomicAdd(&P.counters->walk_overflow, s_ovf);
        if (s_skip) atomicAdd(&P.counters->overlap_rays, s_skip);
    }
}

// Pass 1 (Lambda per pixel) and pass 2 (the scatter) of the adjoint; SQUARED: pass 2 with the segment's terms squared
// and A.grad_out the weights or nullptr for ones (gn_diag_walk).
template <int PASS, bool SQUARED>
__device__ __forceinline__ void adjoint_walk_body(const AdjointParams& A) {
    const WalkParams& P = A.w;
    Ray r;
    double lam = 0.0;                                         // Lambda_k so far
    double lam_total = 0.0, I = 0.0, g_tau = 0.0, g_I = 0.0;  // pass 2

    const EntryHead ent = ray_begin(r, P, [&] {
        if (PASS == 1) return true;
        const float2 g = (SQUARED && !A.grad_out) ? make_float2(1.0f, 1.0f) : A.grad_out[r.lp];
        g_tau = g.x;
        g_I = g.y;
        lam_total = A.lambda[r.lp];
        return g_tau != 0.0 || g_I != 0.0;
    });

    CellRegs cur;
    if (r.cell >= 0) load_cell(cur, P.xrec, r.cell);

    // wave-uniform loop (the scatter wants every lane): a lane whose ray has ended takes part with nothing to add
    for (;;) {
        const bool live = r.cell >= 0;
        if (__builtin_amdgcn_ballot_w64(live) == 0ull) break;
        bool emit = false;
        double ga = 0.0, gq = 0.0;
        const int here = r.cell;
        if (live) {
            double dz, carry_next;
            const int nb = ray_step(r, P, ent, cur, dz, carry_next);
            CellRegs nxt;
            if (nb >= 0) load_cell(nxt, P.xrec, nb);

            if (is_segment(dz)) {
                const double a_raw = cur.r6.a, a = cur.r6.b, q = cur.r7.b;  // a: clamped, 0 = inactive (cell_optics)
                if (PASS == 1) {
                    if (a != 0.0) lam = lambda_add(lam, a, dz);
                } else {
                    emit = true;
                    ga = g_tau * (SQUARED ? dz * dz : dz);  // d tau / d alpha (line.cpp:189: raw alpha, every segment)
                    if (a != 0.0) {
                        lam = lambda_add(lam, a, dz);  // (as in pass 1: Lambda_n == Lambda bit for bit, Lambda - Lambda_k >= 0)
                        const double T = exp_nonpositive(fmin(lam - lam_total, 0.0));
                        const double E = exp_nonpositive(-a * dz);
                        const SegmentTerms t = segment_terms(a, q, dz, E, T, I);
                        gq = g_I * (SQUARED ? t.dI_dq * t.dI_dq : t.dI_dq);
                        // (a clamped alpha does not move: line.cpp:216)
                        if (a == a_raw) ga = fma(g_I, SQUARED ? t.dI_da * t.dI_da : t.dI_da, ga);
                        I = t.I_next;
                    }
                }
            }
            ray_advance(r, nb, carry_next);
            cur = nxt;
        }
        if (PASS == 2) scatter_wave(emit, here, ga, gq, A.grad_a, A.grad_q);
    }

    if (PASS == 1) {
        if (r.in_image) A.lambda[r.lp] = lam;
        ray_count(r, P);
    } else {
        ray_clear_head(r, P);
    }
}

}  // namespace adj

template <int PASS>
__global__ __launch_bounds__(64) void adjoint_walk(AdjointParams A) {
    adj::adjoint_walk_body<PASS, false>(A);
}

// bin_sort_resolve's segments (exact_kernels.hip: Segment; c_api.hip checks the size)
struct alignas(8) AdjSegment {
    double z_hi;
    double dz;
    long long cell;
};
static_assert(sizeof(AdjSegment) == 24, "AdjSegment mirrors exact_kernels.hip's Segment");
size_t adjoint_segment_bytes() { return sizeof(AdjSegment); }

namespace adj {

// The reference's Shell sort of a pixel's list by descending z_hi (line.cpp:138), as resolve_pixels (exact_kernels.hip)
// runs it - with one addition: segments of EQUAL depth (interpenetrating components) are ordered by cell, so that a pixel's
// list, which bin_fill's atomics leave in another order every call, is the same list for every derivative call.
__device__ __forceinline__ void sort_segments(AdjSegment* list, int n) {
    for (int gap = n / 2; gap > 0; gap = (gap == 2) ? 1 : static_cast<int>(gap / 2.2)) {
        for (int i = gap; i < n; ++i) {
            const AdjSegment t = list[i];
            int j = i;
            while (j >= gap && (list[j - gap].z_hi < t.z_hi || (list[j - gap].z_hi == t.z_hi && list[j - gap].cell < t.cell))) {
                list[j] = list[j - gap];
                j -= gap;
            }
            list[j] = t;
        }
    }
}

// a = min(alpha, limit), and whether a segment of such a cell takes part in I (line.cpp:204-224)
struct ClampedAlpha {
    double a;
    bool active, clamped;
};
__device__ __forceinline__ ClampedAlpha clamp_alpha(double a_raw, double alpha_limit) {
    ClampedAlpha c;
    c.clamped = a_raw > alpha_limit;
    c.a = c.clamped ? alpha_limit : a_raw;
    c.active = !(c.a < DBL_EPSILON);
    return c;
}

// resolve_pixels (exact_kernels.hip) differentiated: its list sorted, the recurrence run from the back (i = n - 1 ... 0:
// k = n - i).  SQUARED: the segment's terms squared, `weights` nullptr for ones (gn_diag_resolve).
template <bool SQUARED>
__device__ __forceinline__ void adjoint_resolve_body(const GridView& g, const ImageParams& im, const int64_t* __restrict__ offs,
                                                     AdjSegment* __restrict__ segs, const uint32_t* __restrict__ mask,
                                                     double alpha_limit, const float2* __restrict__ weights,
                                                     double* __restrict__ grad_a, double* __restrict__ grad_q) {
    const int64_t lp = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    const int64_t n_px = static_cast<int64_t>(im.n_local_rows) * im.res_x;
    int n = 0;
    AdjSegment* list = segs;
    double g_tau = 0.0, g_I = 0.0, lam_total = 0.0;
    if (lp < n_px && !(mask && mask[lp])) {
        list = segs + offs[lp];
        n = static_cast<int>(offs[lp + 1] - offs[lp]);
        const float2 gw = (SQUARED && !weights) ? make_float2(1.0f, 1.0f) : weights[lp];
        g_tau = gw.x;
        g_I = gw.y;
        if (g_tau == 0.0 && g_I == 0.0) n = 0;
        sort_segments(list, n);
        for (int i = n - 1; i >= 0; --i) {  // Lambda, in the order the loop below runs
            const ClampedAlpha c = clamp_alpha(g.alpha[list[i].cell], alpha_limit);
            if (c.active) lam_total = lambda_add(lam_total, c.a, list[i].dz);
        }
    }
    double lam = 0.0, I = 0.0;
    // wave-uniform loop over the steps (the scatter wants every lane)
    for (int i = n - 1;; --i) {
        const bool live = i >= 0;
        if (__builtin_amdgcn_ballot_w64(live) == 0ull) break;
        int c = -1;
        double ga = 0.0, gq = 0.0;
        if (live) {
            c = static_cast<int>(list[i].cell);
            const double dz = list[i].dz, q = g.q[c];
            const ClampedAlpha ca = clamp_alpha(g.alpha[c], alpha_limit);
            const double a = ca.a;
            ga = g_tau * (SQUARED ? dz * dz : dz);
            if (ca.active) {
                lam = lambda_add(lam, a, dz);
                const double T = exp(fmin(lam - lam_total, 0.0));
                const double E = exp(-a * dz);
                const SegmentTerms t = segment_terms(a, q, dz, E, T, I);
                gq = g_I * (SQUARED ? t.dI_dq * t.dI_dq : t.dI_dq);
                if (!ca.clamped) ga = fma(g_I, SQUARED ? t.dI_da * t.dI_da : t.dI_da, ga);
                I = t.I_next;
            }
        }
        scatter_wave(live, c, ga, gq, grad_a, grad_q);
    }
}

}  // namespace adj

__global__ __launch_bounds__(256) void adjoint_resolve(GridView g, ImageParams im, const int64_t* __restrict__ offs,
                                                       AdjSegment* __restrict__ segs, const uint32_t* __restrict__ mask,
                                                       double alpha_limit, const float2* __restrict__ grad_out,
                                                       double* __restrict__ grad_a, double* __restrict__ grad_q) {
    adj::adjoint_resolve_body<false>(g, im, offs, segs, mask, alpha_limit, grad_out, grad_a, grad_q);
}

__global__ __launch_bounds__(256) void adjoint_permute(const double* __restrict__ ga_dev, const double* __restrict__ gq_dev,
                                                       const int32_t* __restrict__ perm, int64_t n, double* __restrict__ ga_out,
                                                       double* __restrict__ gq_out) {
    const int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (i >= n) return;
    const int64_t d = perm ? static_cast<int64_t>(perm[i]) : i;
    ga_out[d] = ga_dev[i];
    gq_out[d] = gq_dev[i];
}

// The tangent of one active segment's I: dQ (1 - E) / a + dalpha' (dI/dalpha at T = 1) + E I_dot_{k-1}; I_k from I_{k-1}.
__device__ __forceinline__ void tangent_step(double a, bool clamped, double q, double dz, double E, double da, double dq,
                                             double& I, double& I_dot) {
    const adj::SegmentTerms t = adj::segment_terms(a, q, dz, E, 1.0, I);
    double src = dq * t.dI_dq;
    if (!clamped) src = fma(da, t.dI_da, src);  // (a clamped alpha does not move: line.cpp:216)
    I_dot = fma(E, I_dot, src);
    I = t.I_next;
}

// Nothing is shared between the lanes, so a lane leaves the loop when its ray ends.  The cell's direction is loaded
// beside the next record.
__global__ __launch_bounds__(64) void tangent_walk(TangentParams A) {
    using namespace adj;
    const WalkParams& P = A.w;
    const D2* __restrict__ dir = reinterpret_cast<const D2*>(A.dir);
    Ray r;
    double I = 0.0, I_dot = 0.0, tau_dot = 0.0;

    const EntryHead ent = ray_begin(r, P);

    CellRegs cur;
    D2 d_cur{0.0, 0.0};
    if (r.cell >= 0) {
        load_cell(cur, P.xrec, r.cell);
        d_cur = dir[r.cell];
    }

    while (r.cell >= 0) {
        double dz, carry_next;
        const int nb = ray_step(r, P, ent, cur, dz, carry_next);
        CellRegs nxt;
        D2 d_nxt{0.0, 0.0};
        if (nb >= 0) {
            load_cell(nxt, P.xrec, nb);
            d_nxt = dir[nb];
        }

        if (is_segment(dz)) {
            const double a_raw = cur.r6.a, a = cur.r6.b, q = cur.r7.b;  // a: clamped, 0 = inactive (cell_optics)
            tau_dot = fma(dz, d_cur.a, tau_dot);  // d tau / d alpha (line.cpp:189: raw alpha)
            if (a != 0.0) tangent_step(a, a != a_raw, q, dz, exp_nonpositive(-a * dz), d_cur.a, d_cur.b, I, I_dot);
        }
        ray_advance(r, nb, carry_next);
        cur = nxt;
        d_cur = d_nxt;
    }

    if (r.in_image) A.out[r.lp] = make_float2(static_cast<float>(tau_dot), static_cast<float>(I_dot));
    ray_clear_head(r, P);
    ray_count(r, P);
}

// adjoint_resolve's twin: the same sort, the same back-to-front order, the tangent carried along.
__global__ __launch_bounds__(256) void tangent_resolve(GridView g, ImageParams im, const int64_t* __restrict__ offs,
                                                       AdjSegment* __restrict__ segs, const uint32_t* __restrict__ mask,
                                                       double alpha_limit, const double2* __restrict__ dir_v,
                                                       float2* __restrict__ out) {
    using namespace adj;
    const int64_t lp = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    const int64_t n_px = static_cast<int64_t>(im.n_local_rows) * im.res_x;
    if (lp >= n_px) return;
    const D2* __restrict__ dir = reinterpret_cast<const D2*>(dir_v);
    double I = 0.0, I_dot = 0.0, tau_dot = 0.0;
    if (!(mask && mask[lp])) {
        AdjSegment* const list = segs + offs[lp];
        const int n = static_cast<int>(offs[lp + 1] - offs[lp]);
        sort_segments(list, n);
        for (int i = n - 1; i >= 0; --i) {
            const int c = static_cast<int>(list[i].cell);
            const double dz = list[i].dz, q = g.q[c];
            const ClampedAlpha ca = clamp_alpha(g.alpha[c], alpha_limit);
            const D2 d = dir[c];
            tau_dot = fma(dz, d.a, tau_dot);
            if (ca.active) tangent_step(ca.a, ca.clamped, q, dz, exp(-ca.a * dz), d.a, d.b, I, I_dot);
        }
    }
    out[lp] = make_float2(static_cast<float>(tau_dot), static_cast<float>(I_dot));
}

// dir[i] = {d_alpha[perm[i]], d_q[perm[i]]} (perm nullptr: the identity; a null direction: 0)
__global__ __launch_bounds__(256) void tangent_gather(const double* __restrict__ d_alpha, const double* __restrict__ d_q,
                                                      const int32_t* __restrict__ perm, int64_t n, double2* __restrict__ dir) {
    const int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (i >= n) return;
    const int64_t c = perm ? static_cast<int64_t>(perm[i]) : i;
    D2 d;
    d.a = d_alpha ? d_alpha[c] : 0.0;
    d.b = d_q ? d_q[c] : 0.0;
    reinterpret_cast<D2*>(dir)[i] = d;
}

// ---- batches: KC directions (tangent) or upstream images (adjoint) per walk -------------------------------------------
// The ray's walk - geometry, entries, record loads, E and the segment terms - is shared; only the per-direction sums are
// KC-fold.  A tangent step runs tangent_step's operations on every direction's own registers, so each image is bit for
// bit tangent_walk's for that direction alone.

// dirs[i][j] = {d_alpha[k0 + j][perm[i]], d_q[k0 + j][perm[i]]}, zero beyond n_used (a null direction array: 0); one
// thread per (cell, direction): the 16-byte stores of a wavefront are contiguous
template <int KC>
__global__ __launch_bounds__(256) void tangent_gather_batch(const double* __restrict__ d_alpha, const double* __restrict__ d_q,
                                                            const int32_t* __restrict__ perm, int64_t n, int k0, int n_used,
                                                            double2* __restrict__ dirs) {
    const int64_t t = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (t >= n * KC) return;
    const int64_t i = t / KC;
    const int j = static_cast<int>(t - i * KC);
    const int64_t c = perm ? static_cast<int64_t>(perm[i]) : i;
    D2 d{0.0, 0.0};
    if (j < n_used) {
        const int64_t at = static_cast<int64_t>(k0 + j) * n + c;
        if (d_alpha) d.a = d_alpha[at];
        if (d_q) d.b = d_q[at];
    }
    reinterpret_cast<D2*>(dirs)[t] = d;
}

// tangent_walk for KC directions.  The cell's KC direction pairs are loaded at the top of its step (one 16 * KC-byte
// stretch) and consumed at its end, behind the geometry and the next record's loads.  Params: TangentBatchParams, or
// GnWalkParams for the walk that is also adjoint_walk<1> (gn_walk_a below).
template <int KC, class Params>
__device__ __forceinline__ void tangent_batch_body(const Params& A) {
    using namespace adj;
    constexpr bool kGn = std::is_same<Params, GnWalkParams>::value;
    const WalkParams& P = A.w;
    const D2* __restrict__ dirs = reinterpret_cast<const D2*>(A.dirs);
    Ray r;
    double lam = 0.0;  // (kGn) Lambda, summed as adjoint_walk<1> sums it
    double I = 0.0, I_dot[KC], tau_dot[KC];
#pragma unroll
    for (int j = 0; j < KC; ++j) I_dot[j] = tau_dot[j] = 0.0;

    const EntryHead ent = ray_begin(r, P);

    CellRegs cur;
    if (r.cell >= 0) load_cell(cur, P.xrec, r.cell);

    while (r.cell >= 0) {
        D2 d[KC];
#pragma unroll
        for (int j = 0; j < KC; ++j) d[j] = dirs[static_cast<size_t>(r.cell) * KC + j];
        double dz, carry_next;
        const int nb = ray_step(r, P, ent, cur, dz, carry_next);
        CellRegs nxt;
        if (nb >= 0) load_cell(nxt, P.xrec, nb);

        if (is_segment(dz)) {
            const double a_raw = cur.r6.a, a = cur.r6.b, q = cur.r7.b;  // a: clamped, 0 = inactive (cell_optics)
#pragma unroll
            for (int j = 0; j < KC; ++j) tau_dot[j] = fma(dz, d[j].a, tau_dot[j]);  // d tau / d alpha (raw alpha)
            if (a != 0.0) {
                if (kGn) lam = lambda_add(lam, a, dz);  // (adjoint_walk<1>: pass B's running Lambda_k ends on this to the bit)
                // tangent_step, its direction-free part once: segment_terms at T = 1, E
                const double E = exp_nonpositive(-a * dz);
                const SegmentTerms t = segment_terms(a, q, dz, E, 1.0, I);
                const bool clamped = a != a_raw;
#pragma unroll
                for (int j = 0; j < KC; ++j) {
                    double src = d[j].b * t.dI_dq;
                    if (!clamped) src = fma(d[j].a, t.dI_da, src);  // (a clamped alpha does not move: line.cpp:216)
                    I_dot[j] = fma(E, I_dot[j], src);
                }
                I = t.I_next;
            }
        }
        ray_advance(r, nb, carry_next);
        cur = nxt;
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
__global__ __launch_bounds__(64) void tangent_walk_batch(TangentBatchParams A) {
    tangent_batch_body<KC>(A);
}

// adjoint_walk<2> for KC upstream images.  Per step every lane has 2 KC values (ga_j, gq_j) for its cell.  They are staged
// in LDS, one row per lane; then, per distinct cell of the step, lanes v < 2 KC each sum column v over the cell's member
// rows (four rows per round, an all-zero row 64 filling up) and add it with one atomic: 2 KC atomics in one instruction,
// to one 16 KC-byte stretch of grad.  A 64-lane butterfly per value, as scatter_wave does for two, would cost 2 KC times
// its twelve cross-lane moves per shared cell.
template <int KC>
__global__ __launch_bounds__(64) void adjoint_walk_batch(AdjointBatchParams A) {
    using namespace adj;
    constexpr int kV = 2 * KC, kRow = kV + 1;  // (row pitch: an odd number of doubles)
    __shared__ double stage[65 * kRow];
    const WalkParams& P = A.w;
    Ray r;
    const int lane = r.lane;
    if (lane < kRow) stage[64 * kRow + lane] = 0.0;

    double lam = 0.0, lam_total = 0.0, I = 0.0;
    float2 g[KC];
#pragma unroll
    for (int j = 0; j < KC; ++j) g[j] = make_float2(0.0f, 0.0f);

    const EntryHead ent = ray_begin(r, P, [&] {
        bool any = false;
#pragma unroll
        for (int j = 0; j < KC; ++j)
            if (j < A.n_used) {
                g[j] = A.grad_out[static_cast<size_t>(j) * A.image_px + r.lp];
                any = any || g[j].x != 0.0f || g[j].y != 0.0f;
            }
        lam_total = A.lambda[r.lp];
        return any;
    });

    CellRegs cur;
    if (r.cell >= 0) load_cell(cur, P.xrec, r.cell);

    // wave-uniform loop (the reduction wants every lane): a lane whose ray has ended takes part with nothing to add
    for (;;) {
        const bool live = r.cell >= 0;
        if (__builtin_amdgcn_ballot_w64(live) == 0ull) break;
        bool emit = false;
        const int here = r.cell;
        if (live) {
            double dz, carry_next;
            const int nb = ray_step(r, P, ent, cur, dz, carry_next);
            CellRegs nxt;
            if (nb >= 0) load_cell(nxt, P.xrec, nb);

            if (is_segment(dz)) {
                const double a_raw = cur.r6.a, a = cur.r6.b, q = cur.r7.b;  // a: clamped, 0 = inactive (cell_optics)
                double ga[KC], gq[KC];
#pragma unroll
                for (int j = 0; j < KC; ++j) {
                    ga[j] = static_cast<double>(g[j].x) * dz;  // d tau / d alpha (line.cpp:189: raw alpha)
                    gq[j] = 0.0;
                }
                emit = true;
                if (a != 0.0) {
                    lam = lambda_add(lam, a, dz);
                    const double T = exp_nonpositive(fmin(lam - lam_total, 0.0));
                    const double E = exp_nonpositive(-a * dz);
                    const SegmentTerms t = segment_terms(a, q, dz, E, T, I);
                    const bool moves = a == a_raw;  // (a clamped alpha does not move: line.cpp:216)
#pragma unroll
                    for (int j = 0; j < KC; ++j) {
                        gq[j] = static_cast<double>(g[j].y) * t.dI_dq;
                        if (moves) ga[j] = fma(static_cast<double>(g[j].y), t.dI_da, ga[j]);
                    }
                    I = t.I_next;
                }
#pragma unroll
                for (int j = 0; j < KC; ++j) {
                    stage[lane * kRow + j] = ga[j];
                    stage[lane * kRow + KC + j] = gq[j];
                }
            }
            ray_advance(r, nb, carry_next);
            cur = nxt;
        }
        __syncthreads();  // (one wavefront: the rows are visible to every lane)
        unsigned long long m = __builtin_amdgcn_ballot_w64(emit);
        while (m != 0ull) {
            const int leader = __builtin_ctzll(m);
            const int lc = __builtin_amdgcn_readlane(here, leader);
            const unsigned long long members = __builtin_amdgcn_ballot_w64(emit && here == lc);
            if (lane < kV) {
                double s = 0.0;
                for (unsigned long long rows = members; rows != 0ull;) {
                    const int b0 = __builtin_ctzll(rows);
                    rows &= rows - 1;
                    const int b1 = rows ? __builtin_ctzll(rows) : 64;
                    rows &= rows - 1;
                    const int b2 = rows ? __builtin_ctzll(rows) : 64;
                    rows &= rows - 1;
                    const int b3 = rows ? __builtin_ctzll(rows) : 64;
                    rows &= rows - 1;
                    s += (stage[b0 * kRow + lane] + stage[b1 * kRow + lane]) + (stage[b2 * kRow + lane] + stage[b3 * kRow + lane]);
                }
                if (s != 0.0) atomicAdd(A.grad + static_cast<size_t>(lc) * kV + lane, s);
            }
            m &= ~members;
        }
        __syncthreads();  // (the rows are read before the next step writes them)
    }

    if (!A.keep_entries) ray_clear_head(r, P);
}

// one thread per (cell, image)
template <int KC>
__global__ __launch_bounds__(256) void adjoint_permute_batch(const double* __restrict__ grad, const int32_t* __restrict__ perm, int64_t n,
                                                             int k0, int n_used, double* __restrict__ ga_out, double* __restrict__ gq_out) {
    const int64_t t = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (t >= n * KC) return;
    const int64_t i = t / KC;
    const int j = static_cast<int>(t - i * KC);
    if (j >= n_used) return;
    const int64_t d = perm ? static_cast<int64_t>(perm[i]) : i;
    ga_out[static_cast<int64_t>(k0 + j) * n + d] = grad[i * (2 * KC) + j];
    gq_out[static_cast<int64_t>(k0 + j) * n + d] = grad[i * (2 * KC) + KC + j];
}

// ---- Gauss-Newton renders (c5_render_gn_product*, c5_render_gn_diagonal*) ------------------------------------------------
// H v = J^T W J v and diag(J^T W J), J the Jacobian of the image with respect to (alpha, Q), W a per-pixel, per-channel
// weight image.
//   gn_walk_a<KC>     tangent_walk_batch<KC>'s walk that is also adjoint_walk<1>: per pixel Lambda, and per direction
//                     g = w * (float)(tau_dot, I_dot), ONE fp32 multiply per channel - the bits a caller would get who
//                     multiplied render_tangent_batch's image by the weights in fp32 and handed it to
//                     render_adjoint_batch.  The fp32 intermediate is deliberate: with it the fused product IS that
//                     composition up to the order of pass B's atomics, which is what it is tested against.
//   pass B            adjoint_walk_batch<KC> as it is, on g and Lambda.
//   gn_diag_walk      adjoint_walk<2> with the segment's terms squared: d_alpha += w_tau dz^2 + w_I (dI/dalpha_k)^2,
//                     d_q += w_I (dI/dQ_k)^2 (a ray crosses a convex cell in at most one segment, so the Jacobian's entry
//                     of (pixel, cell) is that segment's term).
//   gn_weight / gn_diag_resolve   the same over bin_sort_resolve's lists ("algorithm" 1).

template <int KC>
__global__ __launch_bounds__(64) void gn_walk_a(GnWalkParams A) {
    tangent_batch_body<KC>(A);
}

// adjoint_walk<2> with squares (after adjoint_walk<1>: A.lambda).  A.grad_out holds the weights, or nullptr for ones.
__global__ __launch_bounds__(64) void gn_diag_walk(AdjointParams A) {
    adj::adjoint_walk_body<2, true>(A);
}

// g = w * t per channel, one fp32 multiply (gn_walk_a's store, for tangent_resolve's images); w nullptr: ones
__global__ __launch_bounds__(256) void gn_weight(const float2* __restrict__ t, const float2* __restrict__ w, int64_t n_px, int n_imgs,
                                                 float2* __restrict__ g) {
    const int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (i >= n_px * n_imgs) return;
    const float2 v = t[i];
    const float2 wp = w ? w[i % n_px] : make_float2(1.0f, 1.0f);
    g[i] = make_float2(__fmul_rn(wp.x, v.x), __fmul_rn(wp.y, v.y));
}

// adjoint_resolve's twin with squares (weights nullptr: ones)
__global__ __launch_bounds__(256) void gn_diag_resolve(GridView g, ImageParams im, const int64_t* __restrict__ offs,
                                                       AdjSegment* __restrict__ segs, const uint32_t* __restrict__ mask,
                                                       double alpha_limit, const float2* __restrict__ weight,
                                                       double* __restrict__ diag_a, double* __restrict__ diag_q) {
    adj::adjoint_resolve_body<true>(g, im, offs, segs, mask, alpha_limit, weight, diag_a, diag_q);
}

// c5_update_scalars_device: the gather into device order, and c5_update_scalars' three statistics as bit-pattern maxima
// (non-negative doubles order as their bits do; the smallest one is the largest complement).  A grid-stride loop over a
// few hundred workgroups, reduced per workgroup: one atomic per statistic and workgroup (atomics on one address are
// serialised at its L2 channel: one per wavefront cost 0.36 ms on a million cells).
constexpr int kScalarBlocks = 512;
__global__ __launch_bounds__(256) void scalars_gather(const double* __restrict__ alpha_src, const double* __restrict__ q_src,
                                                      const int32_t* __restrict__ perm, int64_t n, double* __restrict__ alpha,
                                                      double* __restrict__ q, unsigned long long* __restrict__ stats) {
    __shared__ unsigned long long part[3][4];
    unsigned long long top = 0ull, floor_c = 0ull, nan = 0ull;
    for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < n;
         i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const int64_t c = perm ? static_cast<int64_t>(perm[i]) : i;
        const double a = alpha_src[c];
        alpha[i] = a;
        q[i] = q_src[c];
        if (a > 0.0) top = max(top, static_cast<unsigned long long>(__double_as_longlong(a)));
        if (a >= DBL_EPSILON) floor_c = max(floor_c, ~static_cast<unsigned long long>(__double_as_longlong(a)));
        if (a != a) nan = 1ull;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        top = max(top, static_cast<unsigned long long>(__shfl_xor(top, d)));
        floor_c = max(floor_c, static_cast<unsigned long long>(__shfl_xor(floor_c, d)));
        nan = max(nan, static_cast<unsigned long long>(__shfl_xor(nan, d)));
    }
    const int wave = static_cast<int>(threadIdx.x >> 6);
    if ((threadIdx.x & 63) == 0) {
        part[0][wave] = top;
        part[1][wave] = floor_c;
        part[2][wave] = nan;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const unsigned long long* p = part[threadIdx.x];
        const unsigned long long v = max(max(p[0], p[1]), max(p[2], p[3]));
        if (v) atomicMax(stats + threadIdx.x, v);
    }
}

// ---- motion tangent (c5_render_motion_tangent*) ---------------------------------------------------------------------------

namespace adj {

// dw = u_z(P) - gx u_x(P) - gy u_y(P) at P = (x, y, w) for the field f = {A row-major, b}: how the depth of a face of
// slopes (gx, gy) moves at the pixel.  w is the innermost term: nothing of this is invariant along the ray, so the
// compiler keeps no per-field registers for it.
__device__ __forceinline__ double face_dw(const double* f, double gx, double gy, double x, double y, double w) {
    const double ux = fma(f[0], x, fma(f[1], y, fma(f[2], w, f[9])));
    const double uy = fma(f[3], x, fma(f[4], y, fma(f[5], w, f[10])));
    const double uz = fma(f[6], x, fma(f[7], y, fma(f[8], w, f[11])));
    return fma(-gy, uy, fma(-gx, ux, uz));
}

// The two faces of `cell` the ray of pixel (x, y) runs between, from the cell's view-space vertices: a tetrahedron is
// convex, so among the faces it lies ABOVE (face_plane: kind < 0; a ray along +z enters through one of them) the one
// met is the deepest at (x, y), and among those it lies below the shallowest.  Faces edge-on to rounding (kind 0) are
// never candidates.  found: both exist.
struct FaceAt {
    double w, gx, gy;
};
struct CellFaces {
    FaceAt in, out;
    bool found;
};
__device__ __forceinline__ CellFaces cell_faces(const MotionGeometry& G, int cell, double x, double y) {
    const int4 cv = G.cell_vert[cell];
    const int vid[4] = {cv.x, cv.y, cv.z, cv.w};
    double p[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        p[k][0] = G.vx[vid[k]];
        p[k][1] = G.vy[vid[k]];
        p[k][2] = G.vz[vid[k]];
    }
    CellFaces r;
    r.in = FaceAt{-INFINITY, 0.0, 0.0};
    r.out = FaceAt{INFINITY, 0.0, 0.0};
#pragma unroll
    for (int f = 0; f < 4; ++f) {
        const FacePlane fp = face_plane(p, f);
        const double w = fma(fp.gx, x - p[0][0], fma(fp.gy, y - p[0][1], fp.c));
        if (fp.kind < 0 && w > r.in.w) r.in = FaceAt{w, fp.gx, fp.gy};
        if (fp.kind > 0 && w < r.out.w) r.out = FaceAt{w, fp.gx, fp.gy};
    }
    r.found = r.in.w > -INFINITY && r.out.w < INFINITY;
    return r;
}

}  // namespace adj

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
        const CellFaces cf = cell_faces(A.geo, cell, r.x, r.y);
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
                const double dI_ddz = E * fma(-a, I, q);  // d I_k / d dz_k (the clamp is on alpha, not on the chord)
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

// tangent_resolve's twin: the same sort, the same back-to-front order; both faces of a segment from its cell's vertices.
__global__ __launch_bounds__(256) void motion_resolve(GridView g, ImageParams im, const double* __restrict__ Xtab,
                                                      const double* __restrict__ Ytab, const int64_t* __restrict__ offs,
                                                      AdjSegment* __restrict__ segs, const uint32_t* __restrict__ mask,
                                                      double alpha_limit, MotionField field, float2* __restrict__ out) {
    using namespace adj;
    const int64_t lp = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    const int64_t n_px = static_cast<int64_t>(im.n_local_rows) * im.res_x;
    if (lp >= n_px) return;
    double I = 0.0, I_dot = 0.0, tau_dot = 0.0;
    if (!(mask && mask[lp])) {
        const int lrow = static_cast<int>(lp / im.res_x);
        const double x = Xtab[lp - static_cast<int64_t>(lrow) * im.res_x], y = Ytab[global_row_of(im, lrow)];
        const MotionGeometry geo{g.cell_vert, g.vx, g.vy, g.vz};
        AdjSegment* const list = segs + offs[lp];
        const int n = static_cast<int>(offs[lp + 1] - offs[lp]);
        sort_segments(list, n);
        for (int i = n - 1; i >= 0; --i) {
            const int c = static_cast<int>(list[i].cell);
            const double dz = list[i].dz, q = g.q[c], a_raw = g.alpha[c];
            const ClampedAlpha ca = clamp_alpha(a_raw, alpha_limit);
            const CellFaces cf = cell_faces(geo, c, x, y);
            const double ddz = cf.found ? face_dw(field.f, cf.out.gx, cf.out.gy, x, y, cf.out.w) -
                                              face_dw(field.f, cf.in.gx, cf.in.gy, x, y, cf.in.w)
                                        : 0.0;
            tau_dot = fma(a_raw, ddz, tau_dot);
            if (ca.active) {
                const double E = exp(-ca.a * dz);
                I_dot = fma(E, I_dot, E * fma(-ca.a, I, q) * ddz);
                I = segment_terms(ca.a, q, dz, E, 1.0, I).I_next;
            }
        }
    }
    out[lp] = make_float2(static_cast<float>(tau_dot), static_cast<float>(I_dot));
}

// ---- vertex adjoint (c5_render_vertex_adjoint*) ---------------------------------------------------------------------------
// The gradient of the frame with respect to the grid's points, the reverse mode of the motion tangent.  A segment's chord is
// dz_k = w_exit - w_entry and d loss / d dz_k = G_k = g_tau alpha_k + g_I T_k E_k (Q_k - a_k I_{k-1}) (the second term for
// active segments; T_k as the adjoint's pass 2 forms it).  A face's depth at the pixel is w = sum_i lambda_i z_i, lambda the
// barycentric coordinates of (x, y) in the projected triangle, and dw / d(x_i, y_i, z_i) = lambda_i (-gx, -gy, 1).
//   adjoint_walk<1>   Lambda per pixel, as for the adjoint.
//   vertex_walk       adjoint_walk<2>'s walk; per segment the two faces from the cell's vertices (cell_faces_bary) and
//                     +-G_k lambda added to face_w[cell][face][vertex of the face]: six atomics per segment, no slopes.
//   vertex_resolve    the same over bin_sort_resolve's lists.
//   vertex_finish     per cell: the four faces' slopes again, face_w times (-gx, -gy, 1) added to grad_view[point]; per
//                     point: M^T grad_view, M the linear part of the view, into the caller's array.
// Cells name the representatives of welded points, so a group's sum lands on its representative and the others stay 0.

namespace adj {

__device__ __forceinline__ void load_vertices(const MotionGeometry& G, int4 cv, double (&p)[4][3]) {
    const int vid[4] = {cv.x, cv.y, cv.z, cv.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        p[k][0] = G.vx[vid[k]];
        p[k][1] = G.vy[vid[k]];
        p[k][2] = G.vz[vid[k]];
    }
}

// cell_faces' sibling: the same two faces by the same rule, as the face's index and the pixel's barycentric coordinates in
// its projected triangle (l0, l1, l2: the face's vertices in face_plane's order).  p: the cell's view-space vertices.
struct FaceBary {
    int f;
    double l0, l1, l2;
};
struct CellFacesBary {
    FaceBary in, out;
    bool found;
};
__device__ __forceinline__ CellFacesBary cell_faces_bary(const double (&p)[4][3], double x, double y) {
    constexpr int FV[4][3] = {{0, 1, 2}, {0, 1, 3}, {0, 2, 3}, {1, 2, 3}};
    double w_in = -INFINITY, w_out = INFINITY;
    // of the face chosen so far: the numerators of l1 and l2 and their denominator (divided once, behind the loop)
    double in_n1 = 0.0, in_n2 = 0.0, in_m = 1.0, out_n1 = 0.0, out_n2 = 0.0, out_m = 1.0;
    int f_in = 0, f_out = 0;
#pragma unroll
    for (int f = 0; f < 4; ++f) {
        const FacePlane fp = face_plane(p, f);
        const double w = fma(fp.gx, x - p[0][0], fma(fp.gy, y - p[0][1], fp.c));
        const double* a = p[FV[f][0]];
        const double* b = p[FV[f][1]];
        const double* c = p[FV[f][2]];
        const double m = (b[0] - a[0]) * (c[1] - a[1]) - (c[0] - a[0]) * (b[1] - a[1]);
        const double n1 = (x - a[0]) * (c[1] - a[1]) - (c[0] - a[0]) * (y - a[1]);
        const double n2 = (b[0] - a[0]) * (y - a[1]) - (x - a[0]) * (b[1] - a[1]);
        if (fp.kind < 0 && w > w_in) {
            w_in = w;
            f_in = f;
            in_n1 = n1, in_n2 = n2, in_m = m;
        }
        if (fp.kind > 0 && w < w_out) {
            w_out = w;
            f_out = f;
            out_n1 = n1, out_n2 = n2, out_m = m;
        }
    }
    CellFacesBary r;
    r.found = w_in > -INFINITY && w_out < INFINITY;
    r.in.f = f_in;
    r.in.l1 = in_n1 / in_m;
    r.in.l2 = in_n2 / in_m;
    r.in.l0 = 1.0 - r.in.l1 - r.in.l2;
    r.out.f = f_out;
    r.out.l1 = out_n1 / out_m;
    r.out.l2 = out_n2 / out_m;
    r.out.l0 = 1.0 - r.out.l1 - r.out.l2;
    return r;
}

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
// queue up on a few addresses).  MERGE true (the default): adjoint_walk_batch's reduction - the loop is wave-uniform, every lane stages its cell's
// twelve values (six of them zero) in a row of LDS, and per distinct cell of the step lanes v < 12 each sum column v over
// the cell's member rows and add it with one atomic.
template <bool MERGE>
__global__ __launch_bounds__(64) void vertex_walk(VertexParams A) {
    using namespace adj;
    constexpr int kV = 12, kRow = kV + 1;  // (row pitch: an odd number of doubles)
    __shared__ double stage[MERGE ? 65 * kRow : 1];
    const WalkParams& P = A.w;
    Ray r;
    const int lane = r.lane;
    if (MERGE && lane < kRow) stage[64 * kRow + lane] = 0.0;  // (an all-zero row 64 fills the rounds of four up)
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
                    G = fma(g_I * T, E * fma(-a, I, q), G);  // d I / d dz_k (the clamp is on alpha, not on the chord)
                    I = segment_terms(a, q, dz, E, 1.0, I).I_next;
                }
                if (G != 0.0) {
                    const CellFacesBary cf = cell_faces_bary(p, r.x, r.y);
                    if (cf.found) {
                        if (!MERGE) {
                            scatter_faces(A.face_w, here, G, cf);
                        } else {
                            emit = true;
                            double* const row = stage + lane * kRow;
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
        if (MERGE) {
            __syncthreads();  // (one wavefront: the rows are visible to every lane)
            unsigned long long m = __builtin_amdgcn_ballot_w64(emit);
            while (m != 0ull) {
                const int leader = __builtin_ctzll(m);
                const int lc = __builtin_amdgcn_readlane(here, leader);
                const unsigned long long members = __builtin_amdgcn_ballot_w64(emit && here == lc);
                if (lane < kV) {
                    double s = 0.0;
                    for (unsigned long long rows = members; rows != 0ull;) {
                        const int b0 = __builtin_ctzll(rows);
                        rows &= rows - 1;
                        const int b1 = rows ? __builtin_ctzll(rows) : 64;
                        rows &= rows - 1;
                        const int b2 = rows ? __builtin_ctzll(rows) : 64;
                        rows &= rows - 1;
                        const int b3 = rows ? __builtin_ctzll(rows) : 64;
                        rows &= rows - 1;
                        s += (stage[b0 * kRow + lane] + stage[b1 * kRow + lane]) + (stage[b2 * kRow + lane] + stage[b3 * kRow + lane]);
                    }
                    if (s != 0.0) atomicAdd(A.face_w + static_cast<size_t>(lc) * kV + lane, s);
                }
                m &= ~members;
            }
            __syncthreads();  // (the rows are read before the next step writes them)
        }
    }

    ray_clear_head(r, P);
}

// adjoint_resolve's twin: the same sort, the same back-to-front order; both faces of a segment from its cell's vertices.
__global__ __launch_bounds__(256) void vertex_resolve(GridView g, ImageParams im, const double* __restrict__ Xtab,
                                                      const double* __restrict__ Ytab, const int64_t* __restrict__ offs,
                                                      AdjSegment* __restrict__ segs, const uint32_t* __restrict__ mask,
                                                      double alpha_limit, const float2* __restrict__ grad_out,
                                                      double* __restrict__ face_w) {
    using namespace adj;
    const int64_t lp = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    const int64_t n_px = static_cast<int64_t>(im.n_local_rows) * im.res_x;
    if (lp >= n_px || (mask && mask[lp])) return;
    const float2 gw = grad_out[lp];
    const double g_tau = gw.x, g_I = gw.y;
    if (g_tau == 0.0 && g_I == 0.0) return;
    const int lrow = static_cast<int>(lp / im.res_x);
    const double x = Xtab[lp - static_cast<int64_t>(lrow) * im.res_x], y = Ytab[global_row_of(im, lrow)];
    const MotionGeometry geo{g.cell_vert, g.vx, g.vy, g.vz};
    AdjSegment* const list = segs + offs[lp];
    const int n = static_cast<int>(offs[lp + 1] - offs[lp]);
    sort_segments(list, n);
    double lam_total = 0.0;
    for (int i = n - 1; i >= 0; --i) {  // Lambda, in the order the loop below runs
        const ClampedAlpha c = clamp_alpha(g.alpha[list[i].cell], alpha_limit);
        if (c.active) lam_total = lambda_add(lam_total, c.a, list[i].dz);
    }
    double lam = 0.0, I = 0.0;
    for (int i = n - 1; i >= 0; --i) {
        const int c = static_cast<int>(list[i].cell);
        const double dz = list[i].dz, q = g.q[c], a_raw = g.alpha[c];
        const ClampedAlpha ca = clamp_alpha(a_raw, alpha_limit);
        double G = g_tau * a_raw;
        if (ca.active) {
            lam = lambda_add(lam, ca.a, dz);
            const double T = exp(fmin(lam - lam_total, 0.0));
            const double E = exp(-ca.a * dz);
            G = fma(g_I * T, E * fma(-ca.a, I, q), G);
            I = segment_terms(ca.a, q, dz, E, 1.0, I).I_next;
        }
        if (G != 0.0) {
            double p[4][3];
            load_vertices(geo, g.cell_vert[c], p);
            const CellFacesBary cf = cell_faces_bary(p, x, y);
            if (cf.found) scatter_faces(face_w, c, G, cf);
        }
    }
}

// vertex_finish, per cell: the weights of its faces' vertices times (-gx, -gy, 1) to the points
__global__ __launch_bounds__(256) void vertex_finish_cells(MotionGeometry G, int64_t n_cells, const double* __restrict__ face_w,
                                                           double* __restrict__ grad_view) {
    constexpr int FV[4][3] = {{0, 1, 2}, {0, 1, 3}, {0, 2, 3}, {1, 2, 3}};
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
                double* const gv = grad_view + 3 * static_cast<int64_t>(vid[FV[f][k]]);
                atomicAdd(gv, -fp.gx * wk);
                atomicAdd(gv + 1, -fp.gy * wk);
                atomicAdd(gv + 2, wk);
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
    for (int r = R.n - 1; r >= 0; --r) {
        const double c = R.cosv[r], s = R.sinv[r];
        if (R.axis[r] == 0) {  // y' = c y - s z, z' = s y + c z
            const double t = gy;
            gy = c * t + s * gz;
            gz = c * gz - s * t;
        } else {  // x' = c (x - x0) - s z + x0, z' = s (x - x0) + c z
            const double t = gx;
            gx = c * t + s * gz;
            gz = c * gz - s * t;
        }
    }
    grad_xyz[3 * i] = gx;
    grad_xyz[3 * i + 1] = gy;
    grad_xyz[3 * i + 2] = gz;
}

// ---- vertex tangent (c5_render_vertex_tangent*) ---------------------------------------------------------------------------
// The forward mode of the vertex adjoint: the motion tangent with the velocity u(P) = sum_i lambda_i u_i interpolated from
// the face's three vertices instead of an affine field.  With u_v = M d_xyz[v] (M the linear part of the view) a face's
// depth at the pixel moves by dw = sum_i lambda_i (u_z - gx u_x - gy u_y)[vertex i], the chord by ddz = dw_exit - dw_entry,
// and the sums are the motion tangent's.
//   vertex_velocity<KC>        per point and field: u_view[pt][j] = M d_xyz[k0 + j][pt] (vertex_finish_points run forward).
//   vertex_tangent_walk<KC>    motion_walk's frame; per segment both faces from the cell's own vertices
//                              (cell_faces_sloped: cell_faces_bary's rule, with the slopes) - nothing is carried from the
//                              previous cell, as in vertex_walk, so the two are transposes of each other term by term.
//   vertex_tangent_resolve     the same over bin_sort_resolve's lists, one field per launch.
// No atomics, no LDS, no pre-pass: bit-reproducible, and a field's image does not depend on the width or on its place in
// the chunk (its arithmetic is vertex_ddz, the same for every field).

namespace adj {

// cell_faces_bary's sibling: the same two faces by the same rule, with the slopes face_plane has for them.
struct CellFacesSloped {
    CellFacesBary b;
    double gx_in, gy_in, gx_out, gy_out;
};
__device__ __forceinline__ CellFacesSloped cell_faces_sloped(const double (&p)[4][3], double x, double y) {
    constexpr int FV[4][3] = {{0, 1, 2}, {0, 1, 3}, {0, 2, 3}, {1, 2, 3}};
    double w_in = -INFINITY, w_out = INFINITY;
    double in_n1 = 0.0, in_n2 = 0.0, in_m = 1.0, out_n1 = 0.0, out_n2 = 0.0, out_m = 1.0;
    CellFacesSloped r;
    r.gx_in = r.gy_in = r.gx_out = r.gy_out = 0.0;
    int f_in = 0, f_out = 0;
#pragma unroll
    for (int f = 0; f < 4; ++f) {
        const FacePlane fp = face_plane(p, f);
        const double w = fma(fp.gx, x - p[0][0], fma(fp.gy, y - p[0][1], fp.c));
        const double* a = p[FV[f][0]];
        const double* b = p[FV[f][1]];
        const double* c = p[FV[f][2]];
        const double m = (b[0] - a[0]) * (c[1] - a[1]) - (c[0] - a[0]) * (b[1] - a[1]);
        const double n1 = (x - a[0]) * (c[1] - a[1]) - (c[0] - a[0]) * (y - a[1]);
        const double n2 = (b[0] - a[0]) * (y - a[1]) - (x - a[0]) * (b[1] - a[1]);
        if (fp.kind < 0 && w > w_in) {
            w_in = w;
            f_in = f;
            in_n1 = n1, in_n2 = n2, in_m = m;
            r.gx_in = fp.gx, r.gy_in = fp.gy;
        }
        if (fp.kind > 0 && w < w_out) {
            w_out = w;
            f_out = f;
            out_n1 = n1, out_n2 = n2, out_m = m;
            r.gx_out = fp.gx, r.gy_out = fp.gy;
        }
    }
    r.b.found = w_in > -INFINITY && w_out < INFINITY;
    r.b.in.f = f_in;
    r.b.in.l1 = in_n1 / in_m;
    r.b.in.l2 = in_n2 / in_m;
    r.b.in.l0 = 1.0 - r.b.in.l1 - r.b.in.l2;
    r.b.out.f = f_out;
    r.b.out.l1 = out_n1 / out_m;
    r.b.out.l2 = out_n2 / out_m;
    r.b.out.l0 = 1.0 - r.b.out.l1 - r.b.out.l2;
    return r;
}

// the three points of face f of the cell cv, in face_plane's order
__device__ __forceinline__ void face_points(int4 cv, int f, int (&v)[3]) {
    v[0] = f == 3 ? cv.y : cv.x;
    v[1] = f <= 1 ? cv.y : cv.z;
    v[2] = f == 0 ? cv.z : cv.w;
}

// lambda (u_z - gx u_x - gy u_y) of one vertex: u = its three doubles of one field
__device__ __forceinline__ double vertex_dw(const double* __restrict__ u, double l, double gx, double gy) {
    return l * fma(-gy, u[1], fma(-gx, u[0], u[2]));
}

// ddz = dw_exit - dw_entry of one field: six gathers of three doubles.  u: the field's first double of point 0, pitch
// doubles from point to point.  This is ALL of a field's arithmetic that touches the velocities: the same at every width.
__device__ __forceinline__ double vertex_ddz(const double* __restrict__ u, size_t pitch, const int (&vo)[3], const int (&vi)[3],
                                             const CellFacesSloped& cf) {
    const double dw_out = vertex_dw(u + vo[0] * pitch, cf.b.out.l0, cf.gx_out, cf.gy_out) +
                          vertex_dw(u + vo[1] * pitch, cf.b.out.l1, cf.gx_out, cf.gy_out) +
                          vertex_dw(u + vo[2] * pitch, cf.b.out.l2, cf.gx_out, cf.gy_out);
    const double dw_in = vertex_dw(u + vi[0] * pitch, cf.b.in.l0, cf.gx_in, cf.gy_in) +
                         vertex_dw(u + vi[1] * pitch, cf.b.in.l1, cf.gx_in, cf.gy_in) +
                         vertex_dw(u + vi[2] * pitch, cf.b.in.l2, cf.gx_in, cf.gy_in);
    return dw_out - dw_in;
}

}  // namespace adj

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
        for (int r = 0; r < R.n; ++r) {
            const double c = R.cosv[r], s = R.sinv[r];
            if (R.axis[r] == 0) {  // y' = c y - s z, z' = s y + c z
                const double y = uy;
                uy = c * y - s * uz;
                uz = s * y + c * uz;
            } else {  // x' = c x - s z, z' = s x + c z (the centre drops out of the linear part)
                const double x = ux;
                ux = c * x - s * uz;
                uz = s * x + c * uz;
            }
        }
    }
    u_view[3 * t] = ux;
    u_view[3 * t + 1] = uy;
    u_view[3 * t + 2] = uz;
}

// motion_walk's frame over the per-point velocities.  The next record and the next cell's vertex ids are loaded before the
// arithmetic, the vertices at the top of the step (vertex_walk's order).  Nothing is shared between the lanes.
template <int KC>
__global__ __launch_bounds__(64) void vertex_tangent_walk(VertexTangentParams A) {
    using namespace adj;
    const WalkParams& P = A.w;
    Ray r;
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
            const CellFacesSloped cf = cell_faces_sloped(p, r.x, r.y);
            int vo[3], vi[3];
            face_points(cv, cf.b.out.f, vo);
            face_points(cv, cf.b.in.f, vi);
            double ddz[KC];
#pragma unroll
            for (int j = 0; j < KC; ++j) {
                ddz[j] = cf.b.found ? vertex_ddz(A.u_view + 3 * j, 3 * KC, vo, vi, cf) : 0.0;  // (faces not found: 0)
                tau_dot[j] = fma(a_raw, ddz[j], tau_dot[j]);                                   // d tau / d dz (raw alpha)
            }
            if (a != 0.0) {
                const double E = exp_nonpositive(-a * dz);
                const double dI_ddz = E * fma(-a, I, q);  // d I_k / d dz_k (the clamp is on alpha, not on the chord)
#pragma unroll
                for (int j = 0; j < KC; ++j) I_dot[j] = fma(E, I_dot[j], dI_ddz * ddz[j]);
                I = segment_terms(a, q, dz, E, 1.0, I).I_next;
            }
        }
        ray_advance(r, nb, carry_next);
        cur = nxt;
        cv = cv_nxt;
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

// motion_resolve's twin: the same sort, the same back-to-front order; both faces of a segment from its cell's vertices.
// u: field `j`'s first double of point 0 in a velocity buffer of `pitch` doubles per point.
__global__ __launch_bounds__(256) void vertex_tangent_resolve(GridView g, ImageParams im, const double* __restrict__ Xtab,
                                                              const double* __restrict__ Ytab, const int64_t* __restrict__ offs,
                                                              AdjSegment* __restrict__ segs, const uint32_t* __restrict__ mask,
                                                              double alpha_limit, const double* __restrict__ u, int pitch,
                                                              float2* __restrict__ out) {
    using namespace adj;
    const int64_t lp = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    const int64_t n_px = static_cast<int64_t>(im.n_local_rows) * im.res_x;
    if (lp >= n_px) return;
    double I = 0.0, I_dot = 0.0, tau_dot = 0.0;
    if (!(mask && mask[lp])) {
        const int lrow = static_cast<int>(lp / im.res_x);
        const double x = Xtab[lp - static_cast<int64_t>(lrow) * im.res_x], y = Ytab[global_row_of(im, lrow)];
        const MotionGeometry geo{g.cell_vert, g.vx, g.vy, g.vz};
        AdjSegment* const list = segs + offs[lp];
        const int n = static_cast<int>(offs[lp + 1] - offs[lp]);
        sort_segments(list, n);
        for (int i = n - 1; i >= 0; --i) {
            const int c = static_cast<int>(list[i].cell);
            const double dz = list[i].dz, q = g.q[c], a_raw = g.alpha[c];
            const ClampedAlpha ca = clamp_alpha(a_raw, alpha_limit);
            const int4 cv = g.cell_vert[c];
            double p[4][3];
            load_vertices(geo, cv, p);
            const CellFacesSloped cf = cell_faces_sloped(p, x, y);
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
                I_dot = fma(E, I_dot, E * fma(-ca.a, I, q) * ddz);
                I = segment_terms(ca.a, q, dz, E, 1.0, I).I_next;
            }
        }
    }
    out[lp] = make_float2(static_cast<float>(tau_dot), static_cast<float>(I_dot));
}

// ---- ray matrix (c5_ray_matrix_*): the segments themselves - per pixel the cells its ray crosses, the chord of each
// crossing and where it ends - as CSR arrays.  Two calls with a per-view setup each: the count (pass 1, then launch_scan64
// over the counts) and the fill (pass 2).  Each lane owns its row and appends to it with plain stores: no atomics,
// bit-reproducible.

namespace adj {

// Where a lane's row goes: element k at base + k for k < n_ok, the part of row_ptr's row that lies in [0, capacity).
// fits: all of row_ptr's row does.  Whatever row_ptr holds, base + k stays inside [0, capacity) for k < n_ok.
struct RowSlot {
    long long base = 0;
    unsigned n_ok = 0;
    bool fits = true;
};
__device__ __forceinline__ RowSlot row_slot(const int64_t* __restrict__ row_ptr, size_t lp, long long capacity) {
    RowSlot s;
    s.base = row_ptr[lp];
    const long long end = row_ptr[lp + 1];
    const long long len = (s.base >= 0 && end >= s.base) ? end - s.base : -1;
    const long long room = (s.base >= 0 && s.base < capacity) ? capacity - s.base : 0;  // (0 < room <= capacity: no overflow)
    const long long ok = len < room ? len : room;
    s.n_ok = ok > 0 ? static_cast<unsigned>(ok < 0x7fffffffll ? ok : 0x7fffffffll) : 0u;
    s.fits = len >= 0 && static_cast<long long>(s.n_ok) == len;
    return s;
}

// rows whose length is not row_ptr's or that found no room below capacity, counted once per wavefront
__device__ __forceinline__ void count_changed_rows(bool changed, unsigned* __restrict__ changed_rows) {
    const unsigned n = static_cast<unsigned>(__popcll(__builtin_amdgcn_ballot_w64(changed)));
    if (n && (threadIdx.x & 63) == 0) atomicAdd(changed_rows, n);
}

__device__ __forceinline__ void store_segment(const RayMatrixParams& A, long long at, int cell, double dz, double z_exit) {
    // (plain stores: a lane's next element lands in the line its last one did, and L2 merges them.  Nontemporal stores
    // took 16.1 ms against 4.96 for the benchmark frame's fill: profiles/ray_matrix.md)
    A.col[at] = A.perm ? A.perm[cell] : cell;
    A.dz[at] = dz;
    if (A.z_exit) A.z_exit[at] = z_exit;
}

}  // namespace adj

// PASS 1: the segments per pixel (int32); leaves the entry heads in place and counts as adjoint_walk<1> does.  PASS 2
// (its own per-view setup before it): the same walk, every segment stored; counts, and hands the heads back cleared.
// Nothing is shared between the lanes: a lane leaves the loop when its ray ends, as in tangent_walk.
template <int PASS>
__global__ __launch_bounds__(64) void segment_walk(RayMatrixParams A) {
    using namespace adj;
    const WalkParams& P = A.w;
    Ray r;
    unsigned k = 0;  // segments of the ray so far
    RowSlot slot;

    const EntryHead ent = ray_begin(r, P);
    if (PASS == 2 && r.in_image) slot = row_slot(A.row_ptr, r.lp, A.capacity);

    CellRegs cur;
    if (r.cell >= 0) load_cell(cur, P.xrec, r.cell);

    while (r.cell >= 0) {
        double dz, carry_next;
        const int nb = ray_step(r, P, ent, cur, dz, carry_next);
        CellRegs nxt;
        if (nb >= 0) load_cell(nxt, P.xrec, nb);

        if (is_segment(dz)) {
            // (the exit ray_step took, found again from the same registers: carry_next is already the next entry's depth
            // where the ray re-enters the grid.  The walk coordinate of "integration" 0 is view z.)
            if (PASS == 2 && k < slot.n_ok) store_segment(A, slot.base + k, r.cell, dz, step_geometry(cur, r.x, r.y).w_exit);
            ++k;
        }
        ray_advance(r, nb, carry_next);
        cur = nxt;
    }

    if (PASS == 1) {
        if (r.in_image) A.count[r.lp] = static_cast<int32_t>(k);
    } else {
        count_changed_rows(r.in_image && !(slot.fits && k == slot.n_ok), A.changed_rows);
        ray_clear_head(r, P);
    }
    ray_count(r, P);
}

// segment_walk's twins over bin_sort_resolve's lists ("algorithm" 1): the segments resolve_pixels integrates (those of
// dz > 0: the others add nothing), in the order its recurrence runs (i = n - 1 ... 0 of the sorted list).
__global__ __launch_bounds__(256) void segment_count_resolve(ImageParams im, const int64_t* __restrict__ offs,
                                                             const AdjSegment* __restrict__ segs, const uint32_t* __restrict__ mask,
                                                             int32_t* __restrict__ count) {
    const int64_t lp = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (lp >= static_cast<int64_t>(im.n_local_rows) * im.res_x) return;
    int32_t k = 0;
    if (!(mask && mask[lp]))
        for (int64_t i = offs[lp]; i < offs[lp + 1]; ++i) k += adj::is_segment(segs[i].dz) ? 1 : 0;
    count[lp] = k;
}

__global__ __launch_bounds__(256) void segment_fill_resolve(ImageParams im, const int64_t* __restrict__ offs,
                                                            AdjSegment* __restrict__ segs, const uint32_t* __restrict__ mask,
                                                            RayMatrixParams A) {
    using namespace adj;
    const int64_t lp = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    const bool in_image = lp < static_cast<int64_t>(im.n_local_rows) * im.res_x;
    bool changed = false;
    if (in_image) {
        const RowSlot slot = row_slot(A.row_ptr, static_cast<size_t>(lp), A.capacity);
        unsigned k = 0;
        if (!(mask && mask[lp])) {
            AdjSegment* const list = segs + offs[lp];
            const int n = static_cast<int>(offs[lp + 1] - offs[lp]);
            sort_segments(list, n);
            for (int i = n - 1; i >= 0; --i) {
                if (!is_segment(list[i].dz)) continue;
                if (k < slot.n_ok) store_segment(A, slot.base + k, static_cast<int>(list[i].cell), list[i].dz, list[i].z_hi);
                ++k;
            }
        }
        changed = !(slot.fits && k == slot.n_ok);
    }
    count_changed_rows(changed, A.changed_rows);
}

namespace {
// workgroups of a walk kernel: one wavefront per 8x8 pixel tile (0: no pixel)
unsigned tile_blocks(const ImageParams& im) {
    if (im.res_x <= 0 || im.n_local_rows <= 0) return 0u;
    return static_cast<unsigned>(((im.res_x + 7) / 8) * ((im.n_local_rows + 7) / 8));
}
// workgroups of 256 threads for n items (0: none)
unsigned item_blocks(int64_t n) { return n > 0 ? static_cast<unsigned>((n + 255) / 256) : 0u; }
unsigned pixel_blocks(const ImageParams& im) { return item_blocks(static_cast<int64_t>(im.n_local_rows) * im.res_x); }
}  // namespace

// kernel<4> or kernel<8> by the chunk width kc
#define C5_LAUNCH_KC(kernel, kc, blocks, threads, s, ...)                                      \
    do {                                                                                       \
        if ((kc) == 4) hipLaunchKernelGGL(kernel<4>, dim3(blocks), dim3(threads), 0, s, __VA_ARGS__); \
        else hipLaunchKernelGGL(kernel<8>, dim3(blocks), dim3(threads), 0, s, __VA_ARGS__);    \
    } while (0)

void launch_adjoint_walk(hipStream_t s, const AdjointParams& a, int pass) {
    const unsigned blocks = tile_blocks(a.w.im);
    if (!blocks) return;
    if (pass == 1)
        hipLaunchKernelGGL(adjoint_walk<1>, dim3(blocks), dim3(64), 0, s, a);
    else
        hipLaunchKernelGGL(adjoint_walk<2>, dim3(blocks), dim3(64), 0, s, a);
}

void launch_adjoint_resolve(hipStream_t s, const GridView& g, const ImageParams& im, const int64_t* offs, void* segs,
                            const uint32_t* mask, double alpha_limit, const float2* grad_out, double* grad_a, double* grad_q) {
    const unsigned blocks = pixel_blocks(im);
    if (!blocks) return;
    hipLaunchKernelGGL(adjoint_resolve, dim3(blocks), dim3(256), 0, s, g, im, offs, static_cast<AdjSegment*>(segs), mask, alpha_limit,
                       grad_out, grad_a, grad_q);
}

void launch_adjoint_permute(hipStream_t s, const double* ga_dev, const double* gq_dev, const int32_t* perm, int64_t n,
                            double* ga_out, double* gq_out) {
    if (n <= 0) return;
    hipLaunchKernelGGL(adjoint_permute, dim3(item_blocks(n)), dim3(256), 0, s, ga_dev, gq_dev, perm, n, ga_out, gq_out);
}

void launch_tangent_gather(hipStream_t s, const double* d_alpha, const double* d_q, const int32_t* perm, int64_t n,
                           double2* dir) {
    if (n <= 0) return;
    hipLaunchKernelGGL(tangent_gather, dim3(item_blocks(n)), dim3(256), 0, s, d_alpha, d_q, perm, n, dir);
}

void launch_tangent_walk(hipStream_t s, const TangentParams& t) {
    const unsigned blocks = tile_blocks(t.w.im);
    if (blocks) hipLaunchKernelGGL(tangent_walk, dim3(blocks), dim3(64), 0, s, t);
}

void launch_tangent_resolve(hipStream_t s, const GridView& g, const ImageParams& im, const int64_t* offs, void* segs,
                            const uint32_t* mask, double alpha_limit, const double2* dir, float2* out) {
    const unsigned blocks = pixel_blocks(im);
    if (!blocks) return;
    hipLaunchKernelGGL(tangent_resolve, dim3(blocks), dim3(256), 0, s, g, im, offs, static_cast<AdjSegment*>(segs), mask, alpha_limit,
                       dir, out);
}

void launch_tangent_gather_batch(hipStream_t s, int kc, const double* d_alpha, const double* d_q, const int32_t* perm, int64_t n,
                                 int k0, int n_used, double2* dirs) {
    if (n <= 0) return;
    C5_LAUNCH_KC(tangent_gather_batch, kc, item_blocks(n * kc), 256, s, d_alpha, d_q, perm, n, k0, n_used, dirs);
}

void launch_tangent_walk_batch(hipStream_t s, int kc, const TangentBatchParams& t) {
    const unsigned blocks = tile_blocks(t.w.im);
    if (blocks) C5_LAUNCH_KC(tangent_walk_batch, kc, blocks, 64, s, t);
}

void launch_adjoint_walk_batch(hipStream_t s, int kc, const AdjointBatchParams& a) {
    const unsigned blocks = tile_blocks(a.w.im);
    if (blocks) C5_LAUNCH_KC(adjoint_walk_batch, kc, blocks, 64, s, a);
}

void launch_adjoint_permute_batch(hipStream_t s, int kc, const double* grad, const int32_t* perm, int64_t n, int k0, int n_used,
                                  double* ga_out, double* gq_out) {
    if (n <= 0) return;
    C5_LAUNCH_KC(adjoint_permute_batch, kc, item_blocks(n * kc), 256, s, grad, perm, n, k0, n_used, ga_out, gq_out);
}

void launch_gn_walk_a(hipStream_t s, int kc, const GnWalkParams& a) {
    const unsigned blocks = tile_blocks(a.w.im);
    if (blocks) C5_LAUNCH_KC(gn_walk_a, kc, blocks, 64, s, a);
}

void launch_gn_diag_walk(hipStream_t s, const AdjointParams& a) {
    const unsigned blocks = tile_blocks(a.w.im);
    if (blocks) hipLaunchKernelGGL(gn_diag_walk, dim3(blocks), dim3(64), 0, s, a);
}

void launch_gn_weight(hipStream_t s, const float2* t, const float2* w, int64_t n_px, int n_imgs, float2* g) {
    if (n_px <= 0 || n_imgs <= 0) return;
    hipLaunchKernelGGL(gn_weight, dim3(item_blocks(n_px * n_imgs)), dim3(256), 0, s, t, w, n_px, n_imgs, g);
}

void launch_gn_diag_resolve(hipStream_t s, const GridView& g, const ImageParams& im, const int64_t* offs, void* segs,
                            const uint32_t* mask, double alpha_limit, const float2* weight, double* diag_a, double* diag_q) {
    const unsigned blocks = pixel_blocks(im);
    if (!blocks) return;
    hipLaunchKernelGGL(gn_diag_resolve, dim3(blocks), dim3(256), 0, s, g, im, offs, static_cast<AdjSegment*>(segs), mask, alpha_limit,
                       weight, diag_a, diag_q);
}

void launch_motion_walk(hipStream_t s, int kc, const MotionParams& m) {
    const unsigned blocks = tile_blocks(m.w.im);
    if (blocks) C5_LAUNCH_KC(motion_walk, kc, blocks, 64, s, m);
}

void launch_motion_resolve(hipStream_t s, const GridView& g, const ImageParams& im, const double* Xtab, const double* Ytab,
                           const int64_t* offs, void* segs, const uint32_t* mask, double alpha_limit, const MotionField& field,
                           float2* out) {
    const unsigned blocks = pixel_blocks(im);
    if (!blocks) return;
    hipLaunchKernelGGL(motion_resolve, dim3(blocks), dim3(256), 0, s, g, im, Xtab, Ytab, offs, static_cast<AdjSegment*>(segs), mask,
                       alpha_limit, field, out);
}

void launch_vertex_walk(hipStream_t s, const VertexParams& v, bool merge) {
    const unsigned blocks = tile_blocks(v.w.im);
    if (!blocks) return;
    if (merge) hipLaunchKernelGGL(vertex_walk<true>, dim3(blocks), dim3(64), 0, s, v);
    else hipLaunchKernelGGL(vertex_walk<false>, dim3(blocks), dim3(64), 0, s, v);
}

void launch_vertex_resolve(hipStream_t s, const GridView& g, const ImageParams& im, const double* Xtab, const double* Ytab,
                           const int64_t* offs, void* segs, const uint32_t* mask, double alpha_limit, const float2* grad_out,
                           double* face_w) {
    const unsigned blocks = pixel_blocks(im);
    if (!blocks) return;
    hipLaunchKernelGGL(vertex_resolve, dim3(blocks), dim3(256), 0, s, g, im, Xtab, Ytab, offs, static_cast<AdjSegment*>(segs), mask,
                       alpha_limit, grad_out, face_w);
}

void launch_vertex_finish(hipStream_t s, const MotionGeometry& geo, int64_t n_cells, const double* face_w, double* grad_view,
                          int64_t n_pts, const RotationList& R, double* grad_xyz) {
    if (n_cells > 0) hipLaunchKernelGGL(vertex_finish_cells, dim3(item_blocks(n_cells)), dim3(256), 0, s, geo, n_cells, face_w, grad_view);
    if (n_pts > 0) hipLaunchKernelGGL(vertex_finish_points, dim3(item_blocks(n_pts)), dim3(256), 0, s, grad_view, n_pts, R, grad_xyz);
}

void launch_vertex_velocity(hipStream_t s, int kc, const double* d_xyz, int64_t n_pts, int k0, int n_used, const RotationList& R,
                            double* u_view) {
    if (n_pts <= 0) return;
    C5_LAUNCH_KC(vertex_velocity, kc, item_blocks(n_pts * kc), 256, s, d_xyz, n_pts, k0, n_used, R, u_view);
}

void launch_vertex_tangent_walk(hipStream_t s, int kc, const VertexTangentParams& v) {
    const unsigned blocks = tile_blocks(v.w.im);
    if (blocks) C5_LAUNCH_KC(vertex_tangent_walk, kc, blocks, 64, s, v);
}

void launch_vertex_tangent_resolve(hipStream_t s, const GridView& g, const ImageParams& im, const double* Xtab, const double* Ytab,
                                   const int64_t* offs, void* segs, const uint32_t* mask, double alpha_limit, const double* u_view,
                                   int kc, int j, float2* out) {
    const unsigned blocks = pixel_blocks(im);
    if (!blocks) return;
    hipLaunchKernelGGL(vertex_tangent_resolve, dim3(blocks), dim3(256), 0, s, g, im, Xtab, Ytab, offs, static_cast<AdjSegment*>(segs),
                       mask, alpha_limit, u_view + 3 * j, 3 * kc, out);
}

void launch_segment_walk(hipStream_t s, const RayMatrixParams& m, int pass) {
    const unsigned blocks = tile_blocks(m.w.im);
    if (!blocks) return;
    if (pass == 1)
        hipLaunchKernelGGL(segment_walk<1>, dim3(blocks), dim3(64), 0, s, m);
    else
        hipLaunchKernelGGL(segment_walk<2>, dim3(blocks), dim3(64), 0, s, m);
}

void launch_segment_count_resolve(hipStream_t s, const ImageParams& im, const int64_t* offs, const void* segs, const uint32_t* mask,
                                  int32_t* count) {
    const unsigned blocks = pixel_blocks(im);
    if (blocks) hipLaunchKernelGGL(segment_count_resolve, dim3(blocks), dim3(256), 0, s, im, offs, static_cast<const AdjSegment*>(segs), mask, count);
}

void launch_segment_fill_resolve(hipStream_t s, const ImageParams& im, const int64_t* offs, void* segs, const uint32_t* mask,
                                 const RayMatrixParams& m) {
    const unsigned blocks = pixel_blocks(im);
    if (blocks) hipLaunchKernelGGL(segment_fill_resolve, dim3(blocks), dim3(256), 0, s, im, offs, static_cast<AdjSegment*>(segs), mask, m);
}

void launch_scalars_gather(hipStream_t s, const double* alpha_src, const double* q_src, const int32_t* perm, int64_t n, double* alpha,
                           double* q, unsigned long long* stats) {
    if (n <= 0) return;
    const unsigned blocks = static_cast<unsigned>(std::min<int64_t>((n + 255) / 256, kScalarBlocks));
    hipLaunchKernelGGL(scalars_gather, dim3(blocks), dim3(256), 0, s, alpha_src, q_src, perm, n, alpha, q, stats);
}

}  // namespace c5

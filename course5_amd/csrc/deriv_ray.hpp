// What every walk kernel of the derivative renders shares: the ray and its step, the segment arithmetic, the per-wave and
// per-cell reductions in front of the atomics, the rows a lane owns in a CSR array, the K-image store and the launch helpers.
#pragma once

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

// The walk's per-step helpers (walk_common.hpp: CellRegs, load_cell, step_geometry), the step with the library's fmin: these
// kernels' registers are sensitive to it (see MinFmin there).
__device__ __forceinline__ StepGeometry step_geometry(const CellRegs& cur, double x, double y) { return c5::step_geometry<MinFmin>(cur, x, y); }

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
// rays share cells, which is what the per-wave sums before the atomics live on).  Every walk kernel of the derivative renders
// takes its steps through this struct, and the step is that of walk_composite<*, 0> (walk_kernels.hip; one step_geometry for both: walk_common.hpp) operation for operation: the
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
struct EveryRay {
    __device__ bool operator()() const { return true; }
};
template <class Wanted = EveryRay>
__device__ __forceinline__ EntryHead ray_begin(Ray& r, const WalkParams& P, Wanted wanted = Wanted{}) {
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

// The tangent of one active segment's I: dQ (1 - E) / a + dalpha' (dI/dalpha at T = 1) + E I_dot_{k-1}; I_k from I_{k-1}.
__device__ __forceinline__ void tangent_step(double a, bool clamped, double q, double dz, double E, double da, double dq,
                                             double& I, double& I_dot) {
    const SegmentTerms t = segment_terms(a, q, dz, E, 1.0, I);
    double src = dq * t.dI_dq;
    if (!clamped) src = fma(da, t.dI_da, src);  // (a clamped alpha does not move: line.cpp:216)
    I_dot = fma(E, I_dot, src);
    I = t.I_next;
}

// d^2 S / d a^2 / dz^3 of S = (1 - e^(-a dz)) / a, x = a dz:  (2 (1 - e^-x) - 2 x e^-x - x^2 e^-x) / x^3
//   = sum_m (-1)^m (m + 2)(m + 1) / (m + 3)! x^m = 1/3 - x/4 + x^2/10 - x^3/36 + ...  for 0 <= x < 1/8, cut where
// dalpha_bracket_series is (x^10): the closed form cancels to nothing for short chords, two orders worse than the bracket
__device__ __forceinline__ double d2alpha_series(double x) {
    double p = 1.0 / 47174400.0;
    p = fma(p, x, -1.0 / 4354560.0);
    p = fma(p, x, 1.0 / 443520.0);
    p = fma(p, x, -1.0 / 50400.0);
    p = fma(p, x, 1.0 / 6480.0);
    p = fma(p, x, -1.0 / 960.0);
    p = fma(p, x, 1.0 / 168.0);
    p = fma(p, x, -1.0 / 36.0);
    p = fma(p, x, 0.1);
    p = fma(p, x, -0.25);
    return fma(p, x, 1.0 / 3.0);
}

// The Hessian-vector render's terms of one active segment, free of Q: S = (1 - E) / a and its first and second
// derivatives in a (segment_terms' s_over_q and bracket / Q, and one order more), by their series below a dz = 1/8.
struct SegmentTerms2 {
    double S, S_a, S_aa;
};
__device__ __forceinline__ SegmentTerms2 segment_terms2(double a, double dz, double E) {
    const double x = a * dz;
    SegmentTerms2 t;
    if (x < -kSmallExpArg) {
        const double dz2 = dz * dz;
        t.S = dz * one_minus_exp_over_x(x);
        t.S_a = dz2 * dalpha_bracket_series(x);
        t.S_aa = dz2 * dz * d2alpha_series(x);
    } else {
        t.S = (1.0 - E) / a;
        t.S_a = (dz * E - t.S) / a;
        t.S_aa = -fma(dz * dz, E, 2.0 * t.S_a) / a;
    }
    return t;
}

// Lambda_dot's running sum, sum_{j <= k} a_dot_j dz_j over the active segments whose alpha is not clamped: the same in
// both passes of the Hessian-vector render, so that Lambda_dot_n == Lambda_dot to the bit.  Not capped: behind a segment
// that lambda_add caps, lambda is exactly 0 and so is lambda times anything finite.
__device__ __forceinline__ double lambda_dot_add(double lam_dot, double a_dot, double dz) { return fma(a_dot, dz, lam_dot); }

// One active segment of the Hessian-vector render's second pass.  In: the segment (a clamped, q, dz, E), the direction
// there (a_dot: 0 where alpha is clamped; q_dot), lam = g_I T_k and lam_dot = -lam (Lambda_dot - Lambda_dot_k), and the
// carried I_{k-1}, I_dot_{k-1}.  Out: the segment's (h_alpha, h_q); I and I_dot advance to k (I_dot as tangent_step's).
__device__ __forceinline__ void hvp_step(double a, bool clamped, double q, double dz, double E, double a_dot, double q_dot,
                                         double lam, double lam_dot, double& I, double& I_dot, double& h_a, double& h_q) {
    const SegmentTerms2 t = segment_terms2(a, dz, E);
    const double dzE = dz * E;
    h_q = fma(lam_dot, t.S, lam * (t.S_a * a_dot));
    h_a = 0.0;
    if (!clamped) {  // (a clamped alpha does not move: no row and no column)
        const double G = fma(q, t.S_a, -dzE * I);
        double second = fma(q_dot, t.S_a, q * (t.S_aa * a_dot));
        second = fma(dz * dzE, a_dot * I, second);
        second = fma(-dzE, I_dot, second);
        h_a = fma(lam_dot, G, lam * second);
    }
    double src = fma(q_dot, t.S, a_dot * fma(q, t.S_a, -dzE * I));
    I_dot = fma(E, I_dot, src);
    I = fma(E, I, q * t.S);
}

// The staged per-cell reduction (one wavefront per workgroup).  Every lane stages its kV values of a step in a row of LDS;
// then, per distinct cell of the step, lanes v < kV each sum column v over the cell's member rows (four rows per round, an
// all-zero row 64 filling up) and add it with one atomic: kV atomics in one instruction, to one 8 kV-byte stretch.  A 64-lane
// butterfly per value, as scatter_wave does for two, would cost kV times its twelve cross-lane moves per shared cell.
template <int kV>
struct RowStage {
    static constexpr int kRow = kV + 1;  // (row pitch: an odd number of doubles)
    static constexpr int kDoubles = 65 * kRow;
};

template <int kV>  // once per kernel, before the first step: the all-zero row 64
__device__ __forceinline__ void stage_begin(double* stage, int lane) {
    if (lane < RowStage<kV>::kRow) stage[64 * RowStage<kV>::kRow + lane] = 0.0;
}
template <int kV>
__device__ __forceinline__ double* stage_row(double* stage, int lane) { return stage + lane * RowStage<kV>::kRow; }

// one step's reduction, by every lane: the rows of the lanes with `emit` set, summed per cell `here` into dst[cell][kV]
template <int kV>
__device__ __forceinline__ void reduce_rows(const double* stage, bool emit, int here, int lane, double* __restrict__ dst) {
    constexpr int kRow = RowStage<kV>::kRow;
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
            if (s != 0.0) atomicAdd(dst + static_cast<size_t>(lc) * kV + lane, s);
        }
        m &= ~members;
    }
    __syncthreads();  // (the rows are read before the next step writes them)
}

// The staged reduction of an outer product (the batched vertex adjoint: one wavefront per workgroup).  A lane's step is
// twelve signed weights lambda_v times KC values G_j: it stages the 12 + KC factors, not the 12 KC products, so a row
// stays 17 or 21 doubles where the products' would be 49 or 97 (reduce_rows takes 64 columns at most).  Per distinct cell
// of the step, lane 12 q + v (q < 4) then sums lambda_v G_j over the cell's member rows for j = q, q + 4, ..: KC / 4
// columns per lane with one read of lambda_v, in reduce_rows' four-rows-per-round grouping, and adds each sum with one
// atomic to dst[cell][j][v].  Every product is rounded by itself (__dmul_rn: not contracted into the sum) - the double a
// lane of vertex_walk stages.
template <int KC>
struct FaceStage {
    static constexpr int kG = 12;                // where a row's G_j begin, behind the twelve weights
    static constexpr int kRow = (12 + KC) | 1;   // (row pitch: an odd number of doubles)
    static constexpr int kDoubles = 65 * kRow;
};

template <int KC>  // once per kernel, before the first step: the all-zero row 64
__device__ __forceinline__ void face_stage_begin(double* stage, int lane) {
    if (lane < FaceStage<KC>::kRow) stage[64 * FaceStage<KC>::kRow + lane] = 0.0;
}
template <int KC>
__device__ __forceinline__ double* face_stage_row(double* stage, int lane) { return stage + lane * FaceStage<KC>::kRow; }

// one step's reduction, by every lane: the rows of the lanes with `emit` set, summed per cell `here` into dst[cell][KC][12]
template <int KC>
__device__ __forceinline__ void reduce_faces(const double* stage, bool emit, int here, int lane, double* __restrict__ dst) {
    constexpr int kRow = FaceStage<KC>::kRow, kG = FaceStage<KC>::kG, kPer = KC / 4;
    static_assert(KC % 4 == 0, "four images per round of 48 lanes");
    __syncthreads();  // (one wavefront: the rows are visible to every lane)
    unsigned long long m = __builtin_amdgcn_ballot_w64(emit);
    const int q = lane / 12, v = lane - 12 * q;
    while (m != 0ull) {
        const int leader = __builtin_ctzll(m);
        const int lc = __builtin_amdgcn_readlane(here, leader);
        const unsigned long long members = __builtin_amdgcn_ballot_w64(emit && here == lc);
        if (lane < 48) {
            double s[kPer];
#pragma unroll
            for (int h = 0; h < kPer; ++h) s[h] = 0.0;
            for (unsigned long long rows = members; rows != 0ull;) {
                const int b0 = __builtin_ctzll(rows);
                rows &= rows - 1;
                const int b1 = rows ? __builtin_ctzll(rows) : 64;
                rows &= rows - 1;
                const int b2 = rows ? __builtin_ctzll(rows) : 64;
                rows &= rows - 1;
                const int b3 = rows ? __builtin_ctzll(rows) : 64;
                rows &= rows - 1;
                const double *r0 = stage + b0 * kRow, *r1 = stage + b1 * kRow, *r2 = stage + b2 * kRow, *r3 = stage + b3 * kRow;
                const double l0 = r0[v], l1 = r1[v], l2 = r2[v], l3 = r3[v];
#pragma unroll
                for (int h = 0; h < kPer; ++h) {
                    const int j = kG + q + 4 * h;
                    s[h] += (__dmul_rn(l0, r0[j]) + __dmul_rn(l1, r1[j])) + (__dmul_rn(l2, r2[j]) + __dmul_rn(l3, r3[j]));
                }
            }
#pragma unroll
            for (int h = 0; h < kPer; ++h)  // (image q + 4 h, vertex v: column 48 h + lane of the cell's 12 KC)
                if (s[h] != 0.0) atomicAdd(dst + static_cast<size_t>(lc) * (12 * KC) + 48 * h + lane, s[h]);
        }
        m &= ~members;
    }
    __syncthreads();  // (the rows are read before the next step writes them)
}

// The staged reductions of the exact vertex adjoint ("vertex_exact"; one wavefront per workgroup): reduce_rows' ballot
// loop over other element types.  Pass E stages twelve int32 exponents per lane and takes their max per cell; pass S
// stages 24 int64 words per lane - its six values already rounded onto their grids - and adds them per cell as integers.
// Max and integer add commute: what a cell receives does not depend on which rays share a wavefront, or on the order.
template <class T, int kV>
struct WordStage {
    static constexpr int kRow = kV + 1;  // (row pitch: an odd number of elements)
    static constexpr int kWords = 65 * kRow;
};

template <class T, int kV>  // once per kernel, before the first step: row 64 holds the reduction's neutral element
__device__ __forceinline__ void word_stage_begin(T* stage, int lane, T neutral) {
    if (lane < WordStage<T, kV>::kRow) stage[64 * WordStage<T, kV>::kRow + lane] = neutral;
}
template <class T, int kV>
__device__ __forceinline__ T* word_stage_row(T* stage, int lane) { return stage + lane * WordStage<T, kV>::kRow; }

// pass E's step, by every lane: per distinct cell the max of the member rows' twelve exponents, one atomicMax per slot
// (twelve in one instruction, to one 48-byte stretch); a slot nobody touched (kNone, INT32_MIN: the neutral) is left alone
__device__ __forceinline__ void reduce_rows_max(const int* stage, bool emit, int here, int lane, int neutral, int* __restrict__ dst) {
    constexpr int kV = 12, kRow = WordStage<int, kV>::kRow;
    __syncthreads();  // (one wavefront: the rows are visible to every lane)
    unsigned long long m = __builtin_amdgcn_ballot_w64(emit);
    while (m != 0ull) {
        const int leader = __builtin_ctzll(m);
        const int lc = __builtin_amdgcn_readlane(here, leader);
        const unsigned long long members = __builtin_amdgcn_ballot_w64(emit && here == lc);
        if (lane < kV) {
            int s = neutral;
            for (unsigned long long rows = members; rows != 0ull;) {
                const int b0 = __builtin_ctzll(rows);
                rows &= rows - 1;
                const int b1 = rows ? __builtin_ctzll(rows) : 64;
                rows &= rows - 1;
                const int b2 = rows ? __builtin_ctzll(rows) : 64;
                rows &= rows - 1;
                const int b3 = rows ? __builtin_ctzll(rows) : 64;
                rows &= rows - 1;
                s = max(s, max(max(stage[b0 * kRow + lane], stage[b1 * kRow + lane]), max(stage[b2 * kRow + lane], stage[b3 * kRow + lane])));
            }
            if (s != neutral) atomicMax(dst + static_cast<size_t>(lc) * kV + lane, s);
        }
        m &= ~members;
    }
    __syncthreads();  // (the rows are read before the next step writes them)
}

// pass S's step, by every lane: per distinct cell the int64 sums of the member rows' 24 words, one no-return 64-bit
// integer atomicAdd per word (24 in one instruction, to one 192-byte stretch)
__device__ __forceinline__ void reduce_rows_words(const long long* stage, bool emit, int here, int lane, long long* __restrict__ dst) {
    constexpr int kV = 24, kRow = WordStage<long long, kV>::kRow;
    __syncthreads();  // (one wavefront: the rows are visible to every lane)
    unsigned long long m = __builtin_amdgcn_ballot_w64(emit);
    while (m != 0ull) {
        const int leader = __builtin_ctzll(m);
        const int lc = __builtin_amdgcn_readlane(here, leader);
        const unsigned long long members = __builtin_amdgcn_ballot_w64(emit && here == lc);
        if (lane < kV) {
            unsigned long long s = 0ull;  // (unsigned: the sum of two's-complement words, wrap-free by the format's headroom)
            for (unsigned long long rows = members; rows != 0ull;) {
                const int b0 = __builtin_ctzll(rows);
                rows &= rows - 1;
                const int b1 = rows ? __builtin_ctzll(rows) : 64;
                rows &= rows - 1;
                const int b2 = rows ? __builtin_ctzll(rows) : 64;
                rows &= rows - 1;
                const int b3 = rows ? __builtin_ctzll(rows) : 64;
                rows &= rows - 1;
                s += (static_cast<unsigned long long>(stage[b0 * kRow + lane]) + static_cast<unsigned long long>(stage[b1 * kRow + lane])) +
                     (static_cast<unsigned long long>(stage[b2 * kRow + lane]) + static_cast<unsigned long long>(stage[b3 * kRow + lane]));
            }
            if (s != 0ull) atomicAdd(reinterpret_cast<unsigned long long*>(dst) + static_cast<size_t>(lc) * kV + lane, s);
        }
        m &= ~members;
    }
    __syncthreads();  // (the rows are read before the next step writes them)
}

// ---- rows a lane owns (the ray matrix and the ray Jacobian: CSR arrays, every lane appends to its pixel's row with plain
// stores - no atomics, bit-reproducible)

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

// A lane's way along its row: begin once; put(store) per element - store(at) where row_ptr's row and the capacity have room
// for it, and it counts either way; finish by every lane of the wavefront, after its loop.
struct RowCursor {
    RowSlot slot;
    unsigned k = 0;  // elements of the row so far
    bool in_image = false;
    __device__ __forceinline__ void begin(bool in_img, const int64_t* __restrict__ row_ptr, size_t lp, long long capacity) {
        in_image = in_img;
        if (in_img) slot = row_slot(row_ptr, lp, capacity);
    }
    template <class Store>
    __device__ __forceinline__ void put(Store store) {
        if (k < slot.n_ok) store(slot.base + k);
        ++k;
    }
    __device__ __forceinline__ void finish(unsigned* __restrict__ changed_rows) const {
        count_changed_rows(in_image && !(slot.fits && k == slot.n_ok), changed_rows);
    }
};

}  // namespace adj

// workgroups of a walk kernel: one wavefront per 8x8 pixel tile (0: no pixel)
inline unsigned tile_blocks(const ImageParams& im) {
    if (im.res_x <= 0 || im.n_local_rows <= 0) return 0u;
    return static_cast<unsigned>(((im.res_x + 7) / 8) * ((im.n_local_rows + 7) / 8));
}
// workgroups of 256 threads for n items (0: none)
inline unsigned item_blocks(int64_t n) { return n > 0 ? static_cast<unsigned>((n + 255) / 256) : 0u; }
inline unsigned pixel_blocks(const ImageParams& im) { return item_blocks(static_cast<int64_t>(im.n_local_rows) * im.res_x); }

// kernel<4> or kernel<8> by the chunk width kc
#define C5_LAUNCH_KC(kernel, kc, blocks, threads, s, ...)                                      \
    do {                                                                                       \
        if ((kc) == 4) hipLaunchKernelGGL(kernel<4>, dim3(blocks), dim3(threads), 0, s, __VA_ARGS__); \
        else hipLaunchKernelGGL(kernel<8>, dim3(blocks), dim3(threads), 0, s, __VA_ARGS__);    \
    } while (0)

}  // namespace c5

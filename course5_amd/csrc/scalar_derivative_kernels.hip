// gfx950 kernels of the scalar derivatives.  The adjoint: d(image)/d(alpha) and d(image)/d(Q) per cell, weighted by an upstream image.
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
//   adjoint_exact_*   adjoint_walk<2> / adjoint_resolve with the exact sums' scatter policies (further down); with
//                     "exact_sums" the diagonal's and the Hessian-vector render's bodies take them too (gn_diag_exact_*,
//                     hvp_exact_*), and the product runs adjoint_exact_* on each direction's g.
//
//   jacobian_walk / jacobian_fill_resolve   (c5_ray_jacobian_fill*) adjoint_walk<2> / adjoint_resolve for the upstream image
//                     (0, 1) at every pixel with the scatter policy RowStore: nothing is summed, every lane appends its
//                     segments' (cell, dz, d I / d alpha, d I / d Q) to its own pixel's row of the ray matrix's CSR structure.
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
// Every walk kernel takes its rays through adj::Ray (deriv_ray.hpp): ONE definition of the walk's step, of how a ray begins
// and of what it leaves behind.  The kernels differ in what they accumulate along the ray, and those that differ in nothing
// else share a body with a compile-time parameter (adjoint_walk_body: gn_diag_walk is pass 2 with squares;
// tangent_batch_body: gn_walk_a is tangent_walk_batch plus Lambda and the weighted store).  The *_resolve kernels share the
// reference's sort, its clamp of alpha and one frame around their lists (deriv_lists.hpp).
//
// The sums are fp64 atomics, added in arrival order: the gradients are NOT bit-reproducible from run to run (the last bits
// move) - unless "adjoint_exact" or "exact_sums" is on: then the same bodies run with another scatter policy, every contribution is rounded
// once onto a per-cell fixed-point grid and summed in int64 (exact_sum.hpp; adjoint_exact_walk below).
// Every derivative file is compiled with -munsafe-fp-atomics (build.py): global_atomic_add_f64, no compare-and-swap.
#include "deriv_lists.hpp"
#include "exact_sum.hpp"

namespace c5 {
namespace adj {

// ---- scatter policies: where a step's (ga, gq) per lane go.  adjoint_walk_body and adjoint_resolve_body take one as a
// template parameter.  first / next / advance: the cell the lane is in, the cell it steps to (called beside the record's
// load), and the step's end - for a policy that reads something of its own per cell.  keep_heads: pass 2 leaves the
// entry heads in place (another walk over the same lists follows).

// fp64 atomics in arrival order (scatter_wave): the adjoint, the Gauss-Newton diagonal and the Hessian-vector render as
// they always were
struct WaveScatter {
    double* __restrict__ grad_a;
    double* __restrict__ grad_q;
    __device__ __forceinline__ void first(int) {}
    __device__ __forceinline__ void next(int) {}
    __device__ __forceinline__ void advance() {}
    __device__ __forceinline__ bool keep_heads() const { return false; }
    __device__ __forceinline__ void operator()(bool pending, int cell, double ga, double gq) const {
        scatter_wave(pending, cell, ga, gq, grad_a, grad_q);
    }
};

// Pass E of the exact sums (exact_sum.hpp): per cell the largest exponent of its contributions, by an int32 atomicMax -
// order-free.  The lanes of a wavefront in one cell are reduced first by a max butterfly, in scatter_wave's ballot loop.
struct ExponentScatter {
    int2* __restrict__ exps;
    __device__ __forceinline__ void first(int) {}
    __device__ __forceinline__ void next(int) {}
    __device__ __forceinline__ void advance() {}
    __device__ __forceinline__ bool keep_heads() const { return true; }
    __device__ __forceinline__ void operator()(bool pending, int cell, double ga, double gq) const {
        const int lane = static_cast<int>(threadIdx.x & 63);
        const int ea = pending ? exact::exponent_of(ga) : exact::kNone, eq = pending ? exact::exponent_of(gq) : exact::kNone;
        unsigned long long m = __builtin_amdgcn_ballot_w64(pending);
        while (m != 0ull) {
            const int leader = __builtin_ctzll(m);
            const int lc = __builtin_amdgcn_readlane(cell, leader);
            const bool mine = pending && cell == lc;
            int xa = mine ? ea : exact::kNone, xq = mine ? eq : exact::kNone;
            const unsigned long long mine_mask = __builtin_amdgcn_ballot_w64(mine);
            if (mine_mask != (1ull << leader)) {  // (wave-uniform) more than one lane in this cell
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) {
                    xa = max(xa, __shfl_xor(xa, d));
                    xq = max(xq, __shfl_xor(xq, d));
                }
            }
            // the leader's pair to lanes 0 and 1: both atomics in one instruction, to one 8-byte stretch
            const int ua = __builtin_amdgcn_readlane(xa, leader), uq = __builtin_amdgcn_readlane(xq, leader);
            if (lane < 2) {
                const int v = lane == 0 ? ua : uq;
                if (v != exact::kNone) atomicMax(reinterpret_cast<int*>(exps + lc) + lane, v);
            }
            pending = pending && !mine;
            m &= ~mine_mask;
        }
    }
};

// lane `from`'s 64-bit value, in every lane (from: wave-uniform)
__device__ __forceinline__ unsigned long long uniform_of(long long v, int from) {
    const unsigned lo = static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(v), from));
    const unsigned hi = static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(v >> 32), from));
    return (static_cast<unsigned long long>(hi) << 32) | lo;
}

// Pass S of the exact sums: every lane rounds its own (ga, gq) onto the cell's grid - the only rounding there is - before
// any cross-lane work; the words of the lanes of a wavefront in one cell are summed as int64 on the scalar unit and added
// with no-return 64-bit integer atomics - by four lanes in one instruction, as reduce_rows issues its atomics.  Integer
// adds commute: the words do not depend on the order of arrival or on which rays share a wavefront.  A contribution
// beyond the cell's exponent is added nowhere and counted in *misfits.
struct ExactScatter {
    const int2* __restrict__ exps;
    long long* __restrict__ words;  // [n_cells][4]: {alpha s1, alpha s0, q s1, q s0}
    unsigned* __restrict__ misfits;
    int word_bits;
    bool keep;
    int2 e_cur = {exact::kNone, exact::kNone}, e_nxt = {exact::kNone, exact::kNone};
    __device__ __forceinline__ void first(int cell) { e_cur = exps[cell]; }
    __device__ __forceinline__ void next(int cell) { e_nxt = exps[cell]; }
    __device__ __forceinline__ void advance() { e_cur = e_nxt; }
    __device__ __forceinline__ bool keep_heads() const { return keep; }
    __device__ __forceinline__ void operator()(bool pending, int cell, double ga, double gq) const {
        const int lane = static_cast<int>(threadIdx.x & 63);
        int64_t a1 = 0, a0 = 0, q1 = 0, q0 = 0;
        bool misfit = false;
        if (pending) {  // (a cell marked not finite stays NaN whatever is added: its words are not looked at)
            if (e_cur.x != exact::kNotFinite) misfit = !exact::quantise(ga, e_cur.x, word_bits, a1, a0);
            if (e_cur.y != exact::kNotFinite) misfit = !exact::quantise(gq, e_cur.y, word_bits, q1, q0) || misfit;
        }
        const unsigned long long bad = __builtin_amdgcn_ballot_w64(misfit);
        if (bad != 0ull && lane == 0) atomicAdd(misfits, static_cast<unsigned>(__popcll(bad)));
        unsigned long long m = __builtin_amdgcn_ballot_w64(pending);
        while (m != 0ull) {
            const int leader = __builtin_ctzll(m);
            const int lc = __builtin_amdgcn_readlane(cell, leader);
            const bool mine = pending && cell == lc;
            const unsigned long long mine_mask = __builtin_amdgcn_ballot_w64(mine);
            // the members' words summed on the scalar unit, one member at a time: every lane's words are read once per step
            // (an int64 butterfly over four values is 48 cross-lane moves per shared cell, whoever shares it)
            unsigned long long u0 = 0ull, u1 = 0ull, u2 = 0ull, u3 = 0ull;
            for (unsigned long long rows = mine_mask; rows != 0ull; rows &= rows - 1ull) {
                const int member = __builtin_ctzll(rows);
                u0 += uniform_of(a1, member);
                u1 += uniform_of(a0, member);
                u2 += uniform_of(q1, member);
                u3 += uniform_of(q0, member);
            }
            // lanes 0 .. 3 add them: four atomics in one instruction, to one 32-byte stretch
            if (lane < 4) {
                const unsigned long long v = lane == 0 ? u0 : lane == 1 ? u1 : lane == 2 ? u2 : u3;
                if (v) atomicAdd(reinterpret_cast<unsigned long long*>(words) + 4 * static_cast<size_t>(lc) + lane, v);
            }
            pending = pending && !mine;
            m &= ~mine_mask;
        }
    }
};

// The ray Jacobian's sink: nothing is summed.  The bodies run with the upstream image (0, 1) at every pixel, so a step's
// (ga, gq) ARE the segment's (d I / d alpha, d I / d Q) - the doubles the adjoint adds for a one-hot upstream image - and
// each lane appends them, with the chord, to its own pixel's row (RowCursor: inside [0, capacity) whatever row_ptr holds).
// No lane needs another: with this sink the bodies' loops are per lane, and a lane leaves when its ray ends.
struct RowStore {
    JacobianRows J;
    RowCursor row;
    double chord_dz = 0.0;
    __device__ explicit RowStore(const JacobianRows& j) : J(j) {}
    __device__ __forceinline__ void begin(bool in_image, size_t lp) { row.begin(in_image, J.row_ptr, lp, J.capacity); }
    __device__ __forceinline__ void first(int) {}
    __device__ __forceinline__ void next(int) {}
    __device__ __forceinline__ void advance() {}
    __device__ __forceinline__ bool keep_heads() const { return false; }
    __device__ __forceinline__ void chord(double dz) { chord_dz = dz; }
    __device__ __forceinline__ void operator()(bool emit, int cell, double ga, double gq) {
        if (!emit) return;
        row.put([&](long long at) {  // (plain stores, as store_segment's: ray_matrix_kernels.hip)
            if (J.col) J.col[at] = J.perm ? J.perm[cell] : cell;
            if (J.dz) J.dz[at] = chord_dz;
            if (J.dI_da) J.dI_da[at] = ga;
            if (J.dI_dq) J.dI_dq[at] = gq;
        });
    }
    // by every lane of the wavefront, after its loop
    __device__ __forceinline__ void end() const { row.finish(J.changed_rows); }
};

// Pass 1 (Lambda per pixel) and pass 2 (the scatter) of the adjoint; SQUARED: pass 2 with the segment's terms squared
// and A.grad_out the weights or nullptr for ones (gn_diag_walk).  Scatter: where pass 2's terms go (above); RowStore:
// the upstream image is (0, 1) everywhere, A.grad_out is not read.
template <int PASS, bool SQUARED, class Scatter>
__device__ __forceinline__ void adjoint_walk_body(const AdjointParams& A, Scatter sc) {
    constexpr bool kRows = std::is_same<Scatter, RowStore>::value;
    const WalkParams& P = A.w;
    Ray r;
    double lam = 0.0;                                         // Lambda_k so far
    double lam_total = 0.0, I = 0.0, g_tau = 0.0, g_I = 0.0;  // pass 2

    const EntryHead ent = ray_begin(r, P, [&] {
        if (PASS == 1) return true;
        const float2 g = kRows ? make_float2(0.0f, 1.0f) : (SQUARED && !A.grad_out) ? make_float2(1.0f, 1.0f) : A.grad_out[r.lp];
        g_tau = g.x;
        g_I = g.y;
        lam_total = A.lambda[r.lp];
        return g_tau != 0.0 || g_I != 0.0;
    });
    if constexpr (kRows) sc.begin(r.in_image, r.lp);

    CellRegs cur;
    if (r.cell >= 0) {
        load_cell(cur, P.xrec, r.cell);
        if (PASS == 2) sc.first(r.cell);
    }

    // wave-uniform loop (the scatter wants every lane): a lane whose ray has ended takes part with nothing to add.  kRows:
    // per lane, as tangent_walk's
    for (;;) {
        const bool live = r.cell >= 0;
        if (kRows ? !live : __builtin_amdgcn_ballot_w64(live) == 0ull) break;
        bool emit = false;
        double ga = 0.0, gq = 0.0;
        const int here = r.cell;
        if (live) {
            double dz, carry_next;
            const int nb = ray_step(r, P, ent, cur, dz, carry_next);
            CellRegs nxt;
            if (nb >= 0) {
                load_cell(nxt, P.xrec, nb);
                if (PASS == 2) sc.next(nb);
            }

            if (is_segment(dz)) {
                const double a_raw = cur.r6.a, a = cur.r6.b, q = cur.r7.b;  // a: clamped, 0 = inactive (cell_optics)
                if (PASS == 1) {
                    if (a != 0.0) lam = lambda_add(lam, a, dz);
                } else {
                    emit = true;
                    if constexpr (kRows) sc.chord(dz);
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
        if (PASS == 2) {
            sc(emit, here, ga, gq);
            if (live) sc.advance();
        }
    }

    if (PASS == 1) {
        if (r.in_image) A.lambda[r.lp] = lam;
        ray_count(r, P);
    } else {
        if constexpr (kRows) sc.end();
        if (!sc.keep_heads()) ray_clear_head(r, P);
    }
}


// resolve_pixels (exact_kernels.hip) differentiated: its list sorted, the recurrence run from the back (i = n - 1 ... 0:
// k = n - i).  SQUARED: the segment's terms squared, `weights` nullptr for ones (gn_diag_resolve).
template <bool SQUARED, class Scatter>
__device__ __forceinline__ void adjoint_resolve_body(const ResolveParams& R, const float2* __restrict__ weights, Scatter sc) {
    constexpr bool kRows = std::is_same<Scatter, RowStore>::value;  // (as adjoint_walk_body's: `weights` is not read)
    const GridView& g = R.g;
    double g_tau = 0.0, g_I = 0.0;
    const ListFrame f = list_frame<false>(R, [&](int64_t lp) {
        const float2 gw = kRows ? make_float2(0.0f, 1.0f) : (SQUARED && !weights) ? make_float2(1.0f, 1.0f) : weights[lp];
        g_tau = gw.x;
        g_I = gw.y;
        return !(g_tau == 0.0 && g_I == 0.0);
    });
    if constexpr (kRows) sc.begin(f.in_image, static_cast<size_t>(f.lp));
    const double lam_total = lambda_total(f.list, f.n, g, R.alpha_limit);
    double lam = 0.0, I = 0.0;
    // wave-uniform loop over the steps (the scatter wants every lane; kRows: per lane)
    for (int i = f.n - 1;; --i) {
        const bool live = i >= 0;
        if (kRows ? !live : __builtin_amdgcn_ballot_w64(live) == 0ull) break;
        int c = -1;
        bool emit = live;
        double ga = 0.0, gq = 0.0;
        if (live) {
            c = static_cast<int>(f.list[i].cell);
            sc.first(c);
            const double dz = f.list[i].dz, q = g.q[c];
            if constexpr (kRows) {  // (the rows hold the segments the frame sums, as segment_fill_resolve's: a chord of 0 adds nothing)
                emit = is_segment(dz);
                sc.chord(dz);
            }
            const ClampedAlpha ca = clamp_alpha(g.alpha[c], R.alpha_limit);
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
        sc(emit, c, ga, gq);
    }
    if constexpr (kRows) sc.end();
}

}  // namespace adj

size_t adjoint_segment_bytes() { return sizeof(AdjSegment); }

template <int PASS>
__global__ __launch_bounds__(64) void adjoint_walk(AdjointParams A) {
    adj::adjoint_walk_body<PASS, false>(A, adj::WaveScatter{A.grad_a, A.grad_q});
}

__global__ __launch_bounds__(256) void adjoint_resolve(ResolveParams R, const float2* __restrict__ grad_out,
                                                       double* __restrict__ grad_a, double* __restrict__ grad_q) {
    adj::adjoint_resolve_body<false>(R, grad_out, adj::WaveScatter{grad_a, grad_q});
}

// The ray Jacobian's fill (after adjoint_walk<1>): adjoint_walk<2> with every lane's terms stored to its own row.  Pass 1
// has counted the view's rays (ray_count: once per view).
__global__ __launch_bounds__(64) void jacobian_walk(AdjointParams A, JacobianRows J) {
    adj::adjoint_walk_body<2, false>(A, adj::RowStore(J));
}

__global__ __launch_bounds__(256) void jacobian_fill_resolve(ResolveParams R, JacobianRows J) {
    adj::adjoint_resolve_body<false>(R, nullptr, adj::RowStore(J));
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

// ---- exact adjoint sums ("adjoint_exact", c5_render_adjoint_exact_*; exact_sum.hpp has the format)
//   exact_clear               the exponents to "no contribution" and / or the words to zero
//   adjoint_exact_walk<0>     pass E: pass 2's walk, the exponent of every (ga, gq) into the cell's int32 pair (atomicMax)
//   adjoint_exact_walk<1>     pass S: pass 2's walk again, every (ga, gq) rounded onto the cell's grid and added as int64
//   adjoint_exact_resolve<.>  the same two over bin_sort_resolve's lists ("algorithm" 1)
//   exact_gather_exps         the caller's exponents -> device order;  exact_emit_exps / exact_emit_words: back
//   exact_finish              the words to fp64, rounded once, in the caller's order
// Both walks follow adjoint_walk<1> (Lambda, and the entry heads left in place); pass E leaves the heads in place too.
__global__ __launch_bounds__(256) void exact_clear(ExactSums X, int64_t n, int exps, int words, int misfits) {
    const int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (i == 0 && misfits) *X.misfits = 0u;
    if (i >= n) return;
    if (exps) X.exps[i] = make_int2(exact::kNone, exact::kNone);
    if (words) {
        longlong2* const w = reinterpret_cast<longlong2*>(X.words + 4 * i);
        w[0] = make_longlong2(0, 0);
        w[1] = make_longlong2(0, 0);
    }
}

template <int SUMS>
__global__ __launch_bounds__(64) void adjoint_exact_walk(AdjointParams A, ExactSums X) {
    if (SUMS) adj::adjoint_walk_body<2, false>(A, adj::ExactScatter{X.exps, X.words, X.misfits, X.word_bits, X.keep_entries != 0});
    else adj::adjoint_walk_body<2, false>(A, adj::ExponentScatter{X.exps});
}

template <int SUMS>
__global__ __launch_bounds__(256) void adjoint_exact_resolve(ResolveParams R, const float2* __restrict__ grad_out, ExactSums X) {
    if (SUMS) adj::adjoint_resolve_body<false>(R, grad_out, adj::ExactScatter{X.exps, X.words, X.misfits, X.word_bits, true});
    else adj::adjoint_resolve_body<false>(R, grad_out, adj::ExponentScatter{X.exps});
}

__global__ __launch_bounds__(256) void exact_gather_exps(const int32_t* __restrict__ exp_a, const int32_t* __restrict__ exp_q,
                                                         const int32_t* __restrict__ perm, int64_t n, int2* __restrict__ exps) {
    const int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (i >= n) return;
    const int64_t d = perm ? static_cast<int64_t>(perm[i]) : i;
    exps[i] = make_int2(exp_a[d], exp_q[d]);
}

__global__ __launch_bounds__(256) void exact_emit_exps(const int2* __restrict__ exps, const int32_t* __restrict__ perm, int64_t n,
                                                       int32_t* __restrict__ exp_a, int32_t* __restrict__ exp_q) {
    const int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (i >= n) return;
    const int64_t d = perm ? static_cast<int64_t>(perm[i]) : i;
    const int2 e = exps[i];
    exp_a[d] = e.x;
    exp_q[d] = e.y;
}

__global__ __launch_bounds__(256) void exact_emit_words(const long long* __restrict__ words, const int32_t* __restrict__ perm, int64_t n,
                                                        long long* __restrict__ sums_a, long long* __restrict__ sums_q) {
    const int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (i >= n) return;
    const int64_t d = perm ? static_cast<int64_t>(perm[i]) : i;
    const longlong2* const w = reinterpret_cast<const longlong2*>(words + 4 * i);
    reinterpret_cast<longlong2*>(sums_a)[d] = w[0];
    reinterpret_cast<longlong2*>(sums_q)[d] = w[1];
}

__global__ __launch_bounds__(256) void exact_finish(ExactSums X, const int32_t* __restrict__ perm, int64_t n, double* __restrict__ ga_out,
                                                    double* __restrict__ gq_out) {
    const int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (i >= n) return;
    const int64_t d = perm ? static_cast<int64_t>(perm[i]) : i;
    const int2 e = X.exps[i];
    const longlong2* const w = reinterpret_cast<const longlong2*>(X.words + 4 * i);
    const longlong2 wa = w[0], wq = w[1];
    if (ga_out) ga_out[d] = exact::finish(e.x, wa.x, wa.y, X.word_bits);  // (either may be null: the product's and the hvp's)
    if (gq_out) gq_out[d] = exact::finish(e.y, wq.x, wq.y, X.word_bits);
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

// adjoint_resolve's frame: the same sort, the same back-to-front order, the tangent carried along.
__global__ __launch_bounds__(256) void tangent_resolve(ResolveParams R, const double2* __restrict__ dir_v, float2* __restrict__ out) {
    using namespace adj;
    const ListFrame f = list_frame<false>(R);
    if (!f.in_image) return;
    const GridView& g = R.g;
    const D2* __restrict__ dir = reinterpret_cast<const D2*>(dir_v);
    double I = 0.0, I_dot = 0.0, tau_dot = 0.0;
    for (int i = f.n - 1; i >= 0; --i) {
        const int c = static_cast<int>(f.list[i].cell);
        const double dz = f.list[i].dz, q = g.q[c];
        const ClampedAlpha ca = clamp_alpha(g.alpha[c], R.alpha_limit);
        const D2 d = dir[c];
        tau_dot = fma(dz, d.a, tau_dot);
        if (ca.active) tangent_step(ca.a, ca.clamped, q, dz, exp(-ca.a * dz), d.a, d.b, I, I_dot);
    }
    out[f.lp] = make_float2(static_cast<float>(tau_dot), static_cast<float>(I_dot));
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

// adjoint_walk<2> for KC upstream images.  Per step every lane has 2 KC values (ga_j, gq_j) for its cell: they go through
// the staged reduction (deriv_ray.hpp: reduce_rows), 2 KC atomics in one instruction to one 16 KC-byte stretch of grad.
template <int KC>
__global__ __launch_bounds__(64) void adjoint_walk_batch(AdjointBatchParams A) {
    using namespace adj;
    constexpr int kV = 2 * KC;
    __shared__ double stage[RowStage<kV>::kDoubles];
    const WalkParams& P = A.w;
    Ray r;
    const int lane = r.lane;
    stage_begin<kV>(stage, lane);

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
                double* const row = stage_row<kV>(stage, lane);
#pragma unroll
                for (int j = 0; j < KC; ++j) {
                    row[j] = ga[j];
                    row[KC + j] = gq[j];
                }
            }
            ray_advance(r, nb, carry_next);
            cur = nxt;
        }
        reduce_rows<kV>(stage, emit, here, lane, A.grad);
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
//   gn_diag_exact_walk<0 / 1>, gn_diag_exact_resolve<0 / 1>   pass E and pass S of "exact_sums" on the squared terms.
// The exact product needs no kernel of its own: gn_walk_a leaves g and Lambda, and adjoint_exact_walk / _resolve run on g.

template <int KC>
__global__ __launch_bounds__(64) void gn_walk_a(GnWalkParams A) {
    tangent_batch_body<KC>(A);
}

// adjoint_walk<2> with squares (after adjoint_walk<1>: A.lambda).  A.grad_out holds the weights, or nullptr for ones.
__global__ __launch_bounds__(64) void gn_diag_walk(AdjointParams A) {
    adj::adjoint_walk_body<2, true>(A, adj::WaveScatter{A.grad_a, A.grad_q});
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

// adjoint_resolve with squares (weights nullptr: ones)
__global__ __launch_bounds__(256) void gn_diag_resolve(ResolveParams R, const float2* __restrict__ weight,
                                                       double* __restrict__ diag_a, double* __restrict__ diag_q) {
    adj::adjoint_resolve_body<true>(R, weight, adj::WaveScatter{diag_a, diag_q});
}

// pass E (SUMS 0) and pass S (SUMS 1) of the exact diagonal: gn_diag_walk / gn_diag_resolve with the exact sums' scatter
// policies.  Pass E runs on the SQUARED terms: the exponents of the unsquared adjoint say nothing about them.
template <int SUMS>
__global__ __launch_bounds__(64) void gn_diag_exact_walk(AdjointParams A, ExactSums X) {
    if (SUMS) adj::adjoint_walk_body<2, true>(A, adj::ExactScatter{X.exps, X.words, X.misfits, X.word_bits, X.keep_entries != 0});
    else adj::adjoint_walk_body<2, true>(A, adj::ExponentScatter{X.exps});
}

template <int SUMS>
__global__ __launch_bounds__(256) void gn_diag_exact_resolve(ResolveParams R, const float2* __restrict__ weight, ExactSums X) {
    if (SUMS) adj::adjoint_resolve_body<true>(R, weight, adj::ExactScatter{X.exps, X.words, X.misfits, X.word_bits, true});
    else adj::adjoint_resolve_body<true>(R, weight, adj::ExponentScatter{X.exps});
}

// ---- Hessian-vector render (c5_render_hvp*) ---------------------------------------------------------------------------
// h = Hess(phi) v for phi = sum_p (g_tau tau + g_I I) and a direction v = (a_dot, Q_dot) of the cells' scalars.  tau is
// linear in alpha: only g_I counts.  With lambda_k = g_I T_k, S_k = (1 - E_k) / a_k and its derivatives S_a, S_aa in a,
// G_k = Q_k S_a,k - dz_k E_k I_{k-1}, Lambda_dot_k = sum_{j <= k} a_dot_j dz_j and lambda_dot_k = -lambda_k (Lambda_dot -
// Lambda_dot_k) (a_dot_k = 0 where the cell is inactive or its alpha clamped; I_dot as the tangent carries it):
//     h_q[c]     += lambda_dot_k S_k + lambda_k S_a,k a_dot_k
//     h_alpha[c] += lambda_dot_k G_k + lambda_k (Q_dot_k S_a,k + Q_k S_aa,k a_dot_k + dz_k^2 E_k a_dot_k I_{k-1} - dz_k E_k I_dot_{k-1})
// (h_alpha only where alpha is not clamped).
//   hvp_walk<1>   adjoint_walk<1>'s walk with the direction loaded beside the next record (tangent_walk): Lambda and
//                 Lambda_dot per pixel.  Leaves the entry lists in place for ...
//   hvp_walk<2>   ... adjoint_walk<2>'s frame: I, I_dot, Lambda_k, Lambda_dot_k run along, and the segment's (h_alpha, h_q)
//                 go to the scatter policy (WaveScatter: scatter_wave).  A pixel with g_I == 0 is not walked.
//   hvp_resolve   the same over bin_sort_resolve's lists ("algorithm" 1).
//   hvp_exact_walk<0 / 1>, hvp_exact_resolve<0 / 1>   pass E and pass S of "exact_sums": the same two bodies with
//                 ExponentScatter / ExactScatter, after hvp_walk<1>.
//   hvp_permute   device order -> the caller's; either output may be null.

namespace adj {

// Scatter: where pass 2's (h_alpha, h_q) go, as adjoint_walk_body's (pass 1 takes one and does not use it).
template <int PASS, class Scatter>
__device__ __forceinline__ void hvp_walk_body(const HvpParams& A, Scatter sc) {
    const WalkParams& P = A.w;
    const D2* __restrict__ dir = reinterpret_cast<const D2*>(A.dir);
    Ray r;
    double lam = 0.0, lam_dot = 0.0;                                              // Lambda_k, Lambda_dot_k so far
    double lam_total = 0.0, lam_dot_total = 0.0, I = 0.0, I_dot = 0.0, g_I = 0.0;  // pass 2

    const EntryHead ent = ray_begin(r, P, [&] {
        if (PASS == 1) return true;
        g_I = A.grad_out[r.lp].y;
        lam_total = A.lambda[r.lp];
        lam_dot_total = A.lambda_dot[r.lp];
        return g_I != 0.0;
    });

    CellRegs cur;
    D2 d_cur{0.0, 0.0};
    if (r.cell >= 0) {
        load_cell(cur, P.xrec, r.cell);
        d_cur = dir[r.cell];
        if (PASS == 2) sc.first(r.cell);
    }

    // wave-uniform loop in pass 2 (the scatter wants every lane): a lane whose ray has ended takes part with nothing to add
    for (;;) {
        const bool live = r.cell >= 0;
        if (PASS == 1 ? !live : __builtin_amdgcn_ballot_w64(live) == 0ull) break;
        bool emit = false;
        double ha = 0.0, hq = 0.0;
        const int here = r.cell;
        if (live) {
            double dz, carry_next;
            const int nb = ray_step(r, P, ent, cur, dz, carry_next);
            CellRegs nxt;
            D2 d_nxt{0.0, 0.0};
            if (nb >= 0) {
                load_cell(nxt, P.xrec, nb);
                d_nxt = dir[nb];
                if (PASS == 2) sc.next(nb);
            }

            if (is_segment(dz)) {
                const double a_raw = cur.r6.a, a = cur.r6.b, q = cur.r7.b;  // a: clamped, 0 = inactive (cell_optics)
                if (a != 0.0) {
                    const bool clamped = a != a_raw;
                    const double a_dot = clamped ? 0.0 : d_cur.a;
                    // (the same sums in both passes: Lambda_n == Lambda and Lambda_dot_n == Lambda_dot bit for bit)
                    lam = lambda_add(lam, a, dz);
                    if (!clamped) lam_dot = lambda_dot_add(lam_dot, a_dot, dz);
                    if (PASS == 2) {
                        emit = true;
                        const double T = exp_nonpositive(fmin(lam - lam_total, 0.0));
                        const double E = exp_nonpositive(-a * dz);
                        const double lambda = g_I * T;
                        const double lambda_dot = -lambda * (lam_dot_total - lam_dot);
                        hvp_step(a, clamped, q, dz, E, a_dot, d_cur.b, lambda, lambda_dot, I, I_dot, ha, hq);
                    }
                }
            }
            ray_advance(r, nb, carry_next);
            cur = nxt;
            d_cur = d_nxt;
        }
        if (PASS == 2) {
            sc(emit, here, ha, hq);
            if (live) sc.advance();
        }
    }

    if (PASS == 1) {
        if (r.in_image) {
            A.lambda[r.lp] = lam;
            A.lambda_dot[r.lp] = lam_dot;
        }
        ray_count(r, P);
    } else if (!sc.keep_heads()) {
        ray_clear_head(r, P);
    }
}

}  // namespace adj

template <int PASS>
__global__ __launch_bounds__(64) void hvp_walk(HvpParams A) {
    adj::hvp_walk_body<PASS>(A, adj::WaveScatter{A.h_a, A.h_q});
}

// pass E (SUMS 0) and pass S (SUMS 1) of the exact Hessian-vector sums: hvp_walk<2>'s walk with the exact sums' scatter
// policies; both follow hvp_walk<1> (Lambda, Lambda_dot, and the entry heads left in place)
template <int SUMS>
__global__ __launch_bounds__(64) void hvp_exact_walk(HvpParams A, ExactSums X) {
    if (SUMS) adj::hvp_walk_body<2>(A, adj::ExactScatter{X.exps, X.words, X.misfits, X.word_bits, X.keep_entries != 0});
    else adj::hvp_walk_body<2>(A, adj::ExponentScatter{X.exps});
}

// adjoint_resolve's frame with the tangent carried along; Lambda and Lambda_dot from a pre-pass over the sorted list, in
// the order the loop re-sums them.
namespace adj {
template <class Scatter>
__device__ __forceinline__ void hvp_resolve_body(const ResolveParams& R, const double2* __restrict__ dir_v,
                                                 const float2* __restrict__ grad_out, Scatter sc) {
    const GridView& g = R.g;
    const D2* __restrict__ dir = reinterpret_cast<const D2*>(dir_v);
    double g_I = 0.0;
    const ListFrame f = list_frame<false>(R, [&](int64_t lp) {
        g_I = grad_out[lp].y;
        return g_I != 0.0;
    });
    const double lam_total = lambda_total(f.list, f.n, g, R.alpha_limit);
    double lam_dot_total = 0.0;
    for (int i = f.n - 1; i >= 0; --i) {
        const int c = static_cast<int>(f.list[i].cell);
        const ClampedAlpha ca = clamp_alpha(g.alpha[c], R.alpha_limit);
        if (ca.active && !ca.clamped) lam_dot_total = lambda_dot_add(lam_dot_total, dir[c].a, f.list[i].dz);
    }
    double lam = 0.0, lam_dot = 0.0, I = 0.0, I_dot = 0.0;
    // wave-uniform loop over the steps (the scatter wants every lane)
    for (int i = f.n - 1;; --i) {
        const bool live = i >= 0;
        if (__builtin_amdgcn_ballot_w64(live) == 0ull) break;
        int c = -1;
        bool emit = false;
        double ha = 0.0, hq = 0.0;
        if (live) {
            c = static_cast<int>(f.list[i].cell);
            sc.first(c);
            const double dz = f.list[i].dz, q = g.q[c];
            const ClampedAlpha ca = clamp_alpha(g.alpha[c], R.alpha_limit);
            if (ca.active) {
                const D2 d = dir[c];
                const double a = ca.a, a_dot = ca.clamped ? 0.0 : d.a;
                lam = lambda_add(lam, a, dz);
                if (!ca.clamped) lam_dot = lambda_dot_add(lam_dot, a_dot, dz);
                emit = true;
                const double T = exp(fmin(lam - lam_total, 0.0));
                const double E = exp(-a * dz);
                const double lambda = g_I * T;
                const double lambda_dot = -lambda * (lam_dot_total - lam_dot);
                hvp_step(a, ca.clamped, q, dz, E, a_dot, d.b, lambda, lambda_dot, I, I_dot, ha, hq);
            }
        }
        sc(emit, c, ha, hq);
    }
}
}  // namespace adj

__global__ __launch_bounds__(256) void hvp_resolve(ResolveParams R, const double2* __restrict__ dir_v, const float2* __restrict__ grad_out,
                                                   double* __restrict__ h_a, double* __restrict__ h_q) {
    adj::hvp_resolve_body(R, dir_v, grad_out, adj::WaveScatter{h_a, h_q});
}

template <int SUMS>
__global__ __launch_bounds__(256) void hvp_exact_resolve(ResolveParams R, const double2* __restrict__ dir_v,
                                                         const float2* __restrict__ grad_out, ExactSums X) {
    if (SUMS) adj::hvp_resolve_body(R, dir_v, grad_out, adj::ExactScatter{X.exps, X.words, X.misfits, X.word_bits, true});
    else adj::hvp_resolve_body(R, dir_v, grad_out, adj::ExponentScatter{X.exps});
}

// adjoint_permute with either output null
__global__ __launch_bounds__(256) void hvp_permute(const double* __restrict__ ha_dev, const double* __restrict__ hq_dev,
                                                   const int32_t* __restrict__ perm, int64_t n, double* __restrict__ ha_out,
                                                   double* __restrict__ hq_out) {
    const int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (i >= n) return;
    const int64_t d = perm ? static_cast<int64_t>(perm[i]) : i;
    if (ha_out) ha_out[d] = ha_dev[i];
    if (hq_out) hq_out[d] = hq_dev[i];
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

void launch_adjoint_walk(hipStream_t s, const AdjointParams& a, int pass) {
    const unsigned blocks = tile_blocks(a.w.im);
    if (!blocks) return;
    if (pass == 1) hipLaunchKernelGGL(adjoint_walk<1>, dim3(blocks), dim3(64), 0, s, a);
    else hipLaunchKernelGGL(adjoint_walk<2>, dim3(blocks), dim3(64), 0, s, a);
}

void launch_adjoint_resolve(hipStream_t s, const ResolveParams& r, const float2* grad_out, double* grad_a, double* grad_q) {
    if (const unsigned blocks = pixel_blocks(r.im)) hipLaunchKernelGGL(adjoint_resolve, dim3(blocks), dim3(256), 0, s, r, grad_out, grad_a, grad_q);
}

void launch_jacobian_walk(hipStream_t s, const AdjointParams& a, const JacobianRows& j) {
    if (const unsigned blocks = tile_blocks(a.w.im)) hipLaunchKernelGGL(jacobian_walk, dim3(blocks), dim3(64), 0, s, a, j);
}

void launch_jacobian_fill_resolve(hipStream_t s, const ResolveParams& r, const JacobianRows& j) {
    if (const unsigned blocks = pixel_blocks(r.im)) hipLaunchKernelGGL(jacobian_fill_resolve, dim3(blocks), dim3(256), 0, s, r, j);
}

void launch_adjoint_permute(hipStream_t s, const double* ga_dev, const double* gq_dev, const int32_t* perm, int64_t n,
                            double* ga_out, double* gq_out) {
    if (n <= 0) return;
    hipLaunchKernelGGL(adjoint_permute, dim3(item_blocks(n)), dim3(256), 0, s, ga_dev, gq_dev, perm, n, ga_out, gq_out);
}

void launch_exact_clear(hipStream_t s, const ExactSums& x, int64_t n, bool exps, bool words, bool misfits) {
    hipLaunchKernelGGL(exact_clear, dim3(std::max(1u, item_blocks(n))), dim3(256), 0, s, x, n, exps ? 1 : 0, words ? 1 : 0, misfits ? 1 : 0);
}

void launch_adjoint_exact_walk(hipStream_t s, const AdjointParams& a, const ExactSums& x, bool sums) {
    const unsigned blocks = tile_blocks(a.w.im);
    if (!blocks) return;
    if (sums) hipLaunchKernelGGL(adjoint_exact_walk<1>, dim3(blocks), dim3(64), 0, s, a, x);
    else hipLaunchKernelGGL(adjoint_exact_walk<0>, dim3(blocks), dim3(64), 0, s, a, x);
}

void launch_adjoint_exact_resolve(hipStream_t s, const ResolveParams& r, const float2* grad_out, const ExactSums& x, bool sums) {
    const unsigned blocks = pixel_blocks(r.im);
    if (!blocks) return;
    if (sums) hipLaunchKernelGGL(adjoint_exact_resolve<1>, dim3(blocks), dim3(256), 0, s, r, grad_out, x);
    else hipLaunchKernelGGL(adjoint_exact_resolve<0>, dim3(blocks), dim3(256), 0, s, r, grad_out, x);
}

void launch_exact_gather_exps(hipStream_t s, const int32_t* exp_a, const int32_t* exp_q, const int32_t* perm, int64_t n, const ExactSums& x) {
    if (n > 0) hipLaunchKernelGGL(exact_gather_exps, dim3(item_blocks(n)), dim3(256), 0, s, exp_a, exp_q, perm, n, x.exps);
}

void launch_exact_emit_exps(hipStream_t s, const ExactSums& x, const int32_t* perm, int64_t n, int32_t* exp_a, int32_t* exp_q) {
    if (n > 0) hipLaunchKernelGGL(exact_emit_exps, dim3(item_blocks(n)), dim3(256), 0, s, x.exps, perm, n, exp_a, exp_q);
}

void launch_exact_emit_words(hipStream_t s, const ExactSums& x, const int32_t* perm, int64_t n, int64_t* sums_a, int64_t* sums_q) {
    if (n > 0)
        hipLaunchKernelGGL(exact_emit_words, dim3(item_blocks(n)), dim3(256), 0, s, x.words, perm, n, reinterpret_cast<long long*>(sums_a),
                           reinterpret_cast<long long*>(sums_q));
}

void launch_exact_finish(hipStream_t s, const ExactSums& x, const int32_t* perm, int64_t n, double* ga_out, double* gq_out) {
    if (n > 0) hipLaunchKernelGGL(exact_finish, dim3(item_blocks(n)), dim3(256), 0, s, x, perm, n, ga_out, gq_out);
}

void launch_tangent_gather(hipStream_t s, const double* d_alpha, const double* d_q, const int32_t* perm, int64_t n,
                           double2* dir) {
    if (n <= 0) return;
    hipLaunchKernelGGL(tangent_gather, dim3(item_blocks(n)), dim3(256), 0, s, d_alpha, d_q, perm, n, dir);
}

void launch_tangent_walk(hipStream_t s, const TangentParams& t) {
    if (const unsigned blocks = tile_blocks(t.w.im)) hipLaunchKernelGGL(tangent_walk, dim3(blocks), dim3(64), 0, s, t);
}

void launch_tangent_resolve(hipStream_t s, const ResolveParams& r, const double2* dir, float2* out) {
    if (const unsigned blocks = pixel_blocks(r.im)) hipLaunchKernelGGL(tangent_resolve, dim3(blocks), dim3(256), 0, s, r, dir, out);
}

void launch_tangent_gather_batch(hipStream_t s, int kc, const double* d_alpha, const double* d_q, const int32_t* perm, int64_t n,
                                 int k0, int n_used, double2* dirs) {
    if (n <= 0) return;
    C5_LAUNCH_KC(tangent_gather_batch, kc, item_blocks(n * kc), 256, s, d_alpha, d_q, perm, n, k0, n_used, dirs);
}

void launch_tangent_walk_batch(hipStream_t s, int kc, const TangentBatchParams& t) {
    if (const unsigned blocks = tile_blocks(t.w.im)) C5_LAUNCH_KC(tangent_walk_batch, kc, blocks, 64, s, t);
}

void launch_adjoint_walk_batch(hipStream_t s, int kc, const AdjointBatchParams& a) {
    if (const unsigned blocks = tile_blocks(a.w.im)) C5_LAUNCH_KC(adjoint_walk_batch, kc, blocks, 64, s, a);
}

void launch_adjoint_permute_batch(hipStream_t s, int kc, const double* grad, const int32_t* perm, int64_t n, int k0, int n_used,
                                  double* ga_out, double* gq_out) {
    if (n <= 0) return;
    C5_LAUNCH_KC(adjoint_permute_batch, kc, item_blocks(n * kc), 256, s, grad, perm, n, k0, n_used, ga_out, gq_out);
}

void launch_gn_walk_a(hipStream_t s, int kc, const GnWalkParams& a) {
    if (const unsigned blocks = tile_blocks(a.w.im)) C5_LAUNCH_KC(gn_walk_a, kc, blocks, 64, s, a);
}

void launch_gn_diag_walk(hipStream_t s, const AdjointParams& a) {
    if (const unsigned blocks = tile_blocks(a.w.im)) hipLaunchKernelGGL(gn_diag_walk, dim3(blocks), dim3(64), 0, s, a);
}

void launch_gn_weight(hipStream_t s, const float2* t, const float2* w, int64_t n_px, int n_imgs, float2* g) {
    if (n_px <= 0 || n_imgs <= 0) return;
    hipLaunchKernelGGL(gn_weight, dim3(item_blocks(n_px * n_imgs)), dim3(256), 0, s, t, w, n_px, n_imgs, g);
}

void launch_gn_diag_resolve(hipStream_t s, const ResolveParams& r, const float2* weight, double* diag_a, double* diag_q) {
    if (const unsigned blocks = pixel_blocks(r.im)) hipLaunchKernelGGL(gn_diag_resolve, dim3(blocks), dim3(256), 0, s, r, weight, diag_a, diag_q);
}

void launch_hvp_walk(hipStream_t s, const HvpParams& h, int pass) {
    const unsigned blocks = tile_blocks(h.w.im);
    if (!blocks) return;
    if (pass == 1) hipLaunchKernelGGL(hvp_walk<1>, dim3(blocks), dim3(64), 0, s, h);
    else hipLaunchKernelGGL(hvp_walk<2>, dim3(blocks), dim3(64), 0, s, h);
}

void launch_hvp_resolve(hipStream_t s, const ResolveParams& r, const double2* dir, const float2* grad_out, double* h_a, double* h_q) {
    if (const unsigned blocks = pixel_blocks(r.im)) hipLaunchKernelGGL(hvp_resolve, dim3(blocks), dim3(256), 0, s, r, dir, grad_out, h_a, h_q);
}

void launch_gn_diag_exact_walk(hipStream_t s, const AdjointParams& a, const ExactSums& x, bool sums) {
    const unsigned blocks = tile_blocks(a.w.im);
    if (!blocks) return;
    if (sums) hipLaunchKernelGGL(gn_diag_exact_walk<1>, dim3(blocks), dim3(64), 0, s, a, x);
    else hipLaunchKernelGGL(gn_diag_exact_walk<0>, dim3(blocks), dim3(64), 0, s, a, x);
}

void launch_gn_diag_exact_resolve(hipStream_t s, const ResolveParams& r, const float2* weight, const ExactSums& x, bool sums) {
    const unsigned blocks = pixel_blocks(r.im);
    if (!blocks) return;
    if (sums) hipLaunchKernelGGL(gn_diag_exact_resolve<1>, dim3(blocks), dim3(256), 0, s, r, weight, x);
    else hipLaunchKernelGGL(gn_diag_exact_resolve<0>, dim3(blocks), dim3(256), 0, s, r, weight, x);
}

void launch_hvp_exact_walk(hipStream_t s, const HvpParams& h, const ExactSums& x, bool sums) {
    const unsigned blocks = tile_blocks(h.w.im);
    if (!blocks) return;
    if (sums) hipLaunchKernelGGL(hvp_exact_walk<1>, dim3(blocks), dim3(64), 0, s, h, x);
    else hipLaunchKernelGGL(hvp_exact_walk<0>, dim3(blocks), dim3(64), 0, s, h, x);
}

void launch_hvp_exact_resolve(hipStream_t s, const ResolveParams& r, const double2* dir, const float2* grad_out, const ExactSums& x,
                              bool sums) {
    const unsigned blocks = pixel_blocks(r.im);
    if (!blocks) return;
    if (sums) hipLaunchKernelGGL(hvp_exact_resolve<1>, dim3(blocks), dim3(256), 0, s, r, dir, grad_out, x);
    else hipLaunchKernelGGL(hvp_exact_resolve<0>, dim3(blocks), dim3(256), 0, s, r, dir, grad_out, x);
}

void launch_hvp_permute(hipStream_t s, const double* ha_dev, const double* hq_dev, const int32_t* perm, int64_t n, double* ha_out,
                        double* hq_out) {
    if (n <= 0) return;
    hipLaunchKernelGGL(hvp_permute, dim3(item_blocks(n)), dim3(256), 0, s, ha_dev, hq_dev, perm, n, ha_out, hq_out);
}

void launch_scalars_gather(hipStream_t s,const double* alpha_src, const double* q_src, const int32_t* perm, int64_t n, double* alpha,
                           double* q, unsigned long long* stats) {
    if (n <= 0) return;
    const unsigned blocks = static_cast<unsigned>(std::min<int64_t>((n + 255) / 256, kScalarBlocks));
    hipLaunchKernelGGL(scalars_gather, dim3(blocks), dim3(256), 0, s, alpha_src, q_src, perm, n, alpha, q, stats);
}

}  // namespace c5

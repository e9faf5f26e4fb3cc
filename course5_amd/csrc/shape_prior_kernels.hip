// ------------------------------------------------------------------------------------------
// Shape prior: the kernels (shape_prior_kernels.hpp; the contract: include/course5_hip.h, c5_shape_prior_*).
// Built with -ffp-contract=off: every product below rounds before the sum that takes it, which is what lets a numpy
// restatement reproduce the Dirichlet operators bit for bit and keeps every vector independent of the cells' device order.
// Two launches per operator: one lane per cell of the device's order leaves the cell's [4][3] shares, one lane per point
// adds the shares of its incidence list (ascending in the caller's cell index) and writes the caller's point order.
// No atomics in the operators, LDS only in the value's reduction.
// ------------------------------------------------------------------------------------------
#include "shape_prior_kernels.hpp"

#include "../../include/course5_hip.h"

namespace c5 {

namespace {

// Sum over a wavefront in a fixed tree (lane l takes lane l + 32, + 16, ...): the total is in lane 0.
template <class T>
__device__ inline T wave_sum(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// Sum over the block's wavefronts, in their order: the total is returned to thread 0.
template <class T>
__device__ inline T block_sum(T v, T* lds /*[kShapeBlock / 64]*/) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();  // (lds may still be read from the call before)
    if (lane == 0) lds[wave] = v;
    __syncthreads();
    T t = 0;
    if (threadIdx.x == 0)
        for (int k = 0; k < kShapeBlock / 64; ++k) t = t + lds[k];
    return t;
}

__device__ inline void load_point(const ShapePoints& pts, int id, double (&p)[3]) {
    const int64_t at = static_cast<int64_t>(id) * pts.stride;
    p[0] = pts.c[0][at];
    p[1] = pts.c[1][at];
    p[2] = pts.c[2][at];
}

// D[r][c] = p_{c+1}[r] - p_0[r]: the edge vectors as columns
__device__ inline void edges(const ShapePoints& pts, const int (&id)[4], double (&D)[3][3]) {
    double p0[3], p[3];
    load_point(pts, id[0], p0);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        load_point(pts, id[c + 1], p);
#pragma unroll
        for (int r = 0; r < 3; ++r) D[r][c] = p[r] - p0[r];
    }
}

// the cofactors of A and det A = (A00 C00 + A01 C01) + A02 C02
__device__ inline double cofactors(const double (&A)[3][3], double (&C)[3][3]) {
    C[0][0] = A[1][1] * A[2][2] - A[1][2] * A[2][1];
    C[0][1] = A[1][2] * A[2][0] - A[1][0] * A[2][2];
    C[0][2] = A[1][0] * A[2][1] - A[1][1] * A[2][0];
    C[1][0] = A[0][2] * A[2][1] - A[0][1] * A[2][2];
    C[1][1] = A[0][0] * A[2][2] - A[0][2] * A[2][0];
    C[1][2] = A[0][1] * A[2][0] - A[0][0] * A[2][1];
    C[2][0] = A[0][1] * A[1][2] - A[0][2] * A[1][1];
    C[2][1] = A[0][2] * A[1][0] - A[0][0] * A[1][2];
    C[2][2] = A[0][0] * A[1][1] - A[0][1] * A[1][0];
    return (A[0][0] * C[0][0] + A[0][1] * C[0][1]) + A[0][2] * C[0][2];
}

// F = D B: F[r][c] = (D[r][0] B[0][c] + D[r][1] B[1][c]) + D[r][2] B[2][c]
__device__ inline void times_b(const double (&D)[3][3], const double (&B)[3][3], double (&F)[3][3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) F[r][c] = (D[r][0] * B[0][c] + D[r][1] * B[1][c]) + D[r][2] * B[2][c];
}

// the sum of the squares of A's entries, row by row from the first
__device__ inline double squares(const double (&A)[3][3]) {
    double s = A[0][0] * A[0][0];
#pragma unroll
    for (int k = 1; k < 9; ++k) s = s + A[k / 3][k % 3] * A[k / 3][k % 3];
    return s;
}

// The shares of a cell's four points from a stress P: G = V0 (P B^T), point i + 1 takes column i, point 0 minus their sum.
__device__ inline void to_shares(const double (&P)[3][3], const double (&B)[3][3], double V0, double (&sh)[4][3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int i = 0; i < 3; ++i) sh[i + 1][r] = V0 * ((P[r][0] * B[i][0] + P[r][1] * B[i][1]) + P[r][2] * B[i][2]);
        sh[0][r] = -((sh[1][r] + sh[2][r]) + sh[3][r]);
    }
}

// psi, P and dP of the header, in its order of operations.  State: what the energy keeps of the point between them.
template <int ENERGY>
struct Energy;

template <>
struct Energy<C5_SHAPE_DIRICHLET> {
    static constexpr bool kBarrier = false;         // an inverted cell is counted, and contributes like any other
    static constexpr bool kHessianNeedsPoint = false;
    struct State {};
    __device__ static void at(const double (&)[3][3], const double (&)[3][3], double, double, State&) {}
    __device__ static void stress(const double (&F)[3][3], const State&, double (&P)[3][3]) {
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) P[r][c] = r == c ? F[r][c] - 1.0 : F[r][c];
    }
    __device__ static double psi(const double (&F)[3][3], const State& st) {
        double P[3][3];
        stress(F, st, P);
        return 0.5 * squares(P);
    }
    __device__ static void dstress(const double (&dF)[3][3], const State&, double (&dP)[3][3]) {
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) dP[r][c] = dF[r][c];
    }
};

template <>
struct Energy<C5_SHAPE_NEO_HOOKEAN> {
    static constexpr bool kBarrier = true;          // an inverted cell: value +inf, nothing to any vector
    static constexpr bool kHessianNeedsPoint = true;
    struct State {
        double Fit[3][3];  // F^-T = cofactors / J
        double lnJ, kappa;
    };
    __device__ static void at(const double (&)[3][3], const double (&C)[3][3], double J, double kappa, State& st) {
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) st.Fit[r][c] = C[r][c] / J;
        st.lnJ = log(J);
        st.kappa = kappa;
    }
    __device__ static void stress(const double (&F)[3][3], const State& st, double (&P)[3][3]) {
        const double c0 = st.kappa * st.lnJ - 1.0;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) P[r][c] = F[r][c] + c0 * st.Fit[r][c];
    }
    __device__ static double psi(const double (&F)[3][3], const State& st) {
        return (0.5 * (squares(F) - 3.0) - st.lnJ) + (0.5 * st.kappa) * (st.lnJ * st.lnJ);
    }
    // dP = dF + (1 - kappa ln J) F^-T dF^T F^-T + kappa tr(F^-1 dF) F^-T
    __device__ static void dstress(const double (&dF)[3][3], const State& st, double (&dP)[3][3]) {
        const double c1 = 1.0 - st.kappa * st.lnJ;
        double tr = st.Fit[0][0] * dF[0][0];
#pragma unroll
        for (int k = 1; k < 9; ++k) tr = tr + st.Fit[k / 3][k % 3] * dF[k / 3][k % 3];
        const double kt = st.kappa * tr;
        double T[3][3];  // dF^T F^-T
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) T[a][b] = (dF[0][a] * st.Fit[0][b] + dF[1][a] * st.Fit[1][b]) + dF[2][a] * st.Fit[2][b];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double m = (st.Fit[r][0] * T[0][c] + st.Fit[r][1] * T[1][c]) + st.Fit[r][2] * T[2][c];
                dP[r][c] = (dF[r][c] + c1 * m) + kt * st.Fit[r][c];
            }
    }
};

// The one body of the cell launch: OP says what a cell leaves, ENERGY how, VALUE whether the block's sums are kept.
template <int OP, int ENERGY, bool VALUE>
__global__ __launch_bounds__(kShapeBlock) void shape_cells_kernel(ShapeArgs a) {
    using E = Energy<ENERGY>;
    __shared__ double lds_v[VALUE ? kShapeBlock / 64 : 1];
    __shared__ long long lds_n[VALUE ? kShapeBlock / 64 : 1];
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kShapeBlock + threadIdx.x;
    double cell_value = 0.0;
    long long inverted = 0;
    if (i < a.rest.n_cells) {
        const double V0 = a.rest.vol[i];
        double sh[4][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
        double J = 0.0;
        if (V0 > 0.0) {  // (a degenerate rest cell contributes nothing anywhere)
            const int4 v4 = a.rest.cell_vert[i];
            const int id[4] = {v4.x, v4.y, v4.z, v4.w};
            double B[3][3];
#pragma unroll
            for (int k = 0; k < 9; ++k) B[k / 3][k % 3] = a.rest.binv[9 * i + k];
            constexpr bool at_point = OP == kShapeGradient || OP == kShapeQuality || E::kHessianNeedsPoint;
            constexpr bool need_j = OP == kShapeQuality || E::kBarrier || VALUE;
            double F[3][3], C[3][3];
            typename E::State st;
            bool ok = true;
            if (at_point) {
                double D[3][3];
                edges(a.x, id, D);
                times_b(D, B, F);
                if (need_j) {
                    J = cofactors(F, C);
                    const bool is_inverted = !(J > 0.0 && J < INFINITY);
                    if (is_inverted) inverted = 1;
                    ok = !(E::kBarrier && is_inverted);
                    if (OP != kShapeQuality && ok) E::at(F, C, J, a.kappa, st);
                }
            }
            if (OP == kShapeGradient && ok) {
                double P[3][3];
                E::stress(F, st, P);
                to_shares(P, B, V0, sh);
                if (VALUE) cell_value = V0 * E::psi(F, st);
            }
            if (OP == kShapeProduct && ok) {
                double D[3][3], dF[3][3], dP[3][3];
                edges(a.v, id, D);
                times_b(D, B, dF);
                E::dstress(dF, st, dP);
                to_shares(dP, B, V0, sh);
            }
            if (OP == kShapeDiagonal && ok) {
                // the product applied to the unit vector of (point k, coordinate r), of which entry (k, r) is kept: the
                // same operations on the same operands as the product's, so the same bits
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int r = 0; r < 3; ++r) {
                        double D[3][3], dF[3][3], dP[3][3], one[4][3];
#pragma unroll
                        for (int rr = 0; rr < 3; ++rr)
#pragma unroll
                            for (int c = 0; c < 3; ++c)
                                D[rr][c] = ((k == c + 1 && rr == r) ? 1.0 : 0.0) - ((k == 0 && rr == r) ? 1.0 : 0.0);
                        times_b(D, B, dF);
                        E::dstress(dF, st, dP);
                        to_shares(dP, B, V0, one);
                        sh[k][r] = one[k][r];
                    }
            }
        }
        if (OP == kShapeQuality) {
            if (a.ratio) a.ratio[a.perm ? a.perm[i] : i] = J;
        } else {
            double2* const out = reinterpret_cast<double2*>(a.shares + 12 * i);  // (96 bytes per cell: 16-byte aligned)
#pragma unroll
            for (int k = 0; k < 6; ++k) out[k] = make_double2(sh[(2 * k) / 3][(2 * k) % 3], sh[(2 * k + 1) / 3][(2 * k + 1) % 3]);
        }
    }
    if (VALUE) {
        const double tv = block_sum(cell_value, lds_v);
        const long long tn = block_sum(inverted, lds_n);
        if (threadIdx.x == 0) {
            a.value_partials[blockIdx.x] = tv;
            a.inv_partials[blockIdx.x] = tn;
        }
    }
}

__global__ __launch_bounds__(kShapeBlock) void shape_points_kernel(const double* __restrict__ shares, VertexIncidence inc, int64_t n_pts,
                                                                    double lambda, double* __restrict__ out) {
    const int64_t p = static_cast<int64_t>(blockIdx.x) * kShapeBlock + threadIdx.x;
    if (p >= n_pts) return;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    const int32_t end = inc.ptr[p + 1];
    for (int32_t e = inc.ptr[p]; e < end; ++e) {
        const double* const t = shares + 3 * static_cast<int64_t>(inc.idx[e]);
        s0 = s0 + t[0];
        s1 = s1 + t[1];
        s2 = s2 + t[2];
    }
    out[3 * p] = lambda * s0;
    out[3 * p + 1] = lambda * s1;
    out[3 * p + 2] = lambda * s2;
}

__global__ __launch_bounds__(kShapeBlock) void shape_value_kernel(const double* __restrict__ value_partials,
                                                                   const long long* __restrict__ inv_partials, int64_t n_blocks, double lambda,
                                                                   bool barrier, double* __restrict__ value, long long* __restrict__ n_inverted) {
    __shared__ double lds_v[kShapeBlock / 64];
    __shared__ long long lds_n[kShapeBlock / 64];
    double s = 0.0;
    long long n = 0;
    for (int64_t j = threadIdx.x; j < n_blocks; j += kShapeBlock) {
        s = s + value_partials[j];
        n = n + inv_partials[j];
    }
    const double ts = block_sum(s, lds_v);
    const long long tn = block_sum(n, lds_n);
    if (threadIdx.x == 0) {
        if (value) value[0] = (barrier && tn > 0) ? INFINITY : lambda * ts;
        if (n_inverted) n_inverted[0] = tn;
    }
}

__global__ __launch_bounds__(kShapeBlock) void shape_check_finite_kernel(const double* __restrict__ xyz, int64_t n,
                                                                          unsigned long long* __restrict__ counts) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kShapeBlock + threadIdx.x;
    unsigned bad = 0;
    if (i < n) {
        const double v = xyz[i];
        bad = !(v > -INFINITY && v < INFINITY);
    }
    bad = wave_sum(bad);
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(counts, static_cast<unsigned long long>(bad));  // (an integer sum: any order)
}

__global__ __launch_bounds__(kShapeBlock) void shape_rest_kernel(const int4* __restrict__ cell_vert, int64_t n_cells, ShapePoints X,
                                                                  double* __restrict__ binv, double* __restrict__ vol,
                                                                  unsigned long long* __restrict__ counts) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kShapeBlock + threadIdx.x;
    unsigned degenerate = 0;
    if (i < n_cells) {
        const int4 v4 = cell_vert[i];
        const int id[4] = {v4.x, v4.y, v4.z, v4.w};
        double Dm[3][3], C[3][3], B[3][3];
        edges(X, id, Dm);
        const double det = cofactors(Dm, C);
        double V0 = fabs(det) / 6.0;
        bool ok = V0 > 0.0 && V0 < INFINITY;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                B[r][c] = C[c][r] / det;  // the adjugate over the determinant
                ok = ok && B[r][c] > -INFINITY && B[r][c] < INFINITY;
            }
        if (!ok) {
            degenerate = 1;
            V0 = 0.0;
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) binv[9 * i + k] = ok ? B[k / 3][k % 3] : 0.0;
        vol[i] = V0;
    }
    degenerate = wave_sum(degenerate);
    if ((threadIdx.x & 63) == 0 && degenerate) atomicAdd(counts + 1, static_cast<unsigned long long>(degenerate));
}

__global__ __launch_bounds__(kShapeBlock) void shape_rest_scatter_kernel(ShapeRest r, const int32_t* __restrict__ perm, double* __restrict__ binv_out,
                                                                          double* __restrict__ vol_out, int32_t* __restrict__ vert_out) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kShapeBlock + threadIdx.x;
    if (i >= r.n_cells) return;
    const int64_t c = perm ? perm[i] : i;
    if (binv_out)
        for (int k = 0; k < 9; ++k) binv_out[9 * c + k] = r.binv[9 * i + k];
    if (vol_out) vol_out[c] = r.vol[i];
    if (vert_out) reinterpret_cast<int4*>(vert_out)[c] = r.cell_vert[i];
}

inline dim3 cells_grid(int64_t n) { return dim3(static_cast<unsigned>(shape_blocks(n))); }

template <int OP, int ENERGY, bool VALUE>
void launch_cells(hipStream_t s, const ShapeArgs& a) {
    hipLaunchKernelGGL((shape_cells_kernel<OP, ENERGY, VALUE>), cells_grid(a.rest.n_cells), dim3(kShapeBlock), 0, s, a);
}

template <int ENERGY>
void launch_cells_op(hipStream_t s, int op, bool with_value, const ShapeArgs& a) {
    if (op == kShapeGradient) {
        if (with_value) launch_cells<kShapeGradient, ENERGY, true>(s, a);
        else launch_cells<kShapeGradient, ENERGY, false>(s, a);
    } else if (op == kShapeProduct) {
        launch_cells<kShapeProduct, ENERGY, false>(s, a);
    } else {
        launch_cells<kShapeDiagonal, ENERGY, false>(s, a);
    }
}

}  // namespace

void launch_shape_check_finite(hipStream_t s, const double* xyz, int64_t n, unsigned long long* counts) {
    if (n <= 0) return;
    hipLaunchKernelGGL(shape_check_finite_kernel, cells_grid(n), dim3(kShapeBlock), 0, s, xyz, n, counts);
}

void launch_shape_rest(hipStream_t s, const int4* cell_vert, int64_t n_cells, const ShapePoints& X, double* binv, double* vol,
                       unsigned long long* counts) {
    if (n_cells <= 0) return;
    hipLaunchKernelGGL(shape_rest_kernel, cells_grid(n_cells), dim3(kShapeBlock), 0, s, cell_vert, n_cells, X, binv, vol, counts);
}

void launch_shape_rest_scatter(hipStream_t s, const ShapeRest& r, const int32_t* perm, double* binv_out, double* vol_out, int32_t* vert_out) {
    if (r.n_cells <= 0) return;
    hipLaunchKernelGGL(shape_rest_scatter_kernel, cells_grid(r.n_cells), dim3(kShapeBlock), 0, s, r, perm, binv_out, vol_out, vert_out);
}

void launch_shape_cells(hipStream_t s, int op, int energy, bool with_value, const ShapeArgs& a) {
    if (a.rest.n_cells <= 0) return;
    if (op == kShapeQuality) launch_cells<kShapeQuality, C5_SHAPE_DIRICHLET, true>(s, a);  // (J and the count: no energy enters)
    else if (energy == C5_SHAPE_DIRICHLET) launch_cells_op<C5_SHAPE_DIRICHLET>(s, op, with_value, a);
    else launch_cells_op<C5_SHAPE_NEO_HOOKEAN>(s, op, with_value, a);
}

void launch_shape_points(hipStream_t s, const double* shares, const VertexIncidence& inc, int64_t n_pts, double lambda, double* out) {
    if (n_pts <= 0) return;
    hipLaunchKernelGGL(shape_points_kernel, cells_grid(n_pts), dim3(kShapeBlock), 0, s, shares, inc, n_pts, lambda, out);
}

void launch_shape_value(hipStream_t s, const double* value_partials, const long long* inv_partials, int64_t n_blocks, double lambda,
                        bool barrier, double* value, long long* n_inverted) {
    hipLaunchKernelGGL(shape_value_kernel, dim3(1), dim3(kShapeBlock), 0, s, value_partials, inv_partials, n_blocks, lambda, barrier, value,
                       n_inverted);
}

}  // namespace c5

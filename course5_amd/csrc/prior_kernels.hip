// ------------------------------------------------------------------------------------------
// Cell-field smoothness prior: the kernels (prior_kernels.hpp; the contract: include/course5_hip.h, c5_prior_*).
// Built with -ffp-contract=off: every product below rounds before the sum that takes it, which is what lets a numpy
// restatement reproduce the quadratic operators bit for bit and keeps the vectors independent of the cells' device order.
// One lane per cell of the device's (Morton) order; no atomics in the operators, LDS only in the value's reduction.
// ------------------------------------------------------------------------------------------
#include "prior_kernels.hpp"

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
__device__ inline double block_sum(double v, double* lds /*[kPriorBlock / 64]*/) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();  // (lds may still be read from the call before)
    if (lane == 0) lds[wave] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int k = 0; k < kPriorBlock / 64; ++k) t = t + lds[k];
    return t;
}

__device__ inline void load_point(const PriorGrid& g, int id, double (&p)[3]) {
    p[0] = g.px[id];
    p[1] = g.py[id];
    p[2] = g.pz[id];
}

// A / |x_n - x_c| of the face with point ids t0 < t1 < t2 between the cells whose fourth points are apex_c and apex_n.
// The area from the ids in ascending order, so both cells of the face form the same edges; the centroids share the face's
// three points, so x_n - x_c = (apex_n - apex_c) / 4 without their cancellation, and its square does not know which cell asks.
__device__ inline double tpfa_weight(const PriorGrid& g, int t0, int t1, int t2, int apex_c, int apex_n) {
    double a[3], b[3], c[3], pc[3], pn[3];
    load_point(g, t0, a);
    load_point(g, t1, b);
    load_point(g, t2, c);
    load_point(g, apex_c, pc);
    load_point(g, apex_n, pn);
    const double e1x = b[0] - a[0], e1y = b[1] - a[1], e1z = b[2] - a[2];
    const double e2x = c[0] - a[0], e2y = c[1] - a[1], e2z = c[2] - a[2];
    const double cx = e1y * e2z - e1z * e2y;
    const double cy = e1z * e2x - e1x * e2z;
    const double cz = e1x * e2y - e1y * e2x;
    const double area = 0.5 * sqrt((cx * cx + cy * cy) + cz * cz);
    const double dx = pn[0] - pc[0], dy = pn[1] - pc[1], dz = pn[2] - pc[2];
    const double dist = 0.25 * sqrt((dx * dx + dy * dy) + dz * dz);
    return area / dist;
}

__global__ __launch_bounds__(kPriorBlock) void prior_weights_kernel(PriorGrid g, int weighting, double* __restrict__ w,
                                                                     unsigned long long* __restrict__ counts) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kPriorBlock + threadIdx.x;
    unsigned interior = 0, degenerate = 0;
    if (i < g.n_cells) {
        const int4 v4 = g.cell_vert[i];
        const int4 a4 = g.cell_adj[i];
        const int v[4] = {v4.x, v4.y, v4.z, v4.w};
        const int nb[4] = {a4.x, a4.y, a4.z, a4.w};
        double wf[4];
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            wf[f] = 0.0;
            if (nb[f] < 0) continue;
            ++interior;
            if (weighting == C5_PRIOR_UNIT) {
                wf[f] = 1.0;
                continue;
            }
            // face f leaves out point 3 - f: 0 = (0,1,2), 1 = (0,1,3), 2 = (0,2,3), 3 = (1,2,3)
            int t0 = v[f == 3 ? 1 : 0], t1 = v[f < 2 ? 1 : 2], t2 = v[f == 0 ? 2 : 3];
            if (t0 > t1) { const int s = t0; t0 = t1; t1 = s; }
            if (t1 > t2) { const int s = t1; t1 = t2; t2 = s; }
            if (t0 > t1) { const int s = t0; t0 = t1; t1 = s; }
            const int4 n4 = g.cell_vert[nb[f]];
            int apex_n = n4.w;
            if (n4.x != t0 && n4.x != t1 && n4.x != t2) apex_n = n4.x;
            else if (n4.y != t0 && n4.y != t1 && n4.y != t2) apex_n = n4.y;
            else if (n4.z != t0 && n4.z != t1 && n4.z != t2) apex_n = n4.z;
            const double t = tpfa_weight(g, t0, t1, t2, v[3 - f], apex_n);
            if (t > 0.0 && t < INFINITY) wf[f] = t;
            else ++degenerate;
        }
        double2* const out = reinterpret_cast<double2*>(w) + 2 * i;
        out[0] = make_double2(wf[0], wf[1]);
        out[1] = make_double2(wf[2], wf[3]);
    }
    interior = wave_sum(interior);
    degenerate = wave_sum(degenerate);
    if ((threadIdx.x & 63) == 0) {  // (integer sums: any order gives the same counts)
        if (interior) atomicAdd(counts, static_cast<unsigned long long>(interior));
        if (degenerate) atomicAdd(counts + 1, static_cast<unsigned long long>(degenerate));
    }
}

__global__ __launch_bounds__(kPriorBlock) void prior_weights_scatter_kernel(const double* __restrict__ w, const int32_t* __restrict__ perm,
                                                                             int64_t n_cells, double* __restrict__ w_out) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kPriorBlock + threadIdx.x;
    if (i >= n_cells) return;
    const int64_t c = perm ? perm[i] : i;
    const double2* const in = reinterpret_cast<const double2*>(w) + 2 * i;
    double2* const out = reinterpret_cast<double2*>(w_out) + 2 * c;
    out[0] = in[0];
    out[1] = in[1];
}

// psi, psi', psi'' of the header, in its order of operations
template <int PENALTY>
struct Psi;
template <>
struct Psi<C5_PRIOR_QUADRATIC> {
    static constexpr bool kCurvatureNeedsPoint = false;
    __device__ static double value(double d, double) { return 0.5 * (d * d); }
    __device__ static double slope(double d, double) { return d; }
    __device__ static double curvature(double, double) { return 1.0; }
};
template <>
struct Psi<C5_PRIOR_PSEUDO_HUBER> {
    static constexpr bool kCurvatureNeedsPoint = true;
    // From |u| = 2^256 on the penalty's linear tail is taken in closed form: there s = |u| to the last bit (1 + t rounds to t
    // from 2^27 on, and the square root of a rounded square is the number), and past 2^512 t leaves the format - without
    // the branch the slope would come back as 0 and the value as inf / inf.  A u that is inf takes the branch, a NaN does not.
    static constexpr double kTail = 0x1p256;
    // delta^2 t = d^2: formed as d * d, so that a large delta (delta^2 beyond the format, t below it) gives the quadratic's bits
    __device__ static double value(double d, double delta) {
        const double u = d / delta;
        if (fabs(u) >= kTail) return delta * (fabs(d) - delta);
        const double dd = d * d, s1 = 1.0 + sqrt(1.0 + u * u);
        if (dd < INFINITY) return dd / s1;
        return fabs(d) * (fabs(d) / s1);  // (d d beyond the format while d d / (1 + s) may be inside it)
    }
    __device__ static double slope(double d, double delta) {
        const double u = d / delta;
        if (fabs(u) >= kTail) return copysign(delta, d);
        return d / sqrt(1.0 + u * u);
    }
    __device__ static double curvature(double d, double delta) {
        const double u = d / delta;
        if (fabs(u) >= kTail) return ((1.0 / fabs(u)) / fabs(u)) / fabs(u);  // (|u|^-3, underflowing gradually to 0)
        const double q = 1.0 + u * u;
        return 1.0 / (q * sqrt(q));
    }
};

// The one body of the three operators: OP says what a face contributes.
template <int OP, int PENALTY, bool VALUE>
__global__ __launch_bounds__(kPriorBlock) void prior_apply_kernel(PriorArgs a) {
    using P = Psi<PENALTY>;
    __shared__ double lds[VALUE ? kPriorBlock / 64 : 1];
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kPriorBlock + threadIdx.x;
    const bool active = i < a.n_cells;
    int64_t c = 0;
    int64_t cn[4] = {-1, -1, -1, -1};
    double w[4] = {0.0, 0.0, 0.0, 0.0};
    if (active) {
        const int4 a4 = a.adj[i];
        const double2* const wp = reinterpret_cast<const double2*>(a.w) + 2 * i;
        const double2 w01 = wp[0], w23 = wp[1];
        w[0] = w01.x, w[1] = w01.y, w[2] = w23.x, w[3] = w23.y;
        const int nb[4] = {a4.x, a4.y, a4.z, a4.w};
        c = a.perm ? a.perm[i] : i;
#pragma unroll
        for (int f = 0; f < 4; ++f)
            if (nb[f] >= 0) cn[f] = a.perm ? a.perm[nb[f]] : nb[f];
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const PriorField fld = a.f[k];
        if (fld.lambda == 0.0) {  // (the field is left out: zeros where the caller gave an array)
            if (active && fld.out) fld.out[c] = 0.0;
            continue;
        }
        double sum = 0.0, half = 0.0;
        if (active) {
            constexpr bool need_x = OP == kPriorGradient || P::kCurvatureNeedsPoint;
            const double xc = need_x ? fld.x[c] : 0.0;
            const double pc = OP == kPriorProduct ? fld.p[c] : 0.0;
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                if (cn[f] < 0) continue;
                const double d = need_x ? xc - fld.x[cn[f]] : 0.0;
                double t;
                if (OP == kPriorGradient) {
                    t = w[f] * P::slope(d, fld.delta);
                } else {
                    const double curv = w[f] * P::curvature(d, fld.delta);
                    t = OP == kPriorProduct ? curv * (pc - fld.p[cn[f]]) : curv;
                }
                sum = sum + t;
                if (VALUE) half = half + w[f] * P::value(d, fld.delta);
            }
            fld.out[c] = fld.lambda * sum;
        }
        if (VALUE) {
            const double t = block_sum(0.5 * half, lds);
            if (threadIdx.x == 0) a.partials[static_cast<int64_t>(k) * gridDim.x + blockIdx.x] = t;
        }
    }
}

__global__ __launch_bounds__(kPriorBlock) void prior_value_kernel(const double* __restrict__ partials, int64_t n_blocks, double lambda_alpha,
                                                                   double lambda_q, double* __restrict__ value) {
    __shared__ double lds[kPriorBlock / 64];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const double lambda = k ? lambda_q : lambda_alpha;
        double s = 0.0;
        if (lambda != 0.0)
            for (int64_t j = threadIdx.x; j < n_blocks; j += kPriorBlock) s = s + partials[k * n_blocks + j];
        const double t = block_sum(s, lds);
        if (threadIdx.x == 0) value[k] = lambda != 0.0 ? lambda * t : 0.0;
    }
}

template <int OP, int PENALTY, bool VALUE>
void launch_apply(hipStream_t s, const PriorArgs& a) {
    hipLaunchKernelGGL((prior_apply_kernel<OP, PENALTY, VALUE>), dim3(static_cast<unsigned>(prior_blocks(a.n_cells))), dim3(kPriorBlock), 0, s, a);
}

template <int PENALTY>
void launch_apply_op(hipStream_t s, int op, bool with_value, const PriorArgs& a) {
    if (op == kPriorGradient) {
        if (with_value) launch_apply<kPriorGradient, PENALTY, true>(s, a);
        else launch_apply<kPriorGradient, PENALTY, false>(s, a);
    } else if (op == kPriorProduct) {
        launch_apply<kPriorProduct, PENALTY, false>(s, a);
    } else {
        launch_apply<kPriorDiagonal, PENALTY, false>(s, a);
    }
}

}  // namespace

void launch_prior_weights(hipStream_t s, const PriorGrid& g, int weighting, double* w, unsigned long long* counts) {
    if (g.n_cells <= 0) return;
    hipLaunchKernelGGL(prior_weights_kernel, dim3(static_cast<unsigned>(prior_blocks(g.n_cells))), dim3(kPriorBlock), 0, s, g, weighting, w, counts);
}

void launch_prior_weights_scatter(hipStream_t s, const double* w, const int32_t* perm, int64_t n_cells, double* w_out) {
    if (n_cells <= 0) return;
    hipLaunchKernelGGL(prior_weights_scatter_kernel, dim3(static_cast<unsigned>(prior_blocks(n_cells))), dim3(kPriorBlock), 0, s, w, perm, n_cells,
                       w_out);
}

void launch_prior_apply(hipStream_t s, int op, int penalty, bool with_value, const PriorArgs& a) {
    if (a.n_cells <= 0) return;
    if (penalty == C5_PRIOR_QUADRATIC) launch_apply_op<C5_PRIOR_QUADRATIC>(s, op, with_value, a);
    else launch_apply_op<C5_PRIOR_PSEUDO_HUBER>(s, op, with_value, a);
}

void launch_prior_value(hipStream_t s, const double* partials, int64_t n_blocks, double lambda_alpha, double lambda_q, double* value) {
    hipLaunchKernelGGL(prior_value_kernel, dim3(1), dim3(kPriorBlock), 0, s, partials, n_blocks, lambda_alpha, lambda_q, value);
}

}  // namespace c5

// What the *_resolve kernels of the derivative renders share ("algorithm" 1): bin_sort_resolve's per-pixel segment lists,
// the reference's sort and clamp of alpha, the frame that turns a thread into its pixel's sorted list, and Lambda's pre-pass.
#pragma once

#include "deriv_ray.hpp"

namespace c5 {

// bin_sort_resolve's segments (exact_kernels.hip: Segment; derivatives.hip checks the size)
struct alignas(8) AdjSegment {
    double z_hi;
    double dz;
    long long cell;
};
static_assert(sizeof(AdjSegment) == 24, "AdjSegment mirrors exact_kernels.hip's Segment");

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

// One thread of a *_resolve kernel (256 per workgroup, one per pixel of the context's rows): its pixel and that pixel's
// list, sorted.  A kernel runs its recurrence from the back of the list (i = n - 1 ... 0: the reference's order, z
// ascending).  n is 0 outside the image, on a solid-marked pixel (it shows the solid: nothing of the grid) and where the
// kernel's `wanted` says so - there the list is not sorted either.
struct ListFrame {
    int64_t lp = 0;  // the pixel among the context's rows
    bool in_image = false, masked = false;
    AdjSegment* list = nullptr;
    int n = 0;
    double x = 0.0, y = 0.0;  // (WANT_XY)
};
// WANT_XY: the pixel's coordinates are loaded too (the kernels that look faces up).  wanted(lp): loads what else the
// kernel needs of an unmasked pixel and says whether its list is to be run at all.
struct EveryList {
    __device__ bool operator()(int64_t) const { return true; }
};
template <bool WANT_XY, class Wanted = EveryList>
__device__ __forceinline__ ListFrame list_frame(const ResolveParams& R, Wanted wanted = Wanted{}) {
    ListFrame f;
    f.lp = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    f.list = static_cast<AdjSegment*>(R.segs);
    f.in_image = f.lp < static_cast<int64_t>(R.im.n_local_rows) * R.im.res_x;
    if (!f.in_image) return f;
    f.masked = R.mask && R.mask[f.lp];
    if (f.masked || !wanted(f.lp)) return f;
    if (WANT_XY) {
        const int lrow = static_cast<int>(f.lp / R.im.res_x);
        f.x = R.Xtab[f.lp - static_cast<int64_t>(lrow) * R.im.res_x];
        f.y = R.Ytab[global_row_of(R.im, lrow)];
    }
    f.list += R.offs[f.lp];
    f.n = static_cast<int>(R.offs[f.lp + 1] - R.offs[f.lp]);
    sort_segments(f.list, f.n);
    return f;
}

// Lambda of a sorted list, summed in the order the kernels' loops run (adjoint_walk<1> for a list)
__device__ __forceinline__ double lambda_total(const AdjSegment* list, int n, const GridView& g, double alpha_limit) {
    double lam = 0.0;
    for (int i = n - 1; i >= 0; --i) {
        const ClampedAlpha c = clamp_alpha(g.alpha[list[i].cell], alpha_limit);
        if (c.active) lam = lambda_add(lam, c.a, list[i].dz);
    }
    return lam;
}

}  // namespace adj
}  // namespace c5

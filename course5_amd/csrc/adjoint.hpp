// Host-callable launchers of the adjoint render (adjoint_kernels.hip): gradients of the image with respect to the cells'
// alpha and Q; and of the tangent render: the image's change for a change of them.  All launches are asynchronous on the
// given stream.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "device_types.hpp"
#include "kernels.hpp"

namespace c5 {

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
void launch_adjoint_resolve(hipStream_t s, const GridView& g, const ImageParams& im, const int64_t* offs, void* segs,
                            const uint32_t* mask, double alpha_limit, const float2* grad_out, double* grad_a, double* grad_q);

// out[perm[i]] = dev[i] for both arrays (perm nullptr: the identity)
void launch_adjoint_permute(hipStream_t s, const double* ga_dev, const double* gq_dev, const int32_t* perm, int64_t n,
                            double* ga_out, double* gq_out);

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
void launch_tangent_resolve(hipStream_t s, const GridView& g, const ImageParams& im, const int64_t* offs, void* segs,
                            const uint32_t* mask, double alpha_limit, const double2* dir, float2* out);

// bytes of one segment of the bin-sort lists as this file reads them (c_api.hip checks it against segment_bytes())
size_t adjoint_segment_bytes();

}  // namespace c5

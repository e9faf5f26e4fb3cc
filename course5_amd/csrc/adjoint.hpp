// Host-callable launchers of the adjoint render (adjoint_kernels.hip): gradients of the image with respect to the cells'
// alpha and Q.  All launches are asynchronous on the given stream.
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

// bytes of one segment of the bin-sort lists as this file reads them (c_api.hip checks it against segment_bytes())
size_t adjoint_segment_bytes();

}  // namespace c5

// ------------------------------------------------------------------------------------------
// Cell-field smoothness prior (include/course5_hip.h: c5_prior_*): what prior.hip launches and prior_kernels.hip holds.
// The contract - interior faces, the two weightings, the two penalties, the order of every sum - is the header's; the
// comments here say only how the kernels keep it.
// ------------------------------------------------------------------------------------------
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace c5 {

// the grid as prior_weights reads it: everything in the device's order, the points as the device holds them now
struct PriorGrid {
    const int4* cell_vert;  // [n_cells] the cells' four (welded) point ids
    const int4* cell_adj;   // [n_cells] neighbour across face f; every negative word: none
    const double *px, *py, *pz;
    int64_t n_cells;
};

enum PriorOp : int { kPriorGradient = 0, kPriorProduct = 1, kPriorDiagonal = 2 };

// One field (alpha or Q) of an operator call: arrays in the CALLER's cell order.
struct PriorField {
    const double* x;  // the point (may be null where the penalty is quadratic and the operator needs no value)
    const double* p;  // the product's direction (null for the others)
    double* out;      // gradient / product / diagonal (null with lambda == 0: nothing is written)
    double lambda, delta;
};

struct PriorArgs {
    const int4* adj;      // device order
    const double* w;      // [n_cells][4], device order
    const int32_t* perm;  // device index -> the caller's, or nullptr: the same
    int64_t n_cells;
    PriorField f[2];
    double* partials;     // [2][blocks]: a block's sum of its cells' halves of the value (gradient with value only)
};

constexpr int kPriorBlock = 256;
inline int64_t prior_blocks(int64_t n_cells) { return (n_cells + kPriorBlock - 1) / kPriorBlock; }

// weights [n_cells][4] in device order; counts[0] += interior (cell, face) pairs, counts[1] += those stored as 0 because
// their weight was not finite and positive (each face is seen from both sides: the host halves both)
void launch_prior_weights(hipStream_t s, const PriorGrid& g, int weighting, double* w, unsigned long long* counts);
// w_out[perm[i]][f] = w[i][f]
void launch_prior_weights_scatter(hipStream_t s, const double* w, const int32_t* perm, int64_t n_cells, double* w_out);
// op over both fields in one launch; with_value (gradient only) leaves the blocks' partial sums in a.partials
void launch_prior_apply(hipStream_t s, int op, int penalty, bool with_value, const PriorArgs& a);
// value[k] = lambda[k] * (partials[k][0] + partials[k][1] + ...): one block, a fixed tree
void launch_prior_value(hipStream_t s, const double* partials, int64_t n_blocks, double lambda_alpha, double lambda_q, double* value);

}  // namespace c5

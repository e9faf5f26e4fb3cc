// ------------------------------------------------------------------------------------------
// Shape prior (include/course5_hip.h: c5_shape_prior_*): what shape_prior.hip launches and shape_prior_kernels.hip holds.
// The contract - rest data, deformation gradient, the two energies, the order of every sum - is the header's; the comments
// here say only how the kernels keep it.
// ------------------------------------------------------------------------------------------
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "adjoint.hpp"  // VertexIncidence

namespace c5 {

enum ShapeOp : int { kShapeGradient = 0, kShapeProduct = 1, kShapeDiagonal = 2, kShapeQuality = 3 };

// Where a point's three coordinates are: p[k] = c[k][id * stride] (the caller's [n_pts][3]: stride 3 from xyz, xyz + 1,
// xyz + 2; the context's own points: stride 1 from px, py, pz)
struct ShapePoints {
    const double* c[3];
    int64_t stride;
};
inline ShapePoints shape_points_aos(const double* xyz) { return ShapePoints{{xyz, xyz ? xyz + 1 : nullptr, xyz ? xyz + 2 : nullptr}, 3}; }

// the rest data on the device, in the device's cell order
struct ShapeRest {
    const int4* cell_vert;  // [n_cells] the cells' four (welded) point ids
    const double* binv;     // [n_cells][3][3] B = Dm^-1, row-major; zeros for a degenerate cell
    const double* vol;      // [n_cells] V0; 0 for a degenerate cell
    int64_t n_cells;
};

struct ShapeArgs {
    ShapeRest rest;
    ShapePoints x;           // the point (unused where the operator ignores it)
    ShapePoints v;           // the product's direction
    double kappa;
    double* shares;          // [n_cells][4][3], device order: a cell's share of its four points' result
    double* value_partials;  // [blocks]: a block's sum of V0 psi (VALUE only)
    long long* inv_partials; // [blocks]: a block's number of inverted cells (VALUE only)
    double* ratio;           // [n_cells] J in the CALLER's cell order (kShapeQuality only; may be null)
    const int32_t* perm;     // device index -> the caller's, or nullptr: the same (kShapeQuality only)
};

constexpr int kShapeBlock = 256;
inline int64_t shape_blocks(int64_t n) { return (n + kShapeBlock - 1) / kShapeBlock; }

// counts[0] += coordinates of xyz [n] that are not finite
void launch_shape_check_finite(hipStream_t s, const double* xyz, int64_t n, unsigned long long* counts);
// B and V0 of every cell from the points X (device order); counts[1] += degenerate cells
void launch_shape_rest(hipStream_t s, const int4* cell_vert, int64_t n_cells, const ShapePoints& X, double* binv, double* vol,
                       unsigned long long* counts);
// the rest data into the caller's cell order (every output may be null)
void launch_shape_rest_scatter(hipStream_t s, const ShapeRest& r, const int32_t* perm, double* binv_out, double* vol_out, int32_t* vert_out);
// the cell launch: op over the cells; with_value leaves the blocks' partial sums and counts (gradient and quality)
void launch_shape_cells(hipStream_t s, int op, int energy, bool with_value, const ShapeArgs& a);
// the point launch: out[p][k] = lambda * (a point's incidence list of shares, added in the list's order from 0)
void launch_shape_points(hipStream_t s, const double* shares, const VertexIncidence& inc, int64_t n_pts, double lambda, double* out);
// value[0] = lambda * (partials[0] + ...), +inf where `barrier` and a cell is inverted; n_inverted[0] = the count: one block,
// a fixed tree (either output may be null)
void launch_shape_value(hipStream_t s, const double* value_partials, const long long* inv_partials, int64_t n_blocks, double lambda,
                        bool barrier, double* value, long long* n_inverted);

}  // namespace c5

// ------------------------------------------------------------------------------------------
// The ray matrix (ray_matrix_kernels.hip): per pixel the cells its ray crosses and the chord of each crossing, as CSR
// arrays - rows and fill over derivative_host.hpp and, next to them, their entry points.  And the ray Jacobian: the same
// rows with the adjoint's per-segment terms as values (jacobian_walk / jacobian_fill_resolve, scalar_derivative_kernels.hip).
// And the shape Jacobian: the same rows with the vertex adjoint's per-segment terms (shape_jacobian_walk / _resolve) and the
// faces' points and gradients (face_gradients_kernel; geometry_derivative_kernels.hip).
// ------------------------------------------------------------------------------------------
#include "derivative_host.hpp"

using namespace c5api;

namespace {

// The ray matrix's own buffer: the count per pixel ([padded] int32) and, behind them, the fill's word of changed rows.
int ray_matrix_buffer(c5_context* ctx, const DerivativeView& v, int32_t*& count, unsigned*& changed_rows) {
    C5_HIP(ctx, ctx->deriv.rm_count.ensure(static_cast<size_t>(v.padded + 1) * sizeof(int32_t)));
    count = ctx->deriv.rm_count.as<int32_t>();
    changed_rows = reinterpret_cast<unsigned*>(count + v.padded);
    return C5_OK;
}

// The ray matrix's rows: one per-view setup, the count per pixel (segment_walk<1>, which leaves the entry heads in place:
// the next per-view setup clears them; or segment_count_resolve over bin_sort_resolve's lists) and the scan into row_ptr
// [n_px + 1] on the device.
int enqueue_ray_matrix_rows(c5_context* ctx, int64_t* row_ptr) {
    DerivativeView v;
    int rc = setup_derivative(ctx, v);
    if (rc) return rc;
    if (v.no_cells || v.n_px <= 0) C5_HIP(ctx, hipMemsetAsync(row_ptr, 0, static_cast<size_t>(v.n_px + 1) * sizeof(int64_t), v.s));
    if (v.no_cells) return C5_OK;  // (solids only: every row is empty)
    int32_t* count;
    unsigned* changed_rows;
    rc = ray_matrix_buffer(ctx, v, count, changed_rows);
    if (rc) return rc;
    C5_HIP(ctx, ctx->scratch64.ensure(static_cast<size_t>(v.padded / 1024 + 1024) * sizeof(int64_t)));
    if (v.bin_sort) {
        c5::launch_segment_count_resolve(v.s, v.r, count);
    } else {
        c5::RayMatrixParams m{};
        m.w = v.w;
        m.count = count;
        c5::launch_segment_walk(v.s, m, 1);
    }
    c5::launch_scan64(v.s, count, row_ptr, v.n_px, ctx->scratch64.as<int64_t>());
    return commit_derivative(ctx, v, "ray matrix rows");
}

// A fill on a scene of solids only: every row is empty, and a row_ptr that says otherwise is another frame's; this waits
int fill_without_cells(c5_context* ctx, const DerivativeView& v, const int64_t* row_ptr, const char* what, const char* fill) {
    int64_t total = 0;
    C5_HIP(ctx, hipMemcpyAsync(&total, row_ptr + v.n_px, sizeof total, hipMemcpyDeviceToHost, v.s));
    C5_HIP(ctx, hipStreamSynchronize(v.s));
    if (total != 0)
        return fail(ctx, C5_ERR_STATE, "%s: the frame changed between c5_ray_matrix_rows and %s: "
                    "row_ptr holds %lld segments, the scene has no cells", what, fill, static_cast<long long>(total));
    return C5_OK;
}

// The frame of the three fills: a per-view setup of its own, the word of changed rows cleared, launch(v, changed_rows) - the
// fill's kernels, which write only inside [0, capacity) and count the rows that differ from row_ptr; before its last walk
// launch calls v.keep(false): the fill hands every head back cleared - and that count sent to the host behind the status
// words.  what: the fill's name in messages ("ray matrix fill"); fill: its entry point's.
template <class Launch>
int enqueue_fill(c5_context* ctx, const int64_t* row_ptr, const char* what, const char* fill, Launch launch) {
    DerivativeView v;
    int rc = setup_derivative(ctx, v);
    if (rc) return rc;
    if (v.no_cells) return fill_without_cells(ctx, v, row_ptr, what, fill);
    int32_t* count;
    unsigned* changed_rows;
    rc = ray_matrix_buffer(ctx, v, count, changed_rows);
    if (rc) return rc;
    C5_HIP(ctx, hipMemsetAsync(changed_rows, 0, sizeof(unsigned), v.s));
    rc = launch(v, changed_rows);
    if (rc) return rc;
    rc = commit_derivative(ctx, v, what);
    if (rc) return rc;
    C5_HIP(ctx, hipMemcpyAsync(ctx->deriv.adj_status + 3, changed_rows, sizeof(unsigned), hipMemcpyDeviceToHost, v.s));
    return C5_OK;
}

// The ray matrix's arrays: segment_walk<2>, or segment_fill_resolve over bin_sort_resolve's lists.
int enqueue_ray_matrix_fill(c5_context* ctx, const int64_t* row_ptr, int64_t capacity, int32_t* col, double* dz, double* z_exit) {
    return enqueue_fill(ctx, row_ptr, "ray matrix fill", "c5_ray_matrix_fill", [&](DerivativeView& v, unsigned* changed_rows) -> int {
        c5::RayMatrixParams m{};
        m.w = v.w;
        m.row_ptr = row_ptr;
        m.capacity = capacity;
        m.perm = v.perm;
        m.col = col;
        m.dz = dz;
        m.z_exit = z_exit;
        m.changed_rows = changed_rows;
        if (v.bin_sort) {
            c5::launch_segment_fill_resolve(v.s, v.r, m);
        } else {
            v.keep(false);
            c5::launch_segment_walk(v.s, m, 2);
        }
        return C5_OK;
    });
}

// The ray Jacobian's arrays: the adjoint's two passes - the Lambda pre-pass as adjoint_one runs it (adjoint_walk<1>, the
// heads left in place), then jacobian_walk, which stores where segment_walk<2> would; or jacobian_fill_resolve over
// bin_sort_resolve's lists.  Any array may be null.
int enqueue_ray_jacobian_fill(c5_context* ctx, const int64_t* row_ptr, int64_t capacity, int32_t* col, double* dz, double* dI_da,
                              double* dI_dq) {
    return enqueue_fill(ctx, row_ptr, "ray jacobian fill", "c5_ray_jacobian_fill", [&](DerivativeView& v, unsigned* changed_rows) -> int {
        const c5::JacobianRows j{row_ptr, capacity, v.perm, col, dz, dI_da, dI_dq, changed_rows};
        if (v.bin_sort) {
            c5::launch_jacobian_fill_resolve(v.s, v.r, j);
            return C5_OK;
        }
        c5::AdjointParams ap;
        const int rc = adjoint_params(ctx, v, ap);
        if (rc) return rc;
        c5::launch_adjoint_walk(v.s, ap, 1);
        v.keep(false);
        c5::launch_jacobian_walk(v.s, ap, j);
        return C5_OK;
    });
}

// The shape Jacobian's arrays: the vertex adjoint's two passes - the Lambda pre-pass (adjoint_walk<1>, the heads left in
// place), then shape_jacobian_walk, which stores where segment_walk<2> would; or shape_jacobian_resolve over
// bin_sort_resolve's lists.  Any array may be null.
int enqueue_shape_jacobian_fill(c5_context* ctx, const int64_t* row_ptr, int64_t capacity, double* dI_ddz, uint8_t* faces, double* bary) {
    return enqueue_fill(ctx, row_ptr, "ray shape jacobian fill", "c5_ray_shape_jacobian_fill", [&](DerivativeView& v, unsigned* changed_rows) -> int {
        const c5::ShapeRows j{row_ptr, capacity, dI_ddz, faces, bary, changed_rows};
        if (v.bin_sort) {
            c5::launch_shape_jacobian_resolve(v.s, v.r, j);
            return C5_OK;
        }
        c5::AdjointParams ap;
        const int rc = adjoint_params(ctx, v, ap);
        if (rc) return rc;
        c5::VertexParams vp{};
        vp.w = v.w;
        vp.geo = v.geo;
        vp.lambda = ap.lambda;
        c5::launch_adjoint_walk(v.s, ap, 1);
        v.keep(false);
        c5::launch_shape_jacobian_walk(v.s, vp, j);
        return C5_OK;
    });
}

// What both forms of a fill check of their arguments: check_derivative's (ok: the pointers it needs are there, else
// `missing`) and the capacity's sign.
int check_fill(c5_context* ctx, const char* fill, bool host, bool ok, const char* missing, int64_t capacity) {
    int rc = check_derivative(ctx, {fill, host, 1, nullptr, ok, true, missing});
    if (rc) return rc;
    if (capacity < 0) return fail(ctx, C5_ERR_INVALID, "%s: negative capacity (%lld)", fill, static_cast<long long>(capacity));
    return C5_OK;
}

// The host forms stage their arrays for row_ptr's total, which is also the capacity the kernels are given: nothing beyond
// it is written on the device or copied back.  A total the caller's capacity does not cover is refused.
int staged_elements(c5_context* ctx, const char* fill, const int64_t* row_ptr_host, int64_t capacity, int64_t& n_px, int64_t& need) {
    n_px = local_pixels(ctx->im);
    need = row_ptr_host[n_px];
    if (need < 0 || need > capacity)
        return fail(ctx, C5_ERR_INVALID, "%s: row_ptr asks for %lld elements, capacity is %lld", fill, static_cast<long long>(need),
                    static_cast<long long>(capacity));
    return C5_OK;
}

// The faces' points and gradients: one per-view setup (the cells' vertices in view space), one kernel over the cells.  No walk:
// the entry lists the setup built stay unused, and the next setup clears them (as c5_vertex_exact_finish's).
int enqueue_face_gradients(c5_context* ctx, int32_t* face_points, double* dw_dxyz) {
    DerivativeView v;
    int rc = setup_derivative(ctx, v);
    if (rc || v.no_cells) return rc;
    c5::launch_face_gradients(v.s, v.geo, ctx->n_cells, v.perm, ctx->view, face_points, dw_dxyz);
    return commit_derivative(ctx, v, "face gradients");
}

}  // namespace

extern "C" {

// Waits for the stream: *nnz is valid on return.
int c5_ray_matrix_rows_device(c5_context* ctx, void* row_ptr_dev, int64_t* nnz) {
    int rc = check_derivative(ctx, {"c5_ray_matrix_rows", false, 1, nullptr, row_ptr_dev && nnz, true, "null row_ptr or nnz pointer"});
    if (rc) return rc;
    *nnz = 0;
    int64_t* const row_ptr = static_cast<int64_t*>(row_ptr_dev);
    rc = enqueue_ray_matrix_rows(ctx, row_ptr);
    if (rc) return rc;
    C5_HIP(ctx, hipMemcpyAsync(nnz, row_ptr + local_pixels(ctx->im), sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    return c5_synchronize(ctx);
}

int c5_ray_matrix_rows(c5_context* ctx, int64_t* row_ptr_host, int64_t* nnz) {
    int rc = check_derivative(ctx, {"c5_ray_matrix_rows", true, 1, nullptr, row_ptr_host && nnz, true, "null row_ptr or nnz pointer"});
    if (rc) return rc;
    *nnz = 0;
    const int64_t n_px = local_pixels(ctx->im);
    Staged b[] = {{nullptr, row_ptr_host, static_cast<size_t>(n_px + 1) * sizeof(int64_t)}};
    rc = run_staged(ctx, "ray matrix rows", b, [&] { return enqueue_ray_matrix_rows(ctx, b[0].as<int64_t>()); });
    if (rc) return rc;
    *nnz = row_ptr_host[n_px];
    return C5_OK;
}

int c5_ray_matrix_fill_device(c5_context* ctx, const void* row_ptr_dev, int64_t capacity, void* col_dev, void* dz_dev, void* z_exit_dev) {
    int rc = check_fill(ctx, "c5_ray_matrix_fill", false, row_ptr_dev && col_dev && dz_dev, "null row_ptr, col or dz pointer", capacity);
    if (rc) return rc;
    return enqueue_ray_matrix_fill(ctx, static_cast<const int64_t*>(row_ptr_dev), capacity, static_cast<int32_t*>(col_dev),
                                   static_cast<double*>(dz_dev), static_cast<double*>(z_exit_dev));
}

int c5_ray_matrix_fill(c5_context* ctx, const int64_t* row_ptr_host, int64_t capacity, int32_t* col_host, double* dz_host,
                       double* z_exit_host) {
    int64_t n_px, need;
    int rc = check_fill(ctx, "c5_ray_matrix_fill", true, row_ptr_host && col_host && dz_host, "null row_ptr, col or dz pointer", capacity);
    if (!rc) rc = staged_elements(ctx, "c5_ray_matrix_fill", row_ptr_host, capacity, n_px, need);
    if (rc) return rc;
    const size_t n = static_cast<size_t>(need);
    Staged b[] = {{row_ptr_host, nullptr, static_cast<size_t>(n_px + 1) * sizeof(int64_t)},
                  {nullptr, col_host, n * sizeof(int32_t)},
                  {nullptr, dz_host, n * sizeof(double)},
                  {nullptr, z_exit_host, z_exit_host ? n * sizeof(double) : 0}};
    return run_staged(ctx, "ray matrix fill", b, [&] {
        return enqueue_ray_matrix_fill(ctx, b[0].as<const int64_t>(), need, b[1].as<int32_t>(), b[2].as<double>(), b[3].as<double>());
    });
}

int c5_ray_jacobian_fill_device(c5_context* ctx, const void* row_ptr_dev, int64_t capacity, void* col_dev, void* dz_dev,
                                void* dI_dalpha_dev, void* dI_dq_dev) {
    int rc = check_fill(ctx, "c5_ray_jacobian_fill", false, row_ptr_dev && (dI_dalpha_dev || dI_dq_dev),
                        "null row_ptr, or neither dI_dalpha nor dI_dq", capacity);
    if (rc) return rc;
    return enqueue_ray_jacobian_fill(ctx, static_cast<const int64_t*>(row_ptr_dev), capacity, static_cast<int32_t*>(col_dev),
                                     static_cast<double*>(dz_dev), static_cast<double*>(dI_dalpha_dev), static_cast<double*>(dI_dq_dev));
}

int c5_ray_jacobian_fill(c5_context* ctx, const int64_t* row_ptr_host, int64_t capacity, int32_t* col_host, double* dz_host,
                         double* dI_dalpha_host, double* dI_dq_host) {
    int64_t n_px, need;
    int rc = check_fill(ctx, "c5_ray_jacobian_fill", true, row_ptr_host && (dI_dalpha_host || dI_dq_host),
                        "null row_ptr, or neither dI_dalpha nor dI_dq", capacity);
    if (!rc) rc = staged_elements(ctx, "c5_ray_jacobian_fill", row_ptr_host, capacity, n_px, need);
    if (rc) return rc;
    const size_t n = static_cast<size_t>(need);
    Staged b[] = {{row_ptr_host, nullptr, static_cast<size_t>(n_px + 1) * sizeof(int64_t)},
                  {nullptr, col_host, col_host ? n * sizeof(int32_t) : 0},
                  {nullptr, dz_host, dz_host ? n * sizeof(double) : 0},
                  {nullptr, dI_dalpha_host, dI_dalpha_host ? n * sizeof(double) : 0},
                  {nullptr, dI_dq_host, dI_dq_host ? n * sizeof(double) : 0}};
    return run_staged(ctx, "ray jacobian fill", b, [&] {
        return enqueue_ray_jacobian_fill(ctx, b[0].as<const int64_t>(), need, b[1].as<int32_t>(), b[2].as<double>(), b[3].as<double>(),
                                         b[4].as<double>());
    });
}

int c5_ray_shape_jacobian_fill_device(c5_context* ctx, const void* row_ptr_dev, int64_t capacity, void* dI_ddz_dev, void* faces_dev,
                                      void* bary_dev) {
    int rc = check_fill(ctx, "c5_ray_shape_jacobian_fill", false, row_ptr_dev && (dI_ddz_dev || faces_dev || bary_dev),
                        "null row_ptr, or none of dI_ddz, faces and bary", capacity);
    if (rc) return rc;
    return enqueue_shape_jacobian_fill(ctx, static_cast<const int64_t*>(row_ptr_dev), capacity, static_cast<double*>(dI_ddz_dev),
                                       static_cast<uint8_t*>(faces_dev), static_cast<double*>(bary_dev));
}

int c5_ray_shape_jacobian_fill(c5_context* ctx, const int64_t* row_ptr_host, int64_t capacity, double* dI_ddz_host, uint8_t* faces_host,
                               double* bary_host) {
    int64_t n_px, need;
    int rc = check_fill(ctx, "c5_ray_shape_jacobian_fill", true, row_ptr_host && (dI_ddz_host || faces_host || bary_host),
                        "null row_ptr, or none of dI_ddz, faces and bary", capacity);
    if (!rc) rc = staged_elements(ctx, "c5_ray_shape_jacobian_fill", row_ptr_host, capacity, n_px, need);
    if (rc) return rc;
    const size_t n = static_cast<size_t>(need);
    Staged b[] = {{row_ptr_host, nullptr, static_cast<size_t>(n_px + 1) * sizeof(int64_t)},
                  {nullptr, dI_ddz_host, dI_ddz_host ? n * sizeof(double) : 0},
                  {nullptr, faces_host, faces_host ? n * sizeof(uint8_t) : 0},
                  {nullptr, bary_host, bary_host ? 6 * n * sizeof(double) : 0}};
    return run_staged(ctx, "ray shape jacobian fill", b, [&] {
        return enqueue_shape_jacobian_fill(ctx, b[0].as<const int64_t>(), need, b[1].as<double>(), b[2].as<uint8_t>(), b[3].as<double>());
    });
}

int c5_face_gradients_device(c5_context* ctx, void* face_points_dev, void* dw_dxyz_dev) {
    int rc = check_derivative(ctx, {"c5_face_gradients", false, 1, nullptr, true, face_points_dev && dw_dxyz_dev,
                                    "null face_points or dw_dxyz pointer"});
    if (rc) return rc;
    return enqueue_face_gradients(ctx, static_cast<int32_t*>(face_points_dev), static_cast<double*>(dw_dxyz_dev));
}

int c5_face_gradients(c5_context* ctx, int32_t* face_points_host, double* dw_dxyz_host) {
    int rc = check_derivative(ctx, {"c5_face_gradients", true, 1, nullptr, true, face_points_host && dw_dxyz_host,
                                    "null face_points or dw_dxyz pointer"});
    if (rc) return rc;
    const size_t n = 12 * static_cast<size_t>(ctx->n_cells);
    Staged b[] = {{nullptr, face_points_host, n * sizeof(int32_t)}, {nullptr, dw_dxyz_host, n * sizeof(double)}};
    return run_staged(ctx, "face gradients", b, [&] { return enqueue_face_gradients(ctx, b[0].as<int32_t>(), b[1].as<double>()); });
}

}  // extern "C"

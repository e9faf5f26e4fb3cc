// gfx950 kernels of the ray matrix (c5_ray_matrix_*): the segments every derivative render sums over, themselves - per pixel
// the cells its ray crosses, the chord of each crossing and where it ends - as CSR arrays.  Two calls with a per-view setup
// each: the count (pass 1: segment_walk<1>, then launch_scan64 over the counts) and the fill (pass 2: segment_walk<2> stores
// (cell, dz, z_exit) per segment); segment_count_resolve / segment_fill_resolve over bin_sort_resolve's lists.  The walk is
// adj::Ray's (deriv_ray.hpp), the other derivatives' chords to the bit.  Each lane owns its row and appends to it with plain
// stores: no atomics, bit-reproducible (adj::row_slot, count_changed_rows: deriv_ray.hpp, shared with the ray Jacobian).
// The two fills here spell out what adj::RowCursor does for the Jacobians' sinks: written with it they compile to other
// machine code (profiles/export_refactor.md), and what they do is to stay what was measured.
#include "deriv_lists.hpp"

namespace c5 {
namespace adj {

__device__ __forceinline__ void store_segment(const RayMatrixParams& A, long long at, int cell, double dz, double z_exit) {
    // (plain stores: a lane's next element lands in the line its last one did, and L2 merges them.  Nontemporal stores
    // took 16.1 ms against 4.96 for the benchmark frame's fill: profiles/ray_matrix.md)
    A.col[at] = A.perm ? A.perm[cell] : cell;
    A.dz[at] = dz;
    if (A.z_exit) A.z_exit[at] = z_exit;
}

}  // namespace adj

// PASS 1: the segments per pixel (int32); leaves the entry heads in place and counts as adjoint_walk<1> does.  PASS 2
// (its own per-view setup before it): the same walk, every segment stored; counts, and hands the heads back cleared.
// Nothing is shared between the lanes: a lane leaves the loop when its ray ends, as in tangent_walk.
template <int PASS>
__global__ __launch_bounds__(64) void segment_walk(RayMatrixParams A) {
    using namespace adj;
    const WalkParams& P = A.w;
    Ray r;
    unsigned k = 0;  // segments of the ray so far
    RowSlot slot;

    const EntryHead ent = ray_begin(r, P);
    if (PASS == 2 && r.in_image) slot = row_slot(A.row_ptr, r.lp, A.capacity);

    CellRegs cur;
    if (r.cell >= 0) load_cell(cur, P.xrec, r.cell);

    while (r.cell >= 0) {
        double dz, carry_next;
        const int nb = ray_step(r, P, ent, cur, dz, carry_next);
        CellRegs nxt;
        if (nb >= 0) load_cell(nxt, P.xrec, nb);

        if (is_segment(dz)) {
            // (the exit ray_step took, found again from the same registers: carry_next is already the next entry's depth
            // where the ray re-enters the grid.  The walk coordinate of "integration" 0 is view z.)
            if (PASS == 2 && k < slot.n_ok) store_segment(A, slot.base + k, r.cell, dz, step_geometry(cur, r.x, r.y).w_exit);
            ++k;
        }
        ray_advance(r, nb, carry_next);
        cur = nxt;
    }

    if (PASS == 1) {
        if (r.in_image) A.count[r.lp] = static_cast<int32_t>(k);
    } else {
        count_changed_rows(r.in_image && !(slot.fits && k == slot.n_ok), A.changed_rows);
        ray_clear_head(r, P);
    }
    ray_count(r, P);
}

// segment_walk's twins over bin_sort_resolve's lists ("algorithm" 1): the segments resolve_pixels integrates (those of
// dz > 0: the others add nothing), in the order its recurrence runs (i = n - 1 ... 0 of the sorted list).
__global__ __launch_bounds__(256) void segment_count_resolve(ResolveParams R, int32_t* __restrict__ count) {
    const AdjSegment* const segs = static_cast<const AdjSegment*>(R.segs);
    const int64_t lp = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (lp >= static_cast<int64_t>(R.im.n_local_rows) * R.im.res_x) return;
    int32_t k = 0;
    if (!(R.mask && R.mask[lp]))
        for (int64_t i = R.offs[lp]; i < R.offs[lp + 1]; ++i) k += adj::is_segment(segs[i].dz) ? 1 : 0;
    count[lp] = k;
}

__global__ __launch_bounds__(256) void segment_fill_resolve(ResolveParams R, RayMatrixParams A) {
    using namespace adj;
    const ListFrame f = list_frame<false>(R);
    bool changed = false;
    if (f.in_image) {
        const RowSlot slot = row_slot(A.row_ptr, static_cast<size_t>(f.lp), A.capacity);
        unsigned k = 0;
        for (int i = f.n - 1; i >= 0; --i) {
            if (!is_segment(f.list[i].dz)) continue;
            if (k < slot.n_ok) store_segment(A, slot.base + k, static_cast<int>(f.list[i].cell), f.list[i].dz, f.list[i].z_hi);
            ++k;
        }
        changed = !(slot.fits && k == slot.n_ok);
    }
    count_changed_rows(changed, A.changed_rows);
}

void launch_segment_walk(hipStream_t s, const RayMatrixParams& m, int pass) {
    const unsigned blocks = tile_blocks(m.w.im);
    if (!blocks) return;
    if (pass == 1) hipLaunchKernelGGL(segment_walk<1>, dim3(blocks), dim3(64), 0, s, m);
    else hipLaunchKernelGGL(segment_walk<2>, dim3(blocks), dim3(64), 0, s, m);
}

void launch_segment_count_resolve(hipStream_t s, const ResolveParams& r, int32_t* count) {
    if (const unsigned blocks = pixel_blocks(r.im)) hipLaunchKernelGGL(segment_count_resolve, dim3(blocks), dim3(256), 0, s, r, count);
}

void launch_segment_fill_resolve(hipStream_t s, const ResolveParams& r, const RayMatrixParams& m) {
    if (const unsigned blocks = pixel_blocks(r.im)) hipLaunchKernelGGL(segment_fill_resolve, dim3(blocks), dim3(256), 0, s, r, m);
}

}  // namespace c5

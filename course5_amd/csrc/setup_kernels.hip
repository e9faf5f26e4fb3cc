// gfx950 kernels of the per-view set-up, in front of the walk (walk_kernels.hip; fp64, FMA contraction allowed here).
//
//   build_records   per view: cell -> ONE 128-byte ExitRecord (device_types.hpp): the (up to three) planes a ray
//                    can LEAVE the cell through, in the walk coordinate about the absolute pixel coordinates, the
//                    neighbour words behind them, and the cell's optics (alpha, clamped alpha, 1 / alpha or Q / alpha,
//                    Q).  Replaces the per-segment plane solve line::find_polygon_intersection_z
//                    (line.cpp:150-174) and the per-step clamp/divide of
//                    line::integrate_ray_value_by_i (line.cpp:213-224).
//   entry_raster     boundary faces facing the viewer -> per-pixel entry records (CSR).
//                    Replaces the part of plane::find_intersections (plane.cpp:184-192) that
//                    discovers where a ray meets the grid; re-entries of non-convex grids
//                    are further entries of the same pixel.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "device_types.hpp"
#include "kernels.hpp"
#include "walk_common.hpp"

namespace c5 {

// One thread builds one cell's record in registers; a wavefront then writes its 64 records through a
// wave-private LDS area so that every store instruction covers 1 KiB of consecutive addresses (a
// thread storing its own 128-byte record would touch 64 different lines per instruction).
struct alignas(16) Q4 {
    uint32_t a, b, c, d;
};
constexpr int kRecPad = 9;  // 16-byte units per record in LDS: 8 + 1 pad (conflict-free b128 rows)

// How far beyond a cutting plane a cell may begin and still be listed for it / claim a pixel of it (plane_raster): the
// rounding of a point-in-cell test, generously — a claim this far off moves the start of one chord by as much.
__device__ __forceinline__ double plane_tolerance(double coord, double extent) { return 64.0 * DBL_EPSILON * (coord + extent); }

template <bool SPLIT, bool BF>
__device__ __forceinline__ void build_records_block(const GridView& g, double alpha_limit, int order, unsigned block,
                                                    Q4 (*s_rec)[64 * kRecPad]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (g.block_sphere) {  // (uniform) all of this workgroup's cells outside the context's rows?  (kernels.hpp)
        const double4 s = g.block_sphere[block];
        double cx = s.x, cy = s.y, cz = s.z;
        for (int r = 0; r < g.rot.n; ++r) {  // tetra.cpp:44-62 on the centre (its rounding is covered by the margin below)
            const double co = g.rot.cosv[r], si = g.rot.sinv[r];
            if (g.rot.axis[r] == 0) {
                const double y_old = cy;
                cy = cy * co - cz * si;
                cz = y_old * si + cz * co;
            } else {
                cx -= g.rot.x0[r];
                const double x_old = cx;
                cx = cx * co - cz * si;
                cz = x_old * si + cz * co;
                cx += g.rot.x0[r];
            }
        }
        const double reach = s.w + 1e-9 * (s.w + fabs(cy) + 1.0);
        if (cy + reach < g.cull_y_lo || cy - reach > g.cull_y_hi) return;
    }
    const int64_t cell = block * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    const int64_t wave_first = cell - lane;
    bool valid = cell < g.n_cells;
    CellRecord r;
    CellOptics o;
    double verts[4][3];
    int4 adj = make_int4(0, 0, 0, 0);
    if (valid) valid = build_cell_impl<true>(g, alpha_limit, order, cell, r, o, (SPLIT || BF) ? verts : nullptr, BF ? &adj : nullptr);
    const unsigned long long valid_mask = __builtin_amdgcn_ballot_w64(valid);
    if (valid_mask == 0ull) return;  // wave-uniform
    if (BF) {
        // The cell's boundary faces a ray can ENTER through leave a record for entry_raster_rec (device_types.hpp:
        // BFaceRecord): the vertices and the face planes are in registers here, the raster would have to find them again
        // through three dependent rounds of loads (face -> cell -> vertex ids -> coordinates).  One wavefront in sixteen
        // has a boundary cell on the C3 grid.
        const bool b_cell = valid && (adj.x <= -2 || adj.y <= -2 || adj.z <= -2 || adj.w <= -2);
        if (__builtin_amdgcn_ballot_w64(b_cell) != 0ull && b_cell) {
            const int nbv[4] = {adj.x, adj.y, adj.z, adj.w};
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                if (nbv[f] > -2) continue;
                const FacePlane fp = face_plane(verts, f);
                // walking from +z to -z a ray enters through faces the cell body lies below (upper faces); walking from -z
                // to +z through the others; an edge-on face is entered by no ray
                if (fp.kind == 0 || ((fp.kind > 0) != (g.bf_want_upper != 0))) continue;
                constexpr int FV3[4][3] = {{0, 1, 2}, {0, 1, 3}, {0, 2, 3}, {1, 2, 3}};
                const double* a = verts[FV3[f][0]];
                const double* b = verts[FV3[f][1]];
                const double* c = verts[FV3[f][2]];
                BFaceRecord rec;
                rec.ax = a[0], rec.ay = a[1], rec.bx = b[0], rec.by = b[1], rec.cx = c[0], rec.cy = c[1];
                rec.x0 = verts[0][0], rec.y0 = verts[0][1];
                rec.pc = fp.c, rec.pgx = fp.gx, rec.pgy = fp.gy;
                rec.cell_word = static_cast<uint32_t>(cell) |
                                (face_key_exponent(a[0], a[1], a[2], b[0], b[1], b[2], c[0], c[1], c[2], fp.gx, fp.gy, g.bf_key_slack) << kEntrySlackShift);
                rec.seq = g.bf_seq;
                g.bfrec[-nbv[f] - 2] = rec;
            }
        }
    }
    if (SPLIT) {
        // "depth_split": the cells that straddle a cutting plane go on the list plane_raster works through (one
        // allocation per wavefront and plane; the list has room for every cell at every plane)
        // (a vertex's depth against the planes' common tilt: plane pl passes the cell if it lies between the least and the
        // greatest of the four)
        double z_lo = 0.0, z_hi = 0.0, tol = 0.0;
        if (valid) {
            double d[4], coord = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                d[k] = verts[k][2] - fma(g.split.gx, verts[k][0], g.split.gy * verts[k][1]);
                coord = fmax(coord, fmax(fabs(verts[k][0]), fmax(fabs(verts[k][1]), fabs(verts[k][2]))));
            }
            z_lo = fmin(fmin(d[0], d[1]), fmin(d[2], d[3]));
            z_hi = fmax(fmax(d[0], d[1]), fmax(d[2], d[3]));
            tol = plane_tolerance(coord * (1.0 + fabs(g.split.gx) + fabs(g.split.gy)), z_hi - z_lo);
        }
        // The list is cut into kStraddleShards parts, each with its counter on a line of its own (thousands of wavefronts
        // adding to ONE word would serialise at ~10 ns each); a wavefront belongs to the part (its index mod 64), and a
        // part has room for everything its wavefronts could ever list (64 cells x (K - 1) planes each): no overflow.
        const unsigned shard = static_cast<unsigned>((wave_first >> 6) % kStraddleShards);
        for (int pl = 1; pl < g.split.n_slabs; ++pl) {
            const double w = g.split.w[pl];
            const bool cut = valid && z_lo <= w + tol && z_hi >= w - tol;
            const unsigned long long cut_mask = __builtin_amdgcn_ballot_w64(cut);
            if (cut_mask == 0ull) continue;
            const int leader = __builtin_ctzll(cut_mask);
            unsigned base = 0;
            if (lane == leader) base = atomicAdd(g.split.straddle_count + shard * kStraddleCounterStride, static_cast<unsigned>(__popcll(cut_mask)));
            base = static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(base), leader));
            const unsigned at = base + static_cast<unsigned>(__popcll(cut_mask & ((1ull << lane) - 1ull)));
            if (cut && at < g.split.straddle_capacity)
                g.split.straddle[static_cast<size_t>(shard) * g.split.straddle_capacity + at] = static_cast<uint32_t>(cell) | (static_cast<uint32_t>(pl - 1) << 28);
        }
    }
    Q4* const my_rec = s_rec[wave];
    if (valid) {
        ExitRecord x;
        to_exit_record(r, o, order, x);
        const Q4* rp = reinterpret_cast<const Q4*>(&x);
#pragma unroll
        for (int k = 0; k < 8; ++k) my_rec[lane * kRecPad + k] = rp[k];
    }
    __builtin_amdgcn_wave_barrier();
    Q4* const rec_out = reinterpret_cast<Q4*>(g.xrec + wave_first);
#pragma unroll
    for (int k = 0; k < 8; ++k) {  // 8 x 1 KiB: records 8k .. 8k+7 of the wavefront
        const int rec_i = k * 8 + (lane >> 3);
        if ((valid_mask >> rec_i) & 1ull) rec_out[k * 64 + lane] = my_rec[rec_i * kRecPad + (lane & 7)];
    }
}

template <bool SPLIT, bool BF>
__global__ __launch_bounds__(256) void build_records(GridView g, double alpha_limit, int order) {
    __shared__ Q4 s_rec[4][64 * kRecPad];
    build_records_block<SPLIT, BF>(g, alpha_limit, order, blockIdx.x, s_rec);
}

// entry_raster from the face records of build_records: one wavefront per boundary face, one scalar load of 96 bytes
// instead of three dependent rounds of gathers; a face without a record of THIS frame (turned away from the rays,
// edge-on, its cell outside this context's rows) costs that one load.
__global__ __launch_bounds__(256) void entry_raster_rec(GridView g, RasterArgs A) {
    const int lane = threadIdx.x & 63;
    const int64_t face_idx = __builtin_amdgcn_readfirstlane(static_cast<int>(blockIdx.x * 4u + (threadIdx.x >> 6)));
    if (face_idx >= g.n_bfaces) return;
    const BFaceRecord* __restrict__ rp = g.bfrec + face_idx;
    if (rp->seq != g.bf_seq) return;
    raster_face(A, lane, face_idx, rp->ax, rp->ay, rp->bx, rp->by, rp->cx, rp->cy, rp->x0, rp->y0, rp->pc, rp->pgx, rp->pgy, rp->cell_word);
}

__global__ __launch_bounds__(256) void entry_raster(GridView g, RasterArgs A) { entry_raster_block(g, A, blockIdx.x); }

// The per-view setup as ONE launch: record workgroups (HBM-bound: 304 bytes per cell) and raster workgroups
// (bound by vector instructions and returning atomics) interleaved, so that the two kinds of work share the GPU
// instead of running one after the other.  Neither reads what the other writes (both read the transformed vertices).
__global__ __launch_bounds__(256) void setup_fused(GridView g, double alpha_limit, int order, unsigned n_rec, unsigned n_ras,
                                                   RasterArgs A) {
    __shared__ Q4 s_rec[4][64 * kRecPad];
    const unsigned b = blockIdx.x, m = n_rec < n_ras ? n_rec : n_ras;
    const bool raster = b < 2u * m ? (b & 1u) != 0u : n_ras > n_rec;
    const unsigned idx = b < 2u * m ? b >> 1 : b - m;
    if (raster)
        entry_raster_block(g, A, idx);
    else
        build_records_block<false, false>(g, alpha_limit, order, idx, s_rec);
}

// ------------------------------------------------------------------------------------------
// plane_raster ("depth_split"): where is every ray at the cutting planes?
//
// build_records has listed the cells that straddle a plane w = w[pl] (to a tolerance).  A wavefront takes one listed
// cell: the plane cuts it in a triangle or a quadrilateral; the pixels of the cell's bounding box are tested against
// the cell's four half-spaces at depth w, in NORMAL form — s_f(x, y) = n_f . (x, y, w) - d_f, oriented so that the
// cell's fourth vertex is on the positive side: no division, vertical faces are faces like any other — and a pixel
// inside gets plane_cell[pl - 1][pixel] = stamp << 28 | cell: the cell in which the job of slab pl starts that ray, at
// depth w (walk_composite_lds<..., SPLIT>).  Two claims:
//   * inside, every s_f >= 0: a plain store — cells that share the point (it lies on a common face) both contain it,
//     whichever store lands last is right;
//   * within the rounding of the test, every s_f >= -tol_f: taken only if nobody else has claimed the pixel (compare
//     and swap against a word of another frame) — so that a point within rounding of a face never falls between the
//     two cells that share it; such a start is off by the rounding of one plane evaluation.
// A pixel no cell claims is outside the grid at that depth: its word keeps an old stamp, and the job looks for the
// ray's next boundary entry instead.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void plane_raster(GridView g, const double* __restrict__ Xtab, const double* __restrict__ Ytab,
                                                    ImageParams im) {
    const int lane = threadIdx.x & 63;
    const unsigned gw = blockIdx.x * 4u + (threadIdx.x >> 6), n_waves = gridDim.x * 4u;
    // the shards' fill counts -> one running sum across the lanes (lane k: items of shards 0 .. k)
    unsigned incl = __hip_atomic_load(g.split.straddle_count + lane * kStraddleCounterStride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    incl = incl < g.split.straddle_capacity ? incl : g.split.straddle_capacity;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned up = static_cast<unsigned>(__shfl_up(static_cast<int>(incl), d));
        if (lane >= d) incl += up;
    }
    const unsigned total = static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(incl), 63));
    if (gw == 0) g.split.straddle_count_next[lane * kStraddleCounterStride] = 0u;  // (the half the NEXT frame's build_records fills)
    for (unsigned item = gw; item < total; item += n_waves) {
        const unsigned shard = static_cast<unsigned>(__popcll(__builtin_amdgcn_ballot_w64(incl <= item)));
        const unsigned before = shard ? static_cast<unsigned>(__shfl(static_cast<int>(incl), static_cast<int>(shard) - 1)) : 0u;
        const uint32_t word = g.split.straddle[static_cast<size_t>(shard) * g.split.straddle_capacity + (item - before)];
        const uint32_t cell = word & kIdMask;
        const int pl = static_cast<int>(word >> 28) + 1;
        const double w = g.split.w[pl];
        const int4 cv = g.cell_vert[cell];
        const int vid[4] = {cv.x, cv.y, cv.z, cv.w};
        double p[4][3];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            p[k][0] = g.vx[vid[k]];
            p[k][1] = g.vy[vid[k]];
            p[k][2] = g.vz[vid[k]];
        }
        // the four half-spaces at depth w: s_f(x, y) = fa x + fb y + fc >= 0 inside
        constexpr int FV[4][4] = {{0, 1, 2, 3}, {0, 1, 3, 2}, {0, 2, 3, 1}, {1, 2, 3, 0}};
        double fa[4], fb[4], fc[4], ft[4];
        bool flat = false;
        double coord = fabs(w);
#pragma unroll
        for (int k = 0; k < 4; ++k) coord = fmax(coord, fmax(fabs(p[k][0]), fabs(p[k][1])));
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            const double* a = p[FV[f][0]];
            const double* b = p[FV[f][1]];
            const double* c = p[FV[f][2]];
            const double* o = p[FV[f][3]];
            const double ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2];
            const double vx = c[0] - a[0], vy = c[1] - a[1], vz = c[2] - a[2];
            double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
            const double side = nx * (o[0] - a[0]) + ny * (o[1] - a[1]) + nz * (o[2] - a[2]);
            if (!(side != 0.0)) flat = true;  // (no volume, or NaN: claims nothing)
            if (side < 0.0) nx = -nx, ny = -ny, nz = -nz;
            // the point of pixel (x, y) on plane pl is (x, y, w + gx x + gy y): s_f stays linear in x and y
            fa[f] = fma(nz, g.split.gx, nx);
            fb[f] = fma(nz, g.split.gy, ny);
            fc[f] = nz * (w - a[2]) - nx * a[0] - ny * a[1];
            // rounding of s_f at a pixel: a few ulps of the largest term
            ft[f] = 32.0 * DBL_EPSILON * ((fabs(nx) + fabs(ny) + fabs(nz) * (1.0 + fabs(g.split.gx) + fabs(g.split.gy))) * coord);
        }
        if (flat) continue;
        const double xmin = fmin(fmin(p[0][0], p[1][0]), fmin(p[2][0], p[3][0])), xmax = fmax(fmax(p[0][0], p[1][0]), fmax(p[2][0], p[3][0]));
        const double ymin = fmin(fmin(p[0][1], p[1][1]), fmin(p[2][1], p[3][1])), ymax = fmax(fmax(p[0][1], p[1][1]), fmax(p[2][1], p[3][1]));
        // conservative pixel box, as in entry_raster
        const double fc0 = floor((xmin - im.x_min) / im.step_x), fc1 = ceil((xmax - im.x_min) / im.step_x);
        const double fr0 = floor((ymin - im.y_min) / im.step_y), fr1 = ceil((ymax - im.y_min) / im.step_y);
        if (!(fc1 >= 0.0) || !(fr1 >= 0.0) || !(fc0 <= im.res_x - 1.0) || !(fr0 <= im.res_y - 1.0)) continue;
        const int c0 = static_cast<int>(fmax(fc0, 0.0));
        const int c1 = static_cast<int>(fmin(fc1, im.res_x - 1.0));
        const int r0 = max(static_cast<int>(fmax(fr0, 0.0)), im.row_begin);
        const int r1 = min(static_cast<int>(fmin(fr1, im.res_y - 1.0)), im.row_begin + im.row_count - 1);
        if (r1 < r0) continue;
        int lr0, lr1;
        local_row_span(im, r0, r1, lr0, lr1);
        if (lr1 < lr0) continue;
        const unsigned bw = static_cast<unsigned>(c1 - c0 + 1);
        const unsigned n_box = bw * static_cast<unsigned>(lr1 - lr0 + 1);
        uint32_t* const words = g.split.plane_cell + static_cast<size_t>(pl - 1) * g.split.plane_stride;
        const uint32_t mine = (g.split.stamp << 28) | cell;
        for (unsigned base = 0; base < n_box; base += 64u) {
            const unsigned idx = base + static_cast<unsigned>(lane);
            if (idx >= n_box) continue;
            const unsigned qrow = idx / bw, rcol = idx - qrow * bw;
            const int lrow = lr0 + static_cast<int>(qrow);
            const int col = c0 + static_cast<int>(rcol);
            const double x = Xtab[col], y = Ytab[global_row_of(im, lrow)];
            bool inside = true, near = true;
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                const double sf = fma(fa[f], x, fma(fb[f], y, fc[f]));
                inside = inside && sf >= 0.0;
                near = near && sf >= -ft[f];
            }
            uint32_t* const at = words + static_cast<size_t>(lrow) * im.res_x + col;
            if (inside) {
                *at = mine;
            } else if (near) {
                const uint32_t old = __hip_atomic_load(at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if ((old >> 28) != g.split.stamp) atomicCAS(at, old, mine);
            }
        }
    }
}

void launch_plane_raster(hipStream_t s, const GridView& g, const double* Xtab, const double* Ytab, const ImageParams& im) {
    if (g.split.n_slabs <= 1 || g.n_cells <= 0) return;
    // resident wavefronts share the listed cells between them (the list's length is on the device only)
    long long blocks = (g.n_cells + 255) / 256;
    blocks = blocks < 8 ? 8 : (blocks > 2048 ? 2048 : blocks);
    hipLaunchKernelGGL(plane_raster, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, s, g, Xtab, Ytab, im);
}


void launch_build_records(hipStream_t s, const GridView& g, double alpha_limit, int order) {
    if (g.n_cells <= 0) return;
    const unsigned blocks = static_cast<unsigned>((g.n_cells + 255) / 256);
    if (g.split.n_slabs > 1 && g.bfrec)
        hipLaunchKernelGGL((build_records<true, true>), dim3(blocks), dim3(256), 0, s, g, alpha_limit, order);
    else if (g.split.n_slabs > 1)
        hipLaunchKernelGGL((build_records<true, false>), dim3(blocks), dim3(256), 0, s, g, alpha_limit, order);
    else if (g.bfrec)
        hipLaunchKernelGGL((build_records<false, true>), dim3(blocks), dim3(256), 0, s, g, alpha_limit, order);
    else
        hipLaunchKernelGGL((build_records<false, false>), dim3(blocks), dim3(256), 0, s, g, alpha_limit, order);
}

void launch_entry_lists(hipStream_t s, const GridView& g, const double* Xtab, const double* Ytab,
                        const ImageParams& im, EntryHead* head, Entry* first, Entry* pool, int64_t capacity,
                        FrameCounters* counters, unsigned* sticky, int want_upper, double key_slack, uint32_t* tile_flag,
                        uint32_t tile_stamp) {
    if (g.n_bfaces <= 0) return;
    const unsigned blocks = static_cast<unsigned>((g.n_bfaces + 3) / 4);
    const RasterArgs A{Xtab, Ytab, im, head, first, pool, capacity, counters, sticky, want_upper, key_slack, tile_flag, tile_stamp,
                       (im.res_x + 7) / 8};
    if (g.bfrec)
        hipLaunchKernelGGL(entry_raster_rec, dim3(blocks), dim3(256), 0, s, g, A);
    else
        hipLaunchKernelGGL(entry_raster, dim3(blocks), dim3(256), 0, s, g, A);
}

void launch_setup_fused(hipStream_t s, const GridView& g, double alpha_limit, int order, const double* Xtab, const double* Ytab,
                        const ImageParams& im, EntryHead* head, Entry* first, Entry* pool, int64_t capacity,
                        FrameCounters* counters, unsigned* sticky, int want_upper, double key_slack) {
    const unsigned n_rec = g.n_cells > 0 ? static_cast<unsigned>((g.n_cells + 255) / 256) : 0u;
    const unsigned n_ras = g.n_bfaces > 0 ? static_cast<unsigned>((g.n_bfaces + 3) / 4) : 0u;
    if (n_rec + n_ras == 0u) return;
    const RasterArgs A{Xtab, Ytab, im, head, first, pool, capacity, counters, sticky, want_upper, key_slack, nullptr, 0u, 0};
    hipLaunchKernelGGL(setup_fused, dim3(n_rec + n_ras), dim3(256), 0, s, g, alpha_limit, order, n_rec, n_ras, A);
}

}  // namespace c5

// gfx950 kernels of the render hot path (fp64; FMA contraction allowed here).  The per-view set-up in front of them
// (build_records, entry_raster, plane_raster) is in setup_kernels.hip; what the two walks share in walk_steps.hpp,
// the launch plan and the block-to-tile mapping in walk_plan.hpp, the diagnostic builds' machinery in walk_stamps.hpp.
//
//   walk_composite   one lane per pixel: face-adjacency walk along z; tau and the
//                    emission/absorption integral, either back to front in the reference's own
//                    arithmetic (default) or front to back with a transmittance early-out.
//                    Replaces plane::trace_rays' loop body (plane.cpp:161-169):
//                    line::calculate_intersections + std::sort (line.cpp:84-148),
//                    direct_calculate_ray_value (line.cpp:176-193) and
//                    integrate_ray_value_by_i (line.cpp:195-227), fp32 store (plane.cpp:165-166).
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdio>
#include <cstdlib>

#include "device_types.hpp"
#include "kernels.hpp"
#include "walk_common.hpp"
#include "walk_plan.hpp"
#include "walk_stamps.hpp"
#include "walk_steps.hpp"

namespace c5 {

int64_t walk_tiles(const ImageParams& im) {
    const int64_t tiles_x = (im.res_x + 7) / 8, tiles_y = (im.n_local_rows + 7) / 8;
    return tiles_x * tiles_y;
}

// ------------------------------------------------------------------------------------------
// walk_composite
// ------------------------------------------------------------------------------------------
// ORDER 0: walk from -z to +z and integrate back to front exactly like
//          line::integrate_ray_value_by_i (the reference sorts by z_hi descending and runs the
//          recurrence from the last element, line.cpp:138,206).  Default: parity first.
// ORDER 1: walk from +z (the viewer) to -z, I = sum_k T_k S_k with the transmittance early-out
//          (wavefront-uniform skip of the exp work once every lane's T fell below the cut-off).
//          Algebraically identical; differs from ORDER 0 by rounding only where the reference's
//          recurrence is itself well conditioned.
//
// Structure of a step (one cell of one ray): the record of the current cell is already in
// registers; its three candidate planes give the exit face and therefore the next cell; the loads of
// the NEXT cell's record are issued right there, and the exp/divide work of the CURRENT cell runs
// while they are in flight.  Face selection is branch-free (selects), so a step has two
// data-dependent branches only: "this cell contributes" and "the ray left the grid".
// (CellRegs, load_cell, step_geometry: walk_common.hpp; emission_step: walk_steps.hpp)
template <int TILE, int ORDER>
__global__ __launch_bounds__(256) void walk_composite(WalkParams P) {
    using TS = TileShape<TILE>;
    constexpr int TW = TS::WW * TS::GX, TH = TS::WH * TS::GY;
    constexpr bool kUp = (ORDER == 0);  // walking towards +z
    const ImageParams& im = P.im;
    const int tiles_x = (im.res_x + TW - 1) / TW;
    const int tiles_y = (im.n_local_rows + TH - 1) / TH;

    int tx, ty, slab;
    if (!tile_of_block<false, false>(blockIdx.x, P.xcd_mode, tiles_x, tiles_y, P.band_tiles, 1, 0, nullptr, tx, ty, slab)) return;

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = tx * TW + (wave % TS::GX) * TS::WW + (lane % TS::WW);
    const int lrow = ty * TH + (wave / TS::GX) * TS::WH + (lane / TS::WW);
    const bool in_image = (col < im.res_x) && (lrow < im.n_local_rows);

    unsigned n_seg = 0, n_step = 0, is_solid = 0, overflow = 0;
    bool skipped = false;        // the ray met an entry inside a stretch it had walked (next_entry): interpenetrating components
    double key_taken = -DBL_MAX; // key of the entry the ray took last
    double tau = 0.0, I = 0.0, T = 1.0;
    double x = 0.0, y = 0.0, w_cur = -DBL_MAX, carry = 0.0;  // carry: the depth (walk coordinate) at which the ray entered the current cell
    EntryHead ent{0, 0};
    int cell = -1;
    size_t lp = 0;
    float2 result = make_float2(0.f, 0.f);

    if (in_image) {
        lp = static_cast<size_t>(lrow) * im.res_x + col;
        const uint32_t mv = P.mask ? P.mask[lp] : 0u;
        if (mv) {
            // line.cpp:177-179,197-199: a solid-marked pixel returns the mark on both channels
            double colour = 0.0;
            for (int s = 0; s < P.solids.n_slots; ++s)
                if (mv == static_cast<uint32_t>(s) + 1u) colour = P.solids.colour[s];
            result.x = static_cast<float>(colour);
            result.y = result.x;
            is_solid = 1;
        } else {
            x = P.Xtab[col];
            y = P.Ytab[global_row_of(im, lrow)];
            // touched once per frame: keep them from displacing the cell records in L2 / Infinity Cache
            ent = load_entry_head(P.entry_head + lp);
            if (ent.count > 0) cell = next_entry<kUp>(P, lp, ent, w_cur, carry, -DBL_MAX, -DBL_MAX, skipped);
            key_taken = w_cur;
        }
    }

    CellRegs cur;
    if (cell >= 0) load_cell(cur, P.xrec, cell);

    while (cell >= 0) {
        const StepGeometry sg = step_geometry(cur, x, y);
        ++n_step;
        const bool has_exit = sg.w_exit < INFINITY;
        const double dz = sg.w_exit - carry;  // line.cpp:124-131: the chord through the cell
        const bool contributes = dz > 0.0 && dz < INFINITY;

        // where next?
        int nb = -1;
        double carry_next = carry;
        if (has_exit) {
            carry_next = sg.w_exit;
            w_cur = fmax(w_cur, sg.w_exit);
            const uint32_t id = sg.w_out & kIdMask;
            if (id != kNoCell) nb = static_cast<int>(id);
        }
        if (nb >= 0 && n_step >= P.max_steps) {  // malformed grid: never spin
            overflow = 1;
            nb = -1;
        } else if (nb < 0 && !overflow) {
            // left the grid: re-entry of a non-convex grid?
            nb = next_entry<kUp>(P, lp, ent, w_cur, carry_next, key_taken, has_exit ? sg.w_exit : -DBL_MAX, skipped);
            key_taken = w_cur;
        }

        // issue the next cell's loads now; the arithmetic below does not depend on them
        CellRegs nxt;
        if (nb >= 0) load_cell(nxt, P.xrec, nb);

        if (contributes) {
            ++n_seg;
            tau = fma(dz, cur.r6.a, tau);  // line.cpp:189 (unclamped alpha)
            const Light l = emission_step<ORDER>(I, T, P.t_cutoff, cur.r6.b, cur.r7.a, cur.r7.b, dz, false);
            I = l.I, T = l.T;
        }
        cell = nb;
        carry = carry_next;
        cur = nxt;
    }

    if (in_image) {
        if (!is_solid) {
            result.x = static_cast<float>(tau);  // plane.cpp:165
            result.y = static_cast<float>(I);    // plane.cpp:166
        }
        if (!P.keep_entries) __builtin_nontemporal_store(0ll, reinterpret_cast<long long*>(P.entry_head + lp));  // cleared for the next frame
        __builtin_nontemporal_store(result.x, &P.out[lp].x);
        __builtin_nontemporal_store(result.y, &P.out[lp].y);
    }

    if (P.row_cost) post_row_cost<TILE>(P, lane, lrow, n_seg);

    // per-wavefront statistics -> one atomic each
    const unsigned s_seg = wave_sum_u32(n_seg);
    const unsigned s_step = wave_sum_u32(n_step);
    const unsigned s_cov = wave_sum_u32(n_seg > 0 ? 1u : 0u);
    const unsigned s_sol = wave_sum_u32(is_solid);
    const unsigned s_ovf = wave_sum_u32(overflow);
    const unsigned s_ent = wave_sum_u32(static_cast<unsigned>(ent.count));
    const unsigned s_skip = static_cast<unsigned>(__popcll(__builtin_amdgcn_ballot_w64(skipped)));
    if (lane == 0) {
        count_overlap(P, s_skip);
        count_frame(P, counter_shard(P.counters, blockIdx.x * 4u + static_cast<unsigned>(threadIdx.x >> 6)), s_seg, s_step, s_cov, s_ent, s_sol, s_ovf);
    }
}

// ------------------------------------------------------------------------------------------
// walk_composite_lds: the same walk with the current cells staged through LDS.
//
// Neighbouring pixels of a row tile are mostly inside the same cell, so per step a wavefront
// needs only a handful of distinct 128-byte records, not 64.  The direct kernel still issues
// eight 16-byte loads per lane and step and is bound by the CU's vector-memory address path.
// Here the wavefront
//   1. gives every DISTINCT next-cell id among its lanes a slot (leader election: elect_slots),
//   2. loads each slot's record ONCE, cooperatively: 8 lanes x 16 B per ExitRecord (one 128-byte line),
//   3. parks the pieces in a wave-private LDS area (144-byte stride: conflict-free b128 reads),
//   4. and every lane reads its own cell's record from LDS (lanes of a run broadcast).
// The global loads of step k+1 are issued as soon as the exit face of step k is known and are in
// flight during step k's exp/divide work, as in the direct kernel.
//
// DMA (option "lds_stage" 2): the staging loads write LDS themselves (global_load_lds_dwordx4: destination =
// wave-uniform base + 16 * lane, no vector register in between, no ds_write_b128 — a 16-byte LDS store costs 13
// LDS cycles per wave-instruction, a step's three as much as its ten reads), and a step's emission/absorption is
// integrated at once, behind its geometry — nothing carried to the next iteration, ten registers fewer.  The
// register-staged kernel integrates it in the shadow of the next step's loads (the `pend` values).
// SLOTS: distinct cells staged per wavefront and step: 14 (two DMA passes of seven), or 21 (three) for frames whose
// pixels are coarse against the cells: more distinct cells per 8x8 tile — the host picks by the rays per cell of the
// frame before (c_api.hip).
// SMALLEXP: every exp argument of the frame lies in (-1/8, 0] (WalkParams::small_exp_only): only the short series.
// SPLIT ("depth_split", device_types.hpp: SplitParams): every tile is walked by P.split.n_slabs jobs, one per slab of
// depth; a job leaves partial results and the tile's last job to arrive composes them.  ORDER 0, one wavefront per
// workgroup.  Everything it adds is compiled out of the whole-ray instantiations.
// ------------------------------------------------------------------------------------------
template <int TILE, int ORDER, bool DMA = false, int SLOTS = kStageSlots, bool SMALLEXP = false, bool SPLIT = false>
__global__ __launch_bounds__(256, DMA ? ((SLOTS > 16 || SPLIT) ? 7 : kDmaWaves) : kWalkWaves) void walk_composite_lds(WalkParams P) {
    static_assert(!SPLIT || (ORDER == 0 && DMA && TileShape<TILE>::GX * TileShape<TILE>::GY == 1), "depth_split: reference order, LDS-DMA, one wavefront per workgroup");
    using TS = TileShape<TILE>;
    constexpr int TW = TS::WW * TS::GX, TH = TS::WH * TS::GY;
    constexpr bool kUp = (ORDER == 0);
    constexpr bool kEmitNow = DMA;
    constexpr int kWaves = TileShape<TILE>::GX * TileShape<TILE>::GY;  // wavefronts per workgroup
    __shared__ V2 s_stage[kWaves][SLOTS * kSlotStride];
    __shared__ int s_elect[kWaves][kElectInts];
    __shared__ double s_scur[kWaves][64];

    const ImageParams& im = P.im;
    const int tiles_x = (im.res_x + TW - 1) / TW;
    const int tiles_y = (im.n_local_rows + TH - 1) / TH;
    // block -> (tx, ty, slab), or no tile: tile_of_block<SPLIT, true>, its body in place (tile_of_block_body.hpp says why)
    int tx, ty, slab;
    {
        constexpr bool kLdsKernel = true;
        const unsigned block = blockIdx.x;
        const int32_t &xcd_mode = P.xcd_mode, &band_tiles = P.band_tiles, &n_slabs = P.split.n_slabs, &n_sb_rows = P.n_sb_rows;
        const uint8_t* const sb_order = P.sb_order;
#define C5_NO_TILE return
#include "tile_of_block_body.hpp"
#undef C5_NO_TILE
    }
    // SPLIT: this job's slab of depth [w_lo, w_hi) at the lane's pixel (the first from -DBL_MAX, the last to +DBL_MAX; the
    // planes share a tilt: device_types.hpp); w_lo is wanted at the start and at re-entries only and is worked out there
    double w_hi = DBL_MAX;
    auto slab_lo = [&](double px, double py) { return SPLIT ? P.split.w[slab] + fma(P.split.gx, px, P.split.gy * py) : -DBL_MAX; };

    // Registers are what caps the resident wavefronts here, so per-lane state the steps do not need
    // (pixel index, entry head, solid colour, s_cur) is NOT carried through the loop: it is recomputed
    // or re-read on the rare paths that want it (start, re-entry, end).
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // uniform: LDS bases stay scalar
    auto pixel_col = [&]() { return tx * TW + (wave % TS::GX) * TS::WW + (lane % TS::WW); };
    auto pixel_lrow = [&]() { return ty * TH + (wave / TS::GX) * TS::WH + (lane / TS::WW); };
    auto pixel_index = [&]() { return static_cast<size_t>(pixel_lrow()) * im.res_x + pixel_col(); };
    // the same from a lane index the compiler cannot trace back to `lane`: on the rare paths inside and behind the loop the
    // pixel's index is then COMPUTED there (three instructions) instead of being hoisted in front of the loop and spilled
    auto pixel_index_rare = [&]() {
        int l = lane;
        asm volatile("" : "+v"(l));
        const int c = tx * TW + (wave % TS::GX) * TS::WW + (l % TS::WW), r = ty * TH + (wave / TS::GX) * TS::WH + (l / TS::WW);
        return static_cast<size_t>(r) * im.res_x + c;
    };
    const bool in_image = (pixel_col() < im.res_x) && (pixel_lrow() < im.n_local_rows);
    V2* const my_stage = s_stage[wave];
    int* const my_elect = s_elect[wave];
    double* const my_scur = s_scur[wave];  // s_cur of every lane: only read and written around (re-)entries
    // records and optics are addressed as a uniform base + a 32-bit byte offset per lane (the host
    // only picks this kernel while n_cells * 128 fits 32 bits): one shift-or per load instead of a
    // 64-bit shift and a 64-bit add
    const char* const rec_bytes = reinterpret_cast<const char*>(P.xrec);

    unsigned n_seg = 0;
    unsigned n_step_wave = 0;  // wave-uniform: lane-steps taken by the whole wavefront
    double tau = 0.0, I = 0.0, T = 1.0;
    double tauc = 0.0;  // SPLIT: sum of dz * clamped alpha over the job's cells: exp(-tauc) is what the job does to the I below it
    double x = 0.0, y = 0.0;
    double carry = 0.0;  // the depth (walk coordinate) at which the ray entered the cell it is about to cross
    int nb = -1;

    {
        // Most wavefronts of a frame see neither the grid nor a solid (70 % on the C3 frame): they store
        // their zeros and leave at once (their entry heads are zero already).  An empty pixel used to
        // cost as much as six ray-cell segments.
        size_t lp = 0;
        uint32_t mv = 0;
        EntryHead ent{0, 0};
        // (round 4) The raster marks the tiles that hold an entry (RasterArgs::tile_flag).  One scalar load says whether this
        // one does: if not, the zeros are stored without reading 64 entry heads; if so, heads, first entries and pixel
        // coordinates are asked for in ONE round of loads instead of two dependent ones.  (Default tile shape; no solids.)
        const bool flagged = (TILE == 3) && P.tile_flag != nullptr;
        bool tile_has_entries = true;
        if (flagged) tile_has_entries = P.tile_flag[static_cast<size_t>(ty) * tiles_x + tx] == P.tile_stamp;  // (uniform address)
        double first_z = 0.0;
        uint32_t first_cell = 0u;
        if (in_image) {
            lp = pixel_index();
            mv = P.mask ? P.mask[lp] : 0u;
            if (tile_has_entries) {
                // touched once per frame: keep them from displacing the cell records in L2 / Infinity Cache
                ent = load_entry_head(P.entry_head + lp);
                if (flagged) {
                    const Entry first_ahead = P.entry_first[lp];
                    first_z = first_ahead.z;
                    first_cell = first_ahead.cell;
                    x = P.Xtab[pixel_col()];
                    y = P.Ytab[global_row_of(im, pixel_lrow())];
                }
            }
        }
        if (__builtin_amdgcn_ballot_w64(mv != 0u || ent.count != 0) == 0ull) {
            // (SPLIT: every job of the tile comes to the same verdict; the first one writes the zeros)
            if (in_image && slab == 0) {
                __builtin_nontemporal_store(0.f, &P.out[lp].x);
                __builtin_nontemporal_store(0.f, &P.out[lp].y);
            }
            return;
        }
        if (in_image && !mv) {  // (a solid-marked pixel is written at the end, without a walk)
            if (!flagged) {
                x = P.Xtab[pixel_col()];
                y = P.Ytab[global_row_of(im, pixel_lrow())];
            }
            double w_cur = -DBL_MAX;
            bool skipped = false;
            const double w_lo = slab_lo(x, y);
            if (SPLIT) w_hi = P.split.w[slab + 1] + fma(P.split.gx, x, P.split.gy * y);
            if (SPLIT && slab > 0 && ent.count > 0) {
                // where is the ray at the cutting plane?  (plane_raster; a word of another frame: nowhere inside the grid)
                // Only a ray with a boundary entry can be inside the grid anywhere: plane_raster claims a pixel within
                // rounding of a cell's faces, entry_raster takes closed triangles exactly, and a pixel on an edge-on
                // silhouette that the first claims and the second does not would get the slabs above the first plane only.
                const uint32_t pc = P.split.plane_cell[static_cast<size_t>(slab - 1) * P.split.plane_stride + lp];
                if ((pc >> 28) == P.split.stamp) {
                    nb = static_cast<int>(pc & kIdMask);
                    carry = w_lo;
                }
            }
            if (nb < 0 && ent.count > 0)
                nb = next_entry<kUp>(P, lp, ent, w_cur, carry, -DBL_MAX, -DBL_MAX, skipped, w_lo, w_hi, flagged, first_z, first_cell);
            my_scur[lane] = w_cur;  // the key of the entry taken (-DBL_MAX: started from a plane)
        }
    }
    my_elect[kSlotIds + lane] = 0;  // slot ids: always a valid cell id, whatever the slot's state
    // (recomputed where it is wanted: nothing to keep in a register across the loop)
    auto fc_job = [&]() { return counter_shard(P.counters, blockIdx.x * 4u + static_cast<unsigned>(wave)); };
    // one tile in sixteen (the first of its super-block; 1 x 1 where the launch has no super-blocks) speaks for the estimates
    const bool sampler = P.xcd_mode != 2 || ((tx % P.band_tiles) == 0 && (ty % P.band_tiles) == 0);
    {   // the shallowest depth at which a ray of this job starts (c_api.hip places the next frame's cutting planes by it)
        double lo = nb >= 0 ? carry : DBL_MAX;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) lo = fmin(lo, __shfl_xor(lo, d));
        if (lane == 0 && lo < DBL_MAX && sampler) atomicMax(&fc_job()->entry_min_key, depth_key(-lo));
    }

    // contribution of the step whose record is being replaced (integrated while the next loads fly)
    // (optics kept as the two 16-byte halves they are read in: {alpha_raw, alpha_c}, {aux, q})
    bool pend = false;
    double pend_dz = 0.0;
    V2 pend_o0 = {0.0, 0.0}, pend_o1 = {0.0, 0.0};

    // lane-constant pieces of the staging addresses
    static_assert(SLOTS <= 32, "slot ids live in 64 ints; the register path stages passes of 8 slots");
    constexpr int kPasses = (SLOTS + 7) / 8;  // register path: 8 slots (8 lanes x 16 B each) per pass
    const int piece = lane & 7, sub = lane >> 3;
    const uint32_t rec_piece_off = static_cast<uint32_t>(piece) * 16u;
    V2* const put_rec = my_stage + sub * kSlotStride + piece;         // + 8 * pass * kSlotStride
    // DMA: a pass stages kDmaSlots = 7 whole slots (63 lanes, of which the seven pad lanes and lane 63 idle), so that a
    // lane fetches the same piece of the same slot-within-the-pass in every pass: two registers hold where that
    // slot's cell id is posted and the piece's offset inside the cell's 128-byte line.
    // Pass j: slots 7 j ... 7 j + 6, LDS units from 63 j.
    constexpr int kDmaPasses = (SLOTS + kDmaSlots - 1) / kDmaSlots;
    uint32_t dma_id_at = 0, dma_off = 0;
    if (DMA) {
        const uint32_t ids_at = (uint32_t)(uintptr_t)(LdsInts)(my_elect + kSlotIds);  // LDS byte address
        const int s_ = lane / kSlotStride, pc = lane - s_ * kSlotStride;
        const bool has = s_ < kDmaSlots && pc < 8;
        // (idle lanes: a slot no pass ever stages — still an address inside the workgroup's LDS, so that the id reads
        // below need no predicate and are all in flight before the first load is issued)
        dma_id_at = ids_at + 4u * static_cast<uint32_t>(has ? s_ : 60);
        dma_off = 16u * static_cast<uint32_t>(pc & 7);
    }

    // A lane steps in every iteration from its start to its end (re-entry takes no extra iteration), so
    // the wave-uniform iteration count IS the step count of every lane still walking: the guard
    // against malformed grids (never spin) is one scalar compare per iteration.
    WalkClock clock;
    clock.begin();
    // (the bound against malformed grids, made opaque: read straight from the kernel arguments the compiler re-loaded it -
    // a scalar memory load and its wait - at the head of EVERY step rather than keep it in a register)
    uint32_t max_steps = P.max_steps;
    asm volatile("" : "+s"(max_steps));
    for (unsigned iter = 0;; ++iter) {
        const bool need = nb >= 0;
        const unsigned long long needs = __builtin_amdgcn_ballot_w64(need);
        if (needs == 0ull) break;
        if (iter >= max_steps) {
            if (need) n_seg |= kOverflowBit;
            break;
        }
        n_step_wave += static_cast<unsigned>(__popcll(needs));

        // 1. lanes in the same cell -> one slot.
        int n_runs;
        const int slot = elect_slots(my_elect, need, needs, nb, lane, n_runs);
        // (kept in a scalar register by hand: as a plain min() the compiler compared it on the vector unit)
        const int n_runs_s = __builtin_amdgcn_readfirstlane(n_runs);  // (the count of a ballot: uniform; said so, it is compared on the scalar unit)
        const int n_staged = n_runs_s < SLOTS ? n_runs_s : SLOTS;
        clock.elected(needs, nb, lane, n_runs);
        C5_STAMP(clock, 0);  // lanes -> slots
        // 2. cooperative loads into registers: kPasses passes of 8 slots (8 lanes x 16 B per record)
        //    + one pass for the optics (2 lanes per slot).  Measured on the C3 frame (same GPU): 24
        //    slots 1.31 ms, 32 slots 1.24 ms, 40 slots 1.38 ms and 48 slots 1.31 ms (registers); a
        //    second staging round instead of the direct-load fallback 1.41 ms.
        //    A pass none of whose slots is in use is skipped (wave-uniform branch).
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wsometimes-uninitialized"
#pragma clang diagnostic ignored "-Wconditional-uninitialized"
        V2 stage_r[kPasses];  // a skipped pass leaves its register undefined; it is never stored either
#pragma clang diagnostic pop
        if (DMA) {
            const uint32_t ids_end = (uint32_t)(uintptr_t)(LdsInts)(my_elect + kSlotIds) + 4u * static_cast<uint32_t>(n_staged);
            uint32_t id_of_pass[kDmaPasses];
#pragma unroll
            for (int j = 0; j < kDmaPasses; ++j) id_of_pass[j] = static_cast<uint32_t>(((LdsInts)(uintptr_t)dma_id_at)[kDmaSlots * j]);
#pragma unroll
            for (int j = 0; j < kDmaPasses; ++j) {
                // (the lanes' own test says it all; a wave-uniform "does the pass reach a staged slot at all" in front of
                // it cost three scalar instructions per step and saved a skipped branch in half of them)
                if (dma_id_at < ids_end - 4u * kDmaSlots * j) {  // this lane's slot kDmaSlots j + s is staged (idle lanes: never)
                    const uint32_t off = (id_of_pass[j] << 7) + dma_off;
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(rec_bytes + off),
                                                     (__attribute__((address_space(3))) void*)(my_stage + kDmaSlots * kSlotStride * j), 16, 0, 0);
                }
            }
        } else {
#pragma unroll
            for (int pass = 0; pass < kPasses; ++pass) {  // fully unrolled: stage_r[] stays in registers
                if (pass == 0 || 8 * pass < n_staged) {
                    const uint32_t id_ = static_cast<uint32_t>(my_elect[kSlotIds + 8 * pass + sub]);
                    stage_r[pass] = *reinterpret_cast<const V2*>(rec_bytes + ((id_ << 7) | rec_piece_off));
                }
            }
        }
        C5_STAMP(clock, 1);  // slot ids read back, staging loads issued

        // ... while they are in flight: emission/absorption of the step just taken
        if (!kEmitNow) {
            // (wave-uniform choice of the exp: every pending lane's argument within (-1/8, 0] -> the short series)
            const bool big_arg = pend && !(pend_o0.y * pend_dz < -kSmallExpArg);
            const bool short_exp = SMALLEXP || __builtin_amdgcn_ballot_w64(big_arg) == 0ull;
            if (pend) {
                if (ORDER == 0) {
                    if (pend_o0.y != 0.0)  // line.cpp:220-224
                        I = short_exp ? reference_emission_step<true>(I, pend_o0.y, pend_o1.y, pend_o1.x, pend_dz)
                                      : reference_emission_step<false>(I, pend_o0.y, pend_o1.y, pend_o1.x, pend_dz);
                } else if (T >= P.t_cutoff) {
                    const double ex = short_exp ? exp_small_nonpositive(-pend_o0.y * pend_dz) : exp_nonpositive(-pend_o0.y * pend_dz);
                    I = fma(T * pend_o1.x, 1.0 - ex, I);
                    T *= ex;
                }
                pend = false;
            }
        }
        C5_STAMP(clock, 2);  // emission/absorption of the previous step

        // 3. park the pieces in LDS (the previous step's reads are long done: same wavefront, in order)
        __builtin_amdgcn_wave_barrier();
        if (DMA) {
            // nothing orders a ds_read behind this wavefront's own LDS-DMA but its vmcnt
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        } else {
#pragma unroll
            for (int pass = 0; pass < kPasses; ++pass)
                if (sub < n_staged - 8 * pass) put_rec[8 * pass * kSlotStride] = stage_r[pass];
        }
        __builtin_amdgcn_wave_barrier();
        clock.parked();

        // 4. every ray fetches its cell: eight 16-byte reads (the planes it can leave through, the neighbours behind
        //    them, the optics)
        if (need) {
            CellRegs cur;
            const V2* r = reinterpret_cast<const V2*>(reinterpret_cast<const char*>(my_stage) +
                                                      __umul24(static_cast<unsigned>(slot), kSlotStride * 16u));
            auto read_staged = [&]() {
                cur.r0 = as_d2(r[0]);
                cur.r1 = as_d2(r[1]);
                cur.r2 = as_d2(r[2]);
                cur.r3 = as_d2(r[3]);
                cur.r4 = as_d2(r[4]);
                cur.r5 = as_d2(r[5]);
                // the optics ride along, straight into the pending registers: those are free here (the
                // previous step's emission is done) and only looked at again if this step contributes
                pend_o0 = r[6];
                pend_o1 = r[7];
            };
            if (n_runs_s <= SLOTS) {
                // (wave-uniform, nine steps in ten: every distinct cell has a slot - no per-lane "is my cell staged" at all)
                read_staged();
            } else if (slot < SLOTS) {
                read_staged();
            } else {
                load_cell(cur, P.xrec, nb);  // more distinct cells than slots: rare
                pend_o0 = V2{cur.r6.a, cur.r6.b};
                pend_o1 = V2{cur.r7.a, cur.r7.b};
            }

            const StepGeometry sg = step_geometry(cur, x, y);
            // SPLIT: a cell that reaches beyond the job's slab is cut at the plane: the job ends there, and the job above takes
            // the ray up from the plane (in this cell, if plane_raster found it there)
            const bool clip = SPLIT && sg.w_exit >= w_hi && sg.w_exit < INFINITY;
            const double dz = (clip ? w_hi : sg.w_exit) - carry;  // line.cpp:124-131: the chord through the cell
            const bool contributes = dz > 0.0 && dz < INFINITY;
            // (wave-uniform choice of the exp: every contributing lane's argument within (-1/8, 0] -> the short series;
            // C3 walk 0.4786 -> 0.4738 ms, at 4800x3600 1.614 -> 1.579.  Starting the next step's election — ticket
            // written, winner read — before this arithmetic, so that the LDS round trip runs under it, cost a
            // register pair to scratch and 0.7 %: not kept)
            // With SMALLEXP (the host knows that no cell of the grid can give an argument beyond -1/8) neither the test nor
            // the general exp is in the kernel: C3 walk 0.4735 -> 0.460 ms.  (The same knowledge as a per-frame flag
            // read by the kernel, both paths kept, bought nothing: 0.4747 against 0.4741.)
            const bool short_exp = SMALLEXP || !kEmitNow || __builtin_amdgcn_ballot_w64(contributes && !(pend_o0.y * dz < -kSmallExpArg)) == 0ull;
            if (contributes) {
                // (SPLIT: a cell is counted by the job in which the ray LEAVES it, so that a cell cut by a plane counts once)
                if (!clip) ++n_seg;
                tau = fma(dz, pend_o0.x, tau);  // line.cpp:189 (unclamped alpha); order-independent, done now
                if (SPLIT) tauc = fma(dz, pend_o0.y, tauc);
                if (kEmitNow) {
                    const Light l = emission_step<ORDER>(I, T, P.t_cutoff, pend_o0.y, pend_o1.x, pend_o1.y, dz, short_exp);
                    I = l.I, T = l.T;
                } else {
                    pend = true;
                    pend_dz = dz;
                }
            }
            // the ray enters the next cell where it leaves this one (a cell it cannot leave — flat, or all its
            // candidates edge-on — has w_exit = +inf and no neighbour: the ray ends there, as before)
            const bool has_exit = sg.w_exit < INFINITY;
            if (has_exit) carry = sg.w_exit;
            const uint32_t id = sg.w_out & kIdMask;
            int nxt = static_cast<int>(id);
            if (id == kNoCell || clip) {  // left the grid: re-entry of a non-convex grid?  (or reached the end of the job's slab)
                const size_t lp = pixel_index_rare();
                double w_cur = my_scur[lane];  // (the key of the entry the ray took last: only (re-)entries write it)
                const double key_taken = w_cur;
                bool skipped = false;
                if (has_exit) w_cur = fmax(w_cur, sg.w_exit);
                // (a clipped ray takes no further entry - own_hi = -DBL_MAX owns none - but the entries inside the stretch it
                // has walked, up to the plane, are judged all the same)
                nxt = next_entry<kUp>(P, lp, load_entry_head(P.entry_head + lp), w_cur, carry, key_taken,
                                      clip ? w_hi : (has_exit ? sg.w_exit : -DBL_MAX), skipped, slab_lo(x, y), clip ? -DBL_MAX : w_hi);
                if (SPLIT && clip) n_seg |= kClippedBit;
                if (skipped) n_seg |= kSkippedBit;
                my_scur[lane] = w_cur;
            }
            clock.leaving(nb);
            nb = nxt;
        }
        clock.stepped(need, nb);
    }
    clock.end(lane);
    if (pend) {  // the last step's contribution
        if (ORDER == 0) {
            if (pend_o0.y != 0.0) I = reference_emission_step<SMALLEXP>(I, pend_o0.y, pend_o1.y, pend_o1.x, pend_dz);
        } else if (T >= P.t_cutoff) {
            const double ex = exp_nonpositive(-pend_o0.y * pend_dz);
            I = fma(T * pend_o1.x, 1.0 - ex, I);
            T *= ex;
        }
    }

    {   // the depth sample (DepthSamples): where the rays of the sampled pixels END - in this job, if it did not hand them on
        const bool ended_here = (n_seg & ~(kOverflowBit | kSkippedBit | kClippedBit)) != 0u && (n_seg & kClippedBit) == 0u;
        int l = lane;
        asm volatile("" : "+v"(l));
        const int col = tx * TW + (wave % TS::GX) * TS::WW + (l % TS::WW), lrow = ty * TH + (wave / TS::GX) * TS::WH + (l / TS::WW);
        if (ended_here && col < im.res_x && lrow < im.n_local_rows) {
            const int slot = fit_slot_of(im, col, global_row_of(im, lrow));
            if (slot >= 0) reinterpret_cast<DepthSamples*>(P.counters + kCounterShards)->exit_key[slot] = depth_key(carry);
        }
        n_seg &= ~kClippedBit;
    }
    {   // ... and the deepest at which one of them ends (carry: where the ray left its last cell)
        double hi = (n_seg & ~(kOverflowBit | kSkippedBit)) ? carry : -DBL_MAX;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) hi = fmax(hi, __shfl_xor(hi, d));
        if (lane == 0 && hi > -DBL_MAX && sampler) atomicMax(&fc_job()->exit_max_key, depth_key(hi));
    }
    if (SPLIT) {
        // The job's partial results, indexed tile * 64 + lane (whole 512-byte rows per array and wavefront), then the
        // tile's arrival count: the job that finds K - 1 others already there composes the K partials in depth order and
        // goes on to the common end (image, entry heads, statistics).  The partials travel as RELAXED ATOMIC stores and
        // loads at agent scope (write-through / read-through: coherent across the XCDs' L2s by themselves) with the
        // wavefront's own vmcnt between its stores and its arrival — NOT as plain stores behind a release fence: an
        // agent-scope release writes back the WHOLE L2 (buffer_wbl2), and 80 000 of those per launch made the first
        // version of this kernel five times slower than the walk it replaces (profiles/r04_split_probe.md).
        const unsigned K = static_cast<unsigned>(P.split.n_slabs);
        const size_t tile = static_cast<size_t>(ty) * tiles_x + tx;
        const size_t at = tile * 64u + static_cast<unsigned>(lane);
        const size_t mine = static_cast<size_t>(slab) * P.split.part_stride + at;
        __hip_atomic_store(P.split.part_tau + mine, tau, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(P.split.part_tauc + mine, tauc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(P.split.part_b + mine, I, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(P.split.part_nseg + mine, n_seg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the four stores above have been performed
        unsigned before = 0;
        if (lane == 0) before = atomicAdd(P.split.arrivals + tile, 1u);
        before = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(before)));
        if (before + 1u != K) {
            if (lane == 0 && n_step_wave)
                atomicAdd(&fc_job()->steps_cov, static_cast<unsigned long long>(n_step_wave));
            return;
        }
        if (lane == 0) P.split.arrivals[tile] = 0u;  // (for the next frame; every job of this one has arrived)
        tau = 0.0;
        I = 0.0;
        n_seg = 0u;
        for (unsigned k = 0; k < K; ++k) {  // line.cpp:206-225 is affine in I: I <- exp(-tauc_k) I + b_k, from the back
            const size_t from = static_cast<size_t>(k) * P.split.part_stride + at;
            const double t_k = __hip_atomic_load(P.split.part_tau + from, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const double c_k = __hip_atomic_load(P.split.part_tauc + from, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const double b_k = __hip_atomic_load(P.split.part_b + from, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned n_k = __hip_atomic_load(P.split.part_nseg + from, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            tau += t_k;
            I = fma(exp_nonpositive(-c_k), I, b_k);
            n_seg = (n_seg + (n_k & ~(kOverflowBit | kSkippedBit))) | (n_k & (kOverflowBit | kSkippedBit));
        }
    }
    const unsigned overflow = n_seg >> 31;
    const bool skipped = (n_seg & kSkippedBit) != 0u;
    n_seg &= ~(kOverflowBit | kSkippedBit);
    unsigned is_solid = 0, n_entries = 0;
    if (in_image) {
        const size_t lp = pixel_index();
        float2 result = make_float2(static_cast<float>(tau), static_cast<float>(I));  // plane.cpp:165-166
        const uint32_t mv = P.mask ? P.mask[lp] : 0u;
        if (mv) {
            double colour = 0.0;
            for (int s = 0; s < P.solids.n_slots; ++s)
                if (mv == static_cast<uint32_t>(s) + 1u) colour = P.solids.colour[s];
            result.x = static_cast<float>(colour);
            result.y = result.x;
            is_solid = 1;
        }
        // every pixel hands its entry head back cleared: the next frame's raster needs no memset
        n_entries = static_cast<unsigned>(load_entry_head(P.entry_head + lp).count);
        if (n_entries && !P.keep_entries) __builtin_nontemporal_store(0ll, reinterpret_cast<long long*>(P.entry_head + lp));
        __builtin_nontemporal_store(result.x, &P.out[lp].x);
        __builtin_nontemporal_store(result.y, &P.out[lp].y);
    }

    if (P.row_cost) {
        int l = lane;
        asm volatile("" : "+v"(l));  // (as in pixel_index_rare: nothing of this is kept across the loop)
        const int lrow = ty * TH + (wave / TS::GX) * TS::WH + (l / TS::WW);
        post_row_cost<TILE>(P, l, lrow, n_seg);
    }
    const unsigned s_seg = wave_sum_u32(n_seg);
    const unsigned s_cov = wave_sum_u32(n_seg > 0 ? 1u : 0u);
    const unsigned s_sol = wave_sum_u32(is_solid);
    const unsigned s_ovf = wave_sum_u32(overflow);
    const unsigned s_ent = wave_sum_u32(n_entries);
    const unsigned s_skip = static_cast<unsigned>(__popcll(__builtin_amdgcn_ballot_w64(skipped)));
    unsigned s_longest = n_seg;  // the longest ray of the tile, in segments
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s_longest = max(s_longest, static_cast<unsigned>(__shfl_xor(static_cast<int>(s_longest), d)));
    if (lane == 0) {
        count_overlap(P, s_skip);
        FrameCounters* const fc = fc_job();
        // The longest ray of this tile, to its row of super-blocks (the order the next frames' rows start in, c_api.hip) - from ONE
        // tile per super-block only (its first: the one a cut-off super-block at the image's edge has too): every wavefront
        // adding to its row's word put thousands of same-address atomics on a handful of words (a share of 248 rows has 8
        // rows of super-blocks: walk 0.219 -> 0.231 ms; the C3 frame + 0.7 %).
        if (s_seg) atomicMax(&fc->seg_max, s_longest);  // (exact: "depth_split" 0 decides by it, and the decision has a threshold)
        if (s_seg && sampler) {
            const int sb_row = ty / P.band_tiles;
            if (P.sb_cost && P.xcd_mode == 2 && sb_row < kMaxSbRows) atomicMax(P.sb_cost + sb_row, s_longest);
        }
        count_frame(P, fc, s_seg, n_step_wave, s_cov, s_ent, s_sol, s_ovf);
    }
}

// One launch plan (walk_plan.hpp), one switch to the instantiation it names.  The plan keeps SMALLEXP to the default tile
// shape, and SPLIT to it and the reference order: the other shapes do not hold those kernels.
template <int TILE, int ORDER>
static void launch_walk_t(hipStream_t s, const WalkParams& p) {
    const WalkPlan plan = walk_plan(WalkPlanInput{TILE, ORDER, p.xcd_mode, p.lds_stage, p.stage_slots, p.small_exp_only, p.split.n_slabs, p.band_rows,
                                                  p.im.res_x, p.im.n_local_rows});
    if (plan.grid <= 0) return;
    WalkParams q = p;
    if (plan.layout != WalkLayout::kRowMajor) q.band_tiles = plan.band_tiles;
    const dim3 grid(static_cast<unsigned>(plan.grid)), threads(64u * TileShape<TILE>::GX * TileShape<TILE>::GY);
    auto go = [&](auto kernel, int lds_pad) { hipLaunchKernelGGL(kernel, grid, threads, static_cast<size_t>(lds_pad), s, q); };
    constexpr int kDma = static_cast<int>(WalkFamily::kLdsDma), k21 = WalkPlan::kSlots21, kSmall = WalkPlan::kSmallExp, kSplit = WalkPlan::kSplit;
    constexpr bool kDefault = TILE == 3, kDefaultRef = TILE == 3 && ORDER == 0;
    // a plan without a kernel of this tile shape and order is a mistake in walk_plan, not a frame to drop quietly
    auto no_kernel = [&]() {
        fprintf(stderr, "launch_walk: no kernel for plan %d (tile %d, order %d)\n", plan.instantiation(), TILE, ORDER);
        abort();
    };
    switch (plan.instantiation()) {
        case static_cast<int>(WalkFamily::kDirect): go(walk_composite<TILE, ORDER>, 0); break;
        case static_cast<int>(WalkFamily::kLdsRegisters): go(walk_composite_lds<TILE, ORDER>, p.lds_pad); break;
        case kDma: go(walk_composite_lds<TILE, ORDER, true>, p.lds_pad); break;
        case kDma | k21: go(walk_composite_lds<TILE, ORDER, true, 21>, p.lds_pad); break;
        case kDma | kSmall:
            if constexpr (kDefault) go(walk_composite_lds<3, ORDER, true, kStageSlots, true>, p.lds_pad);
            else no_kernel();
            break;
        case kDma | kSplit:
            if constexpr (kDefaultRef) go(walk_composite_lds<3, 0, true, kStageSlots, false, true>, p.lds_pad);
            else no_kernel();
            break;
        case kDma | kSplit | k21:
            if constexpr (kDefaultRef) go(walk_composite_lds<3, 0, true, 21, false, true>, p.lds_pad);
            else no_kernel();
            break;
        case kDma | kSplit | kSmall:
            if constexpr (kDefaultRef) go(walk_composite_lds<3, 0, true, kStageSlots, true, true>, p.lds_pad);
            else no_kernel();
            break;
        default: no_kernel();
    }
}

int walk_sb_rows(int tile_shape, int band_rows) {
    const int th = tile_extent(tile_shape).th;
    return super_block_tiles(th, band_rows) * th;
}

void launch_walk(hipStream_t s, const WalkParams& p, int tile_shape) {
    if (p.order == 0) {
        switch (tile_shape) {
            case 1: launch_walk_t<1, 0>(s, p); break;
            case 2: launch_walk_t<2, 0>(s, p); break;
            case 3: launch_walk_t<3, 0>(s, p); break;
            default: launch_walk_t<0, 0>(s, p); break;
        }
    } else {
        switch (tile_shape) {
            case 1: launch_walk_t<1, 1>(s, p); break;
            case 2: launch_walk_t<2, 1>(s, p); break;
            case 3: launch_walk_t<3, 1>(s, p); break;
            default: launch_walk_t<0, 1>(s, p); break;
        }
    }
}

}  // namespace c5

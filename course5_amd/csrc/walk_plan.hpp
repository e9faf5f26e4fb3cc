// The walk's launch plan: which instantiation of walk_composite / walk_composite_lds a frame's state launches, over how
// many workgroups, and how a workgroup finds its tile.  The host's count (walk_plan) and the kernels' inverse
// (tile_of_block) live side by side here, in plain C++ over plain values: launch_walk, walk_sb_rows and both kernels use
// them, and tests/cpp/walk_plan_check.cpp checks them against each other with g++, no GPU.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define C5_PLAN_FN __host__ __device__ inline
#else
#define C5_PLAN_FN inline
#endif

namespace c5 {

template <int TILE>
struct TileShape;
template <>
struct TileShape<0> {  // each wavefront owns a 64x1 row tile; workgroup 64 x 4
    static constexpr int WW = 64, WH = 1, GX = 1, GY = 4;
};
template <>
struct TileShape<1> {  // 16x4 per wavefront; workgroup 32 x 8
    static constexpr int WW = 16, WH = 4, GX = 2, GY = 2;
};
template <>
struct TileShape<2> {  // 8x8 per wavefront; workgroup 16 x 16
    static constexpr int WW = 8, WH = 8, GX = 2, GY = 2;
};
template <>
struct TileShape<3> {  // 8x8 per wavefront, ONE wavefront per workgroup: a wavefront's slot (and its LDS) is free for
                       // the next tile the moment its own rays are done, not when the slowest of four is
    static constexpr int WW = 8, WH = 8, GX = 1, GY = 1;
};

// pixels of a workgroup's tile (option "tile": 0 .. 3)
struct TileExtent {
    int tw, th;
};
template <int TILE>
C5_PLAN_FN TileExtent tile_extent_of() {
    return TileExtent{TileShape<TILE>::WW * TileShape<TILE>::GX, TileShape<TILE>::WH * TileShape<TILE>::GY};
}
C5_PLAN_FN TileExtent tile_extent(int tile) {
    return tile == 0 ? tile_extent_of<0>() : tile == 1 ? tile_extent_of<1>() : tile == 2 ? tile_extent_of<2>() : tile_extent_of<3>();
}

// How the workgroups of a launch are laid over the tiles (option "xcd_mode"; blocks b and b + 8 share an XCD's L2).
enum class WalkLayout : int {
    kRowMajor,     // xcd_mode 0: block = ty * tiles_x + tx
    kBands,        // xcd_mode 1, and 2 with direct loads: bands of tile rows dealt round-robin to the 8 XCDs
    kSuperBlocks,  // xcd_mode 2 with LDS staging: squares of S x S tiles dealt round-robin to the 8 XCDs
};
C5_PLAN_FN WalkLayout walk_layout(int xcd_mode, bool lds_kernel) {
    return xcd_mode == 0 ? WalkLayout::kRowMajor : (xcd_mode == 2 && lds_kernel) ? WalkLayout::kSuperBlocks : WalkLayout::kBands;
}

// tiles along a super-block's side.  Measured (C3 grid, 8x8 tiles, walk ms at 1200x900 / 2400x1800 / 4800x3600):
// super-blocks of 32 rows 0.303 / 0.601 / 2.070, of 64 rows 0.350 / 0.602 / 2.063; bands of 16 rows 0.310 / 0.610 / 2.065;
// row-major blocks 0.372 / 0.597 / 2.059
C5_PLAN_FN int super_block_tiles(int th, int band_rows) {
    const int sb_rows = band_rows > 0 ? band_rows : 32;
    return sb_rows / th > 0 ? sb_rows / th : 1;
}

enum class WalkFamily : int {
    kDirect = 0,        // walk_composite: every lane loads its own cell's record
    kLdsRegisters = 1,  // walk_composite_lds<.., DMA = false>: staged through registers
    kLdsDma = 2,        // walk_composite_lds<.., DMA = true>: the staging loads write LDS themselves
};

struct WalkPlanInput {
    int tile, order;  // tile shape 0 .. 3; 0: reference order
    int xcd_mode, lds_stage, stage_slots, small_exp_only, n_slabs, band_rows;  // as in WalkParams (n_slabs: split.n_slabs)
    int res_x, n_local_rows;
};

struct WalkPlan {
    WalkFamily family;
    int slots;          // distinct cells staged per step: 14 or 21 (0: direct loads)
    bool small_exp;     // SMALLEXP: the instantiation without the general exp
    bool split;         // SPLIT ("depth_split"): n_slabs jobs per tile
    WalkLayout layout;
    int tiles_x, tiles_y;
    int band_tiles;     // WalkParams::band_tiles of the launch: tile rows per band, or tiles along a super-block's side (row-major: unused, 0)
    long long blocks;   // workgroups that cover the tiles once (a multiple of 8 where XCDs are dealt to); 0: no tile
    long long grid;     // workgroups of the launch: blocks, times n_slabs with split; 0: no launch
    // the instantiation as one number, for the launcher's switch
    static constexpr int kSlots21 = 4, kSmallExp = 8, kSplit = 16;
    C5_PLAN_FN int instantiation() const {
        return static_cast<int>(family) | (slots > 14 ? kSlots21 : 0) | (small_exp ? kSmallExp : 0) | (split ? kSplit : 0);
    }
};

C5_PLAN_FN WalkPlan walk_plan(const WalkPlanInput& in) {
    const TileExtent t = tile_extent(in.tile);
    WalkPlan p{};
    p.tiles_x = (in.res_x + t.tw - 1) / t.tw;
    p.tiles_y = (in.n_local_rows + t.th - 1) / t.th;
    p.layout = walk_layout(in.xcd_mode, in.lds_stage != 0);
    // the kernel.  SMALLEXP is kept to the default tile shape and to launches that deal tiles to XCDs; SPLIT to what the
    // host asks for it in: default tile, reference order, super-blocks, LDS-DMA.
    const bool dma = in.lds_stage == 2;
    p.family = dma ? WalkFamily::kLdsDma : in.lds_stage ? WalkFamily::kLdsRegisters : WalkFamily::kDirect;
    p.slots = (dma && in.stage_slots > 14) ? 21 : in.lds_stage ? 14 : 0;
    p.small_exp = dma && p.slots == 14 && in.tile == 3 && in.small_exp_only != 0 && p.layout != WalkLayout::kRowMajor;
    p.split = dma && in.tile == 3 && in.order == 0 && in.n_slabs > 1 && p.layout == WalkLayout::kSuperBlocks;
    if (p.tiles_x <= 0 || p.tiles_y <= 0) return p;
    // the workgroups
    if (p.layout == WalkLayout::kRowMajor) {
        p.blocks = static_cast<long long>(p.tiles_x) * p.tiles_y;
    } else if (p.layout == WalkLayout::kSuperBlocks) {
        const int S = super_block_tiles(t.th, in.band_rows);
        const long long n_sb = static_cast<long long>((p.tiles_x + S - 1) / S) * ((p.tiles_y + S - 1) / S);
        p.blocks = 8ll * ((n_sb + 7) / 8) * S * S;
        p.band_tiles = S;
    } else {
        // ~16 image rows per band (one row of workgroups), but never fewer than 16 bands (2 per XCD) on a short strip.
        // Measured (C3 grid, 8x8 tiles, walk ms at 1200x900 / 2400x1800 / 4800x3600): row-major blocks
        // 0.378 / 0.629 / 2.140, bands of 16 rows 0.319 / 0.645 / 2.137, 32 rows 0.322 / 0.657 / 2.146
        const int band_rows = in.band_rows > 0 ? in.band_rows : 16;
        int band = (band_rows / t.th) > 0 ? (band_rows / t.th) : 1;
        while (band > 1 && (p.tiles_y + band - 1) / band < 16) band >>= 1;
        const int n_bands = (p.tiles_y + band - 1) / band;
        p.blocks = 8ll * ((n_bands + 7) / 8) * band * p.tiles_x;
        p.band_tiles = band;
    }
    p.grid = p.split ? p.blocks * in.n_slabs : p.blocks;
    return p;
}

// The inverse, on the device: workgroup `block` of the launch -> its tile (tx, ty) and, with SPLIT, its slab; false: no
// tile (the launch is rounded up to whole rounds of 8 XCDs, whole bands and whole super-blocks).  band_tiles, n_slabs: the
// plan's; xcd_mode, sb_order / n_sb_rows: WalkParams'.  The layout is walk_layout(xcd_mode, kLdsKernel), spelled as the
// tests on xcd_mode it comes down to in either kernel.  The body is tile_of_block_body.hpp: walk_composite calls this
// function, walk_composite_lds includes the same text in place.
template <bool SPLIT, bool kLdsKernel>
C5_PLAN_FN bool tile_of_block(unsigned block, int xcd_mode, int tiles_x, int tiles_y, const int32_t& band_tiles, const int32_t& n_slabs,
                              const int32_t& n_sb_rows, const uint8_t* sb_order, int& tx, int& ty, int& slab) {
#define C5_NO_TILE return false
#include "tile_of_block_body.hpp"
#undef C5_NO_TILE
    return true;
}

}  // namespace c5

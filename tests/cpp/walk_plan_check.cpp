// walk_plan.hpp with g++, no GPU: `plan` compares walk_plan with the launch rules written out again below, over every
// combination of the options; `layout` runs tile_of_block (the text both walk kernels compile) over a launch's workgroups and wants every
// (tile, slab) exactly once.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "walk_plan.hpp"

using namespace c5;

// pixels of a workgroup's tile, written out (64x1 x 1x4 wavefronts, 16x4 x 2x2, 8x8 x 2x2, 8x8 x 1x1)
static const int kTW[4] = {64, 32, 16, 8}, kTH[4] = {4, 8, 16, 8};
static const int kImages[5][2] = {{1, 1}, {7, 3}, {64, 64}, {65, 65}, {1200, 900}};
static const int kBandRows[5] = {0, 8, 16, 32, 64};

static long long ceil_div(long long a, long long b) { return (a + b - 1) / b; }

enum { kDirect = 0, kRegisters = 1, kDma = 2 };
struct Want {
    int family = kDirect, slots = 0;
    bool small_exp = false, split = false;
    long long grid = 0;
    int band_tiles = 0;
};

// The rules, restated (not calling the code under test).
static Want want(int tile, int order, int xcd_mode, int lds_stage, int stage_slots, int small_exp_only, int n_slabs, int band_rows, int res_x,
                 int n_local_rows) {
    const long long tiles_x = ceil_div(res_x, kTW[tile]), tiles_y = ceil_div(n_local_rows, kTH[tile]);
    Want w;
    // the choice of a launch that is not split; SMALLEXP only where the layout allows it
    auto whole_ray_kernel = [&](bool small_allowed) {
        if (lds_stage == 2 && stage_slots > 14) {
            w.family = kDma, w.slots = 21;
        } else if (small_allowed && tile == 3 && lds_stage == 2 && small_exp_only) {
            w.family = kDma, w.slots = 14, w.small_exp = true;
        } else if (lds_stage == 2) {
            w.family = kDma, w.slots = 14;
        } else if (lds_stage) {
            w.family = kRegisters, w.slots = 14;
        } else {
            w.family = kDirect, w.slots = 0;
        }
    };
    long long blocks;
    if (xcd_mode == 0) {  // row-major: never SMALLEXP, never SPLIT
        blocks = tiles_x * tiles_y;
        whole_ray_kernel(false);
    } else if (xcd_mode == 2 && lds_stage != 0) {  // super-blocks
        const int sb_rows = band_rows > 0 ? band_rows : 32;
        const int S = std::max(sb_rows / kTH[tile], 1);
        const long long n_sb = ceil_div(tiles_x, S) * ceil_div(tiles_y, S);
        blocks = 8 * ceil_div(n_sb, 8) * S * S;
        w.band_tiles = S;
        if (tile == 3 && order == 0 && n_slabs > 1 && lds_stage == 2) {
            w.split = true;
            w.family = kDma;
            if (stage_slots > 14)
                w.slots = 21;
            else if (small_exp_only)
                w.slots = 14, w.small_exp = true;
            else
                w.slots = 14;
            blocks *= n_slabs;
        } else {
            whole_ray_kernel(true);
        }
    } else {  // bands: xcd_mode 1, and xcd_mode 2 with direct loads
        const int rows = band_rows > 0 ? band_rows : 16;
        int band = std::max(rows / kTH[tile], 1);
        while (band > 1 && ceil_div(tiles_y, band) < 16) band /= 2;
        blocks = 8 * ceil_div(ceil_div(tiles_y, band), 8) * band * tiles_x;
        w.band_tiles = band;
        whole_ray_kernel(true);
    }
    w.grid = (tiles_x > 0 && tiles_y > 0) ? blocks : 0;  // no launch when there are no tiles
    return w;
}

static WalkPlan plan_of(int tile, int order, int xcd_mode, int lds_stage, int stage_slots, int small_exp_only, int n_slabs, int band_rows, int res_x,
                        int n_local_rows) {
    return walk_plan(WalkPlanInput{tile, order, xcd_mode, lds_stage, stage_slots, small_exp_only, n_slabs, band_rows, res_x, n_local_rows});
}

static int check_plan() {
    long checked = 0;
    for (int tile = 0; tile < 4; ++tile)
        for (int order = 0; order < 2; ++order)
            for (int xcd_mode = 0; xcd_mode < 3; ++xcd_mode)
                for (int lds_stage = 0; lds_stage < 3; ++lds_stage)
                    for (int stage_slots : {0, 14, 21})
                        for (int small = 0; small < 2; ++small)
                            for (int n_slabs = 1; n_slabs <= 3; ++n_slabs)
                                for (int band_rows : kBandRows)
                                    for (int i = 0; i < 6; ++i) {
                                        // (a sixth image without a pixel: no launch)
                                        const int res_x = i < 5 ? kImages[i][0] : 0, rows = i < 5 ? kImages[i][1] : 0;
                                        const Want w = want(tile, order, xcd_mode, lds_stage, stage_slots, small, n_slabs, band_rows, res_x, rows);
                                        const WalkPlan p = plan_of(tile, order, xcd_mode, lds_stage, stage_slots, small, n_slabs, band_rows, res_x, rows);
                                        const bool same = static_cast<int>(p.family) == w.family && p.slots == w.slots && p.small_exp == w.small_exp &&
                                                          p.split == w.split && p.grid == w.grid &&
                                                          (xcd_mode == 0 || w.grid == 0 || p.band_tiles == w.band_tiles);
                                        if (!same) {
                                            printf("MISMATCH tile %d order %d xcd %d lds %d slots %d small %d slabs %d band_rows %d image %dx%d: want family %d "
                                                   "slots %d small %d split %d grid %lld band_tiles %d, got %d %d %d %d %lld %d\n",
                                                   tile, order, xcd_mode, lds_stage, stage_slots, small, n_slabs, band_rows, res_x, rows, w.family, w.slots,
                                                   w.small_exp, w.split, w.grid, w.band_tiles, static_cast<int>(p.family), p.slots, p.small_exp, p.split, p.grid,
                                                   p.band_tiles);
                                            return 1;
                                        }
                                        ++checked;
                                    }
    printf("ok %ld plans\n", checked);
    return 0;
}

template <bool SPLIT, bool kLdsKernel>
static bool covers(const WalkPlan& p, int xcd_mode, int n_slabs, int n_sb_rows, const uint8_t* sb_order) {
    std::vector<int> seen(static_cast<size_t>(p.tiles_x) * p.tiles_y * n_slabs, 0);
    for (long long b = 0; b < p.grid; ++b) {
        int tx = -1, ty = -1, slab = -1;
        if (!tile_of_block<SPLIT, kLdsKernel>(static_cast<unsigned>(b), xcd_mode, p.tiles_x, p.tiles_y, p.band_tiles, n_slabs, n_sb_rows, sb_order, tx, ty, slab)) continue;
        if (tx < 0 || tx >= p.tiles_x || ty < 0 || ty >= p.tiles_y || slab < 0 || slab >= n_slabs) return false;
        ++seen[(static_cast<size_t>(ty) * p.tiles_x + tx) * n_slabs + slab];
    }
    for (int n : seen)
        if (n != 1) return false;
    return true;
}

static int check_layout() {
    long checked = 0;
    // the three layouts as either kernel inverts them: row-major; bands; super-blocks (LDS-DMA, so that the default tile in
    // reference order may split); and the direct kernel's row-major and bands (xcd_mode 1, and 2: bands there)
    const int modes[6][2] = {{0, 2}, {1, 2}, {2, 2}, {0, 0}, {1, 0}, {2, 0}};  // {xcd_mode, lds_stage}
    for (const auto& mode : modes)
        for (int tile = 0; tile < 4; ++tile)
            for (const auto& image : kImages)
                for (int band_rows : kBandRows)
                    for (int n_slabs = 1; n_slabs <= 3; ++n_slabs)
                        for (int table = 0; table < 3; ++table) {  // sb_order: none given, identity, reversed
                            const WalkPlan p = plan_of(tile, 0, mode[0], mode[1], 14, 0, n_slabs, band_rows, image[0], image[1]);
                            if (p.split != (n_slabs > 1 && mode[0] == 2 && mode[1] == 2 && tile == 3)) {
                                printf("SPLIT where it does not apply\n");
                                return 1;
                            }
                            if (n_slabs > 1 && !p.split) continue;  // (n_slabs 2, 3 only where SPLIT applies)
                            // the order of the rows of super-blocks: image order (no table given, or the identity), or the last row first
                            uint8_t sb_order[128];
                            std::memset(sb_order, 0, sizeof(sb_order));
                            int n_sb_rows = 0;
                            if (table) {
                                if (p.layout != WalkLayout::kSuperBlocks) continue;
                                n_sb_rows = (p.tiles_y + p.band_tiles - 1) / p.band_tiles;
                                if (n_sb_rows > 128) continue;  // (the host gives no order to more rows than the table holds)
                                for (int k = 0; k < n_sb_rows; ++k) sb_order[k] = static_cast<uint8_t>(table == 1 ? k : n_sb_rows - 1 - k);
                            }
                            const bool ok = p.split   ? covers<true, true>(p, mode[0], n_slabs, n_sb_rows, sb_order)
                                            : mode[1] ? covers<false, true>(p, mode[0], 1, n_sb_rows, sb_order)
                                                      : covers<false, false>(p, mode[0], 1, n_sb_rows, sb_order);
                            if (!ok) {
                                printf("MISMATCH xcd %d tile %d image %dx%d band_rows %d slabs %d sb_order %d: grid %lld does not cover every tile once\n",
                                       mode[0], tile, image[0], image[1], band_rows, n_slabs, table, p.grid);
                                return 1;
                            }
                            ++checked;
                        }
    printf("ok %ld layouts\n", checked);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "plan")) return check_plan();
    if (argc == 2 && !std::strcmp(argv[1], "layout")) return check_layout();
    printf("usage: walk_plan_check plan|layout\n");
    return 2;
}

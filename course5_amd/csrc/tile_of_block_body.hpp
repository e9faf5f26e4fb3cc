// The body of tile_of_block (walk_plan.hpp), as text: block index -> (tx, ty, slab), or C5_NO_TILE.  No include guard and no
// namespace: it is included INSIDE a function body, once in tile_of_block itself (C5_NO_TILE: return false) and once at the
// head of walk_composite_lds (walk_kernels.hip; C5_NO_TILE: return), so that the kernel and the host's check of the block
// count compile one and the same text.  (Called as a function the mapping moved walk_composite_lds's machine code - one
// more block at the "no tile" exits; walk_composite calls the function and is unchanged.)
// In scope where it is included:
//   constants   bool SPLIT, kLdsKernel
//   in          unsigned block; int tiles_x, tiles_y; xcd_mode, band_tiles, n_slabs, n_sb_rows: int32_t, in the kernel as
//               REFERENCES to the kernel arguments (each is then read where the text reads it, as the kernel's machine code
//               has it: by value they were read once in front, and the SPLIT instantiations came out differently);
//               const uint8_t* sb_order
//   out         int tx, ty, slab
    // SPLIT: the K jobs of a tile follow one another on the same XCD: block -> (tile block, slab)
    slab = 0;
    unsigned bid = block;
    if (SPLIT) {
        const unsigned K = static_cast<unsigned>(n_slabs);
        if (xcd_mode == 0) {
            slab = static_cast<int>(bid % K);
            bid = bid / K;
        } else {
            const unsigned seq_k = bid >> 3;
            slab = static_cast<int>(seq_k % K);
            bid = ((seq_k / K) << 3) | (bid & 7u);
        }
    }
    if (xcd_mode == 0) {
        ty = bid / tiles_x;
        tx = bid - ty * tiles_x;
    } else if (kLdsKernel && xcd_mode == 2) {
        // square super-blocks of S x S workgroups dealt round-robin to the 8 XCDs: the workgroups an XCD
        // runs at a time are neighbours in x AND y, so a cell's record is fetched into few L2s
        const int S = band_tiles;
        const int sbx_n = (tiles_x + S - 1) / S, sby_n = (tiles_y + S - 1) / S;
        const int xcd = bid & 7;
        const int seq = bid >> 3;
        const int sb = (seq / (S * S)) * 8 + xcd;
        const int within = seq - (seq / (S * S)) * (S * S);
        if (sb >= sbx_n * sby_n) C5_NO_TILE;
        int sby = sb / sbx_n;
        const int sbx = sb - sby * sbx_n;
        if (n_sb_rows == sby_n) sby = static_cast<int>(sb_order[sby]);  // rows with the longest rays first (kernel argument)
        ty = sby * S + within / S;
        tx = sbx * S + (within - (within / S) * S);
        if (tx >= tiles_x || ty >= tiles_y) C5_NO_TILE;
    } else {
        // Bands of tile rows are dealt round-robin to the 8 XCDs: every XCD sweeps the image top to bottom, so load
        // stays balanced, while the workgroups resident on one XCD at a time cover a compact region of the grid.
        const int BAND = band_tiles;  // tile rows per band
        const int n_bands = (tiles_y + BAND - 1) / BAND;
        const int per_band = BAND * tiles_x;
        const int xcd = bid & 7;
        const int seq = bid >> 3;
        const int band = (seq / per_band) * 8 + xcd;
        const int within = seq - (seq / per_band) * per_band;
        if (band >= n_bands) C5_NO_TILE;
        ty = band * BAND + within % BAND;
        tx = within / BAND;
        if (ty >= tiles_y) C5_NO_TILE;
    }

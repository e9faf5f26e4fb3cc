"""Randomised parity sweep: GPU (C ABI) vs CPU oracle on many small random scenes.

    python tests/fuzz_parity.py [n_scenes] [seed0]

Scenes: tests/fuzz_scenes.py (jittered Kuhn boxes with holes, refined interfaces with hanging nodes, dense sub-pixel
grids; random views, scalars, image sizes and alpha limits), every kernel variant.  Reports every mismatch.
"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # noqa: F401  (HIP runtime load order)
from course5_amd import capi, meshgen as mg
from oracle.pyoracle import Oracle

from tests.fuzz_scenes import VARIANTS, scene  # noqa: F401  (the scenes live there: CPU tests draw them too)


def main():
    n_scenes = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    o = Oracle("port")
    ctx = capi.Context(0)
    bad = 0
    for k in range(n_scenes):
        seed = seed0 + k
        if k % 50 == 0:
            print(f"... scene {k} of {n_scenes}, {bad} mismatching renders so far", flush=True)
        xyz, cells, alpha, q, rots, res, limit = scene(seed)
        # A grid that reaches the last pixel column / row of the image is outside the contract: the reference clamps what
        # lies beyond a border into the border pixels (plane.cpp:194-212 - or aborts, plane.cpp:39-41), the walk renders what
        # is inside (tests/test_gpu_edges.py has those cases on purpose).  One scene in ~700 does.
        v = o.rotate_points(xyz, rots)
        bx = mg.REFERENCE_BOUNDS
        px, py = (bx[0] - bx[1]) / (res[0] - 1), (bx[2] - bx[3]) / (res[1] - 1)
        if v[:, 0].min() < bx[1] + px or v[:, 0].max() > bx[0] - px or v[:, 1].min() < bx[3] + py or v[:, 1].max() > bx[2] - py:
            print(f"seed {seed}: the grid reaches the image's border - outside the contract, skipped")
            continue
        try:
            ref = o.render(xyz, cells, alpha, q, rots, res[0], res[1], mg.REFERENCE_BOUNDS, alpha_limit=limit, threads=8)
        except RuntimeError as e:
            print(f"seed {seed}: oracle rejects the scene ({e}) - degenerate alignment, skipped")
            continue
        ctx.upload_grid(xyz, cells, alpha, q)
        ctx.set_image(res[0], res[1], mg.REFERENCE_BOUNDS)
        ctx.set_view(rots)
        ctx.set_alpha_limit(limit)
        for lds, order, tile in VARIANTS:
            ctx.set_option("lds_stage", min(lds, 2)); ctx.set_option("stage_slots", 21 if lds == 3 else 14)
            ctx.set_option("integration", order); ctx.set_option("tile", tile)
            img = ctx.render(); st = ctx.stats()
            a, b = img.astype(np.float64), ref["image"].astype(np.float64)
            tol = 1e-5 * np.maximum(np.abs(a), np.abs(b)) + 1e-6 * np.abs(b).max()
            n_bad = int((np.abs(a - b) > tol).sum())
            if st["segments"] > 0 and st["steps"] == 0:
                bad += 1  # the walk declared the components interpenetrating (next_entry) and left the frame to bin_sort_resolve
                print(f"seed {seed} lds {lds} order {order} tile {tile}: rendered by bin_sort_resolve, not by the walk", flush=True)
                ctx.upload_grid(xyz, cells, alpha, q)  # (judge every variant anew)
            if n_bad or st["segments"] != ref["segments"] or st["covered_pixels"] != ref["covered"]:
                bad += 1
                print(f"seed {seed} lds {lds} order {order} tile {tile}: {n_bad} px beyond tolerance, "
                      f"S {st['segments']} vs {ref['segments']}, covered {st['covered_pixels']} vs {ref['covered']}, "
                      f"cells {len(cells)} res {res}", flush=True)
        # the rays cut in slabs ("depth_split" forced: 2 to 6 slabs, planes from the view alone): same bar, same counts
        ctx.set_option("lds_stage", 2); ctx.set_option("integration", 0); ctx.set_option("tile", 3)
        ctx.set_option("stage_slots", 21 if seed % 2 else 14)
        slabs = 2 + seed % 5
        ctx.set_option("depth_split", slabs)
        tilt = np.random.default_rng(seed).uniform(-1.5, 1.5, 2) if seed % 3 else np.zeros(2)  # (planes tilted: 2 in 3)
        ctx.set_option("split_tilt_x", float(tilt[0])); ctx.set_option("split_tilt_y", float(tilt[1]))
        img = ctx.render(); st = ctx.stats()
        ctx.set_option("depth_split", 0); ctx.set_option("stage_slots", 0)
        ctx.set_option("split_tilt_x", 0.0); ctx.set_option("split_tilt_y", 0.0)
        a, b = img.astype(np.float64), ref["image"].astype(np.float64)
        tol = 1e-5 * np.maximum(np.abs(a), np.abs(b)) + 1e-6 * np.abs(b).max()
        n_bad = int((np.abs(a - b) > tol).sum())
        if st["segments"] > 0 and st["steps"] == 0:
            bad += 1
            print(f"seed {seed} SPLIT in {slabs} slabs: rendered by bin_sort_resolve, not by the walk", flush=True)
            ctx.upload_grid(xyz, cells, alpha, q)
        if n_bad or st["segments"] != ref["segments"] or st["covered_pixels"] != ref["covered"]:
            bad += 1
            print(f"seed {seed} SPLIT in {slabs} slabs: {n_bad} px beyond tolerance, S {st['segments']} vs {ref['segments']}, "
                  f"covered {st['covered_pixels']} vs {ref['covered']}, steps {st['steps']}, cells {len(cells)} res {res}", flush=True)
        # sharded renders of the same scene (what the ranks of a multi-GPU run do), reassembled on the host:
        # cyclic row tiles and contiguous blocks, random world size and tile height, product-default kernel
        from course5_amd import sharding
        rng = np.random.default_rng(seed + 77)
        ctx.set_option("lds_stage", 2); ctx.set_option("integration", 0); ctx.set_option("tile", 3)
        ctx.set_option("depth_split", 1)  # (bit-equality across tilings: whole rays)
        ctx.set_row_tiles(0, 0, 1)
        ctx.set_row_range(0, -1)
        full = ctx.render()
        world = int(rng.integers(2, 6))
        tile_rows = int(rng.choice([1, 3, 8, 16]))
        strips = []
        for r in range(world):
            ctx.set_row_tiles(tile_rows, r, world)
            strips.append(ctx.render())
        ctx.set_row_tiles(0, 0, 1)
        cyc = sharding.assemble(strips, res[1], tile_rows, world)
        blocks = sharding.equal_blocks(res[1], world)
        parts = []
        for b, n_rows in blocks:
            ctx.set_row_range(b, n_rows)
            parts.append(ctx.render())
        ctx.set_row_range(0, -1)
        blk = np.concatenate(parts, axis=0)
        ctx.set_option("depth_split", 0)
        for name, img2 in (("cyclic", cyc), ("blocks", blk)):
            if not np.array_equal(img2.view(np.uint32), full.view(np.uint32)):
                bad += 1
                print(f"seed {seed}: {name} shards (world {world}, tile_rows {tile_rows}) differ from the full frame", flush=True)
    print(f"{n_scenes} scenes x ({len(VARIANTS)} variants + 1 render cut in slabs + 2 sharded layouts): {bad} mismatching renders")
    return bad

if __name__ == "__main__":
    sys.exit(1 if main() else 0)

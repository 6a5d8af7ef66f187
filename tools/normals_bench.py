#!/usr/bin/env python3
"""Times the two surface-normal calls; prints one JSON line.  Not the headline benchmark (bench.py).

Query (bt_tile_tree_sample_normal): raycast_bench.py's terrains (planar and sphere, T = 512, 4 LODs, streamed along a short camera path, so
positions fall on tiles of several LODs and in blend rings); wall time of one synchronous call at 1, 64 and 4096 positions, beside
bt_tile_tree_sample_attachment on the same positions.
Bake (bt_atlas_tile_normals): the tiles of bench.py's 16k job (synth_fbm_r16 16384^2, T = 512, lod_count 6, 1365 tiles); wall time of one
synchronous call at 1, 16 and 1365 tiles (the last moves 1.4 GB to the host), beside bt_atlas_tile_bounds at grid 1 on the same layers.

    python tools/normals_bench.py [--repeats N]
    rocprofv3 --kernel-trace --stats --output-format csv -- python tools/normals_bench.py --trace
        # kernel times: tile_tree_normal_kernel beside tile_tree_sample_kernel on the same 262144 positions per model, and
        # tile_normals_kernel (43 launches of 32 tiles per call: sum them) beside tile_bounds_kernel on the 1365 layers; the JSON line
        # gives the counts and the algorithmic bytes to divide by
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import ctypes as C

import bevy_terrain_amd as bt
import raycast_bench as RB
from bevy_terrain_amd import _ffi

SIZE, TEXTURE_SIZE, BORDER, LOD_COUNT, ATLAS_SIZE, SEED = 16384, 512, 2, 6, 2048, 42  # bench.py's 16k job
TRACE_POSITIONS, TRACE_CALLS = 262144, 5


def wall_ms(device, fn, repeats):
    """host wall time per call, the median of `repeats` calls (each call ends in a device synchronise)"""
    times = []
    for _ in range(repeats):
        device.synchronize()
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    times.sort()
    return times[len(times) // 2]


def positions(model, view, n, seed):
    """ground-level positions within a few tiles of the view (and, planar, over the whole terrain)"""
    rng = np.random.default_rng(seed)
    pos = np.asarray(model.translation)
    if model.kind == "planar":
        return pos + np.column_stack([rng.uniform(-500, 500, n), rng.uniform(0, 250, n), rng.uniform(-500, 500, n)])
    centre = RB.unit(np.asarray(view) - pos)
    return pos + RB.unit(centre + rng.normal(size=(n, 3)) * 0.35) * (model.scale_vec[0] + rng.uniform(-1.0e3, 5.0e3, (n, 1)))


def bake_job(device):
    cfg = bt.TerrainConfig(lod_count=LOD_COUNT, atlas_size=ATLAS_SIZE, path="terrains/bench16k",
                           model=bt.TerrainModel.planar((0.0, 0.0, 0.0), 1000.0, 0.0, 250.0))
    cfg.add_attachment(bt.AttachmentConfig(name="height", texture_size=TEXTURE_SIZE, border_size=BORDER, format=bt.AttachmentFormat.R16))
    atlas = bt.TileAtlas.new(cfg, device)
    src = device.synth_fbm_r16(SIZE, SIZE, SEED)
    pre = bt.Preprocessor.new().clear_attachment(0, atlas).preprocess_tile(
        bt.PreprocessDataset(attachment_index=0, path="synthetic/fbm16k", lod_range=range(0, LOD_COUNT)),
        bt.AssetServer().insert("synthetic/fbm16k", (src, SIZE, SIZE)), atlas)
    pre.run(atlas)
    pre.close()
    device.free(src)
    tiles = atlas.tiles()
    assert len(tiles) == 1365, len(tiles)
    return atlas, [c for c, _ in tiles], [i for _, i in tiles]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    device = bt.Device(0)
    c = TEXTURE_SIZE - 2 * BORDER
    result = {"tool": "normals_bench", "texture_size": TEXTURE_SIZE, "repeats": args.repeats,
              "bake_algorithmic_bytes_per_tile": TEXTURE_SIZE * TEXTURE_SIZE * 2 + c * c * 4,
              "bounds_algorithmic_bytes_per_tile": TEXTURE_SIZE * TEXTURE_SIZE * 2 + 4}
    root = tempfile.mkdtemp(prefix="normals_bench_")
    try:
        for kind in ("planar", "sphere"):
            model, atlas, tree, view, lods = RB.build(device, kind, root)
            result[f"{kind}_entry_lods"] = lods
            if args.trace:
                pts = positions(model, view, TRACE_POSITIONS, 5)
                for _ in range(TRACE_CALLS):
                    tree.sample_attachment(0, pts)
                    tree.sample_normal(0, pts)
                result["trace_positions"], result["trace_calls"] = TRACE_POSITIONS, TRACE_CALLS
                result[f"{kind}_steep_share"] = round(float((tree.sample_normal(0, pts[:4096])[1] < 0.999).mean()), 3)
            else:
                for n in (1, 64, 4096):
                    pts = positions(model, view, n, 5)
                    for _ in range(5):
                        tree.sample_normal(0, pts)
                        tree.sample_attachment(0, pts)
                    result[f"{kind}_normal_{n}_wall_ms"] = round(wall_ms(device, lambda: tree.sample_normal(0, pts), args.repeats), 4)
                    result[f"{kind}_sample_{n}_wall_ms"] = round(wall_ms(device, lambda: tree.sample_attachment(0, pts), args.repeats), 4)
            tree.close()
            del atlas
            device.trim()
    finally:
        shutil.rmtree(root, ignore_errors=True)
    atlas, coords, layers = bake_job(device)
    # the C call into one buffer whose pages exist already: the wrapper's fresh 1.4 GB array would be timed as page faults
    out = np.zeros((len(coords), c, c, 4), np.uint8)
    out.fill(1)
    arr = (_ffi.TileCoordinateC * len(coords))(*[t._c() for t in coords])
    model = bt.tile_tree.model_c(atlas.config.model)

    def bake(n):
        _ffi.check(_ffi.lib().bt_atlas_tile_normals(atlas._h, 0, C.byref(model), arr, n, out.ctypes.data_as(C.POINTER(C.c_uint8)), out.nbytes))

    if args.trace:
        for _ in range(TRACE_CALLS):
            atlas.tile_bounds(0, layers, 1)
            bake(len(coords))
        result["trace_tiles"] = len(coords)
    else:
        for n in (1, 16, 1365):
            repeats = args.repeats if n < 1365 else max(3, args.repeats // 6)
            for _ in range(2):
                bake(n)
                atlas.tile_bounds(0, layers[:n], 1)
            result[f"bake_{n}_wall_ms"] = round(wall_ms(device, lambda: bake(n), repeats), 4)
            result[f"bounds_grid1_{n}_wall_ms"] = round(wall_ms(device, lambda: atlas.tile_bounds(0, layers[:n], 1), repeats), 4)
        assert np.array_equal(out[:16], atlas.tile_normals(0, coords[:16]))
        flat = atlas.tile_normals(0, coords[-16:])
        result["bake_finest_steep_share"] = round(float((flat[..., 2] < 250).mean()), 3)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()

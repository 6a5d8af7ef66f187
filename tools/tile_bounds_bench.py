#!/usr/bin/env python3
"""Times bt_atlas_tile_bounds on the tiles of bench.py's 16k job (synth_fbm_r16 16384^2, T = 512, lod_count 6, 1365 tiles); prints one JSON
line.  Not the headline benchmark (bench.py).

Per call: the whole pyramid of every listed layer, one synchronous call (layer list up, kernel, pyramids down, synchronise).  The wall
times below therefore include the device-to-host copy of the result (30 MB at grid 64) and the host's copy out of pinned memory: kernel
time comes from a separate `rocprofv3 --kernel-trace --stats` run of this script (kernel tile_bounds_kernel), and the rates of that run are
what DESIGN.md reports.  The 1365 layers are 716 MB, more than the 256 MiB Infinity Cache, so back-to-back calls read mostly from HBM.

    python tools/tile_bounds_bench.py [--repeats N]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bevy_terrain_amd as bt

SIZE, TEXTURE_SIZE, BORDER, LOD_COUNT, ATLAS_SIZE, SEED = 16384, 512, 2, 6, 2048, 42  # bench.py's 16k job


def algorithmic_bytes(layers, T, grid):
    """each texel read once + each cell written once"""
    return layers * T * T * 2 + layers * (4 * grid * grid - 1) // 3 * 4


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=50)
    args = ap.parse_args()
    device = bt.Device(0)
    cfg = bt.TerrainConfig(lod_count=LOD_COUNT, atlas_size=ATLAS_SIZE, path="terrains/bench16k",
                           model=bt.TerrainModel.planar((0.0, 0.0, 0.0), 1000.0, 0.0, 1.0))
    cfg.add_attachment(bt.AttachmentConfig(name="height", texture_size=TEXTURE_SIZE, border_size=BORDER, format=bt.AttachmentFormat.R16))
    atlas = bt.TileAtlas.new(cfg, device)
    src = device.synth_fbm_r16(SIZE, SIZE, SEED)
    pre = bt.Preprocessor.new().clear_attachment(0, atlas).preprocess_tile(
        bt.PreprocessDataset(attachment_index=0, path="synthetic/fbm16k", lod_range=range(0, LOD_COUNT)),
        bt.AssetServer().insert("synthetic/fbm16k", (src, SIZE, SIZE)), atlas)
    pre.run(atlas)
    layers = [i for _, i in atlas.tiles()]
    assert len(layers) == 1365, len(layers)
    result = {"tool": "tile_bounds_bench", "layers": len(layers), "texture_size": TEXTURE_SIZE, "repeats": args.repeats,
              "note": "wall ms per synchronous call, median; includes the result's device-to-host copy; kernel time: rocprofv3 run"}
    for grid in (1, 64):
        for _ in range(5):  # warm-up: code object, scratch growth
            atlas.tile_bounds(0, layers, grid)
        ms = wall_ms(device, lambda: atlas.tile_bounds(0, layers, grid), args.repeats)
        result[f"grid{grid}_all_layers_wall_ms"] = round(ms, 4)
        result[f"grid{grid}_algorithmic_bytes"] = algorithmic_bytes(len(layers), TEXTURE_SIZE, grid)
        result[f"grid{grid}_wall_TBps"] = round(algorithmic_bytes(len(layers), TEXTURE_SIZE, grid) / (ms * 1e-3) / 1e12, 3)
    small = layers[:16]
    for _ in range(5):
        atlas.tile_bounds(0, small, 8)
    result["grid8_16_layers_wall_us"] = round(wall_ms(device, lambda: atlas.tile_bounds(0, small, 8), args.repeats) * 1e3, 1)
    print(json.dumps(result), flush=True)
    pre.close()
    device.free(src)


if __name__ == "__main__":
    main()

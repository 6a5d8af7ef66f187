#!/usr/bin/env python3
"""Times bt_atlas_scatter_instances; prints one JSON line.  Not the headline benchmark (bench.py).

The terrain: synth_fbm_r16 2048^2, T = 260, b = 2 (c = 256), lod_count 4, so the 64 tiles of the finest level are a 2048^2 window of the
heights; a second, Rgba8 attachment of the same tiling receives a weights splat map.  The call scatters those 64 tiles with two rules (one on
a mask byte with height and slope bands that fade, one on steep ground) whose densities are scaled to --density.  Wall time of one
synchronous call: sizing (cap 0: decide and scan), and the full call with the list copied out; for scale, bt_atlas_splat_from_height on the
same window (not synchronising: the wall time includes a device synchronise).

    python tools/scatter_bench.py [--repeats N] [--density 0.01 0.25]
    rocprofv3 --kernel-trace --stats --output-format csv -- python tools/scatter_bench.py --trace --density 0.25
        # kernel times of scatter_decide_kernel, scatter_scan_kernel, scatter_emit_kernel and edit_splat_kernel: TRACE_CALLS calls each
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bevy_terrain_amd as bt

SIZE, TEXTURE_SIZE, BORDER, LOD_COUNT, SEED = 2048, 260, 2, 4, 42
HEIGHT, SPLAT = 0, 1
TRACE_CALLS = 10
INF = math.inf
SPLAT_RULES = [bt.SplatRule(height=(-INF, 90.0), height_fade=10.0), bt.SplatRule(height=(90.0, 170.0), height_fade=20.0, slope=(0.0, 30.0), slope_fade=0.08),
               bt.SplatRule(height=(180.0, INF), height_fade=20.0, weight=2.0), bt.SplatRule(slope=(32.0, 90.0), slope_fade=0.08, weight=1.5)]


def rules(density):
    return [bt.ScatterRule(height=(60.0, 200.0), height_fade=20.0, slope=(0.0, 35.0), slope_fade=0.08, density=density, mask_channel="g", scale=(0.8, 1.6)),
            bt.ScatterRule(slope=(30.0, 90.0), slope_fade=0.08, density=density, scale=(0.4, 1.2)), bt.ScatterRule(density=density / 4)]


def wall_ms(device, fn, repeats):
    """host wall time per call, the median of `repeats` calls (each ends in a device synchronise)"""
    times = []
    for _ in range(repeats):
        device.synchronize()
        t0 = time.perf_counter()
        fn()
        device.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    times.sort()
    return times[len(times) // 2]


def job(device):
    cfg = bt.TerrainConfig(lod_count=LOD_COUNT, atlas_size=128, path="terrains/scatter_bench", model=bt.TerrainModel.planar((0.0, 0.0, 0.0), 1000.0, 0.0, 250.0))
    cfg.add_attachment(bt.AttachmentConfig(name="height", texture_size=TEXTURE_SIZE, border_size=BORDER, format=bt.AttachmentFormat.R16))
    cfg.add_attachment(bt.AttachmentConfig(name="splat", texture_size=TEXTURE_SIZE, border_size=BORDER, format=bt.AttachmentFormat.Rgba8))
    atlas = bt.TileAtlas.new(cfg, device)
    src = device.synth_fbm_r16(SIZE, SIZE, SEED)
    pre = bt.Preprocessor.new().clear_attachment(HEIGHT, atlas).preprocess_tile(
        bt.PreprocessDataset(attachment_index=HEIGHT, path="synthetic/fbm", lod_range=range(0, LOD_COUNT)), bt.AssetServer().insert("synthetic/fbm", (src, SIZE, SIZE)), atlas)
    pre.run(atlas)
    pre.close()
    device.free(src)
    coords = [c for c, _ in atlas.tiles() if c.lod == LOD_COUNT - 1]
    assert len(coords) == 64, len(coords)
    return atlas, coords


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--density", type=float, nargs="+", default=[0.01, 0.25])
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    device = bt.Device(0)
    atlas, coords = job(device)
    splat = lambda: atlas.splat_from_height(HEIGHT, SPLAT, SPLAT_RULES, mode="weights", fallback=(0, 0, 0, 255))
    splat()
    c = TEXTURE_SIZE - 2 * BORDER
    result = {"tool": "scatter_bench", "window": SIZE, "texture_size": TEXTURE_SIZE, "tiles": len(coords), "cells": len(coords) * c * c, "repeats": args.repeats}
    if args.trace:
        for _ in range(TRACE_CALLS):
            splat()
        result["trace_calls"] = TRACE_CALLS
    else:
        result["splat_wall_ms"] = round(wall_ms(device, splat, args.repeats), 4)
    for density in args.density:
        r = rules(density)
        instances, first, stats = atlas.scatter_instances(HEIGHT, r, coords, mask_attachment=SPLAT, seed=1)
        again, _, _ = atlas.scatter_instances(HEIGHT, r, coords, mask_attachment=SPLAT, seed=1)
        assert instances.tobytes() == again.tobytes() and int(first[-1]) == stats["total"] == len(instances)
        key = f"density_{density:g}"
        result[key + "_instances"], result[key + "_per_rule"], result[key + "_no_data"] = stats["total"], stats["per_rule"][:3], stats["cells_no_data"]
        full = lambda: atlas.scatter_instances(HEIGHT, r, coords, mask_attachment=SPLAT, seed=1, cap=stats["total"])
        sizing = lambda: atlas.scatter_instances(HEIGHT, r, coords, mask_attachment=SPLAT, seed=1, cap=0)
        if args.trace:
            for _ in range(TRACE_CALLS):
                full()
        else:
            result[key + "_sizing_wall_ms"] = round(wall_ms(device, sizing, args.repeats), 4)
            result[key + "_full_wall_ms"] = round(wall_ms(device, full, args.repeats), 4)
            result[key + "_list_bytes"] = stats["total"] * 56
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()

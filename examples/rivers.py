#!/usr/bin/env python3
"""Lakes and rivers: where water collects on a terrain and where it runs, on the device.

A small synthetic planar terrain (the R16 height of examples/erosion.py, preprocessed from fBm noise).  TileAtlas.drainage analyses the whole
finest mosaic: it fills every depression to the level at which it spills (the lakes: filled > height), gives every cell the neighbour its
water goes to, and sums what drains through each cell (the rivers: a large accumulation).  Both are drawn over the shaded heights, and one
river is followed with trace_path from the highest cell of the terrain down to where it leaves the window: the direction plane uses the
codes of the path field's next plane.

    python examples/rivers.py [--texture-size 64] [--lods 3] [--threshold 200] [--ppm rivers.ppm]
"""
import argparse
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bevy_terrain_amd as bt  # noqa: E402
from bevy_terrain_amd import AssetServer, AttachmentConfig, AttachmentFormat, PreprocessDataset, Preprocessor, TerrainConfig, TerrainModel, TileAtlas  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))  # (for a caller that imports this file instead of running it)
import _sources  # noqa: E402
from erosion import BORDER_SIZE, HEIGHT, MAX_HEIGHT, MIN_HEIGHT, TERRAIN_SIZE, shaded  # noqa: E402

LAKE, RIVER, TRACED = (40, 90, 200), (90, 170, 255), (255, 60, 40)


def run(device, texture_size=64, lod_count=3, threshold=200, seed=1234):
    """builds the terrain and analyses its finest mosaic; returns what it made"""
    center_size = texture_size - 2 * BORDER_SIZE
    size = center_size << (lod_count - 1)  # the finest mosaic, which the source matches
    model = TerrainModel.planar((0.0, 0.0, 0.0), TERRAIN_SIZE, MIN_HEIGHT, MAX_HEIGHT)
    tile_count = (4 ** lod_count - 1) // 3
    config = (TerrainConfig(lod_count=lod_count, atlas_size=tile_count, path="terrains/rivers", model=model)
              .add_attachment(AttachmentConfig(name="height", texture_size=texture_size, border_size=BORDER_SIZE, format=AttachmentFormat.R16)))
    tile_atlas = TileAtlas.new(config, device)
    asset_server = AssetServer().insert("height", _sources.height(device, size, seed))
    (Preprocessor.new().clear_attachment(HEIGHT, tile_atlas)
     .preprocess_tile(PreprocessDataset(attachment_index=HEIGHT, path="height", lod_range=range(0, lod_count)), asset_server, tile_atlas)
     .run(tile_atlas))

    heights, _ = tile_atlas.read_region(HEIGHT, 0, 0, size, size)
    filled, flat, direction, accumulation, stats = tile_atlas.drainage(HEIGHT, 0, 0, size, size)
    lakes = filled > heights
    rivers = (accumulation >= threshold) & ~lakes
    top = np.unravel_index(np.argmax(heights), heights.shape)
    river, status = bt.trace_path(direction, (int(top[1]), int(top[0])))
    return types.SimpleNamespace(tile_atlas=tile_atlas, size=size, threshold=threshold, heights=heights, filled=filled, flat=flat, direction=direction,
                                 accumulation=accumulation, stats=stats, lakes=lakes, rivers=rivers, river=river, river_status=status)


def picture(made):
    rgb = shaded(made.heights)
    rgb[made.rivers] = RIVER
    rgb[made.lakes] = LAKE
    rgb[made.river[:, 1], made.river[:, 0]] = TRACED
    return rgb


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--texture-size", type=int, default=64)
    ap.add_argument("--lods", type=int, default=3)
    ap.add_argument("--threshold", type=int, default=200, help="cells that drain through a texel before it is drawn as a river")
    ap.add_argument("--ppm", default=None, help="draw the lakes and rivers over the shaded heights")
    args = ap.parse_args(argv)
    made = run(bt.Device(0), args.texture_size, args.lods, args.threshold)
    s = made.stats
    print(f"drainage of a {made.size} x {made.size} mosaic: {s['outlets']} outlets, {s['voids']} void cells, {s['launches']} launches "
          f"({s['sweeps_fill']} fill, {s['sweeps_flat']} flat and {s['sweeps_accumulate']} accumulation sweeps)")
    print(f"lake texels: {int(made.lakes.sum())} (the deepest {int((made.filled.astype(np.int64) - made.heights)[made.lakes].max(initial=0))} raw units, "
          f"flat distances up to {s['max_flat_distance']}); river texels at {made.threshold} cells or more: {int(made.rivers.sum())}; "
          f"the largest accumulation is {s['max_accumulation']} of {s['outflow']} cells")
    end = made.river[-1]
    print(f"the river from the summit: {len(made.river)} cells, {made.river_status}, it leaves at ({int(end[0])}, {int(end[1])}) with "
          f"{int(made.accumulation[end[1], end[0]])} cells drained")
    if args.ppm:
        rgb = picture(made)
        bt.write_ppm(args.ppm, rgb)
        print(f"drew {rgb.shape[1]} x {rgb.shape[0]} to {args.ppm}")
    return made


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""A setback from the rivers: trees keep their distance from running water, all of it on the device.

The small synthetic planar terrain of examples/rivers.py (an R16 height preprocessed from fBm noise) with an Rgba8 mask attachment beside
it.  TileAtlas.drainage finds the rivers (the cells through which at least --threshold cells drain); they are the seeds of
TileAtlas.distance_field, which gives every cell its exact distance to the nearest river cell and bakes it into a byte of the mask: 0 on
the river, 255 from --reach cells on.  TileAtlas.scatter_instances then places trees with that byte as their mask, so none stands on a
river and they thin out towards the banks.

    python examples/setback.py [--texture-size 64] [--lods 3] [--threshold 200] [--reach 12] [--seed 7] [--ppm setback.ppm]
"""
import argparse
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bevy_terrain_amd as bt  # noqa: E402
from bevy_terrain_amd import AssetServer, AttachmentConfig, AttachmentFormat, PreprocessDataset, Preprocessor, ScatterRule, TerrainConfig, TerrainModel, TileAtlas  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))  # (for a caller that imports this file instead of running it)
import _sources  # noqa: E402
from erosion import BORDER_SIZE, HEIGHT, MAX_HEIGHT, MIN_HEIGHT, TERRAIN_SIZE, shaded  # noqa: E402

MASK = 1          # the Rgba8 attachment beside the heights
CHANNEL = 1       # its byte that takes the setback ("g")
TREE_RULES = [ScatterRule(density=0.25, mask_channel=CHANNEL, scale=(0.8, 1.6))]
RIVER, TREE = (90, 170, 255), (10, 60, 20)


def run(device, texture_size=64, lod_count=3, threshold=200, reach=12, seed=7, source_seed=1234):
    """builds the terrain, finds the rivers, bakes the setback and scatters the trees; returns what it made"""
    center_size = texture_size - 2 * BORDER_SIZE
    size = center_size << (lod_count - 1)  # the finest mosaic, which the source matches
    model = TerrainModel.planar((0.0, 0.0, 0.0), TERRAIN_SIZE, MIN_HEIGHT, MAX_HEIGHT)
    tile_count = (4 ** lod_count - 1) // 3
    config = (TerrainConfig(lod_count=lod_count, atlas_size=tile_count, path="terrains/setback", model=model)
              .add_attachment(AttachmentConfig(name="height", texture_size=texture_size, border_size=BORDER_SIZE, format=AttachmentFormat.R16))
              .add_attachment(AttachmentConfig(name="mask", texture_size=texture_size, border_size=BORDER_SIZE, format=AttachmentFormat.Rgba8)))
    tile_atlas = TileAtlas.new(config, device)
    asset_server = AssetServer().insert("height", _sources.height(device, size, source_seed))
    (Preprocessor.new().clear_attachment(HEIGHT, tile_atlas).clear_attachment(MASK, tile_atlas)
     .preprocess_tile(PreprocessDataset(attachment_index=HEIGHT, path="height", lod_range=range(0, lod_count)), asset_server, tile_atlas)
     .run(tile_atlas))

    heights, _ = tile_atlas.read_region(HEIGHT, 0, 0, size, size)
    _, _, _, accumulation, _ = tile_atlas.drainage(HEIGHT, 0, 0, size, size)
    rivers = accumulation >= threshold
    dist2, nearest, stats = tile_atlas.distance_field(HEIGHT, 0, 0, size, size, seeds=rivers, bake=dict(attachment=MASK, channel=CHANNEL, reach=reach))
    mask, _ = tile_atlas.read_region(MASK, 0, 0, size, size)
    coords = sorted((t for t, _ in tile_atlas.tiles() if t.lod == lod_count - 1), key=lambda t: (t.y, t.x))
    instances, _, scatter_stats = tile_atlas.scatter_instances(HEIGHT, TREE_RULES, coords, mask_attachment=MASK, seed=seed)
    return types.SimpleNamespace(tile_atlas=tile_atlas, size=size, threshold=threshold, reach=reach, heights=heights, rivers=rivers, dist2=dist2, nearest=nearest,
                                 stats=stats, byte=mask[:, :, CHANNEL], trees=instances["cell"], scatter_stats=scatter_stats)


def picture(made):
    """the heights shaded, darker towards the rivers, the rivers and a dot per tree"""
    rgb = shaded(made.heights)
    rgb = (rgb.astype(np.uint16) * (96 + made.byte.astype(np.uint16) * 159 // 255)[:, :, None] // 255).astype(np.uint8)
    rgb[made.rivers] = RIVER
    rgb[made.trees[:, 1], made.trees[:, 0]] = TREE
    return rgb


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--texture-size", type=int, default=64)
    ap.add_argument("--lods", type=int, default=3)
    ap.add_argument("--threshold", type=int, default=200, help="cells that drain through a texel before it is a river")
    ap.add_argument("--reach", type=int, default=12, help="the distance from a river, in cells, from which trees stand at their full density")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--ppm", default=None, help="draw the rivers, the distance shading and the trees")
    ap.add_argument("--save", default=None, help="save the rivers, the distances, the baked byte and the trees' cells (.npz)")
    args = ap.parse_args(argv)
    made = run(bt.Device(0), args.texture_size, args.lods, args.threshold, args.reach, args.seed)
    s = made.stats
    on_river = int(made.rivers[made.trees[:, 1], made.trees[:, 0]].sum())
    within = int((made.byte[made.trees[:, 1], made.trees[:, 0]] < 255).sum())
    print(f"distance field of a {made.size} x {made.size} mosaic: {s['seeds']} river cells at {made.threshold} cells or more, the farthest cell is "
          f"{s['max_dist2']} away squared, {s['launches']} launches and {s['edit']['launches']} of the bake over {s['edit']['tiles_edited']} tiles")
    print(f"trees: {len(made.trees)}, on a river cell: {on_river}, within {made.reach} cells of a river: {within}")
    if args.save:
        np.savez(args.save, rivers=made.rivers, dist2=made.dist2, nearest=made.nearest, byte=made.byte, trees=made.trees)
    if args.ppm:
        rgb = picture(made)
        bt.write_ppm(args.ppm, rgb)
        print(f"drew {rgb.shape[1]} x {rgb.shape[0]} to {args.ppm}")
    return made


if __name__ == "__main__":
    main()

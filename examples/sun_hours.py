#!/usr/bin/env python3
"""Hours of sun: a day of suns over a terrain, the shadows of every one of them from a single call, all of it on the device.

The small synthetic planar terrain of examples/erosion.py (an R16 height preprocessed from fBm noise) with an Rgba8 mask attachment beside
it.  TileAtlas.sun_directions turns --suns sun positions of one day (rising at +x, culminating over +y at --max-elevation degrees, setting
at -x) into integer directions; TileAtlas.skyline finds every cell's horizon towards each of them, counts the suns that light the cell and
bakes that count into a byte of the mask: 0 where no sun of the day reaches, 255 where all do.  TileAtlas.scatter_instances then places
trees with that byte as their mask, so none stands where the sun never shines and they thin out towards the shade.

    python examples/sun_hours.py [--texture-size 64] [--lods 3] [--suns 24] [--max-elevation 30] [--seed 7] [--ppm sun_hours.ppm]
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
CHANNEL = 2       # its byte that takes the hours of sun ("b")
TREE_RULES = [ScatterRule(density=0.25, mask_channel=CHANNEL, scale=(0.8, 1.6))]
TREE = (10, 60, 20)


def day(suns, max_elevation):
    """(azimuth, elevation) in degrees of `suns` moments of a day, none of them on the horizon"""
    t = (np.arange(suns) + 0.5) / suns
    return 180.0 * t, max_elevation * np.sin(np.pi * t)


def run(device, texture_size=64, lod_count=3, suns=24, max_elevation=30.0, seed=7, source_seed=1234):
    """builds the terrain, finds the hours of sun, bakes them and scatters the trees; returns what it made"""
    center_size = texture_size - 2 * BORDER_SIZE
    size = center_size << (lod_count - 1)  # the finest mosaic, which the source matches
    model = TerrainModel.planar((0.0, 0.0, 0.0), TERRAIN_SIZE, MIN_HEIGHT, MAX_HEIGHT)
    tile_count = (4 ** lod_count - 1) // 3
    config = (TerrainConfig(lod_count=lod_count, atlas_size=tile_count, path="terrains/sun_hours", model=model)
              .add_attachment(AttachmentConfig(name="height", texture_size=texture_size, border_size=BORDER_SIZE, format=AttachmentFormat.R16))
              .add_attachment(AttachmentConfig(name="mask", texture_size=texture_size, border_size=BORDER_SIZE, format=AttachmentFormat.Rgba8)))
    tile_atlas = TileAtlas.new(config, device)
    asset_server = AssetServer().insert("height", _sources.height(device, size, source_seed))
    (Preprocessor.new().clear_attachment(HEIGHT, tile_atlas).clear_attachment(MASK, tile_atlas)
     .preprocess_tile(PreprocessDataset(attachment_index=HEIGHT, path="height", lod_range=range(0, lod_count)), asset_server, tile_atlas)
     .run(tile_atlas))

    heights, _ = tile_atlas.read_region(HEIGHT, 0, 0, size, size)
    azimuth, elevation = day(suns, max_elevation)
    directions = TileAtlas.sun_directions(azimuth, elevation, cell_size=TERRAIN_SIZE / size, raw_unit=(MAX_HEIGHT - MIN_HEIGHT) / 65535.0)
    _, _, mask, count, stats = tile_atlas.skyline(HEIGHT, 0, 0, size, size, directions, steps=False, rise=False, bake=dict(attachment=MASK, channel=CHANNEL))
    baked, _ = tile_atlas.read_region(MASK, 0, 0, size, size)
    coords = sorted((t for t, _ in tile_atlas.tiles() if t.lod == lod_count - 1), key=lambda t: (t.y, t.x))
    instances, _, scatter_stats = tile_atlas.scatter_instances(HEIGHT, TREE_RULES, coords, mask_attachment=MASK, seed=seed)
    return types.SimpleNamespace(tile_atlas=tile_atlas, size=size, suns=suns, directions=directions, heights=heights, mask=mask, count=count, stats=stats,
                                 byte=baked[:, :, CHANNEL], trees=instances["cell"], scatter_stats=scatter_stats)


def picture(made):
    """the heights shaded, from a cold dark tone where no sun reaches to a warm full one where all do, and a dot per tree"""
    rgb = shaded(made.heights).astype(np.uint16)
    sun = made.byte.astype(np.uint16)
    tint = np.stack([110 + sun * 145 // 255, 110 + sun * 135 // 255, 150 + sun * 60 // 255], axis=2)
    rgb = (rgb * tint // 255).astype(np.uint8)
    rgb[made.trees[:, 1], made.trees[:, 0]] = TREE
    return rgb


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--texture-size", type=int, default=64)
    ap.add_argument("--lods", type=int, default=3)
    ap.add_argument("--suns", type=int, default=24, help="moments of the day, 64 at most")
    ap.add_argument("--max-elevation", type=float, default=30.0, help="the sun's elevation at noon, in degrees")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--ppm", default=None, help="draw the hours of sun over the shaded heights, and the trees")
    ap.add_argument("--save", default=None, help="save the heights, the directions, the mask, the count, the baked byte and the trees' cells (.npz)")
    args = ap.parse_args(argv)
    made = run(bt.Device(0), args.texture_size, args.lods, args.suns, args.max_elevation, args.seed)
    s = made.stats
    at = made.count[made.trees[:, 1], made.trees[:, 0]]
    print(f"skyline of a {made.size} x {made.size} mosaic: {s['directions']} suns over {s['lines']} lines, the farthest horizon {s['max_steps']} steps away, "
          f"{s['launches']} launches and {s['edit']['launches']} of the bake over {s['edit']['tiles_edited']} tiles")
    print(f"cells: {s['cells']}, without any sun: {int((made.count == 0).sum())}, with every sun: {int((made.count == made.suns).sum())}, sun on average: "
          f"{s['lit'] / s['cells']:.2f} of {made.suns}")
    print(f"trees: {len(made.trees)}, on a cell without sun: {int((at == 0).sum())}, on a cell with every sun: {int((at == made.suns).sum())}")
    if args.save:
        np.savez(args.save, heights=made.heights, directions=made.directions, mask=made.mask, count=made.count, byte=made.byte, trees=made.trees)
    if args.ppm:
        rgb = picture(made)
        bt.write_ppm(args.ppm, rgb)
        print(f"drew {rgb.shape[1]} x {rgb.shape[0]} to {args.ppm}")
    return made


if __name__ == "__main__":
    main()

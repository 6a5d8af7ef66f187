#!/usr/bin/env python3
"""Watchtowers: what a set of observers sees of a terrain, on the device.

A small synthetic planar terrain (the R16 height of examples/erosion.py, preprocessed from fBm noise) and two watchtowers: one on the
summit with an unlimited view, one on the highest cell of the opposite half of the map that watches a disc of a third of the map.
TileAtlas.viewshed walks the line of sight from each tower to every cell of the finest mosaic, in integers: count says how many towers
see a target of --target-height raw units on the cell, mask which ones, and clearance how tall a mast on the cell must be to be seen by
the tower that sees it soonest.  The seen cells are drawn over the shaded heights: by the first tower, by the second, by both.

    python examples/viewshed.py [--texture-size 64] [--lods 3] [--eye-height 400] [--target-height 30] [--ppm viewshed.ppm] [--heights heights.npy]
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

FIRST, SECOND, BOTH, TOWER = (255, 210, 60), (90, 200, 255), (255, 255, 255), (255, 40, 40)


def towers(heights, eye_height):
    """(x, y, eye_height, radius) of the two: the summit, and the highest cell of the half of the map the summit is not in"""
    size = heights.shape[0]
    y0, x0 = np.unravel_index(np.argmax(heights), heights.shape)
    other = heights.copy()
    if x0 < size // 2:
        other[:, :size // 2] = 0
    else:
        other[:, size // 2:] = 0
    y1, x1 = np.unravel_index(np.argmax(other), other.shape)
    return [(int(x0), int(y0), eye_height, 0), (int(x1), int(y1), eye_height, size // 3)]


def run(device, texture_size=64, lod_count=3, eye_height=400, target_height=30, seed=1234):
    """builds the terrain and asks what the two towers see of its finest mosaic; returns what it made"""
    center_size = texture_size - 2 * BORDER_SIZE
    size = center_size << (lod_count - 1)  # the finest mosaic, which the source matches
    model = TerrainModel.planar((0.0, 0.0, 0.0), TERRAIN_SIZE, MIN_HEIGHT, MAX_HEIGHT)
    tile_count = (4 ** lod_count - 1) // 3
    config = (TerrainConfig(lod_count=lod_count, atlas_size=tile_count, path="terrains/viewshed", model=model)
              .add_attachment(AttachmentConfig(name="height", texture_size=texture_size, border_size=BORDER_SIZE, format=AttachmentFormat.R16)))
    tile_atlas = TileAtlas.new(config, device)
    asset_server = AssetServer().insert("height", _sources.height(device, size, seed))
    (Preprocessor.new().clear_attachment(HEIGHT, tile_atlas)
     .preprocess_tile(PreprocessDataset(attachment_index=HEIGHT, path="height", lod_range=range(0, lod_count)), asset_server, tile_atlas)
     .run(tile_atlas))

    heights, _ = tile_atlas.read_region(HEIGHT, 0, 0, size, size)
    observers = towers(heights, eye_height)
    clearance, count, mask, stats = tile_atlas.viewshed(HEIGHT, 0, 0, size, size, observers, target_height=target_height, mask=True)
    return types.SimpleNamespace(tile_atlas=tile_atlas, size=size, heights=heights, observers=observers, target_height=target_height, clearance=clearance,
                                 count=count, mask=mask, stats=stats)


def picture(made):
    rgb = shaded(made.heights)
    for bits, colour in ((1, FIRST), (2, SECOND), (3, BOTH)):
        seen = made.mask == bits
        rgb[seen] = (rgb[seen].astype(np.uint16) + np.array(colour, np.uint16)) // 2
    for x, y, _, _ in made.observers:
        rgb[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = TOWER
    return rgb


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--texture-size", type=int, default=64)
    ap.add_argument("--lods", type=int, default=3)
    ap.add_argument("--eye-height", type=int, default=400, help="of both towers, in raw height units")
    ap.add_argument("--target-height", type=int, default=30, help="of what is to be seen on a cell, in raw height units")
    ap.add_argument("--ppm", default=None, help="draw the seen cells over the shaded heights")
    ap.add_argument("--heights", default=None, help="save the mosaic's raw heights (numpy .npy)")
    args = ap.parse_args(argv)
    made = run(bt.Device(0), args.texture_size, args.lods, args.eye_height, args.target_height)
    s = made.stats
    print(f"viewshed of a {made.size} x {made.size} mosaic from {s['observers_used']} towers at " + " and ".join(f"({x}, {y})" for x, y, _, _ in made.observers)
          + f": {s['samples']} line samples in {s['launches']} launches")
    print(f"covered cells: {s['covered']}; cells on which a target of {made.target_height} is seen: {s['visible']} "
          f"(by the first tower {int((made.mask & 1 != 0).sum())}, by the second {int((made.mask & 2 != 0).sum())}, by both {int((made.count == 2).sum())}); "
          f"the tallest mast needed: {s['max_clearance']}")
    for x, y in ((0, 0), (made.size // 2, made.size // 2), (made.size - 1, made.size // 3)):
        c = int(made.clearance[y, x])
        print(f"cell ({x}, {y}): height {int(made.heights[y, x])}, " + ("not covered" if c == bt._ffi.VIEWSHED_NONE else f"seen from {c} above the ground, by {int(made.count[y, x])} towers"))
    if args.heights:
        np.save(args.heights, made.heights)
    if args.ppm:
        rgb = picture(made)
        bt.write_ppm(args.ppm, rgb)
        print(f"drew {rgb.shape[1]} x {rgb.shape[0]} to {args.ppm}")
    return made


if __name__ == "__main__":
    main()

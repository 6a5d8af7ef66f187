#!/usr/bin/env python3
"""Vegetation placement on the device: the use of terrain data the reference's documents name ("vegetation placement",
docs/development.md; "a vegetation map (for placing trees and bushes)", docs/implementation.md) and leave to the application.

The small synthetic planar terrain of examples/procedural_texture.py: an R16 height preprocessed from fBm noise and an Rgba8 attachment
that no job fills.  TileAtlas.splat_from_height derives a weights splat map into it (byte 0: water and sand, byte 1: grass, byte 2: snow,
byte 3: rock), then TileAtlas.scatter_instances places trees where the grass weight is high and rocks on steep ground whatever the map
says.  The result is a list of instances (world position, world normal, scale, yaw) a renderer would draw; here their counts and a few of
them are printed and, with --ppm, they are drawn over the colour map as dots.

    python examples/vegetation.py [--texture-size 64] [--lods 3] [--seed 7] [--ppm vegetation.ppm]
"""
import argparse
import math
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bevy_terrain_amd as bt  # noqa: E402
from bevy_terrain_amd import (AssetServer, AttachmentConfig, AttachmentFormat, PreprocessDataset, Preprocessor, ScatterRule, SplatRule, TerrainConfig,  # noqa: E402
                              TerrainModel, TileAtlas)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))  # (for a caller that imports this file instead of running it)
import _sources  # noqa: E402

TERRAIN_SIZE = 1000.0
MIN_HEIGHT, MAX_HEIGHT = -40.0, 360.0
BORDER_SIZE = 2
HEIGHT, SPLAT = 0, 1  # attachment indices
INF = math.inf

# the splat map: four weights per texel (bytes r, g, b, a)
SPLAT_RULES = [
    SplatRule(height=(-INF, 125.0), height_fade=10.0),                                                 # r: water and sand
    SplatRule(height=(125.0, 230.0), height_fade=25.0, slope=(0.0, 30.0), slope_fade=0.08),            # g: grass
    SplatRule(height=(250.0, INF), height_fade=25.0, slope=(0.0, 35.0), slope_fade=0.08, weight=2.0),  # b: snow
    SplatRule(height=(115.0, INF), height_fade=5.0, slope=(32.0, 90.0), slope_fade=0.08, weight=1.5),  # a: rock
]
FALLBACK = (0, 0, 0, 255)
TREES, ROCKS = 0, 1
SCATTER_RULES = [
    ScatterRule(density=0.30, mask_channel="g", scale=(0.8, 1.6)),                                # trees: on the grass weight
    ScatterRule(height=(115.0, INF), slope=(32.0, 90.0), slope_fade=0.08, density=0.08, scale=(0.4, 1.2)),  # rocks: steep ground, no mask
]
COLOURS = np.array([(60, 110, 190), (70, 140, 50), (240, 245, 255), (115, 102, 92)], np.float32)  # of the four weights, for --ppm
DOTS = {TREES: (10, 60, 20), ROCKS: (40, 40, 40)}


def run(device, texture_size=64, lod_count=3, seed=7, source_seed=1234):
    """builds the terrain, derives the splat map, scatters the finest level; returns what it made (the tests compare it with the model)"""
    center_size = texture_size - 2 * BORDER_SIZE
    size = center_size << (lod_count - 1)  # the source has the finest mosaic's size
    model = TerrainModel.planar((0.0, 0.0, 0.0), TERRAIN_SIZE, MIN_HEIGHT, MAX_HEIGHT)
    tile_count = (4 ** lod_count - 1) // 3
    config = (TerrainConfig(lod_count=lod_count, atlas_size=tile_count, path="terrains/vegetation", model=model)
              .add_attachment(AttachmentConfig(name="height", texture_size=texture_size, border_size=BORDER_SIZE, format=AttachmentFormat.R16))
              .add_attachment(AttachmentConfig(name="splat", texture_size=texture_size, border_size=BORDER_SIZE, format=AttachmentFormat.Rgba8)))
    tile_atlas = TileAtlas.new(config, device)
    asset_server = AssetServer().insert("height", _sources.height(device, size, source_seed))
    (Preprocessor.new().clear_attachment(HEIGHT, tile_atlas)
     .preprocess_tile(PreprocessDataset(attachment_index=HEIGHT, path="height", lod_range=range(0, lod_count)), asset_server, tile_atlas)
     .run(tile_atlas))
    tile_atlas.splat_from_height(HEIGHT, SPLAT, SPLAT_RULES, mode="weights", fallback=FALLBACK)
    # per tile: a streaming view would pass the tiles it has just loaded, or those an edit changed
    coords = sorted((t for t, _ in tile_atlas.tiles() if t.lod == lod_count - 1), key=lambda t: (t.y, t.x))
    instances, first, stats = tile_atlas.scatter_instances(HEIGHT, SCATTER_RULES, coords, mask_attachment=SPLAT, seed=seed)
    return types.SimpleNamespace(tile_atlas=tile_atlas, coords=coords, instances=instances, first=first, stats=stats, size=size)


def picture(made):
    """the splat map as colours with a dot per instance: (size, size, 4) uint8"""
    weights, _ = made.tile_atlas.read_region(SPLAT, 0, 0, made.size, made.size)
    w = weights.astype(np.float32)
    rgb = (w @ COLOURS) / np.maximum(w.sum(axis=-1, keepdims=True), 1.0)
    image = np.concatenate([rgb.astype(np.uint8), np.full((made.size, made.size, 1), 255, np.uint8)], axis=-1)
    for rule, colour in DOTS.items():
        cells = made.instances["cell"][made.instances["rule"] == rule]
        image[cells[:, 1], cells[:, 0], :3] = colour
    return image


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--texture-size", type=int, default=64)
    ap.add_argument("--lods", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--ppm", default=None, help="draw the instances over the colour map into this file")
    args = ap.parse_args(argv)
    made = run(bt.Device(0), args.texture_size, args.lods, args.seed)
    s = made.stats
    print(f"scattered {len(made.coords)} tiles: {s['cells']} cells, {s['cells_no_data']} without data, {s['total']} instances in {s['launches']} launches")
    print(f"per rule: trees {s['per_rule'][TREES]} rocks {s['per_rule'][ROCKS]}")
    for inst in made.instances[:: max(1, len(made.instances) // 5)][:5]:
        x, y, z = inst["position"]
        print(f"  {'tree' if inst['rule'] == TREES else 'rock'} at ({x:9.3f}, {y:8.3f}, {z:9.3f}) normal ({inst['normal'][0]:+.3f}, {inst['normal'][1]:+.3f}, {inst['normal'][2]:+.3f})"
              f" scale {inst['scale']:.2f} yaw {math.degrees(inst['yaw']):5.1f} deg cell ({inst['cell'][0]}, {inst['cell'][1]})")
    if args.ppm:
        bt.write_ppm(args.ppm, picture(made))
        print(f"drew them over the splat map: {args.ppm}")
    return made


if __name__ == "__main__":
    main()

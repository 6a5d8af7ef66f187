#!/usr/bin/env python3
"""Procedural texturing, the first item of the reference's roadmap (docs/development.md: "splat maps or something similar"), on the device.

A small synthetic planar terrain with two attachments of one texture and border size: an R16 height, preprocessed from fBm noise, and an
Rgba8 albedo that no job ever fills.  TileAtlas.splat_from_height derives the albedo from the heights in place: water, sand, grass and
snow by height, rock wherever the ground is steep, whatever the height; the parents, aprons and mips of the albedo follow as after any
edit.  Then the terrain is ray-cast with that attachment as its colour (TileTree.render) and written as a binary PPM.

    python examples/procedural_texture.py [--texture-size 64] [--lods 3] [--width 640] [--height 360] [--out procedural_texture.ppm]
"""
import argparse
import math
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bevy_terrain_amd as bt  # noqa: E402
from bevy_terrain_amd import (AssetServer, AttachmentConfig, AttachmentFormat, PreprocessDataset, Preprocessor, SplatRule, TerrainConfig,  # noqa: E402
                              TerrainModel, TerrainViewConfig, TileAtlas, TileTree)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))  # (for a caller that imports this file instead of running it)
import _sources  # noqa: E402

TERRAIN_SIZE = 1000.0
MIN_HEIGHT, MAX_HEIGHT = -40.0, 360.0
BORDER_SIZE = 2
HEIGHT, ALBEDO = 0, 1  # attachment indices
INF = math.inf

# heights in world units, slopes in degrees from flat; a texel's colour is the rules' colours weighted by how well it fits each
RULES = [
    SplatRule(height=(-INF, 110.0), height_fade=10.0, colour=(0.10, 0.30, 0.65)),                                                # water
    SplatRule(height=(110.0, 125.0), height_fade=10.0, slope=(0.0, 25.0), slope_fade=0.05, colour=(0.80, 0.74, 0.50)),           # sand
    SplatRule(height=(125.0, 230.0), height_fade=25.0, slope=(0.0, 30.0), slope_fade=0.08, colour=(0.25, 0.55, 0.18)),           # grass
    SplatRule(height=(250.0, INF), height_fade=25.0, slope=(0.0, 35.0), slope_fade=0.08, colour=(0.95, 0.96, 1.00), weight=2.0),  # snow
    SplatRule(height=(115.0, INF), height_fade=5.0, slope=(32.0, 90.0), slope_fade=0.08, colour=(0.45, 0.40, 0.36), weight=1.5),  # rock
]
FALLBACK = (115, 102, 92, 255)  # a texel no rule reaches: bare ground


def run(device, texture_size=64, lod_count=3, width=640, height=360, seed=1234):
    """builds the terrain, derives the texture, renders it; returns what it made (the tests compare it with the definitions)"""
    center_size = texture_size - 2 * BORDER_SIZE
    size = center_size << (lod_count - 1)  # the source has the finest mosaic's size
    model = TerrainModel.planar((0.0, 0.0, 0.0), TERRAIN_SIZE, MIN_HEIGHT, MAX_HEIGHT)
    tile_count = (4 ** lod_count - 1) // 3
    config = (TerrainConfig(lod_count=lod_count, atlas_size=tile_count, path="terrains/procedural", model=model)
              .add_attachment(AttachmentConfig(name="height", texture_size=texture_size, border_size=BORDER_SIZE, format=AttachmentFormat.R16))
              .add_attachment(AttachmentConfig(name="albedo", texture_size=texture_size, border_size=BORDER_SIZE, format=AttachmentFormat.Rgba8)))
    tile_atlas = TileAtlas.new(config, device)
    asset_server = AssetServer().insert("height", _sources.height(device, size, seed))
    (Preprocessor.new().clear_attachment(HEIGHT, tile_atlas)
     .preprocess_tile(PreprocessDataset(attachment_index=HEIGHT, path="height", lod_range=range(0, lod_count)), asset_server, tile_atlas)
     .run(tile_atlas))

    # the texture: one call, queued behind the job, nothing comes back to the host
    changed, stats = tile_atlas.splat_from_height(HEIGHT, ALBEDO, RULES, mode="colour", fallback=FALLBACK)

    # a view from above a corner towards the middle, every tile of the atlas loaded
    tile_tree = TileTree.new(tile_atlas, TerrainViewConfig(tree_size=4, load_distance=1.2, blend_distance=1.0))
    view_position = (-0.55 * TERRAIN_SIZE, MAX_HEIGHT + 0.35 * TERRAIN_SIZE, -0.45 * TERRAIN_SIZE)
    tile_tree.update(view_position)
    tile_tree.adjust_to_tile_atlas()
    camera = bt.RenderCamera.perspective(view_position, (0.55, -0.55, 0.45), (0.0, 1.0, 0.0), math.radians(55.0), width, height, 0.0, 3.0 * TERRAIN_SIZE,
                                         lighting=True, albedo_attachment=ALBEDO, sun=(0.45, 0.8, 0.4), ambient=0.35, background=(120, 170, 230, 255))
    image = tile_tree.render(camera, steps=256, refine_rounds=2, planes=("rgba",), attachment_index=HEIGHT)
    return types.SimpleNamespace(tile_atlas=tile_atlas, tile_tree=tile_tree, view_position=view_position, camera=camera, image=image, changed=changed, stats=stats,
                                 steps=256, refine_rounds=2)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--texture-size", type=int, default=64)
    ap.add_argument("--lods", type=int, default=3)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=360)
    ap.add_argument("--out", default="procedural_texture.ppm")
    args = ap.parse_args(argv)
    made = run(bt.Device(0), args.texture_size, args.lods, args.width, args.height)
    bt.write_ppm(args.out, made.image["rgba"])
    s = made.stats
    print(f"derived the albedo of {s['tiles_edited']} tiles ({s['changed_count']} layers written, {s['launches']} launches) from their heights and slopes")
    print(f"rendered {args.width} x {args.height} to {args.out}: {made.image['stats']}")
    return made


if __name__ == "__main__":
    main()

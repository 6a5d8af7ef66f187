#!/usr/bin/env python3
"""Collision, the last item of the reference's roadmap (docs/development.md) that it does not have, on the device.

A small synthetic planar terrain (the R16 height of examples/procedural_texture.py, preprocessed from fBm noise; examples/minimal.py's
terrain needs preprocessed assets, this one is made here).  A grid of balls is dropped onto it: TileTree.sweep_spheres moves every ball
straight down until it touches (continuous collision: the "move" of move-and-slide).  Then each ball takes a few slide steps: the pull of
gravity with its part along the contact normal taken out (TileTree.collide_spheres gives the normal), swept so that the ground stops it,
and a drop that puts it back on the ground.  The example prints where the balls come to rest.

A ball rests at the free end of its last sweep's bracket, t_above: within (t - t_above) * |direction| of touching, far less than SLACK,
which also covers the contact search (include/bevy_terrain_amd.h: at most about 3 s^2 / (8 r) on a 45 degree slope, s = r (2/7)^3).

    python examples/collision.py [--texture-size 64] [--lods 3] [--grid 6] [--slides 4]
"""
import argparse
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bevy_terrain_amd as bt  # noqa: E402
from bevy_terrain_amd import (AssetServer, AttachmentConfig, AttachmentFormat, PreprocessDataset, Preprocessor, TerrainConfig, TerrainModel,  # noqa: E402
                              TerrainViewConfig, TileAtlas, TileTree, _ffi)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))  # (for a caller that imports this file instead of running it)
import _sources  # noqa: E402

TERRAIN_SIZE = 1000.0
MIN_HEIGHT, MAX_HEIGHT = -40.0, 360.0
BORDER_SIZE = 2
HEIGHT = 0  # attachment index
RADIUS = 5.0
SLACK = RADIUS / 100.0  # every ball ends within this of touching
STRIDE = 8.0  # the length of a slide step on a vertical wall; on flat ground a ball does not slide
STEPS, BISECTIONS, ROUNDS = 128, 20, 2
DOWN = np.array([0.0, -1.0, 0.0])


def move(tile_tree, positions, motion):
    """move-and-stop: every ball goes along its motion until it touches; returns the new positions (the free end of the bracket) and the hits"""
    hits = tile_tree.sweep_spheres(HEIGHT, positions, motion, RADIUS, 0.0, 1.0, steps=STEPS, bisections=BISECTIONS, refine_rounds=ROUNDS)
    t = np.where(hits["status"] == _ffi.RAY_HIT, hits["t_above"], np.where(hits["status"] == _ffi.RAY_MISS, 1.0, 0.0))  # (INSIDE: stay)
    return positions + t[:, None] * motion, hits


def run(device, texture_size=64, lod_count=3, grid=6, slides=4, seed=1234):
    """builds the terrain, drops the balls, slides them; returns what it made"""
    center_size = texture_size - 2 * BORDER_SIZE
    size = center_size << (lod_count - 1)
    model = TerrainModel.planar((0.0, 0.0, 0.0), TERRAIN_SIZE, MIN_HEIGHT, MAX_HEIGHT)
    tile_count = (4 ** lod_count - 1) // 3
    config = (TerrainConfig(lod_count=lod_count, atlas_size=tile_count, path="terrains/collision", model=model)
              .add_attachment(AttachmentConfig(name="height", texture_size=texture_size, border_size=BORDER_SIZE, format=AttachmentFormat.R16)))
    tile_atlas = TileAtlas.new(config, device)
    asset_server = AssetServer().insert("height", _sources.height(device, size, seed))
    (Preprocessor.new().clear_attachment(HEIGHT, tile_atlas)
     .preprocess_tile(PreprocessDataset(attachment_index=HEIGHT, path="height", lod_range=range(0, lod_count)), asset_server, tile_atlas)
     .run(tile_atlas))
    tile_tree = TileTree.new(tile_atlas, TerrainViewConfig(tree_size=4, load_distance=1.2, blend_distance=1.0))
    tile_tree.update((0.0, MAX_HEIGHT + 200.0, 0.0))
    tile_tree.adjust_to_tile_atlas()

    # the balls: a grid over the middle of the terrain, above the highest ground
    span = np.linspace(-0.3 * TERRAIN_SIZE, 0.3 * TERRAIN_SIZE, grid)
    start = np.array([(x, MAX_HEIGHT + 2.0 * RADIUS, z) for z in span for x in span])
    fall = DOWN * (MAX_HEIGHT - MIN_HEIGHT + 4.0 * RADIUS)
    positions, drop = move(tile_tree, start, np.tile(fall, (len(start), 1)))
    landed = positions.copy()
    for _ in range(slides):
        normal = tile_tree.collide_spheres(HEIGHT, positions, RADIUS, refine_rounds=ROUNDS)["normal"]
        slide = STRIDE * (DOWN[None, :] - (normal @ DOWN)[:, None] * normal)  # gravity without its part along the normal
        positions, _ = move(tile_tree, positions, slide)
        positions, _ = move(tile_tree, positions, np.tile(fall, (len(positions), 1)))  # back onto the ground
    contacts = tile_tree.collide_spheres(HEIGHT, positions, RADIUS, refine_rounds=ROUNDS)
    return types.SimpleNamespace(tile_atlas=tile_atlas, tile_tree=tile_tree, start=start, drop=drop, landed=landed, positions=positions, contacts=contacts)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--texture-size", type=int, default=64)
    ap.add_argument("--lods", type=int, default=3)
    ap.add_argument("--grid", type=int, default=6)
    ap.add_argument("--slides", type=int, default=4)
    args = ap.parse_args(argv)
    made = run(bt.Device(0), args.texture_size, args.lods, args.grid, args.slides)
    names = {_ffi.CONTACT_NONE: "none", _ffi.CONTACT_TOUCHING: "touching", _ffi.CONTACT_BELOW: "below", _ffi.CONTACT_INVALID: "invalid", _ffi.CONTACT_FAR: "far"}
    print(f"dropped {len(made.start)} balls of radius {RADIUS:g} and slid each {args.slides} times; slack {SLACK:g}")
    for i, (a, b, p, c) in enumerate(zip(made.start, made.landed, made.positions, made.contacts)):
        print(f"ball {i}: landed at ({b[0]:.3f}, {b[1]:.3f}, {b[2]:.3f}), rests at ({p[0]:.3f}, {p[1]:.3f}, {p[2]:.3f}), slid {np.linalg.norm(p - b):.3f}, "
              f"{names[int(c['status'])]}, depth {c['depth']:.3e}, normal ({c['normal'][0]:.3f}, {c['normal'][1]:.3f}, {c['normal'][2]:.3f})")
    return made


if __name__ == "__main__":
    main()

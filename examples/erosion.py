#!/usr/bin/env python3
"""Hydraulic erosion, the simulation a terrain editor runs over its heights ("sculpting the terrain" of the reference's docs/development.md,
"Real-Time Editing"), on the device.

A small synthetic planar terrain (the R16 height of examples/procedural_texture.py, preprocessed from fBm noise).  TileAtlas.erode_height
lets it rain on a window of the finest mosaic for a number of steps: the water runs downhill, takes ground with it where it is fast and the
slope steep, and leaves it where it slows down.  A round weight plane blends the result in: all of it in the middle of the window, none at
its edge, so the eroded patch joins the ground around it.  The atlas comes back whole: ancestors, aprons and mips follow as after any edit.

    python examples/erosion.py [--texture-size 64] [--lods 3] [--steps 200] [--ppm before_after.ppm]
"""
import argparse
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bevy_terrain_amd as bt  # noqa: E402
from bevy_terrain_amd import (AssetServer, AttachmentConfig, AttachmentFormat, ErosionParams, PreprocessDataset, Preprocessor, TerrainConfig,  # noqa: E402
                              TerrainModel, TileAtlas)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))  # (for a caller that imports this file instead of running it)
import _sources  # noqa: E402

TERRAIN_SIZE = 1000.0
MIN_HEIGHT, MAX_HEIGHT = -40.0, 360.0
BORDER_SIZE = 2
HEIGHT = 0  # attachment index


def round_weight(size):
    """255 inside half the window's radius, falling to 0 at its edge"""
    y, x = np.mgrid[0:size, 0:size]
    r = np.hypot(x - (size - 1) / 2.0, y - (size - 1) / 2.0) / (size / 2.0)
    return np.clip(np.round(255.0 * (1.0 - r) * 2.0), 0, 255).astype(np.uint8)


def run(device, texture_size=64, lod_count=3, steps=200, seed=1234):
    """builds the terrain and erodes a window in the middle of it; returns what it made"""
    center_size = texture_size - 2 * BORDER_SIZE
    size = center_size << (lod_count - 1)  # the finest mosaic, which the source matches
    model = TerrainModel.planar((0.0, 0.0, 0.0), TERRAIN_SIZE, MIN_HEIGHT, MAX_HEIGHT)
    tile_count = (4 ** lod_count - 1) // 3
    config = (TerrainConfig(lod_count=lod_count, atlas_size=tile_count, path="terrains/erosion", model=model)
              .add_attachment(AttachmentConfig(name="height", texture_size=texture_size, border_size=BORDER_SIZE, format=AttachmentFormat.R16)))
    tile_atlas = TileAtlas.new(config, device)
    asset_server = AssetServer().insert("height", _sources.height(device, size, seed))
    (Preprocessor.new().clear_attachment(HEIGHT, tile_atlas)
     .preprocess_tile(PreprocessDataset(attachment_index=HEIGHT, path="height", lod_range=range(0, lod_count)), asset_server, tile_atlas)
     .run(tile_atlas))

    before, _ = tile_atlas.read_region(HEIGHT, 0, 0, size, size)
    window = size - size // 4  # the window: three quarters of the face, in its middle
    origin = (size - window) // 2
    cell = TERRAIN_SIZE / size
    # dt * gravity * depth / cell^2 stays far below 1: the water is centimetres deep and a cell metres wide
    params = ErosionParams(min_height=MIN_HEIGHT, max_height=MAX_HEIGHT, cell_size=cell, dt=0.05 * cell, rain=0.4, evaporation=0.2 / cell, gravity=9.81, capacity=0.02,
                           erode=0.3, deposit=0.3, min_tilt=0.05, min_depth=0.01, steps=steps)
    weight = round_weight(window)
    zeros = np.zeros((window, window), np.float32)
    changed, stats, water, sediment = tile_atlas.erode_height(HEIGHT, origin, origin, window, window, params, weight=weight, water=zeros, sediment=zeros)
    after, _ = tile_atlas.read_region(HEIGHT, 0, 0, size, size)
    return types.SimpleNamespace(tile_atlas=tile_atlas, size=size, window=(origin, origin, window, window), params=params, weight=weight, before=before, after=after,
                                 changed=changed, stats=stats, water=water, sediment=sediment)


def shaded(raw):
    """the heights lit from the north-west, (h, w, 3) uint8"""
    h = raw.astype(np.float32) / 65535.0 * (MAX_HEIGHT - MIN_HEIGHT)
    cell = TERRAIN_SIZE / raw.shape[0]
    gy, gx = np.gradient(h, cell)
    n = np.stack([-gx, -gy, np.ones_like(h)], axis=2)
    n /= np.linalg.norm(n, axis=2, keepdims=True)
    light = np.array([-0.5, -0.5, 0.7]) / np.linalg.norm([-0.5, -0.5, 0.7])
    lit = np.clip(0.25 + 0.75 * (n @ light), 0.0, 1.0)
    tone = 0.55 + 0.45 * (raw.astype(np.float32) / 65535.0)
    grey = np.clip(255.0 * lit * tone, 0, 255).astype(np.uint8)
    return np.stack([grey, grey, grey], axis=2)


def picture(made):
    """before and after side by side, with a white column between them"""
    gap = np.full((made.size, 2, 3), 255, np.uint8)
    return np.concatenate([shaded(made.before), gap, shaded(made.after)], axis=1)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--texture-size", type=int, default=64)
    ap.add_argument("--lods", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--ppm", default=None, help="draw the heights before and after, shaded, side by side")
    args = ap.parse_args(argv)
    made = run(bt.Device(0), args.texture_size, args.lods, args.steps)
    x0, y0, w, h = made.window
    moved = made.before != made.after
    inside = np.zeros_like(moved)
    inside[y0:y0 + h, x0:x0 + w] = True
    s = made.stats
    print(f"eroded a window of {w} x {h} cells at ({x0}, {y0}) of a {made.size} x {made.size} mosaic: {s['steps']} steps, {s['sim_launches']} simulation launches, "
          f"{s['edit']['launches']} launches of the write-back, {len(made.changed)} tiles changed")
    print(f"texels changed: {int(moved.sum())} of {w * h} in the window, {int((moved & ~inside).sum())} outside it; the largest change is "
          f"{float(np.abs(made.after.astype(np.int64) - made.before).max()) / 65535.0 * (MAX_HEIGHT - MIN_HEIGHT):.3f} of {MAX_HEIGHT - MIN_HEIGHT:.0f} height units")
    print(f"water left: {float(made.water.sum(dtype=np.float64)):.6g}, sediment in suspension: {float(made.sediment.sum(dtype=np.float64)):.6g}")
    if args.ppm:
        rgb = picture(made)
        bt.write_ppm(args.ppm, rgb)
        print(f"drew {rgb.shape[1]} x {rgb.shape[0]} to {args.ppm}")
    return made


if __name__ == "__main__":
    main()

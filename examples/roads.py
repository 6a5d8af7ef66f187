#!/usr/bin/env python3
"""Roads and a lake from vector shapes: trees keep off both, and the lake gets a level floor, all of it on the device.

The small synthetic planar terrain of examples/setback.py (an R16 height preprocessed from fBm noise) with an Rgba8 mask attachment beside
it.  A few road polylines with a width and one lake polygon with an island go into byte 0 of the mask with TileAtlas.rasterize_shapes; its
count plane says which cells they cover.  TileAtlas.distance_field takes that byte as its seeds and bakes the distance to the nearest road or
shore into byte 1: 0 on them, 255 from --reach cells on.  TileAtlas.scatter_instances then places trees with that byte as their mask, so
none stands on a road or in the lake, which the example asserts on the instances it gets back.  Last, the lake's floor is levelled with the
same polygon as a SET shape on the heights.

    python examples/roads.py [--texture-size 64] [--lods 3] [--reach 6] [--seed 7] [--ppm roads.ppm]
"""
import argparse
import math
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

MASK = 1                 # the Rgba8 attachment beside the heights
SHAPES, SETBACK = 0, 1   # its bytes: 255 on a road or the lake; the baked distance to them
TREE_RULES = [ScatterRule(density=0.25, mask_channel=SETBACK, scale=(0.8, 1.6))]
ROAD, LAKE, TREE = (70, 70, 70), (90, 170, 255), (10, 60, 20)


def shapes_of(size):
    """the roads (strokes) and the lake (a polygon with an island), in cells of the size x size mosaic; the lake is the last shape"""
    s = float(size)
    circle = lambda cx, cy, r, n: [(cx + r * math.cos(2 * math.pi * k / n), cy + r * math.sin(2 * math.pi * k / n)) for k in range(n)]
    roads = [dict(stroke=[(-2.0, 0.2 * s), (0.4 * s, 0.35 * s), (0.6 * s, 0.3 * s), (s + 2.0, 0.55 * s)], half_width=1.5, value=255),
             dict(stroke=[(0.55 * s, -2.0), (0.5 * s, 0.33 * s), (0.7 * s, 0.75 * s), (0.65 * s, s + 2.0)], half_width=1.0, value=255),
             dict(stroke=circle(0.78 * s, 0.22 * s, 0.09 * s, 16), half_width=0.75, closed=True, value=255)]
    lake = dict(polygon=[circle(0.27 * s, 0.7 * s, 0.14 * s, 24), circle(0.25 * s, 0.72 * s, 0.04 * s, 9)[::-1]], value=255)
    return roads + [lake]


def run(device, texture_size=64, lod_count=3, reach=6, seed=7, source_seed=1234):
    """builds the terrain, rasterises the shapes, bakes the setback, scatters the trees and levels the lake; returns what it made"""
    center_size = texture_size - 2 * BORDER_SIZE
    size = center_size << (lod_count - 1)  # the finest mosaic, which the source matches
    model = TerrainModel.planar((0.0, 0.0, 0.0), TERRAIN_SIZE, MIN_HEIGHT, MAX_HEIGHT)
    tile_count = (4 ** lod_count - 1) // 3
    config = (TerrainConfig(lod_count=lod_count, atlas_size=tile_count, path="terrains/roads", model=model)
              .add_attachment(AttachmentConfig(name="height", texture_size=texture_size, border_size=BORDER_SIZE, format=AttachmentFormat.R16))
              .add_attachment(AttachmentConfig(name="mask", texture_size=texture_size, border_size=BORDER_SIZE, format=AttachmentFormat.Rgba8)))
    tile_atlas = TileAtlas.new(config, device)
    asset_server = AssetServer().insert("height", _sources.height(device, size, source_seed))
    (Preprocessor.new().clear_attachment(HEIGHT, tile_atlas).clear_attachment(MASK, tile_atlas)
     .preprocess_tile(PreprocessDataset(attachment_index=HEIGHT, path="height", lod_range=range(0, lod_count)), asset_server, tile_atlas)
     .run(tile_atlas))

    shapes = shapes_of(size)
    count, last, stats = tile_atlas.rasterize_shapes(MASK, 0, 0, size, size, shapes, channel=SHAPES)
    covered, lake = count > 0, last == len(shapes) - 1
    _, _, distance_stats = tile_atlas.distance_field(MASK, 0, 0, size, size, lo=255, hi=255, channel=SHAPES, bake=dict(attachment=MASK, channel=SETBACK, reach=reach))
    mask, _ = tile_atlas.read_region(MASK, 0, 0, size, size)
    coords = sorted((t for t, _ in tile_atlas.tiles() if t.lod == lod_count - 1), key=lambda t: (t.y, t.x))
    instances, _, scatter_stats = tile_atlas.scatter_instances(HEIGHT, TREE_RULES, coords, mask_attachment=MASK, seed=seed)
    trees = instances["cell"]
    assert not covered[trees[:, 1], trees[:, 0]].any(), "a tree stands on a road or in the lake"
    # the lake's floor: its lowest texel, everywhere in it
    before, _ = tile_atlas.read_region(HEIGHT, 0, 0, size, size)
    level = max(int(before[lake].min()), 1)
    _, _, level_stats = tile_atlas.rasterize_shapes(HEIGHT, 0, 0, size, size, [dict(shapes[-1], value=level)], count=False, last=False)
    heights, _ = tile_atlas.read_region(HEIGHT, 0, 0, size, size)
    assert (heights[lake] == level).all() and np.array_equal(heights[~lake], before[~lake])
    return types.SimpleNamespace(tile_atlas=tile_atlas, size=size, reach=reach, shapes=shapes, count=count, last=last, covered=covered, lake=lake, stats=stats,
                                 distance_stats=distance_stats, mask=mask, trees=trees, scatter_stats=scatter_stats, level=level, level_stats=level_stats, heights=heights)


def picture(made):
    """the heights shaded, darker towards the roads and the shore, the roads, the lake and a dot per tree"""
    rgb = shaded(made.heights)
    byte = made.mask[:, :, SETBACK]
    rgb = (rgb.astype(np.uint16) * (96 + byte.astype(np.uint16) * 159 // 255)[:, :, None] // 255).astype(np.uint8)
    rgb[made.covered & ~made.lake] = ROAD
    rgb[made.lake] = LAKE
    rgb[made.trees[:, 1], made.trees[:, 0]] = TREE
    return rgb


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--texture-size", type=int, default=64)
    ap.add_argument("--lods", type=int, default=3)
    ap.add_argument("--reach", type=int, default=6, help="the distance from a road or the shore, in cells, from which trees stand at their full density")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--ppm", default=None, help="draw the roads, the lake, the distance shading and the trees")
    ap.add_argument("--save", default=None, help="save the packed shapes, the planes, the mask, the heights and the trees' cells (.npz)")
    args = ap.parse_args(argv)
    made = run(bt.Device(0), args.texture_size, args.lods, args.reach, args.seed)
    s = made.stats
    print(f"shapes into a {made.size} x {made.size} mosaic: {s['shapes']} shapes, {s['shapes_culled']} culled, {s['covered']} cells covered, {s['written']} texels written, "
          f"{s['launches']} launches and {s['edit']['launches']} of the write over {s['edit']['tiles_edited']} tiles")
    print(f"lake: {int(made.lake.sum())} cells levelled to {made.level}, {made.level_stats['written']} texels written")
    on_shape = int(made.covered[made.trees[:, 1], made.trees[:, 0]].sum())
    within = int((made.mask[:, :, SETBACK][made.trees[:, 1], made.trees[:, 0]] < 255).sum())
    print(f"trees: {len(made.trees)}, on a road or in the lake: {on_shape}, within {made.reach} cells of one: {within}")
    if args.save:
        vertices, entries = TileAtlas.pack_shapes(made.shapes)
        np.savez(args.save, vertices=vertices, entries=entries, count=made.count, last=made.last, mask=made.mask, heights=made.heights, trees=made.trees, lake=made.lake)
    if args.ppm:
        rgb = picture(made)
        bt.write_ppm(args.ppm, rgb)
        print(f"drew {rgb.shape[1]} x {rgb.shape[0]} to {args.ppm}")
    return made


if __name__ == "__main__":
    main()

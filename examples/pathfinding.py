#!/usr/bin/env python3
"""Path-finding, an item of the reference's roadmap (docs/development.md) that it does not have, on the device.

A small synthetic planar terrain (the R16 height of examples/procedural_texture.py, preprocessed from fBm noise).  TileAtlas.path_field
computes, for one goal, the cost of walking to it from every texel of the finest mosaic: steps cost their length, more on a grade, more
again uphill, and not at all beyond a maximum grade; `next` holds the step to take from every texel.  trace_path follows it from three
starts, and the example prints each route's length and cost, the cost once as the field gives it and once added up along the route.

    python examples/pathfinding.py [--texture-size 64] [--lods 3] [--ppm routes.ppm]
"""
import argparse
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bevy_terrain_amd as bt  # noqa: E402
from bevy_terrain_amd import (AssetServer, AttachmentConfig, AttachmentFormat, PathCost, PreprocessDataset, Preprocessor, TerrainConfig,  # noqa: E402
                              TerrainModel, TileAtlas, trace_path)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))  # (for a caller that imports this file instead of running it)
import _sources  # noqa: E402

TERRAIN_SIZE = 1000.0
MIN_HEIGHT, MAX_HEIGHT = -40.0, 360.0
BORDER_SIZE = 2
HEIGHT = 0  # attachment index
F = np.float32


def route_cost(raw, cost, cells):
    """the cost of a route added up from its goal back to its start, every step's weight by the definition, in binary32"""
    h = F(cost.min_height) + (F(cost.max_height) - F(cost.min_height)) * (raw.astype(F) / F(65535.0))
    cell = F(cost.cell_size)
    diag = cell * F(1.41421356)
    total, length = F(0.0), 0.0
    for (ax, ay), (bx, by) in reversed(list(zip(cells[:-1], cells[1:]))):
        run = diag if ax != bx and ay != by else cell
        rise = h[by, bx] - h[ay, ax]
        g = np.abs(rise) / run
        up, down = (rise, F(0.0)) if rise > 0 else (F(0.0), -rise)
        total = total + (((run * (F(1.0) + F(cost.grade_weight) * g)) + F(cost.climb_weight) * up) + F(cost.descend_weight) * down)
        length += float(run)
    return total, length


def run(device, texture_size=64, lod_count=3, seed=1234):
    """builds the terrain, computes the field of one goal, traces three routes; returns what it made"""
    center_size = texture_size - 2 * BORDER_SIZE
    size = center_size << (lod_count - 1)  # the finest mosaic, which the source matches
    model = TerrainModel.planar((0.0, 0.0, 0.0), TERRAIN_SIZE, MIN_HEIGHT, MAX_HEIGHT)
    tile_count = (4 ** lod_count - 1) // 3
    config = (TerrainConfig(lod_count=lod_count, atlas_size=tile_count, path="terrains/pathfinding", model=model)
              .add_attachment(AttachmentConfig(name="height", texture_size=texture_size, border_size=BORDER_SIZE, format=AttachmentFormat.R16)))
    tile_atlas = TileAtlas.new(config, device)
    asset_server = AssetServer().insert("height", _sources.height(device, size, seed))
    (Preprocessor.new().clear_attachment(HEIGHT, tile_atlas)
     .preprocess_tile(PreprocessDataset(attachment_index=HEIGHT, path="height", lod_range=range(0, lod_count)), asset_server, tile_atlas)
     .run(tile_atlas))

    # walking: a step costs its length, twice that per unit of grade on top, three times the metres climbed; nothing steeper than 100 %
    cost = PathCost(min_height=MIN_HEIGHT, max_height=MAX_HEIGHT, cell_size=TERRAIN_SIZE / size, max_grade=1.0, grade_weight=2.0, climb_weight=3.0, descend_weight=0.5)
    goal = (size // 2, size // 2)
    field, next_plane, stats = tile_atlas.path_field(HEIGHT, 0, 0, size, size, cost, [goal])
    raw, _ = tile_atlas.read_region(HEIGHT, 0, 0, size, size)
    starts = [(size // 16, size // 16), (size - 1 - size // 16, size // 8), (size // 5, size - 1 - size // 16)]
    routes = []
    for start in starts:
        cells, status = trace_path(next_plane, start)
        cells = [(int(x), int(y)) for x, y in cells]
        added, length = route_cost(raw, cost, cells) if status == "ok" else (F(np.inf), 0.0)
        routes.append(types.SimpleNamespace(start=start, cells=cells, status=status, cost=field[start[1], start[0]], added=added, length=length))
    return types.SimpleNamespace(tile_atlas=tile_atlas, size=size, cost=cost, goal=goal, field=field, next=next_plane, stats=stats, raw=raw, routes=routes)


def picture(made):
    """the heights in grey, cells no route can leave in dark red, the routes in colours, the goal in white"""
    grey = (made.raw >> 8).astype(np.uint8)
    rgb = np.stack([grey, grey, grey], axis=2)
    rgb[np.isinf(made.field)] = (70, 20, 20)
    for route, colour in zip(made.routes, ((255, 80, 60), (70, 220, 90), (80, 140, 255))):
        for x, y in route.cells:
            rgb[y, x] = colour
    gx, gy = made.goal
    rgb[max(gy - 1, 0):gy + 2, max(gx - 1, 0):gx + 2] = (255, 255, 255)
    return rgb


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--texture-size", type=int, default=64)
    ap.add_argument("--lods", type=int, default=3)
    ap.add_argument("--ppm", default=None, help="draw the routes over a grey picture of the heights")
    args = ap.parse_args(argv)
    made = run(bt.Device(0), args.texture_size, args.lods)
    s = made.stats
    print(f"field of {made.size} x {made.size} cells towards goal {made.goal}: {s['reachable']} reachable, {s['blocked']} blocked, {s['sweeps']} sweeps, {s['launches']} launches")
    for r in made.routes:
        end = r.cells[-1]
        print(f"route from {r.start}: {r.status}, {len(r.cells)} cells, {r.length:.1f} long, ends at {end}, cost {float(r.cost):.9g}, added up along the route {float(r.added):.9g}")
    if args.ppm:
        bt.write_ppm(args.ppm, picture(made))
        print(f"drew {made.size} x {made.size} to {args.ppm}")
    return made


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Lakes: the pieces of a mask, listed, measured and cleaned on the device.

A small synthetic planar terrain (the R16 height of examples/erosion.py, preprocessed from fBm noise) with an Rgba8 mask layer beside it.
TileAtlas.drainage fills every depression to the level at which it spills; the cells with level > height are water.  That mask goes to
TileAtlas.label_regions as a host plane: every lake comes back as one region with its area, its bounding box and the sum of its heights,
so the five largest can be printed with their mean height, and each lake drawn in a colour of its own.  The same mask is kept as byte 0 of
the mask layer (255 = water); a second call with a bake sets that byte back to 0 on every lake of fewer than --min-area cells, on the device:
the puddles are gone from the layer and no lake of --min-area cells or more has lost a cell.

    python examples/lakes.py [--texture-size 64] [--lods 3] [--min-area 12] [--ppm lakes.ppm]
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

MASK = 1  # attachment index: Rgba8, byte 0 = 255 on water
NONE = 0xFFFFFFFF


def run(device, texture_size=64, lod_count=3, min_area=12, seed=1234):
    """builds the terrain, labels its lakes and removes the puddles from the mask layer; returns what it made"""
    center_size = texture_size - 2 * BORDER_SIZE
    size = center_size << (lod_count - 1)  # the finest mosaic, which the source matches
    model = TerrainModel.planar((0.0, 0.0, 0.0), TERRAIN_SIZE, MIN_HEIGHT, MAX_HEIGHT)
    tile_count = (4 ** lod_count - 1) // 3
    config = (TerrainConfig(lod_count=lod_count, atlas_size=tile_count, path="terrains/lakes", model=model)
              .add_attachment(AttachmentConfig(name="height", texture_size=texture_size, border_size=BORDER_SIZE, format=AttachmentFormat.R16))
              .add_attachment(AttachmentConfig(name="mask", texture_size=texture_size, border_size=BORDER_SIZE, format=AttachmentFormat.Rgba8)))
    tile_atlas = TileAtlas.new(config, device)
    asset_server = AssetServer().insert("height", _sources.height(device, size, seed))
    (Preprocessor.new().clear_attachment(HEIGHT, tile_atlas).clear_attachment(MASK, tile_atlas)
     .preprocess_tile(PreprocessDataset(attachment_index=HEIGHT, path="height", lod_range=range(0, lod_count)), asset_server, tile_atlas)
     .run(tile_atlas))

    heights, _ = tile_atlas.read_region(HEIGHT, 0, 0, size, size)
    level = tile_atlas.drainage(HEIGHT, 0, 0, size, size, want_flat=False, want_direction=False, want_accumulation=False)[0]
    water = level > heights
    mask = np.zeros((size, size, 4), np.uint8)
    mask[:, :, 0] = water * 255
    tile_atlas.write_region(MASK, mask, 0, 0)

    # the lakes: v is the height, so v_sum / area is a lake's mean bed height
    label, ids, lakes, stats = tile_atlas.label_regions(HEIGHT, 0, 0, size, size, members=water)
    # the puddles leave the mask layer: one call, the bake on the device
    *_, bake_stats, changed = tile_atlas.label_regions(HEIGHT, 0, 0, size, size, members=water, label=False, id=False, region_cap=0,
                                                       bake=dict(attachment=MASK, channel=0, min_area=0, max_area=max(min_area, 1) - 1, value=0))
    after, _ = tile_atlas.read_region(MASK, 0, 0, size, size)
    removed = water & (after[:, :, 0] == 0)
    area = np.zeros(size * size + 1, np.int64)
    area[lakes["label"]] = lakes["area"]
    cell_area = area[np.where(label == NONE, size * size, label)]
    assert not (cell_area[removed] >= min_area).any(), "a baked-away cell belongs to a lake of min_area cells or more"
    assert np.array_equal(after[:, :, 0] == 255, water & (cell_area >= min_area)) and not after[:, :, 1:].any()
    return types.SimpleNamespace(tile_atlas=tile_atlas, size=size, min_area=min_area, heights=heights, level=level, water=water, label=label, ids=ids, lakes=lakes,
                                 stats=stats, bake_stats=bake_stats, changed=changed, removed=removed, mask_after=after[:, :, 0])


def picture(made):
    """the shaded heights with every lake in a colour of its own (by its id), the removed puddles in magenta"""
    rgb = shaded(made.heights)
    on = made.ids != NONE
    k = made.ids[on].astype(np.int64)
    rgb[on] = np.stack([40 + (k * 97) % 160, 60 + (k * 57) % 160, 200 + (k * 31) % 56], axis=1).astype(np.uint8)
    rgb[made.removed] = (255, 0, 255)
    return rgb


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--texture-size", type=int, default=64)
    ap.add_argument("--lods", type=int, default=3)
    ap.add_argument("--min-area", type=int, default=12, help="lakes of fewer cells are puddles: removed from the mask layer")
    ap.add_argument("--ppm", default=None, help="draw every lake in its own colour over the shaded heights")
    args = ap.parse_args(argv)
    made = run(bt.Device(0), args.texture_size, args.lods, args.min_area)
    s, b = made.stats, made.bake_stats
    print(f"lakes of a {made.size} x {made.size} mosaic: {s['regions']} lakes of {s['members']} water cells in {s['launches']} launches; "
          f"the largest has {s['largest_area']} cells and starts at cell {s['largest_label']}")
    for r in made.lakes[np.argsort(-made.lakes["area"].astype(np.int64), kind="stable")[:5]]:
        print(f"  lake {int(made.ids.ravel()[r['label']])}: {int(r['area'])} cells, x {int(r['x_min'])}..{int(r['x_max'])}, y {int(r['y_min'])}..{int(r['y_max'])}, "
              f"mean height {int(r['v_sum']) / int(r['area']):.1f} raw units ({int(r['v_min'])}..{int(r['v_max'])}), shore {int(r['edges'])} edges")
    puddles = int((made.lakes["area"] < made.min_area).sum())
    print(f"puddles below {made.min_area} cells: {puddles} lakes, {b['baked']} cells removed from the mask layer in {b['launches']} launches and "
          f"{b['edit']['launches']} of the edit, {len(made.changed)} tiles changed; {int((made.mask_after == 255).sum())} water cells stay")
    if args.ppm:
        rgb = picture(made)
        bt.write_ppm(args.ppm, rgb)
        print(f"drew {rgb.shape[1]} x {rgb.shape[0]} to {args.ppm}")
    return made


if __name__ == "__main__":
    main()

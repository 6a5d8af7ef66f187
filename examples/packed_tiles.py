#!/usr/bin/env python3
"""Packed tile files: a small planar terrain saved raw (`.bin`) and packed (`.btp`), and loaded back.

The terrain is preprocessed as examples/preprocess_planar.py does it (fBm heights and a colour ramp of them, synthesised), every tile of
both attachments is written twice into the same directories, the two sizes are printed per LOD, and the packed files are decoded on the
device into a fresh atlas that must equal, in every layer and every mip level, a twin loaded from the raw files.

    python examples/packed_tiles.py [--assets DIR] [--size 1024] [--texture-size 256] [--lods 3]
"""
import argparse
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bevy_terrain_amd as bt  # noqa: E402
from bevy_terrain_amd import AssetServer, AttachmentConfig, AttachmentFormat, PreprocessDataset, Preprocessor, TerrainConfig, TerrainModel, TileAtlas  # noqa: E402

import _sources  # noqa: E402

PATH = "terrains/packed"
MIPS = 3


def config(args):
    return (TerrainConfig(lod_count=args.lods, atlas_size=(4 ** args.lods - 1) // 3, path=PATH, model=TerrainModel.planar((0.0, 0.0, 0.0), 1000.0, 0.0, 250.0))
            .add_attachment(AttachmentConfig(name="height", texture_size=args.texture_size, border_size=2, format=AttachmentFormat.R16, mip_level_count=MIPS))
            .add_attachment(AttachmentConfig(name="albedo", texture_size=args.texture_size, border_size=2, format=AttachmentFormat.Rgba8, mip_level_count=MIPS)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--assets", default=None, help="where the tiles go (default: a temporary directory)")
    ap.add_argument("--size", type=int, default=1024, help="side of the synthesised sources")
    ap.add_argument("--texture-size", type=int, default=256)
    ap.add_argument("--lods", type=int, default=3)
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as scratch:
        run(args, args.assets or scratch)


def run(args, assets):
    device = bt.Device(0)
    height = _sources.height(device, args.size, 1234)
    server = AssetServer().insert("height", height).insert("albedo", _sources.albedo_of(height))
    atlas = TileAtlas.new(config(args), device)
    pre = Preprocessor.new()
    for ai, name in enumerate(("height", "albedo")):
        pre.clear_attachment(ai, atlas).preprocess_tile(PreprocessDataset(attachment_index=ai, path=name, lod_range=range(0, args.lods)), server, atlas)
    pre.run(atlas)
    atlas.save_tile_config(assets)
    tiles = atlas.tiles()
    for ai, a in enumerate(atlas.config.attachments):
        directory = atlas.attachment_directory(assets, ai)
        atlas.save_attachment(ai, directory)
        atlas.save_tiles_packed(ai, directory)
        print(f"{a.name} ({a.format.name}, {len(tiles)} tiles of {a.texture_size} x {a.texture_size}) in {directory}")
        total = [0, 0]
        for lod in range(args.lods):
            raw = sum(os.path.getsize(os.path.join(directory, f"{c}.bin")) for c, _ in tiles if c.lod == lod)
            packed = sum(os.path.getsize(os.path.join(directory, f"{c}.btp")) for c, _ in tiles if c.lod == lod)
            total = [total[0] + raw, total[1] + packed]
            print(f"  lod {lod}: raw {raw:10d} bytes, packed {packed:10d} bytes, ratio {raw / packed:.3f}")
        print(f"  all  : raw {total[0]:10d} bytes, packed {total[1]:10d} bytes, ratio {total[0] / total[1]:.3f}")

    from_raw, from_packed = TileAtlas.new(config(args), device), TileAtlas.new(config(args), device)
    compared = 0
    from_raw.load_tile_config(assets)
    from_packed.load_tile_config(assets)
    for ai in range(2):
        from_raw.load_tiles(ai, assets)
        from_packed.load_tiles_packed(ai, from_packed.attachment_directory(assets, ai))
        for c, layer in tiles:
            for mip in range(MIPS):
                a, b = from_raw.download_mip(ai, mip, from_raw.get_tile(c)[1]), from_packed.download_mip(ai, mip, from_packed.get_tile(c)[1])
                assert np.array_equal(a, b), (ai, c, mip)
                if mip == 0:
                    assert np.array_equal(a, atlas.download_tile(ai, layer)), (ai, c)
                compared += 1
    print(f"loaded the packed files into a fresh atlas: {compared} layers and mip levels equal to the twin loaded from the raw files")


if __name__ == "__main__":
    main()

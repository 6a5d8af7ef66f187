"""The context's pinned staging ring with MORE chunks than buffers, and content that shows a misplaced chunk.

Every chunked transfer between host memory and the device goes through three pinned buffers.  The region paths (bt_atlas_write_region,
bt_atlas_read_region) reuse a buffer only when a call has more than three chunks, which takes more than 96 MiB once the buffers are 32 MiB;
the tile file paths (bt_atlas_save_tiles, bt_atlas_load_tiles) only above 3 x 64 tiles in one call.  The buffers grow only when they are smaller
than one row, so the region test first makes them two rows small (trim, then a two-row write) and keeps every later call many-chunked.

Tiles are 4 x 4 texels with a one-texel border (centre 2 x 2): the smallest texture the edit paths accept with a border (the centre must be
even), so the model's per-texel stitch stays cheap and 85 tiles cost nothing."""
import os

import numpy as np
import pytest

import _edit_model as EM
import bevy_terrain_amd as bt
from test_gpu_edit import Snapshot, check_edit

T, B, CENTRE = 4, 1, 2
LODS, FINEST = 4, 3           # the finest LOD is a mosaic of 16 x 16 centre texels
X0, Y0, W = 3, 1, 9           # odd origin, odd width: mosaic columns 3 .. 11 lie in tiles 1 .. 5
HEIGHTS = (2, 7, 13)          # the sizing call, then 2 + 2 + 2 + 1 rows, then 7 chunks: every buffer is used at least twice
FORMATS = {"r16": (bt.AttachmentFormat.R16, np.uint16, ()), "rgba8": (bt.AttachmentFormat.Rgba8, np.uint8, (4,))}


@pytest.fixture(scope="module")
def device():
    return bt.Device(0)


def chunks(rows, rows_per_buffer):
    """the rows of each chunk of a region call: chunk_rows = min(height, bytes per buffer / bytes per row), whole rows, a short last chunk"""
    per = min(rows, rows_per_buffer)
    return [min(per, rows - r) for r in range(0, rows, per)]


def start_state(fmt):
    """every tile of LODs 0 .. 3 of a planar terrain: random finest centres (no zeros), everything else derived by the model (the invariant F)"""
    _, dtype, tail = FORMATS[fmt]
    rng = np.random.default_rng(11)
    tiles = {(0, lod, x, y): np.zeros((T, T) + tail, dtype) for lod in range(LODS) for y in range(1 << lod) for x in range(1 << lod)}
    for k in tiles:
        if k[1] == FINEST:
            tiles[k][B:-B, B:-B] = rng.integers(1, np.iinfo(dtype).max + 1, size=(CENTRE, CENTRE) + tail, dtype=dtype)
    return EM.propagate(tiles, B, False)


def region_texels(fmt, height):
    """every texel distinct and none zero, in an order that differs from call to call: a chunk in the wrong rows cannot go unnoticed"""
    _, dtype, tail = FORMATS[fmt]
    ids = np.random.default_rng(height).permutation(np.arange(1, W * height + 1)) * 251 + 7 * height  # < 2^16, distinct
    if not tail:
        return ids.reshape(height, W).astype(dtype)
    out = np.stack([ids & 255, ids >> 8, np.full_like(ids, 1 + height), np.full_like(ids, 200)], axis=-1)
    return out.reshape(height, W, 4).astype(dtype)


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_region_cases_on_the_model(fmt):
    """no GPU: the rectangles and values are what the test below takes them for"""
    assert chunks(2, 2) == [2] and chunks(7, 2) == [2, 2, 2, 1] and chunks(13, 2) == [2] * 6 + [1]
    tiles = start_state(fmt)
    assert len(tiles) == 85 and all(np.array_equal(v, tiles[k]) for k, v in EM.propagate(tiles, B, False).items())
    for height in HEIGHTS:
        texels = region_texels(fmt, height)
        flat = texels.reshape(W * height, -1)
        assert len(np.unique(flat, axis=0)) == W * height and flat.any(axis=1).all()
        edited = EM.region_tiles(FINEST, 0, X0, Y0, W, height, CENTRE)
        assert len({k[2] for k in edited}) == 5 and len({k[3] for k in edited}) == (Y0 + height - 1) // CENTRE + 1 and edited <= set(tiles)
        written = EM.write_region(tiles, FINEST, 0, X0, Y0, texels, B)
        mosaic = np.concatenate([np.concatenate([written[(0, FINEST, x, y)][B:-B, B:-B] for x in range(8)], axis=1) for y in range(8)], axis=0)
        assert np.array_equal(mosaic[Y0:Y0 + height, X0:X0 + W], texels)
        tiles = EM.propagate(written, B, False)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_region_rows_through_a_small_ring(device, fmt):
    """write_region and read_region of 7 and of 13 rows through buffers of two rows: 4 chunks (buffer 0 twice, a short last chunk) and 7
    chunks (every buffer at least twice).  What is read back is what was written, and every layer is the model's"""
    cfg = bt.TerrainConfig(lod_count=LODS, atlas_size=96, path="terrains/ring", model=bt.TerrainModel.planar((0, 0, 0), 1000.0, 0.0, 1.0))
    cfg.add_attachment(bt.AttachmentConfig(name="att", texture_size=T, border_size=B, format=FORMATS[fmt][0]))
    atlas = bt.TileAtlas.new(cfg, device)
    for k, tile in start_state(fmt).items():
        atlas.upload_tile(0, atlas.get_or_allocate_tile(bt.TileCoordinate(*k))[1], tile)
    device.trim()  # no buffers: the first region call sizes them, for its two rows
    for height in HEIGHTS:
        texels = region_texels(fmt, height)
        before = Snapshot(atlas)
        changed, stats = atlas.write_region(0, texels, X0, Y0)
        expected = EM.propagate(EM.write_region(before.tiles, FINEST, 0, X0, Y0, texels, B), B, False)
        check_edit(atlas, before, expected, changed, stats, EM.region_tiles(FINEST, 0, X0, Y0, W, height, CENTRE), FINEST)
        got, missing = atlas.read_region(0, X0, Y0, W, height)
        assert missing == 0 and np.array_equal(got, texels)
    # three buffers of two rows, the region scratch and the 2 MiB plan ring: buffers of 32 MiB (one chunk per call) would give back 96 MiB
    assert device.trim() < 8 << 20


@pytest.mark.gpu
def test_two_hundred_tile_files_in_one_call(device, tmp_path):
    """save_tiles and load_tiles of 200 tiles in one call: chunks of 64, 64, 64 and 8, so the fourth lands in the first buffer.  Each
    tile holds its coordinate; the two atlases keep the tiles in different layers"""
    cfg = bt.TerrainConfig(lod_count=5, atlas_size=256, path="terrains/ring", model=bt.TerrainModel.planar((0, 0, 0), 1000.0, 0.0, 1.0))
    cfg.add_attachment(bt.AttachmentConfig(name="att", texture_size=T, border_size=B, format=bt.AttachmentFormat.R16))
    coords = [bt.TileCoordinate(0, 4, i % 16, i // 16) for i in range(200)]

    def content(c):
        return (1 + c.x + 16 * c.y + 256 * np.arange(T * T)).astype(np.uint16).reshape(T, T)

    atlas = bt.TileAtlas.new(cfg, device)
    order = np.random.default_rng(4).permutation(200)
    for i in order:  # layers in a shuffled order: the saver sorts by layer, not by the caller's list
        atlas.upload_tile(0, atlas.get_or_allocate_tile(coords[i])[1], content(coords[i]))
    directory = atlas.attachment_directory(str(tmp_path), 0)
    atlas.save_tiles(0, directory, coords)
    assert sorted(os.listdir(directory)) == sorted(f"{c}.bin" for c in coords)
    for c in coords:
        assert open(os.path.join(directory, f"{c}.bin"), "rb").read() == content(c).tobytes(), c
    other = bt.TileAtlas.new(cfg, device)
    other.load_tiles(0, str(tmp_path), coords[::-1])
    index = {(c.x, c.y): i for c, i in other.tiles()}
    assert len(index) == 200 and index != {(c.x, c.y): i for c, i in atlas.tiles()}
    data = other.download_tiles(0, 0, other.atlas_size)
    for c in coords:
        assert np.array_equal(data[index[(c.x, c.y)]], content(c)), c

"""bt_atlas_tile_bounds on the device against the second model (tests/_bounds_model.py) applied to download_tiles of the same layers, every
level compared: known answers, crafted extremes on and next to the cells' shared rows and columns, noise at several tile sizes (both kernel
paths), preprocessed tiles with no data, layer lists, stream ordering, reads that must not count as writes, the load path and the errors."""
import ctypes as C
import os

import numpy as np
import pytest

import _bounds_model as BM
import bevy_terrain_amd as bt
from bevy_terrain_amd import _ffi

GRIDS = (1, 2, 4, 8, 16, 32, 64)
BT_ERR_INVALID_ARGUMENT, BT_ERR_UNSUPPORTED = -1, -5
EXAMPLE = np.array([[10, 20, 30, 40], [50, 60, 70, 80], [90, 15, 25, 35], [45, 55, 65, 0]], dtype=np.uint16)


@pytest.fixture(scope="module")
def device():
    return bt.Device(0)


def make_atlas(device, T, layers, fmt=bt.AttachmentFormat.R16, lod_count=4, border=2):
    cfg = bt.TerrainConfig(lod_count=lod_count, atlas_size=layers, path="terrains/bounds", model=bt.TerrainModel.planar((0, 0, 0), 1000.0, 0.0, 1.0))
    cfg.add_attachment(bt.AttachmentConfig(name="height", texture_size=T, border_size=min(border, (T - 1) // 2), format=fmt))
    return bt.TileAtlas.new(cfg, device)


def layer_data(atlas, layers):
    data = atlas.download_tiles(0, 0, max(layers) + 1)
    return data[np.asarray(layers, dtype=np.int64)]


def assert_bounds(atlas, layers, grid, skip_zero=False, data=None):
    """the device's pyramid of `layers` == the second model's of the downloaded layers, level by level"""
    got = atlas.tile_bounds(0, layers, grid, skip_zero)
    exp = BM.tile_bounds(layer_data(atlas, layers) if data is None else data, grid, skip_zero)
    assert len(got) == len(exp) == grid.bit_length()
    for k, (g, e) in enumerate(zip(got, exp)):
        assert g.shape == e.shape, (k, g.shape, e.shape)
        if not np.array_equal(g, e):
            i = tuple(np.argwhere(g != e)[0][:3])
            pytest.fail(f"grid {grid} skip_zero {skip_zero} level {k}: {int((g != e).any(axis=-1).sum())} cells differ, first (layer slot, cy, cx) "
                        f"{i}: got {g[i].tolist()}, want {e[i].tolist()}")
    return got


@pytest.mark.gpu
def test_known_answer_layer(device):
    """the hand-worked T = 4 layer of the header's contract, uploaded into layer 1 of a fresh atlas"""
    atlas = make_atlas(device, 4, 3)
    atlas.upload_tile(0, 1, EXAMPLE)
    level0, level1 = atlas.tile_bounds(0, [1], 2)
    assert level0[0].tolist() == [[[10, 90], [25, 80]], [[15, 90], [0, 65]]] and level1[0].tolist() == [[[0, 90]]]
    level0, level1 = atlas.tile_bounds(0, [1], 2, skip_zero=True)
    assert level0[0].tolist() == [[[10, 90], [25, 80]], [[15, 90], [25, 65]]] and level1[0].tolist() == [[[10, 90]]]
    for grid in (1, 2, 4):
        for skip_zero in (False, True):
            assert_bounds(atlas, [1, 0, 2], grid, skip_zero)


def crafted_layers(T=512):
    """extremes 1 and 0xFFFF on a base of mid values: on the shared rows and columns 64 / 128 / 256, one row or column before them, in the
    last row and column (the clamped edge), in the corners and inside a block next to a boundary; and a layer whose every 8th row holds
    small values and every 8th column large ones, so that each cell's minimum and maximum sit on its own or its inclusive row / column"""
    rng = np.random.default_rng(11)
    places = [((64, 100), (200, 128)), ((128, 128), (256, 256)), ((256, 33), (40, 64)), ((63, 300), (300, 255)), ((127, 127), (255, 200)),
              ((T - 1, 77), (400, T - 1)), ((0, 0), (T - 1, T - 1)), ((0, T - 1), (T - 1, 0)), ((65, 65), (127, 190)), ((191, 129), (129, 383))]
    layers = []
    for lo, hi in places:
        layer = rng.integers(20000, 40000, size=(T, T), dtype=np.uint16)
        layer[lo], layer[hi] = 1, 0xFFFF
        layers.append(layer)
    layer = rng.integers(20000, 40000, size=(T, T), dtype=np.uint16)
    layer[::8, :] = rng.integers(1, 1000, size=(T // 8, T), dtype=np.uint16)
    layer[:, ::8] = rng.integers(60000, 65536, size=(T, T // 8), dtype=np.uint16)
    layers.append(layer)
    zeros = layer.copy()
    zeros[::16, :] = 0  # under skip-zero the inclusive row is all no-data for the 16-row cells
    layers.append(zeros)
    return np.stack(layers)


@pytest.mark.gpu
def test_crafted_extremes_on_shared_rows_and_columns(device):
    layers = crafted_layers()
    atlas = make_atlas(device, 512, len(layers) + 2)
    for i, layer in enumerate(layers):
        atlas.upload_tile(0, i + 1, layer)
    idx = list(range(1, len(layers) + 1))
    for grid in GRIDS:
        for skip_zero in (False, True):
            assert_bounds(atlas, idx, grid, skip_zero, data=layers)


@pytest.mark.gpu
@pytest.mark.parametrize("T, grids", [(512, GRIDS), (1024, GRIDS), (64, GRIDS), (768, (1, 2, 64)), (100, (1, 2, 4)), (32, (32,))],
                         ids=["512", "1024", "64", "768", "100", "32"])
def test_noise(device, T, grids):
    """uniform u16 noise (+ 5 % zeros in half the layers); 512 / 1024 / 64 take the vector path at s >= 8, 768 and 100 (rows not 16-byte
    multiples) the plain one, T = 32 at grid 32 has one bilinear patch per cell"""
    rng = np.random.default_rng(T)
    layers = rng.integers(0, 65536, size=(4, T, T), dtype=np.uint16)
    layers[2:][rng.random(layers[2:].shape) < 0.05] = 0
    atlas = make_atlas(device, T, 6)
    for i, layer in enumerate(layers):
        atlas.upload_tile(0, i + 2, layer)
    for grid in grids:
        for skip_zero in (False, True):
            assert_bounds(atlas, [2, 3, 4, 5], grid, skip_zero, data=layers)


def holed_job(device, atlas_size=96, seed=1234):
    """config 2's height job (4096^2 R16, T = 512, b = 2, lod_count 4, 85 tiles) with 5 % no-data texels in its source"""
    src = device.download(device.synth_fbm_r16(4096, 4096, seed), (4096, 4096), np.uint16)
    src[np.random.default_rng(seed).random(src.shape) < 0.05] = 0
    atlas = make_atlas(device, 512, atlas_size)
    pre = bt.Preprocessor.new().clear_attachment(0, atlas).preprocess_tile(
        bt.PreprocessDataset(attachment_index=0, path="h", lod_range=range(0, 4)), bt.AssetServer().insert("h", src), atlas)
    return atlas, pre


@pytest.mark.gpu
def test_preprocessed_tiles_with_no_data(device):
    atlas, pre = holed_job(device)
    pre.run(atlas)
    tiles = [i for _, i in atlas.tiles()]
    assert len(tiles) == 85 and 90 not in tiles
    data = layer_data(atlas, tiles)
    assert (data == 0).any()
    for grid in (1, 8, 64):
        for skip_zero in (False, True):
            got = assert_bounds(atlas, None, grid, skip_zero, data=data)  # layers=None: the layers of tiles(), in that order
            if skip_zero:
                assert (got[0][..., 0] > 0).all()
    unused = atlas.tile_bounds(0, [90], 8)
    assert all((l == 0).all() for l in unused)
    unused = atlas.tile_bounds(0, [90], 8, skip_zero=True)
    assert all((l[..., 0] == 0xFFFF).all() and (l[..., 1] == 0).all() for l in unused)


@pytest.mark.gpu
def test_layer_lists(device):
    """a non-contiguous, unsorted list with a repeat; layers = NULL in the C call is 0 .. count-1"""
    rng = np.random.default_rng(5)
    atlas = make_atlas(device, 512, 12)
    for i in range(12):
        atlas.upload_tile(0, i, rng.integers(0, 65536, size=(512, 512), dtype=np.uint16))
    listed = [9, 2, 7, 2, 0, 11]
    got = assert_bounds(atlas, listed, 16)
    single = {i: atlas.tile_bounds(0, [i], 16) for i in set(listed)}
    for slot, i in enumerate(listed):
        assert all(np.array_equal(g[slot], s[0]) for g, s in zip(got, single[i]))
    for grid, skip_zero in ((64, False), (4, True)):
        cells = BM.cells_per_layer(grid)
        out = np.empty((12, cells, 2), dtype=np.uint16)
        _ffi.check(_ffi.lib().bt_atlas_tile_bounds(atlas._h, 0, None, 12, grid, _ffi.BOUNDS_SKIP_ZERO if skip_zero else 0,
                                                   out.ctypes.data_as(C.POINTER(C.c_uint16)), out.nbytes))
        listed = np.concatenate([l.reshape(12, -1, 2) for l in atlas.tile_bounds(0, list(range(12)), grid, skip_zero)], axis=1)
        assert np.array_equal(out, listed)


@pytest.mark.gpu
def test_ordered_behind_queued_work(device):
    """a preprocessor run left unsynchronised (8192^2 source from the device, 341 tiles), bounds at once == bounds after a synchronise"""
    cfg = bt.TerrainConfig(lod_count=5, atlas_size=400, path="terrains/bounds8k", model=bt.TerrainModel.planar((0, 0, 0), 1000.0, 0.0, 1.0))
    cfg.add_attachment(bt.AttachmentConfig(name="height", texture_size=512, border_size=2))
    atlas = bt.TileAtlas.new(cfg, device)
    ptr = device.synth_fbm_r16(8192, 8192, 77)
    pre = bt.Preprocessor.new().clear_attachment(0, atlas).preprocess_tile(
        bt.PreprocessDataset(attachment_index=0, path="h", lod_range=range(0, 5)), bt.AssetServer().insert("h", (ptr, 8192, 8192)), atlas)
    pre.run(atlas, keep_queue=True, sync=False)
    early = atlas.tile_bounds(0, None, 32)
    device.synchronize()
    late = atlas.tile_bounds(0, None, 32)
    assert len(atlas.tiles()) == 341 and early[0].shape == (341, 32, 32, 2)
    assert all(np.array_equal(a, b) for a, b in zip(early, late))
    assert (late[-1][:, 0, 0, 1] > 0).all()  # every tile was written
    pre.close()
    device.free(ptr)


@pytest.mark.gpu
def test_reads_are_not_writes(device):
    """bounds of every layer of a fresh atlas leave Attachment::written alone: the job with no-data texels that follows takes prev_zero as often
    as it does without the call"""
    counts = []
    for read_first in (False, True):
        atlas, pre = holed_job(device)
        if read_first:
            atlas.tile_bounds(0, list(range(96)), 64)
            atlas.tile_bounds(0, None, 4, skip_zero=True)
        pre.run(atlas)
        counts.append(pre.stats()["prev_zero_launches"])
    assert counts[0] > 0 and counts[1] == counts[0], counts


@pytest.mark.gpu
def test_loaded_tiles(device, tmp_path):
    """tiles saved to files and loaded into a new atlas (bt_atlas_load_tiles) have the original's bounds, tile for tile"""
    atlas, pre = holed_job(device)
    pre.run(atlas)
    root = str(tmp_path)
    os.makedirs(atlas.attachment_directory(root, 0), exist_ok=True)
    atlas.save_attachment(0, atlas.attachment_directory(root, 0))
    atlas.save_tile_config(root)
    loaded = make_atlas(device, 512, 96)
    loaded.load_tile_config(root)
    coords = [c for c, _ in atlas.tiles()]
    loaded.load_tiles(0, root, coords)
    where = {c: i for c, i in loaded.tiles()}
    before = atlas.tile_bounds(0, [i for _, i in atlas.tiles()], 16, skip_zero=True)
    after = loaded.tile_bounds(0, [where[c] for c in coords], 16, skip_zero=True)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    assert_bounds(loaded, [where[c] for c in coords], 16, True)


@pytest.mark.gpu
def test_errors_and_scratch(device):
    L = _ffi.lib()
    rgba = make_atlas(device, 64, 2, fmt=bt.AttachmentFormat.Rgba8)
    out = np.full((4, BM.cells_per_layer(64), 2), 0x1234, dtype=np.uint16)
    ptr = out.ctypes.data_as(C.POINTER(C.c_uint16))
    one = (C.c_uint32 * 1)(0)
    assert L.bt_atlas_tile_bounds(rgba._h, 0, one, 1, 1, 0, ptr, out.nbytes) == BT_ERR_UNSUPPORTED
    r16 = make_atlas(device, 100, 3)
    calls = {"grid 0": (0, 1, 0, 0), "grid 3": (0, 1, 3, 0), "grid 128": (0, 1, 128, 0), "grid 8 of T 100": (0, 1, 8, 0),
             "unknown flag": (0, 1, 4, 2), "attachment 1": (1, 1, 4, 0)}
    for what, (ai, n, grid, flags) in calls.items():
        assert L.bt_atlas_tile_bounds(r16._h, ai, one, n, grid, flags, ptr, out.nbytes) == BT_ERR_INVALID_ARGUMENT, what
        assert L.bt_last_error(), what
    bad = (C.c_uint32 * 2)(0, 3)
    assert L.bt_atlas_tile_bounds(r16._h, 0, bad, 2, 4, 0, ptr, out.nbytes) == BT_ERR_INVALID_ARGUMENT  # layer >= atlas_size
    assert L.bt_atlas_tile_bounds(r16._h, 0, None, 4, 4, 0, ptr, out.nbytes) == BT_ERR_INVALID_ARGUMENT  # NULL list past atlas_size
    assert L.bt_atlas_tile_bounds(r16._h, 0, one, 1, 4, 0, ptr, 21 * 4 - 1) == BT_ERR_INVALID_ARGUMENT  # short out_bytes
    assert L.bt_atlas_tile_bounds(r16._h, 0, one, 1, 4, 0, None, 0) == BT_ERR_INVALID_ARGUMENT  # NULL out_host
    assert L.bt_atlas_tile_bounds(r16._h, 0, one, 0, 4, 0, ptr, 0) == _ffi.BT_OK
    assert L.bt_atlas_tile_bounds(r16._h, 0, None, 0, 4, 0, None, 0) == _ffi.BT_OK
    assert (out == 0x1234).all()
    assert L.bt_atlas_tile_bounds(r16._h, 0, one, 1, 4, 0, ptr, 21 * 4) == _ffi.BT_OK
    assert (out.reshape(-1)[:42] == 0).all() and (out.reshape(-1)[42:] == 0x1234).all()  # exactly one layer's pyramid written
    # the scratch stays in the context until bt_ctx_trim, and the call works again after it
    assert device.trim() > 0
    assert device.trim() == 0
    r16.upload_tile(0, 2, np.full((100, 100), 7, dtype=np.uint16))
    assert [l[0].tolist() for l in r16.tile_bounds(0, [2], 2)] == [[[[7, 7], [7, 7]], [[7, 7], [7, 7]]], [[[7, 7]]]]

"""Packed tiles on the device against the model of the format (tests/_pack_model.py, pinned by test_pack_model.py).

Everything is compared byte for byte: the device's streams and offsets with the model's encoding of the layers, a decoded atlas (level 0
and every mip level) with a twin that took the raw texels, the files with the model's streams, and bt_atlas_update reading `.btp` with a
twin reading `.bin`.  The layers are filled with upload_tile, so the tile sizes are those at which the kernels can go wrong: a partial
group and a partial strip (24), one exact group (64), a second group of 8 lanes and a last strip of 8 rows (72), three groups and five
strips (136), eight group columns and sixteen strips (512), and the b + 1 groups a row needs to hold every width (1088, 576)."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

import _cases as K
import _pack_cases as PC
import _pack_model as M
import bevy_terrain_amd as bt
from bevy_terrain_amd import _ffi

R16, RGBA8 = M.FORMAT_R16, M.FORMAT_RGBA8
FMT = {R16: bt.AttachmentFormat.R16, RGBA8: bt.AttachmentFormat.Rgba8}
BT_ERR_INVALID_ARGUMENT, BT_ERR_IO, BT_ERR_UNSUPPORTED, BT_ERR_OVERFLOW = -1, -4, -5, -7
MIPS = 3


@pytest.fixture(scope="module")
def device():
    return bt.Device(0)


def make_atlas(device, fmt, T, layers, mips=MIPS):
    cfg = bt.TerrainConfig(lod_count=1, atlas_size=layers, path="terrains/pack", model=bt.TerrainModel.planar((0, 0, 0), 1000.0, 0.0, 1.0))
    cfg.add_attachment(bt.AttachmentConfig(name="att", texture_size=T, border_size=1, format=FMT[fmt], mip_level_count=mips))
    return bt.TileAtlas.new(cfg, device)


def raw_twin(device, fmt, T, tiles, layers=None, mips=MIPS):
    """an atlas whose layers took the raw texels through upload_tile, with their mip levels"""
    atlas = make_atlas(device, fmt, T, len(tiles), mips)
    for i, t in enumerate(tiles):
        atlas.upload_tile(0, i if layers is None else layers[i], t)
    atlas.generate_mipmaps(0)
    return atlas


def assert_layers_equal(got, want, layers, mips=MIPS, what=""):
    for layer in layers:
        for mip in range(mips):
            g, w = got.download_mip(0, mip, layer), want.download_mip(0, mip, layer)
            assert g.shape == w.shape and np.array_equal(g, w), (what, layer, mip, np.argwhere(g != w)[:4])


def concatenated(streams):
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in streams])]).astype(np.uint64)
    return b"".join(streams), offsets


def kinds_of(fmt, T):
    return [kind for kind, f, t in PC.names() if (f, t) == (fmt, T)]


@pytest.mark.gpu
@pytest.mark.parametrize("fmt,T", PC.SHAPES + [PC.BIG] + PC.EVERY_WIDTH)
def test_streams_equal_the_model_and_decode_back(device, fmt, T):
    kinds = kinds_of(fmt, T)
    tiles = [PC.tile(kind, fmt, T) for kind in kinds]
    source = raw_twin(device, fmt, T, tiles)
    n = len(tiles)
    downloaded = source.download_tiles(0, 0, n)
    assert all(np.array_equal(downloaded[i], tiles[i]) for i in range(n))
    data, offsets = source.pack_tiles(0, range(n))
    want, want_offsets = concatenated([M.encode(downloaded[i]) for i in range(n)])
    assert list(offsets) == list(want_offsets), (kinds, list(offsets), list(want_offsets))
    for i, kind in enumerate(kinds):
        lo, hi = int(offsets[i]), int(offsets[i + 1])
        assert data[lo:hi] == want[lo:hi], (kind, fmt, T, next(j for j in range(hi - lo) if data[lo + j] != want[lo + j]))
        assert bt.packed_tile_check(data[lo:hi]) == (FMT[fmt], T)
    again, offsets_again = source.pack_tiles(0, range(n))
    assert again == data and list(offsets_again) == list(offsets), "the encoding depends on nothing but the tile"
    fresh = make_atlas(device, fmt, T, n)
    fresh.unpack_tiles(0, range(n), data, offsets)
    assert_layers_equal(fresh, source, range(n), what=(kinds, fmt, T))


@pytest.mark.gpu
@pytest.mark.parametrize("fmt,T", [(R16, 24), (RGBA8, 24), (R16, 72), (RGBA8, 72), (R16, 136), (RGBA8, 136)])
def test_accepted_streams_that_are_not_canonical(device, fmt, T):
    """widths above the minimal ones and garbage in the dead lanes' bits: the same tile"""
    kinds = kinds_of(fmt, T)
    tiles = [PC.tile(kind, fmt, T) for kind in kinds]
    loose = [PC.loosened(kind, fmt, T) for kind in kinds]
    assert sum(l != PC.stream(kind, fmt, T) for l, kind in zip(loose, kinds)) >= len(kinds) - 2
    data, offsets = concatenated(loose)
    fresh = make_atlas(device, fmt, T, len(tiles))
    fresh.unpack_tiles(0, range(len(tiles)), data, offsets)
    assert_layers_equal(fresh, raw_twin(device, fmt, T, tiles), range(len(tiles)), what=(kinds, fmt, T))


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [R16, RGBA8])
def test_lists_with_repeats_and_in_descending_order(device, fmt):
    T, kinds = 72, ["smooth", "noise", "spikes", "inclined"]
    tiles = [PC.tile(kind, fmt, T) for kind in kinds]
    source = raw_twin(device, fmt, T, tiles)
    order = [3, 1, 1, 0, 2, 3]
    data, offsets = source.pack_tiles(0, order)
    want, want_offsets = concatenated([PC.stream(kinds[i], fmt, T) for i in order])
    assert data == want and list(offsets) == list(want_offsets)
    fresh = make_atlas(device, fmt, T, 4)
    down = [3, 2, 1, 0]
    data, offsets = concatenated([PC.stream(kinds[3 - i], fmt, T) for i in down])  # layer l receives tile 3 - l
    fresh.unpack_tiles(0, down, data, offsets)
    assert_layers_equal(fresh, raw_twin(device, fmt, T, tiles[::-1]), range(4))
    with pytest.raises(_ffi.BtError) as e:  # a layer twice: refused, nothing touched
        fresh.unpack_tiles(0, [0, 1, 0], *concatenated([PC.stream(kinds[0], fmt, T)] * 3))
    assert e.value.status == BT_ERR_INVALID_ARGUMENT
    assert_layers_equal(fresh, raw_twin(device, fmt, T, tiles[::-1]), range(4))


@pytest.mark.gpu
def test_sizing_overflow_and_chunks(device):
    """dst_host = NULL fills the offsets only; a buffer that is too small is BT_ERR_OVERFLOW with the offsets filled; more than one chunk
    of 64 tiles"""
    T, n = 24, 150
    kinds = kinds_of(R16, T)
    tiles = [PC.tile(kinds[i % len(kinds)], R16, T) for i in range(n)]
    source = raw_twin(device, R16, T, tiles)
    want, want_offsets = concatenated([PC.stream(kinds[i % len(kinds)], R16, T) for i in range(n)])
    empty, offsets = source.pack_tiles(0, range(n), sizes_only=True)
    assert empty == b"" and list(offsets) == list(want_offsets)
    data, offsets = source.pack_tiles(0, range(n))
    assert data == want and list(offsets) == list(want_offsets)
    for capacity in (len(want) - 8, int(want_offsets[70]), 0):
        with pytest.raises(_ffi.BtError) as e:
            source.pack_tiles(0, range(n), capacity=capacity)
        assert e.value.status == BT_ERR_OVERFLOW and list(e.value.offsets) == list(want_offsets), capacity
    data, offsets = source.pack_tiles(0, range(n), capacity=len(want) + 100)
    assert data == want
    fresh = make_atlas(device, R16, T, n)
    fresh.unpack_tiles(0, range(n), data, offsets)
    assert_layers_equal(fresh, source, range(n))
    assert source.pack_tiles(0, [])[1].tolist() == [0]
    # chunks in which every stream reaches the bound (a group takes 64 lanes' bits, the dead lanes' included: 3112 bytes for 1152 of texels)
    worst = raw_twin(device, R16, T, [PC.tile("most_negative", R16, T)] * 70)
    data, offsets = worst.pack_tiles(0, range(70))
    assert data == PC.stream("most_negative", R16, T) * 70 and int(offsets[-1]) == 70 * M.bound(R16, T) == 70 * 3112
    fresh = make_atlas(device, R16, T, 70)
    fresh.unpack_tiles(0, range(70), data, offsets)
    assert_layers_equal(fresh, worst, range(70))


# ------------------------------------------------------------------------------------------------ a small real job and its files

LODS, JOB_T, JOB_B = 3, 64, 2


def job_config(atlas_size=64):
    cfg = bt.TerrainConfig(lod_count=LODS, atlas_size=atlas_size, path="terrains/pack", model=bt.TerrainModel.planar((0, 0, 0), 1000.0, 0.0, 1.0))
    cfg.add_attachment(bt.AttachmentConfig(name="height", texture_size=JOB_T, border_size=JOB_B, format=bt.AttachmentFormat.R16, mip_level_count=MIPS))
    cfg.add_attachment(bt.AttachmentConfig(name="albedo", texture_size=JOB_T, border_size=JOB_B, format=bt.AttachmentFormat.Rgba8, mip_level_count=MIPS))
    return cfg


def job_sources(seed=0):
    height = K.smooth_raster(300, 300, seed=7 + seed).copy()
    height[40:60, 100:130] = 0
    albedo = np.empty((300, 300, 4), np.uint8)
    albedo[..., 0] = np.maximum(height >> 8, 1)
    albedo[..., 1] = (height >> 4) & 255
    albedo[..., 2] = 255 - (height >> 9)
    albedo[..., 3] = 255
    albedo[200:230, 30:80, 0] = 0
    return height, albedo


def run_job(atlas, seed=0, clear=True):
    height, albedo = job_sources(seed)
    server = bt.AssetServer().insert("height", height).insert("albedo", albedo)
    pre = bt.Preprocessor.new()
    if clear:
        pre.clear_attachment(0, atlas).clear_attachment(1, atlas)
    for ai, path in enumerate(("height", "albedo")):
        pre.preprocess_tile(bt.PreprocessDataset(attachment_index=ai, path=path, lod_range=range(0, LODS)), server, atlas)
    pre.run(atlas)
    return pre


@pytest.fixture(scope="module")
def job(device, tmp_path_factory):
    """the job's atlas, saved raw and packed under one root, and the tile -> layer map"""
    root = str(tmp_path_factory.mktemp("pack_job"))
    atlas = bt.TileAtlas.new(job_config(), device)
    run_job(atlas)
    for ai in range(2):
        atlas.generate_mipmaps(ai)
        atlas.save_attachment(ai, atlas.attachment_directory(root, ai))
        atlas.save_tiles_packed(ai, atlas.attachment_directory(root, ai))
    atlas.save_tile_config(root)
    return atlas, root, atlas.tiles()


def assert_atlases_equal(got, want, tiles, what=""):
    for coord, _ in tiles:
        for ai in range(2):
            lg, lw = got.get_tile(coord)[1], want.get_tile(coord)[1]
            assert lg != _ffi.INVALID_ATLAS_INDEX and lw != _ffi.INVALID_ATLAS_INDEX, (what, coord)
            for mip in range(MIPS):
                assert np.array_equal(got.download_mip(ai, mip, lg), want.download_mip(ai, mip, lw)), (what, coord, ai, mip)


@pytest.mark.gpu
def test_a_real_jobs_tiles_and_files(device, job):
    atlas, root, tiles = job
    assert len(tiles) == 21
    for ai in range(2):
        layers = [layer for _, layer in tiles]
        data, offsets = atlas.pack_tiles(ai, layers)
        directory = atlas.attachment_directory(root, ai)
        raw = packed = 0
        for i, (coord, layer) in enumerate(tiles):
            want = M.encode(atlas.download_tile(ai, layer))
            assert data[int(offsets[i]):int(offsets[i + 1])] == want, (ai, coord)
            with open(os.path.join(directory, f"{coord}.btp"), "rb") as f:
                assert f.read() == want, (ai, coord)
            raw, packed = raw + os.path.getsize(os.path.join(directory, f"{coord}.bin")), packed + len(want)
        assert packed < raw, "a smooth terrain packs"
    # save then load through the files equals save_tiles then load_tiles
    twin_raw, twin_packed = bt.TileAtlas.new(job_config(), device), bt.TileAtlas.new(job_config(), device)
    for twin in (twin_raw, twin_packed):
        twin.load_tile_config(root)
    for ai in range(2):
        twin_raw.load_tiles(ai, root)
        twin_packed.load_tiles_packed(ai, twin_packed.attachment_directory(root, ai))
    assert_atlases_equal(twin_packed, twin_raw, tiles, "all")
    assert_atlases_equal(twin_packed, atlas, tiles, "source")
    # a list of coordinates, saved and loaded
    some = [coord for coord, _ in tiles[3:9]]
    directory = os.path.join(root, "some")
    atlas.save_tiles_packed(0, directory, some)
    assert sorted(os.listdir(directory)) == sorted(f"{c}.btp" for c in some)
    third = bt.TileAtlas.new(job_config(), device)
    third.load_tiles_packed(0, directory, some)
    for coord in some:
        for mip in range(MIPS):
            assert np.array_equal(third.download_mip(0, mip, third.get_tile(coord)[1]), atlas.download_mip(0, mip, atlas.get_tile(coord)[1]))
    with pytest.raises(_ffi.BtError) as e:
        third.load_tiles_packed(0, directory, [tiles[0][0]])  # no such file
    assert e.value.status == BT_ERR_IO
    with pytest.raises(_ffi.BtError) as e:
        atlas.save_tiles_packed(0, directory, [bt.TileCoordinate(0, 9, 1, 1)])  # no such tile
    assert e.value.status == BT_ERR_INVALID_ARGUMENT


def streaming_state(atlas, coords):
    return [atlas.get_best_tile(c) for c in coords], atlas.pending_loads()


@pytest.mark.gpu
def test_update_reads_packed_files_in_lock_step(device, job, tmp_path):
    source, root, tiles = job
    coords = [c for c, _ in tiles]
    broken = str(tmp_path / "broken")
    shutil.copytree(root, broken)
    gone, short = coords[5], coords[11]
    for ai, ext in ((0, ".bin"), (0, ".btp")):
        directory = source.attachment_directory(broken, ai)
        os.remove(os.path.join(directory, f"{gone}{ext}"))
        path = os.path.join(directory, f"{short}{ext}")
        with open(path, "rb") as f:
            content = f.read()
        with open(path, "wb") as f:
            f.write(content[:-8])
    for assets, failures in ((root, 0), (broken, 2)):
        twin_raw, twin_packed = bt.TileAtlas.new(job_config(32), device), bt.TileAtlas.new(job_config(32), device)
        twin_packed.set_tile_files(True)
        for twin in (twin_raw, twin_packed):
            twin.load_tile_config(assets)
        failed = 0
        frames = [(coords[:6], [], 5), (coords[6:14], coords[:2], 0), (coords[14:], coords[2:4], 7), ([], [], 0)]
        for requested, released, max_loads in frames:
            outcomes = []
            for twin in (twin_raw, twin_packed):
                for c in requested:
                    twin.request_tile(c)
                for c in released:
                    twin.release_tile(c)
                outcomes.append(twin.update(assets, max_loads))
            assert outcomes[0] == outcomes[1], (assets, outcomes)
            assert streaming_state(twin_raw, coords) == streaming_state(twin_packed, coords)
            failed += outcomes[1][1]
        assert failed == failures and twin_packed.pending_loads() == 0
        loaded = [c for c in coords if twin_packed.get_best_tile(c)[1] == c.lod]
        assert len(loaded) == len(coords) - failures
        if failures:  # both are left Loading: their best tile is an ancestor
            assert gone not in loaded and short not in loaded
        for c in loaded:
            for ai in range(2):
                for mip in range(MIPS):
                    g, w = twin_packed.download_mip(ai, mip, twin_packed.get_tile(c)[1]), source.download_mip(ai, mip, source.get_tile(c)[1])
                    assert np.array_equal(g, w), (assets, c, ai, mip)
        twin_packed.set_tile_files(False)  # and back: `.bin` again


@pytest.mark.gpu
def test_layers_count_as_written_like_after_load_tiles(device, job):
    """the prepared-write flag: a masked job (no-data texels keep the previous value) over layers that came from packed files equals its
    twin's over layers that came from `.bin`, in its tiles and in the launches that took the previous value as zero"""
    source, root, tiles = job
    twin_raw, twin_packed, fresh = (bt.TileAtlas.new(job_config(), device) for _ in range(3))
    for twin in (twin_raw, twin_packed):
        twin.load_tile_config(root)
    for ai in range(2):
        twin_raw.load_tiles(ai, root)
        twin_packed.load_tiles_packed(ai, twin_packed.attachment_directory(root, ai))
    stats = [run_job(twin, seed=3, clear=False).stats() for twin in (twin_raw, twin_packed)]
    assert stats[0] == stats[1] and stats[1]["prev_zero_launches"] == 0, stats
    assert_atlases_equal(twin_packed, twin_raw, tiles)
    assert run_job(fresh, seed=3, clear=False).stats()["prev_zero_launches"] > 0  # what the flag is for
    # and through unpack_tiles
    again = bt.TileAtlas.new(job_config(), device)
    again.load_tile_config(root)
    for ai in range(2):
        layers = [again.get_or_allocate_tile(c)[1] for c, _ in tiles]
        data, offsets = source.pack_tiles(ai, [layer for _, layer in tiles])
        again.unpack_tiles(ai, layers, data, offsets)
    assert run_job(again, seed=3, clear=False).stats() == stats[0]
    assert_atlases_equal(again, twin_raw, tiles)
    # packing is a read: the layers of a fresh atlas stay fresh
    fresh2 = bt.TileAtlas.new(job_config(), device)
    fresh2.pack_tiles(0, range(8))
    assert run_job(fresh2, seed=3, clear=False).stats()["prev_zero_launches"] > 0


# ------------------------------------------------------------------------------------------------ refusals

@pytest.mark.gpu
def test_invalid_streams_touch_nothing(device, tmp_path):
    T, n = 27, 3
    atlas = make_atlas(device, R16, T, n, mips=1)
    before = [PC.tile(kind, R16, T) for kind in ("noise", "smooth", "checker")]
    for i, t in enumerate(before):
        atlas.upload_tile(0, i, t)

    def unchanged():
        return all(np.array_equal(atlas.download_tile(0, i), before[i]) for i in range(n))

    good = PC.stream("inclined", R16, T)
    cases = [(name, data, BT_ERR_UNSUPPORTED if name == "strip rows 16" else BT_ERR_IO) for name, data, _ in PC.invalid_streams()]
    cases += [("another size", PC.stream("smooth", R16, 24), BT_ERR_INVALID_ARGUMENT), ("another format", PC.stream("smooth", RGBA8, 24), BT_ERR_INVALID_ARGUMENT)]
    coord = bt.TileCoordinate(0, 0, 0, 0)
    assert atlas.get_or_allocate_tile(coord)[1] == 0
    for name, data, status in cases:
        with pytest.raises(_ffi.BtError) as e:
            atlas.unpack_tiles(0, [1], data, [0, len(data)])
        assert e.value.status == status and unchanged(), name
        with pytest.raises(_ffi.BtError) as e:  # behind a valid one: the valid one is not decoded either
            atlas.unpack_tiles(0, [2, 0], *concatenated([good, data]))
        assert e.value.status == status and unchanged(), name
        with open(tmp_path / f"{coord}.btp", "wb") as f:
            f.write(data)
        with pytest.raises(_ffi.BtError) as e:
            atlas.load_tiles_packed(0, str(tmp_path), [coord])
        assert e.value.status == BT_ERR_IO and unchanged(), name
    with pytest.raises(_ffi.BtError) as e:
        atlas.unpack_tiles(0, [n], good, [0, len(good)])  # a layer the atlas does not have
    assert e.value.status == BT_ERR_INVALID_ARGUMENT and unchanged()
    atlas.unpack_tiles(0, [1], good, [0, len(good)])
    assert np.array_equal(atlas.download_tile(0, 1), PC.tile("inclined", R16, T)) and np.array_equal(atlas.download_tile(0, 0), before[0])


@pytest.mark.gpu
def test_null_arguments_and_unsupported_attachments(device):
    L = _ffi.lib()
    atlas = make_atlas(device, R16, 24, 2, mips=1)
    layers, offsets = (C.c_uint32 * 2)(0, 1), (C.c_uint64 * 3)()
    buf = (C.c_uint8 * 64)()
    assert L.bt_atlas_pack_tiles(None, 0, layers, 2, None, 0, offsets) == BT_ERR_INVALID_ARGUMENT
    assert L.bt_atlas_pack_tiles(atlas._h, 0, None, 2, None, 0, offsets) == BT_ERR_INVALID_ARGUMENT
    assert L.bt_atlas_pack_tiles(atlas._h, 0, layers, 2, None, 0, None) == BT_ERR_INVALID_ARGUMENT
    assert L.bt_atlas_pack_tiles(atlas._h, 1, layers, 2, None, 0, offsets) == BT_ERR_INVALID_ARGUMENT
    assert L.bt_atlas_pack_tiles(atlas._h, 0, (C.c_uint32 * 2)(0, 2), 2, None, 0, offsets) == BT_ERR_INVALID_ARGUMENT
    assert L.bt_atlas_unpack_tiles(None, 0, layers, 2, buf, offsets) == BT_ERR_INVALID_ARGUMENT
    assert L.bt_atlas_unpack_tiles(atlas._h, 0, None, 2, buf, offsets) == BT_ERR_INVALID_ARGUMENT
    assert L.bt_atlas_unpack_tiles(atlas._h, 0, layers, 2, None, offsets) == BT_ERR_INVALID_ARGUMENT
    assert L.bt_atlas_unpack_tiles(atlas._h, 0, layers, 2, buf, None) == BT_ERR_INVALID_ARGUMENT
    assert L.bt_atlas_unpack_tiles(atlas._h, 0, None, 0, None, None) == 0
    for fn in (L.bt_atlas_save_tiles_packed, L.bt_atlas_load_tiles_packed):
        assert fn(None, 0, b"x", None, 0) == BT_ERR_INVALID_ARGUMENT
        assert fn(atlas._h, 0, None, None, 0) == BT_ERR_INVALID_ARGUMENT
        assert fn(atlas._h, 0, b"x", None, 3) == BT_ERR_INVALID_ARGUMENT
        assert fn(atlas._h, 4, b"x", None, 0) == BT_ERR_INVALID_ARGUMENT
    assert L.bt_atlas_set_tile_files(None, 1) == BT_ERR_INVALID_ARGUMENT
    assert L.bt_atlas_set_tile_files(atlas._h, 2) == BT_ERR_INVALID_ARGUMENT
    cfg = bt.TerrainConfig(lod_count=1, atlas_size=2, path="terrains/pack", model=bt.TerrainModel.planar((0, 0, 0), 1000.0, 0.0, 1.0))
    cfg.add_attachment(bt.AttachmentConfig(name="att", texture_size=24, border_size=1, format=bt.AttachmentFormat.Rg16))
    other = bt.TileAtlas.new(cfg, device)
    assert L.bt_atlas_pack_tiles(other._h, 0, layers, 2, None, 0, offsets) == BT_ERR_UNSUPPORTED
    assert L.bt_atlas_unpack_tiles(other._h, 0, layers, 2, buf, offsets) == BT_ERR_UNSUPPORTED
    assert L.bt_atlas_save_tiles_packed(other._h, 0, b"x", None, 0) == BT_ERR_UNSUPPORTED
    assert L.bt_atlas_load_tiles_packed(other._h, 0, b"x", None, 0) == BT_ERR_UNSUPPORTED
    assert L.bt_atlas_set_tile_files(other._h, 1) == BT_ERR_UNSUPPORTED and L.bt_atlas_set_tile_files(other._h, 0) == 0

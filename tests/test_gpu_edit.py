"""In-place editing on the device (bt_atlas_edit_height / bt_atlas_write_region / bt_atlas_save_tiles) against the numpy model of the
definition (tests/_edit_model.py, pinned to the goldens by test_edit_model.py).

Every comparison downloads ALL layers of the attachment and compares every existing tile of every LOD byte for byte with
propagate(apply_stamps(before)); layers that are not in `changed` must hold their bytes from before (layers without a tile included), every
differing layer must be in `changed`, and `changed` must be a subset of {edited tiles, their ancestors, existing neighbours of those}.
The shapes these cases leave out (a row beyond one lane trip, Rgba8 beyond one block, the plan's rarer branches, the cube at lod_count 3,
256 stamps, the plan ring's wrap) are in tests/test_gpu_edit_shapes.py."""
import os

import numpy as np
import pytest

import _cases as K
import _edit_model as EM
import _oracle as O
import bevy_terrain_amd as bt
from bevy_terrain_amd import EditStamp as S

R16, RGBA8 = O.FORMAT_R16, O.FORMAT_RGBA8
BT_ERR_INVALID_ARGUMENT, BT_ERR_UNSUPPORTED = -1, -5
ATLAS = 32


@pytest.fixture(scope="module")
def device():
    return bt.Device(0)


def source_r16(n=64, seed=5):
    """fBm with a few zero holes: a block, a single texel and a column piece"""
    src = K.smooth_raster(n, n, seed).copy()
    src[20:24, 30:34] = 0
    src[50, 9] = 0
    src[40:47, 55] = 0
    return src


def planar(device, T, b, lods=3, fmt=R16, src=None, mips=1, lod_range=None, then=(), **ds):
    """lod_range: the LODs the job fills (default: all of them); then: further jobs as (lod_range, extent keywords), each queued WITHOUT
    the clear and run on its own behind the first"""
    if src is None:
        src = source_r16() if fmt == R16 else K.random_raster(RGBA8, 64, 64, seed=8, holes=0.03)
    if lod_range is None and not then:
        atlas, pre = K.product_planar(device, src, lods, T, b, fmt, atlas_size=ATLAS, mips=mips, **ds)
        return atlas
    cfg = bt.TerrainConfig(lod_count=lods, atlas_size=ATLAS, path="terrains/edit", model=bt.TerrainModel.planar((0, 0, 0), 1000.0, 0.0, 1.0))
    cfg.add_attachment(bt.AttachmentConfig(name="att", texture_size=T, border_size=b, format=K.FMT[fmt], mip_level_count=mips))
    atlas = bt.TileAtlas.new(cfg, device)
    server = bt.AssetServer().insert("src", src)
    for k, (levels, extent) in enumerate([(lod_range or range(0, lods), ds)] + list(then)):
        pre = bt.Preprocessor.new()
        if k == 0:
            pre.clear_attachment(0, atlas)
        pre.preprocess_tile(bt.PreprocessDataset(attachment_index=0, path="src", lod_range=levels, **extent), server, atlas).run(atlas)
    return atlas


def cube_faces(n=40):
    """the six source rasters of cube(): fBm with a zero block each"""
    faces = []
    for s in range(6):
        face = K.smooth_raster(n, n, 100 + s).copy()
        face[3 + s:6 + s, 30:33] = 0
        faces.append(face)
    return faces


def cube(device, T=16, b=2, lods=2, n=40, mips=1, atlas_size=ATLAS):
    cfg = bt.TerrainConfig(lod_count=lods, atlas_size=atlas_size, path="terrains/edit")
    cfg.add_attachment(bt.AttachmentConfig(name="att", texture_size=T, border_size=b, format=bt.AttachmentFormat.R16, mip_level_count=mips))
    atlas = bt.TileAtlas.new(cfg, device)
    server = bt.AssetServer()
    paths = [f"face{s}" for s in range(6)]
    for p, face in zip(paths, cube_faces(n)):
        server.insert(p, face)
    pre = bt.Preprocessor.new().clear_attachment(0, atlas)
    pre.preprocess_spherical(bt.SphericalDataset(attachment_index=0, paths=paths, lod_range=range(0, lods)), server, atlas)
    pre.run(atlas)
    return atlas


class Snapshot:
    """all layers of attachment 0 and the tiles among them"""

    def __init__(self, atlas):
        self.index = {(c.side, c.lod, c.x, c.y): i for c, i in atlas.tiles()}
        self.data = atlas.download_tiles(0, 0, atlas.atlas_size)
        self.tiles = {c: self.data[i] for c, i in self.index.items()}


def geometry(atlas):
    a = atlas.config.attachments[0]
    return a.border_size, a.texture_size - 2 * a.border_size, atlas.config.model.is_spherical()


def check_edit(atlas, before, expected, changed, stats, edited, levels_above):
    """the comparisons of the module docstring + the stats; returns the snapshot after"""
    b, c, spherical = geometry(atlas)
    after = Snapshot(atlas)
    assert after.index == before.index
    bad = [k for k in before.index if not np.array_equal(after.tiles[k], expected[k])]
    if bad:
        k = bad[0]
        d = np.argwhere(after.tiles[k] != expected[k])
        pytest.fail(f"{len(bad)}/{len(before.index)} tiles differ from the model: {bad[:6]}; first {k}: {len(d)} texels, at (y, x) {d[0][:2].tolist()} "
                    f"got {after.tiles[k][tuple(d[0][:2])]} want {expected[k][tuple(d[0][:2])]}")
    changed = [(t.side, t.lod, t.x, t.y) for t in changed]
    assert len(set(changed)) == len(changed) == stats["changed_count"]
    assert all(k in before.index for k in changed)
    assert changed == sorted(changed, key=lambda k: (-k[1], before.index[k])), "changed: LOD descending, then atlas index"
    changed_layers = {before.index[k] for k in changed}
    for i in range(atlas.atlas_size):
        if i not in changed_layers:
            assert np.array_equal(after.data[i], before.data[i]), f"layer {i} is not in `changed` and differs from before"
    allowed = EM.allowed_changed(before.tiles, edited, spherical)
    assert set(changed) <= allowed, sorted(set(changed) - allowed)
    existing = {k for k in edited if k in before.index}
    assert stats["tiles_edited"] == len(existing) and stats["tiles_missing"] == len(edited) - len(existing)
    assert existing <= set(changed)
    assert stats["tiles_stitched"] == (len(changed) if b else 0)
    if existing:
        assert stats["launches"] >= 1 + levels_above + (1 if b else 0) and stats["tiles_downsampled"] >= levels_above
    else:
        assert stats["launches"] == 0 and not changed
    return after


def ancestors_levels(before, edited):
    """the number of LODs above the edited one that hold an ancestor of an edited tile: one downsample launch each"""
    cur, levels = {k for k in edited if k in before.index}, 0
    while cur:
        cur = {(s, l - 1, x >> 1, y >> 1) for s, l, x, y in cur if l > 0}
        cur = {k for k in cur if k in before.index}
        levels += bool(cur)
    return levels


def edit_and_check(atlas, stamps, lod=None):
    b, c, spherical = geometry(atlas)
    lod = atlas.lod_count - 1 if lod is None else lod
    before = Snapshot(atlas)
    held = EM.propagate(before.tiles, b, spherical)
    assert all(np.array_equal(held[k], before.tiles[k]) for k in before.tiles), "the state before the edit is not F of its primary centres"
    changed, stats = atlas.edit_height(0, stamps, lod)
    # tiles finer than `lod` are not touched: the definition is F over the tiles of LODs <= lod
    coarse = {k: v for k, v in before.tiles.items() if k[1] <= lod}
    expected = dict(before.tiles)
    expected.update(EM.propagate(EM.apply_stamps(coarse, lod, stamps, b), b, spherical))
    edited = EM.stamp_tiles(stamps, lod, c)
    after = check_edit(atlas, before, expected, changed, stats, edited, ancestors_levels(before, edited))
    if atlas.config.attachments[0].mip_level_count == 1:
        assert stats["layers_mipped"] == 0 and stats["launches"] == (1 + ancestors_levels(before, edited) + (1 if b else 0) if stats["tiles_edited"] else 0)
    return before, after, changed, stats


# ---------------------------------------------------------------------------------------------- 1. planar R16, T = 16, b = 2 (c = 12)

STAMP_SETS = {
    "inside_one_tile": [S((5.0, 6.0), 2.5, 0.2)],
    "four_tile_corner_odd_edges": [S((12.3, 11.6), 3.5, -0.15)],
    "mosaic_corner_and_edge": [S((0.5, 47.0), 5.0, 0.3)],
    "add_then_flatten_overlapping": [S((20.0, 20.0), 6.0, 0.25), S((23.0, 21.0), 5.0, 0.4, mode="flatten")],
    "larger_than_the_mosaic": [S((24.0, 24.0), 100.0, 0.1)],
    "hard_falloff": [S((30.5, 13.5), 4.0, -0.2, falloff="hard")],
    "over_a_hole": [S((24.0, 16.0), 5.0, 0.2)],
    "saturates_and_bottoms_out": [S((8.0, 40.0), 3.0, 2.0, falloff="hard"), S((40.0, 8.0), 3.0, -2.0, falloff="hard")],
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(STAMP_SETS))
def test_planar_r16_stamps(device, name):
    atlas = planar(device, 16, 2)
    before, after, changed, stats = edit_and_check(atlas, STAMP_SETS[name])
    differing = sum(1 for k in before.tiles if not np.array_equal(before.tiles[k], after.tiles[k]))
    assert differing >= 3, "the stamp changed nothing: the comparison would be empty"
    finest = {k: v[2:14, 2:14] for k, v in after.tiles.items() if k[1] == 2}
    if name == "over_a_hole":
        tile = before.tiles[(0, 2, 2, 1)][2:14, 2:14]
        gy, gx = np.mgrid[0:12, 0:12]
        near = (gx + 24 - 24.0) ** 2 + (gy + 12 - 16.0) ** 2 < 16
        assert (tile[near] == 0).any(), "no hole under the stamp"
        assert np.array_equal(tile == 0, finest[(0, 2, 2, 1)] == 0), "the hole mask changed"
    if name == "saturates_and_bottoms_out":
        assert (finest[(0, 2, 0, 3)] == 65535).sum() >= 9 and (finest[(0, 2, 3, 0)] == 1).sum() >= 9
    if name == "larger_than_the_mosaic":
        assert stats["tiles_edited"] == 16 and stats["changed_count"] == 21 and stats["tiles_downsampled"] == 5
    if name == "inside_one_tile":
        assert stats["tiles_edited"] == 1 and stats["tiles_downsampled"] == 2 and stats["launches"] == 4 and stats["tiles_with_children"] == 0


# ---------------------------------------------------------------------------------------------- 2. odd quadrant boundaries

@pytest.mark.gpu
@pytest.mark.parametrize("T,b", [(16, 1), (32, 3)])
def test_odd_quadrant_boundaries(device, T, b):
    """c = 14 (child quadrants of 7 texels) and c = 26 (13): a parent's dirty rectangle starts and ends on odd texels, and with an odd
    border every row of the centre starts in the upper half of a dword"""
    c = T - 2 * b
    atlas = planar(device, T, b)
    edit_and_check(atlas, [S((c + 0.3, c - 0.4), 3.5, 0.2)])
    edit_and_check(atlas, [S((2 * c - 1.0, 2 * c + 1.0), 2.0, -0.2, falloff="hard")])  # a second edit onto the edited state


# ---------------------------------------------------------------------------------------------- 3. cube

@pytest.mark.gpu
def test_cube_face_edges_and_corner_tiles(device):
    """T = 16, b = 2, lod_count 2: every finest tile is a cube-corner tile; stamps at a face edge on an even side and on an odd side.  All 30
    tiles are compared: the seams to the neighbouring faces go through project_to_side"""
    atlas = cube(device)
    assert len(atlas.tiles()) == 30
    before, after, changed, stats = edit_and_check(atlas, [S((0.5, 11.0), 4.0, 0.25, side=0)])
    assert {t.side for t in changed} - {0}, "no tile of a neighbouring face was re-stitched"
    before, after, changed, stats = edit_and_check(atlas, [S((22.0, 23.0), 3.5, -0.2, side=3), S((1.0, 1.0), 3.0, 0.2, side=3, falloff="hard")])
    assert {t.side for t in changed} - {3}
    edit_and_check(atlas, [S((12.0, 0.0), 5.0, 0.15, side=4), S((12.0, 0.0), 5.0, 0.15, side=1)])


# ---------------------------------------------------------------------------------------------- 4. missing tiles

@pytest.mark.gpu
def test_missing_tiles_are_skipped_and_counted(device):
    atlas = planar(device, 16, 2, top_left=(0.3, 0.3), bottom_right=(0.9, 0.9))
    index = {(c.side, c.lod, c.x, c.y) for c, _ in atlas.tiles()}
    assert (0, 2, 1, 1) in index and (0, 2, 0, 0) not in index and (0, 2, 0, 1) not in index and len(index) < 21
    before, after, changed, stats = edit_and_check(atlas, [S((10.0, 14.0), 4.0, 0.2)])
    assert stats["tiles_missing"] == 3 and stats["tiles_edited"] == 1
    before, after, changed, stats = edit_and_check(atlas, [S((3.0, 3.0), 2.0, 0.2)])  # only absent tiles
    assert stats["tiles_missing"] == 1 and stats["tiles_edited"] == 0 and stats["launches"] == 0 and changed == []


# ---------------------------------------------------------------------------------------------- 5. lod = lod_count - 2

@pytest.mark.gpu
def test_edit_below_the_finest_lod_leaves_finer_tiles(device):
    atlas = planar(device, 16, 2)
    before, after, changed, stats = edit_and_check(atlas, [S((11.5, 12.5), 4.0, 0.25)], lod=1)
    assert stats["tiles_edited"] == 4 and stats["tiles_with_children"] == 4 and stats["tiles_downsampled"] == 1
    assert all(t.lod <= 1 for t in changed)
    assert all(np.array_equal(before.tiles[k], after.tiles[k]) for k in before.tiles if k[1] == 2)


# ---------------------------------------------------------------------------------------------- 6. write_region

@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [R16, RGBA8], ids=["r16", "rgba8"])
@pytest.mark.parametrize("b", [2, 1])
def test_write_region(device, fmt, b):
    """odd x0 and width, crossing four tiles, zeros inside"""
    atlas = planar(device, 16, b, fmt=fmt)
    _, c, spherical = geometry(atlas)
    before = Snapshot(atlas)
    rng = np.random.default_rng(3)
    x0, y0, w, h = c - 5, c - 3, 11, 8
    texels = rng.integers(1, 65536, size=(h, w), dtype=np.uint16) if fmt == R16 else rng.integers(1, 256, size=(h, w, 4), dtype=np.uint8)
    texels[2:4, 3:9] = 0
    texels[7, 0] = 0
    changed, stats = atlas.write_region(0, texels, x0, y0)
    expected = EM.propagate(EM.write_region(before.tiles, 2, 0, x0, y0, texels, b), b, spherical)
    edited = EM.region_tiles(2, 0, x0, y0, w, h, c)
    assert len(edited) == 4
    after = check_edit(atlas, before, expected, changed, stats, edited, 2)
    assert stats["launches"] == 4 and stats["tiles_edited"] == 4
    centre = after.tiles[(0, 2, 0, 0)][b:b + c, b:b + c]
    assert np.array_equal(centre[c - 3:, c - 5:], texels[:3, :5])
    # a region over absent tiles only: nothing happens; a region that ends on the mosaic's last texel is inside
    n = 4 * c
    changed, stats = atlas.write_region(0, texels[:1, :1], n - 1, n - 1)
    assert stats["tiles_edited"] == 1 and Snapshot(atlas).tiles[(0, 2, 3, 3)][b + c - 1, b + c - 1].tolist() == texels[0, 0].tolist()


# ---------------------------------------------------------------------------------------------- 7. mips

@pytest.mark.gpu
def test_mips_of_changed_layers_follow(device):
    atlas = planar(device, 16, 2, mips=3)
    atlas.generate_mipmaps(0)
    mips_before = {i: [atlas.download_mip(0, k, i) for k in (1, 2)] for i in range(ATLAS)}
    before, after, changed, stats = edit_and_check(atlas, [S((30.0, 30.0), 4.0, 0.3)])
    layers = {before.index[(t.side, t.lod, t.x, t.y)] for t in changed}
    assert stats["layers_mipped"] == len(layers) > 0 and stats["launches"] > 4
    for i in range(ATLAS):
        got = [atlas.download_mip(0, k, i) for k in (1, 2)]
        if i in layers:
            chain = O.generate_mipmaps(R16, after.data[i], 3)
            want = [chain[256:320].reshape(8, 8), chain[320:336].reshape(4, 4)]
            assert all(np.array_equal(g, w) for g, w in zip(got, want)), f"mips of changed layer {i}"
        else:
            assert all(np.array_equal(g, w) for g, w in zip(got, mips_before[i])), f"mips of untouched layer {i}"


# ---------------------------------------------------------------------------------------------- 8. stream order

@pytest.mark.gpu
def test_edit_is_ordered_behind_a_run_without_synchronising(device):
    results = []
    for sync in (False, True):
        cfg = bt.TerrainConfig(lod_count=3, atlas_size=ATLAS, path="terrains/edit", model=bt.TerrainModel.planar((0, 0, 0), 1000.0, 0.0, 1.0))
        cfg.add_attachment(bt.AttachmentConfig(name="att", texture_size=16, border_size=2, format=bt.AttachmentFormat.R16))
        atlas = bt.TileAtlas.new(cfg, device)
        server = bt.AssetServer().insert("src", source_r16())
        pre = bt.Preprocessor.new().clear_attachment(0, atlas).preprocess_tile(bt.PreprocessDataset(attachment_index=0, path="src", lod_range=range(0, 3)), server, atlas)
        pre.run(atlas, sync=sync)
        for k in range(3):  # back to back: the plan ring serves several calls in flight
            atlas.edit_height(0, [S((12.3 + 7 * k, 11.6 + 5 * k), 3.5, 0.1)])
        results.append(atlas.download_tiles(0, 0, ATLAS))
    assert np.array_equal(results[0], results[1]) and results[0].any()


# ---------------------------------------------------------------------------------------------- 9. written flags

@pytest.mark.gpu
def test_edited_layers_count_as_written(device):
    """write_region onto allocated, never-written layers, then a fused job whose source has no-data texels: they keep the edited values (a
    launch that took the layers for fresh zeros would lose them).  The oracle is primed with the edited state (set_tile) and runs the job."""
    T, b, lods, W = 128, 2, 3, 496  # source : mosaic = 1.0 -> a fused job (tests/test_gpu_prev_values.py)
    src = K.low_half(K.random_raster(R16, W, W, seed=3, holes=0.01), R16)
    src[118:131, 20:300] = 0
    src[200:420, 244:253] = 0
    cfg = bt.TerrainConfig(lod_count=lods, atlas_size=ATLAS, path="terrains/edit", model=bt.TerrainModel.planar((0, 0, 0), 1000.0, 0.0, 1.0))
    cfg.add_attachment(bt.AttachmentConfig(name="att", texture_size=T, border_size=b, format=bt.AttachmentFormat.R16))
    atlas = bt.TileAtlas.new(cfg, device)
    server = bt.AssetServer().insert("src", src)
    pre = bt.Preprocessor.new().clear_attachment(0, atlas).preprocess_tile(bt.PreprocessDataset(attachment_index=0, path="src", lod_range=range(0, lods)), server, atlas)
    assert len(atlas.tiles()) == 21 and not atlas.download_tiles(0, 0, ATLAS).any()
    y, x = np.mgrid[0:W, 0:W]
    paint = (0x8000 | ((x * 37 + y * 101) & 0x7FFF)).astype(np.uint16)  # upper half: no blend of the lower-half source gives such a value
    changed, stats = atlas.write_region(0, paint, 0, 0)
    assert stats["tiles_edited"] == 16 and stats["changed_count"] == 21
    edited = Snapshot(atlas)
    pre.run(atlas)
    assert pre.stats()["prev_zero_launches"] == 0
    oracle = O.OracleAtlas(lods, ATLAS, False, [(T, b, 1, R16)])
    oracle.clear_attachment(0).preprocess_tile(0, src, (0, lods))
    for coord, i in edited.index.items():
        oracle.set_tile(0, i, edited.data[i])
    oracle.run(16)
    assert K.assert_atlas_equal(atlas, oracle) == 21
    centre = atlas.download_tile(0, edited.index[(0, 2, 0, 0)])[b:T - b, b:T - b]
    kept = centre == paint[:124, :124]
    assert kept[118:124, 20:124].all() and 0 < kept.sum() < kept.size


# ---------------------------------------------------------------------------------------------- 10. save_tiles

@pytest.mark.gpu
def test_save_tiles_writes_the_listed_files_only(device, tmp_path):
    atlas = planar(device, 16, 2)
    changed, stats = atlas.edit_height(0, [S((5.0, 6.0), 2.5, 0.2)])
    directory = str(tmp_path / "data" / "att")
    atlas.save_tiles(0, directory, changed)
    snap = Snapshot(atlas)
    assert sorted(os.listdir(directory)) == sorted(f"{t.side}_{t.lod}_{t.x}_{t.y}.bin" for t in changed) and 0 < len(changed) < 21
    for t in changed:
        assert open(os.path.join(directory, f"{t.side}_{t.lod}_{t.x}_{t.y}.bin"), "rb").read() == snap.tiles[(t.side, t.lod, t.x, t.y)].tobytes()
    with pytest.raises(bt.BtError) as e:
        atlas.save_tiles(0, str(tmp_path / "other"), [changed[0], bt.TileCoordinate(0, 2, 9, 9)])
    assert e.value.status == BT_ERR_INVALID_ARGUMENT and not os.path.exists(str(tmp_path / "other"))


# ---------------------------------------------------------------------------------------------- 11. errors

@pytest.mark.gpu
def test_errors_on_the_device(device):
    atlas = planar(device, 16, 2)
    before = Snapshot(atlas)

    def status(call):
        with pytest.raises(bt.BtError) as e:
            call()
        return e.value.status

    rgba = planar(device, 16, 2, fmt=RGBA8)
    assert status(lambda: rgba.edit_height(0, [S((5.0, 5.0), 2.0, 0.1)])) == BT_ERR_UNSUPPORTED
    cfg = bt.TerrainConfig(lod_count=3, atlas_size=4, path="terrains/edit", model=bt.TerrainModel.planar((0, 0, 0), 1000.0, 0.0, 1.0))
    cfg.add_attachment(bt.AttachmentConfig(name="att", texture_size=17, border_size=2, format=bt.AttachmentFormat.R16))  # c = 13
    odd = bt.TileAtlas.new(cfg, device)
    assert status(lambda: odd.edit_height(0, [S((5.0, 5.0), 2.0, 0.1)])) == BT_ERR_UNSUPPORTED
    assert status(lambda: odd.write_region(0, np.ones((2, 2), np.uint16), 0, 0)) == BT_ERR_UNSUPPORTED
    ones = np.ones((4, 4), np.uint16)
    assert status(lambda: atlas.write_region(0, ones, 45, 0)) == BT_ERR_INVALID_ARGUMENT  # 45 + 4 > 48
    assert status(lambda: atlas.write_region(0, ones, 0, 45)) == BT_ERR_INVALID_ARGUMENT
    assert status(lambda: atlas.write_region(0, ones, 0, 0, lod=3)) == BT_ERR_INVALID_ARGUMENT
    assert status(lambda: atlas.write_region(0, ones, 0, 0, side=1)) == BT_ERR_INVALID_ARGUMENT
    assert status(lambda: atlas.edit_height(0, [S((5.0, 5.0), 2.0, 0.1)], lod=3)) == BT_ERR_INVALID_ARGUMENT
    assert status(lambda: atlas.edit_height(0, [S((5.0, 5.0), 2.0, 0.1, side=1)])) == BT_ERR_INVALID_ARGUMENT  # a planar atlas has side 0 only
    assert status(lambda: atlas.edit_height(0, [S((5.0, 5.0), 2.0, 0.1)] * 257)) == BT_ERR_INVALID_ARGUMENT
    assert status(lambda: atlas.edit_height(1, [S((5.0, 5.0), 2.0, 0.1)])) == BT_ERR_INVALID_ARGUMENT
    changed, stats = atlas.edit_height(0, [])
    assert changed == [] and not any(stats.values())
    assert atlas.write_region(0, np.ones((0, 3), np.uint16), 1, 1)[0] == []
    assert np.array_equal(Snapshot(atlas).data, before.data), "a refused or empty call wrote something"
    # changed_cap smaller than the count: the list is cut, the count is whole
    from bevy_terrain_amd import _ffi
    import ctypes as C
    stamp = (_ffi.EditStampC * 1)(S((24.0, 24.0), 100.0, 0.1)._c())
    few = (_ffi.TileCoordinateC * 3)()
    stats = _ffi.EditStatsC()
    _ffi.check(_ffi.lib().bt_atlas_edit_height(atlas._h, 0, 2, stamp, 1, few, 3, C.byref(stats)))
    assert stats.changed_count == 21 and [t.lod for t in few] == [2, 2, 2]
    _ffi.check(_ffi.lib().bt_atlas_edit_height(atlas._h, 0, 2, stamp, 1, None, 0, None))  # no list, no stats


# ---------------------------------------------------------------------------------------------- shape sanity at the workload's tile size

@pytest.mark.gpu
def test_workload_tile_size_once(device):
    """T = 512, b = 2, lod_count 3, a synthetic source: one r = 40 stamp across a tile corner, compared on the changed tiles and their
    neighbours (the model's per-pixel stitch over all 21 tiles of this size is not worth its seconds)"""
    T, b, lods = 512, 2, 3
    c = T - 2 * b
    atlas = planar(device, T, b, lods, src=K.smooth_raster(1024, 1024, 9, device=device))
    before = Snapshot(atlas)
    stamps = [S((c + 0.25, 2 * c - 0.5), 40.0, 0.2)]
    changed, stats = atlas.edit_height(0, stamps)
    after = Snapshot(atlas)
    changed = [(t.side, t.lod, t.x, t.y) for t in changed]
    assert stats["tiles_edited"] == 4 and stats["launches"] == 4 and {(0, 0, 0, 0), (0, 1, 0, 0), (0, 1, 0, 1), (0, 2, 0, 1), (0, 2, 1, 2)} <= set(changed)
    expected = EM.propagate(EM.apply_stamps(before.tiles, 2, stamps, b), b, False, only=changed)
    for k in before.index:
        if k in changed:
            assert np.array_equal(after.tiles[k], expected[k]), k
        else:
            assert np.array_equal(after.tiles[k], before.tiles[k]), k
    assert sum(1 for k in changed if not np.array_equal(after.tiles[k], before.tiles[k])) >= 7

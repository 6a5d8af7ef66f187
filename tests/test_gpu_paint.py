"""bt_atlas_paint (the Rgba8 brush) and bt_atlas_read_region (the inverse of bt_atlas_write_region) on the device, against the numpy models
of their definitions (tests/_paint_model.py, held to the header's lines by test_paint_model.py; propagation is _edit_model.propagate).

Every paint comparison is the one of tests/test_gpu_edit.py (its helpers are imported, not copied): all layers downloaded, every existing
tile byte-equal to propagate(apply_paint(before)), every layer outside `changed` byte-equal to before, `changed` inside the allowed set, the
stats identities.  The sources are random Rgba8 rasters; the no-data texels (rgb == 0, alpha 200: a block, one texel, a column piece on
every side) are planted with bt_atlas_write_region, since a job resamples its source.

Every paint case proves from its own inputs that it has something to compare: test_cases_reach_their_branches asserts, without a GPU and on
states the CPU oracle makes from the same jobs, that every edit changes a texel of the model, that the cases named for the zero rule reach
it, that those named for holes have a no-data texel under a disc, and that those named for the walker's later trips reach them."""
import ctypes as C
import functools

import numpy as np
import pytest

import _cases as K
import _edit_model as EM
import _oracle as O
import _paint_model as PM
import bevy_terrain_amd as bt
from bevy_terrain_amd import EditStamp, SmoothStamp, _ffi
from bevy_terrain_amd import PaintStamp as P
from test_gpu_edit import ATLAS, R16, RGBA8, Snapshot, ancestors_levels, check_edit, geometry, planar, source_r16
from test_gpu_edit_shapes import big_r16, branches_reached, plan_levels, stamp_boxes

BT_ERR_INVALID_ARGUMENT, BT_ERR_UNSUPPORTED = -1, -5
MAX_STAMPS = 256  # BT_EDIT_MAX_STAMPS

# no-data texels planted on every side, (y0, x0, h, w) in mosaic texels of the finest LOD: inside the smallest mosaic used (24 x 24)
HOLES = [(5, 14, 4, 4), (20, 3, 1, 1), (12, 21, 6, 1)]


@pytest.fixture(scope="module")
def device():
    return bt.Device(0)


def hole_texels(h, w):
    texels = np.zeros((h, w, 4), np.uint8)
    texels[..., 3] = 200
    return texels


SPECS = {
    "planar_b2": dict(kind="planar", T=16, b=2, lods=3, n=64),
    "planar_b1": dict(kind="planar", T=16, b=1, lods=3, n=64),
    "planar_72": dict(kind="planar", T=72, b=2, lods=3, n=272),
    "cube": dict(kind="cube", T=16, b=2, lods=2, n=40),
    "partial": dict(kind="planar", T=16, b=2, lods=3, n=64, extent=dict(top_left=(0.3, 0.3), bottom_right=(0.9, 0.9))),
}


def rgba_source(n):
    return K.random_raster(RGBA8, n, n, seed=8)


def rgba_faces(n):
    return [K.random_raster(RGBA8, n, n, seed=100 + s) for s in range(6)]


def device_atlas(device, spec_name, mips=1, holes=True):
    spec = SPECS[spec_name]
    if spec["kind"] == "planar":
        atlas = planar(device, spec["T"], spec["b"], spec["lods"], RGBA8, src=rgba_source(spec["n"]), mips=mips, **spec.get("extent", {}))
    else:
        cfg = bt.TerrainConfig(lod_count=spec["lods"], atlas_size=ATLAS, path="terrains/paint")
        cfg.add_attachment(bt.AttachmentConfig(name="att", texture_size=spec["T"], border_size=spec["b"], format=bt.AttachmentFormat.Rgba8, mip_level_count=mips))
        atlas = bt.TileAtlas.new(cfg, device)
        server = bt.AssetServer()
        paths = [f"face{s}" for s in range(6)]
        for p, face in zip(paths, rgba_faces(spec["n"])):
            server.insert(p, face)
        pre = bt.Preprocessor.new().clear_attachment(0, atlas)
        pre.preprocess_spherical(bt.SphericalDataset(attachment_index=0, paths=paths, lod_range=range(0, spec["lods"])), server, atlas)
        pre.run(atlas)
    if holes:
        for side in range(6 if spec["kind"] == "cube" else 1):
            for y, x, h, w in HOLES:
                atlas.write_region(0, hole_texels(h, w), x, y, side=side)
    return atlas


@functools.lru_cache(maxsize=None)
def oracle_tiles(spec_name):
    """the state device_atlas() leaves, made by the CPU oracle and the model of write_region: {(side, lod, x, y): tile}"""
    spec = SPECS[spec_name]
    T, b, lods, cube = spec["T"], spec["b"], spec["lods"], spec["kind"] == "cube"
    atlas = O.OracleAtlas(lods, 128, cube, [(T, b, 1, RGBA8)])
    atlas.clear_attachment(0)
    if cube:
        atlas.preprocess_spherical(0, rgba_faces(spec["n"]), (0, lods)).run(4)
    else:
        atlas.preprocess_tile(0, rgba_source(spec["n"]), (0, lods), **spec.get("extent", {})).run(4)
    tiles = {coord: atlas.tile(0, i) for coord, i in atlas.tiles()}
    for side in range(6 if cube else 1):
        for y, x, h, w in HOLES:
            tiles = EM.write_region(tiles, lods - 1, side, x, y, hole_texels(h, w), b)
    return EM.propagate(tiles, b, cube)


# ---------------------------------------------------------------------------------------------- the cases

RED, TEAL = (0.9, 0.2, 0.4, 1.0), (0.1, 0.7, 0.6, 0.3)


def Paint(stamps, lod=None, reach=()):
    """one bt_atlas_paint call; reach: "zero_rule", "holes", or a name of test_gpu_edit_shapes.branches_reached"""
    return dict(stamps=stamps, lod=lod, reach=set(reach))


def stamps_256():
    """mixed modes, falloffs and masks, radii of 0.75 .. 3 texels, colours and deltas in [-1, 2]; one over the hole block"""
    rng = np.random.default_rng(21)
    stamps = []
    for k in range(MAX_STAMPS):
        cx, cy = (rng.integers(0, 48 * 4, size=2) / 4.0).tolist()
        colour = tuple((rng.integers(-8, 17, size=4) / 8.0).tolist())
        stamps.append(P((cx, cy), float(rng.integers(3, 13)) / 4.0, colour, opacity=float(rng.integers(1, 9)) / 8.0, mode="add" if k % 3 else "blend",
                        falloff="hard" if k % 4 == 1 else "smooth", channels=int(rng.integers(1, 16))))
    stamps[17] = P((16.0, 7.0), 5.0, RED, opacity=0.5)
    return stamps


WHOLE_72 = {"edit_second_trip", "edit_second_row_block", "parent_second_trip", "parent_second_row_block"}

CASES = {
    # 1. planar, T = 16, b = 2 (c = 12), lod_count 3: a mosaic of 48 x 48
    "inside_one_tile": ("planar_b2", [Paint([P((5.0, 6.0), 2.5, RED, opacity=0.8)])]),
    "four_tile_corner_fractional": ("planar_b2", [Paint([P((12.3, 11.6), 3.5, TEAL, opacity=0.6)])]),
    "mosaic_corner_and_edge": ("planar_b2", [Paint([P((0.5, 47.0), 5.0, RED)])]),
    "blend_then_add_different_masks": ("planar_b2", [Paint([P((20.0, 20.0), 6.0, RED, opacity=0.7, channels="rg"),
                                                           P((23.0, 21.0), 5.0, (0.3, -0.2, 0.25, -0.5), mode="add", channels="gba")])]),
    "larger_than_the_mosaic": ("planar_b2", [Paint([P((24.0, 24.0), 100.0, TEAL, opacity=0.3)], reach={"holes"})]),
    "hard_falloff": ("planar_b2", [Paint([P((30.5, 13.5), 4.0, TEAL, opacity=0.5, falloff="hard")])]),
    "over_the_hole_block": ("planar_b2", [Paint([P((16.0, 7.0), 5.0, RED, opacity=0.9)], reach={"holes"})]),
    "saturating_add": ("planar_b2", [Paint([P((8.0, 40.0), 3.0, (2.0, 2.0, 2.0, 2.0), mode="add", falloff="hard"),
                                           P((40.0, 8.0), 3.0, (-2.0, -2.0, -2.0, -2.0), mode="add", falloff="hard")], reach={"zero_rule"})]),
    "blend_to_black": ("planar_b2", [Paint([P((24.0, 30.0), 9.5, (0.0, 0.0, 0.0, 1.0), falloff="hard")], reach={"zero_rule"}),
                                     Paint([P((24.0, 12.0), 12.0, (-1.0, -1.0, -1.0, 0.0), opacity=0.5, mode="add", channels="rgb")], reach={"zero_rule", "holes"})]),
    "alpha_only_mask": ("planar_b2", [Paint([P((30.0, 30.0), 5.0, (0.0, 0.0, 0.0, 0.25), falloff="hard", channels="a")])]),
    "single_channel_mask": ("planar_b2", [Paint([P((36.5, 20.5), 4.5, (0.0, 1.0, 0.0, 0.0), channels="g")])]),
    # 2. an odd border: c = 14, child quadrants of 7 texels
    "odd_border": ("planar_b1", [Paint([P((14.3, 13.6), 3.5, RED, opacity=0.6)]),
                                 Paint([P((27.0, 29.0), 2.0, TEAL, falloff="hard"), P((16.0, 7.0), 5.0, RED, mode="add", opacity=0.25)], reach={"holes"})]),
    # 3. T = 72, b = 2 (c = 68): rows beyond one trip of the 64 lanes, rectangles beyond one row block of 16, at the edited LOD and the parents
    "beyond_one_block": ("planar_72", [Paint([P((136.0, 136.0), 1088.0, TEAL, opacity=0.3)], reach=WHOLE_72 | {"holes"}),
                                       # texels 1 .. 66 of tile (1, 1): an odd origin, a second trip and five row blocks inside one tile
                                       Paint([P((101.5, 100.0), 32.0, RED, opacity=0.7, falloff="hard")], reach={"edit_second_trip", "edit_second_row_block"})]),
    # 4. cube, T = 16, b = 2, lod_count 2: every finest tile is a corner tile; mosaics of 24 x 24 (LOD 1) and 12 x 12 (LOD 0)
    "cube": ("cube", [Paint([P((0.5, 11.0), 4.0, RED, opacity=0.8, side=0)], reach={"corner_tile"}),        # a face edge of an even side
                      Paint([P((22.0, 23.0), 3.5, TEAL, side=3), P((1.0, 1.0), 3.0, RED, side=3, falloff="hard")], reach={"corner_tile"}),  # of an odd side
                      Paint([P((12.0, 0.0), 5.0, RED, opacity=0.5, side=4), P((0.0, 12.0), 5.0, TEAL, mode="add", opacity=0.5, side=1),
                             P((16.0, 7.0), 5.0, RED, opacity=0.6, side=2)], reach={"holes"}),
                      Paint([P((11.5, 12.5), 4.0, TEAL, opacity=0.7, side=5)], lod=1),
                      Paint([P((6.0, 0.5), 3.0, RED, opacity=0.7, side=2)], lod=0)]),
    # 5. the plan
    "missing_tiles": ("partial", [Paint([P((13.0, 15.0), 5.0, RED)]), Paint([P((30.0, 30.0), 6.0, TEAL, opacity=0.5)])]),
    "below_the_finest_lod": ("planar_b2", [Paint([P((11.5, 12.5), 4.0, RED, opacity=0.8)], lod=1)]),
    "256_stamps": ("planar_b2", [Paint(stamps_256(), reach={"256_stamps", "holes"})]),
}
PLANAR_B2 = ["inside_one_tile", "four_tile_corner_fractional", "mosaic_corner_and_edge", "blend_then_add_different_masks", "larger_than_the_mosaic",
             "hard_falloff", "over_the_hole_block", "saturating_add", "blend_to_black", "alpha_only_mask", "single_channel_mask"]


def edit_reaches(spec, edit, existing):
    """the names of test_gpu_edit_shapes.branches_reached for one paint call on an atlas that holds `existing`"""
    c = spec["T"] - 2 * spec["b"]
    lod = spec["lods"] - 1 if edit["lod"] is None else edit["lod"]
    boxes = stamp_boxes(edit["stamps"], lod, c)
    levels = plan_levels(boxes, lod, c, existing)
    return branches_reached(boxes, levels, lod, c, spec["b"], RGBA8, existing, spec["kind"] == "cube", edit["stamps"])


def model_paint(tiles, spec, edit, reached):
    """the model's tiles after one paint call: the stamps on the tiles of its LOD, then F over the LODs up to it"""
    lod = spec["lods"] - 1 if edit["lod"] is None else edit["lod"]
    coarse = {k: v for k, v in tiles.items() if k[1] <= lod}
    out = dict(tiles)
    out.update(EM.propagate(PM.apply_paint(coarse, lod, edit["stamps"], spec["b"], reached), spec["b"], spec["kind"] == "cube"))
    return out


def assert_reached(name, n, edit, names, reached):
    shape_names = edit["reach"] - {"zero_rule", "holes"}
    assert shape_names <= names, (name, n, sorted(shape_names - names))
    if "zero_rule" in edit["reach"]:
        assert reached.get("zero_rule", 0) >= 1, (name, n, reached)
    if "holes" in edit["reach"]:
        assert reached.get("holes_under_disc", 0) >= 1, (name, n, reached)


@pytest.mark.parametrize("name", list(CASES))
def test_cases_reach_their_branches(name):
    """no GPU: what the GPU cases assert of their inputs, on the oracle's state of the same jobs"""
    spec_name, edits = CASES[name]
    spec = SPECS[spec_name]
    b = spec["b"]
    tiles = oracle_tiles(spec_name)
    assert any((t[b:-b, b:-b, :3] == 0).all(axis=-1).any() for k, t in tiles.items() if k[1] == spec["lods"] - 1), "no no-data texel was planted"
    for n, edit in enumerate(edits):
        reached = {}
        after = model_paint(tiles, spec, edit, reached)
        assert_reached(name, n, edit, edit_reaches(spec, edit, set(tiles)), reached)
        changed_texels = sum(int((tiles[k][b:-b, b:-b] != after[k][b:-b, b:-b]).any(axis=-1).sum()) for k in tiles)
        assert changed_texels >= 1, (name, n, "the paint changes nothing")
        holes_before = {k: (t[..., :3] == 0).all(axis=-1) for k, t in tiles.items() if k[1] == spec["lods"] - 1}
        assert all(np.array_equal(h, (after[k][..., :3] == 0).all(axis=-1)) for k, h in holes_before.items()), "the hole mask of the finest tiles changed"
        tiles = after


# ---------------------------------------------------------------------------------------------- running a case on the device

def paint_and_check(atlas, stamps, lod=None):
    """test_gpu_edit.edit_and_check for bt_atlas_paint; returns (before, after, changed, stats, what the model reached)"""
    b, c, spherical = geometry(atlas)
    lod = atlas.lod_count - 1 if lod is None else lod
    before = Snapshot(atlas)
    held = EM.propagate(before.tiles, b, spherical)
    assert all(np.array_equal(held[k], before.tiles[k]) for k in before.tiles), "the state before the paint is not F of its primary centres"
    changed, stats = atlas.paint(0, stamps, lod)
    coarse = {k: v for k, v in before.tiles.items() if k[1] <= lod}  # tiles finer than `lod` are not touched
    reached = {}
    expected = dict(before.tiles)
    expected.update(EM.propagate(PM.apply_paint(coarse, lod, stamps, b, reached), b, spherical))
    edited = EM.stamp_tiles(stamps, lod, c)
    levels = ancestors_levels(before, edited)
    after = check_edit(atlas, before, expected, changed, stats, edited, levels)
    if atlas.config.attachments[0].mip_level_count == 1:
        assert stats["layers_mipped"] == 0 and stats["launches"] == (1 + levels + (1 if b else 0) if stats["tiles_edited"] else 0)
    return before, after, changed, stats, reached


def run_case(device, name, atlas=None):
    spec_name, edits = CASES[name]
    spec = SPECS[spec_name]
    atlas = atlas or device_atlas(device, spec_name)
    results = []
    for n, edit in enumerate(edits):
        existing = {(c.side, c.lod, c.x, c.y) for c, _ in atlas.tiles()}
        before, after, changed, stats, reached = paint_and_check(atlas, edit["stamps"], edit["lod"])
        assert_reached(name, n, edit, edit_reaches(spec, edit, existing), reached)
        if stats["tiles_edited"]:
            assert sum(1 for k in before.tiles if not np.array_equal(before.tiles[k], after.tiles[k])) >= 1, "the paint changed nothing: the comparison would be empty"
        results.append((before, after, changed, stats))
    return atlas, results


def centres(snapshot, lod, b):
    return {k: v[b:-b, b:-b] for k, v in snapshot.tiles.items() if k[1] == lod}


# ---------------------------------------------------------------------------------------------- 1. planar, T = 16, b = 2

@pytest.mark.gpu
@pytest.mark.parametrize("name", PLANAR_B2)
def test_planar_stamps(device, name):
    atlas, results = run_case(device, name)
    before, after, changed, stats = results[0]
    old, new = centres(before, 2, 2), centres(after, 2, 2)
    assert all(np.array_equal((old[k][..., :3] == 0).all(axis=-1), (new[k][..., :3] == 0).all(axis=-1)) for k in old), "the hole mask changed"
    if name == "inside_one_tile":
        assert stats["tiles_edited"] == 1 and stats["tiles_downsampled"] == 2 and stats["launches"] == 4 and stats["tiles_with_children"] == 0
    if name == "larger_than_the_mosaic":
        assert stats["tiles_edited"] == 16 and stats["changed_count"] == 21 and stats["tiles_downsampled"] == 5
    if name == "saturating_add":
        assert (new[(0, 2, 0, 3)] == 255).all(axis=-1).sum() >= 9 and (new[(0, 2, 3, 0)] == (1, 1, 1, 0)).all(axis=-1).sum() >= 9
    if name == "alpha_only_mask":
        assert all(np.array_equal(old[k][..., :3], new[k][..., :3]) for k in old) and any(not np.array_equal(old[k][..., 3], new[k][..., 3]) for k in old)
    if name == "single_channel_mask":
        assert all(np.array_equal(old[k][..., (0, 2, 3)], new[k][..., (0, 2, 3)]) for k in old)


# ---------------------------------------------------------------------------------------------- 2. an odd border, 3. beyond one block

@pytest.mark.gpu
def test_odd_border(device):
    run_case(device, "odd_border")


@pytest.mark.gpu
def test_rows_beyond_one_lane_trip_and_row_block(device):
    atlas, results = run_case(device, "beyond_one_block")
    assert results[0][3]["tiles_edited"] == 16 and results[1][3]["tiles_edited"] == 1


# ---------------------------------------------------------------------------------------------- 4. cube

@pytest.mark.gpu
def test_cube(device):
    """all 30 tiles compared after every call: the seams to the neighbouring faces go through project_to_side, and a stamp stops at its face"""
    atlas, results = run_case(device, "cube")
    assert len(atlas.tiles()) == 30
    for (before, after, changed, stats), side in zip(results[:2], (0, 3)):
        assert {t.side for t in changed} - {side}, "no tile of a neighbouring face was re-stitched"
        differing = {k[0] for k in before.tiles if not np.array_equal(before.tiles[k][2:-2, 2:-2], after.tiles[k][2:-2, 2:-2])}
        assert differing == {side}, "a centre texel of another face changed"
    assert results[2][3]["tiles_edited"] >= 3 and {t.side for t in results[2][2]} >= {1, 2, 4}
    before, after, changed, stats = results[4]
    assert all(t.lod == 0 for t in changed) and stats["tiles_with_children"] == stats["tiles_edited"] == 1
    assert all(np.array_equal(before.tiles[k], after.tiles[k]) for k in before.tiles if k[1] == 1)


# ---------------------------------------------------------------------------------------------- 5. the plan

@pytest.mark.gpu
def test_missing_tiles_are_skipped_and_counted(device):
    atlas, results = run_case(device, "missing_tiles")
    index = set(results[0][0].index)
    assert (0, 2, 1, 1) in index and (0, 2, 0, 0) not in index and (0, 2, 0, 1) not in index and len(index) < 21
    assert results[0][3]["tiles_missing"] == 3 and results[0][3]["tiles_edited"] == 1
    before, after, changed, stats, _ = paint_and_check(atlas, [P((3.0, 3.0), 2.0, RED)])  # only absent tiles
    assert stats["tiles_missing"] == 1 and stats["tiles_edited"] == 0 and stats["launches"] == 0 and changed == []


@pytest.mark.gpu
def test_paint_below_the_finest_lod_leaves_finer_tiles(device):
    atlas, [(before, after, changed, stats)] = run_case(device, "below_the_finest_lod")
    assert stats["tiles_edited"] == 4 and stats["tiles_with_children"] == 4 and stats["tiles_downsampled"] == 1
    assert all(t.lod <= 1 for t in changed)
    assert all(np.array_equal(before.tiles[k], after.tiles[k]) for k in before.tiles if k[1] == 2)


@pytest.mark.gpu
def test_mips_of_changed_layers_follow(device):
    atlas = device_atlas(device, "planar_b2", mips=3)
    atlas.generate_mipmaps(0)
    mips_before = {i: [atlas.download_mip(0, k, i) for k in (1, 2)] for i in range(ATLAS)}
    before, after, changed, stats, _ = paint_and_check(atlas, [P((30.0, 30.0), 4.0, RED, opacity=0.8)])
    layers = {before.index[(t.side, t.lod, t.x, t.y)] for t in changed}
    runs = sum(1 for i in layers if i - 1 not in layers)
    assert stats["layers_mipped"] == len(layers) > 0 and stats["launches"] == 1 + 2 + 1 + 2 * runs
    for i in range(ATLAS):
        got = [atlas.download_mip(0, k, i) for k in (1, 2)]
        if i in layers:
            chain = O.generate_mipmaps(RGBA8, after.data[i], 3)
            want = [chain[1024:1280].reshape(8, 8, 4), chain[1280:1344].reshape(4, 4, 4)]
            assert all(np.array_equal(g, w) for g, w in zip(got, want)), f"mips of changed layer {i}"
        else:
            assert all(np.array_equal(g, w) for g, w in zip(got, mips_before[i])), f"mips of untouched layer {i}"


@pytest.mark.gpu
def test_paint_is_ordered_behind_a_run_without_synchronising(device):
    results = []
    for sync in (False, True):
        cfg = bt.TerrainConfig(lod_count=3, atlas_size=ATLAS, path="terrains/paint", model=bt.TerrainModel.planar((0, 0, 0), 1000.0, 0.0, 1.0))
        cfg.add_attachment(bt.AttachmentConfig(name="att", texture_size=16, border_size=2, format=bt.AttachmentFormat.Rgba8))
        atlas = bt.TileAtlas.new(cfg, device)
        server = bt.AssetServer().insert("src", rgba_source(64))
        pre = bt.Preprocessor.new().clear_attachment(0, atlas).preprocess_tile(bt.PreprocessDataset(attachment_index=0, path="src", lod_range=range(0, 3)), server, atlas)
        pre.run(atlas, sync=sync)
        for k in range(3):  # back to back: the plan ring serves several calls in flight
            atlas.paint(0, [P((12.3 + 7 * k, 11.6 + 5 * k), 3.5, RED, opacity=0.5)])
            if sync:
                device.synchronize()
        results.append(atlas.download_tiles(0, 0, ATLAS))
    assert np.array_equal(results[0], results[1]) and results[0].any()
    unpainted = K.product_planar(device, rgba_source(64), 3, 16, 2, RGBA8, atlas_size=ATLAS)[0].download_tiles(0, 0, ATLAS)
    assert not np.array_equal(results[0], unpainted), "the paints changed nothing"


@pytest.mark.gpu
def test_painted_layers_count_as_written(device):
    """a paint onto allocated, never-written layers changes no texel (they hold no data) and still writes them: the fused job behind it may not
    take the layers for fresh zeros (bt_run_stats.prev_zero_launches), as it does without the paint"""
    T, b, lods, W = 128, 2, 3, 496  # source : mosaic = 1.0 -> a fused job (tests/test_gpu_prev_values.py)
    src = K.low_half(K.random_raster(RGBA8, W, W, seed=3, holes=0.01), RGBA8)
    src[118:131, 20:300, 0] = 0
    flagged = {}
    for painted in (False, True):
        cfg = bt.TerrainConfig(lod_count=lods, atlas_size=ATLAS, path="terrains/paint", model=bt.TerrainModel.planar((0, 0, 0), 1000.0, 0.0, 1.0))
        cfg.add_attachment(bt.AttachmentConfig(name="att", texture_size=T, border_size=b, format=bt.AttachmentFormat.Rgba8))
        atlas = bt.TileAtlas.new(cfg, device)
        server = bt.AssetServer().insert("src", src)
        pre = bt.Preprocessor.new().clear_attachment(0, atlas).preprocess_tile(bt.PreprocessDataset(attachment_index=0, path="src", lod_range=range(0, lods)), server, atlas)
        assert len(atlas.tiles()) == 21 and not atlas.download_tiles(0, 0, ATLAS).any()
        if painted:
            changed, stats = atlas.paint(0, [P((248.0, 248.0), 1000.0, RED)])
            assert stats["tiles_edited"] == 16 and stats["changed_count"] == 21 and not atlas.download_tiles(0, 0, ATLAS).any()
        pre.run(atlas)
        flagged[painted] = pre.stats()["prev_zero_launches"]
        oracle = O.OracleAtlas(lods, ATLAS, False, [(T, b, 1, RGBA8)])
        oracle.clear_attachment(0).preprocess_tile(0, src, (0, lods)).run(16)
        assert K.assert_atlas_equal(atlas, oracle) == 21
    assert flagged[False] >= 1 and flagged[True] == 0, flagged


@pytest.mark.gpu
def test_256_stamps_in_one_call(device):
    atlas, [(before, after, changed, stats)] = run_case(device, "256_stamps")
    assert stats["tiles_edited"] == 16


# ---------------------------------------------------------------------------------------------- 6. errors

def stamp_c(side=0, mode=0, falloff=0, mask=15, center=(5.0, 5.0), radius=2.0, opacity=0.5, color=(0.5, 0.5, 0.5, 0.5)):
    return _ffi.PaintStampC(side, mode, falloff, mask, (C.c_float * 2)(*center), radius, opacity, (C.c_float * 4)(*color))


INF, NAN = float("inf"), float("nan")
BAD_STAMPS = {
    "side 6": dict(side=6), "side 1 of a planar atlas": dict(side=1), "mode": dict(mode=2), "falloff": dict(falloff=2), "mask 0": dict(mask=0), "mask 16": dict(mask=16),
    "center nan": dict(center=(NAN, 5.0)), "center inf": dict(center=(5.0, INF)), "colour nan": dict(color=(0.5, NAN, 0.5, 0.5)),
    "colour inf": dict(color=(0.5, 0.5, 0.5, -INF)), "radius 0": dict(radius=0.0), "radius negative": dict(radius=-1.0), "radius inf": dict(radius=INF),
    "radius nan": dict(radius=NAN), "opacity 0": dict(opacity=0.0), "opacity above 1": dict(opacity=1.5), "opacity nan": dict(opacity=NAN),
    "opacity negative": dict(opacity=-0.5),
}


@pytest.mark.gpu
def test_errors_on_the_device(device):
    L = _ffi.lib()
    atlas = device_atlas(device, "planar_b2")
    before = Snapshot(atlas)
    one = (_ffi.PaintStampC * 1)(stamp_c())
    few = (_ffi.TileCoordinateC * 4)()

    def paint(h=atlas._h, ai=0, lod=2, stamps=one, count=1, changed=None, cap=0):
        return L.bt_atlas_paint(h, ai, lod, stamps, count, changed, cap, None)

    for name, fields in BAD_STAMPS.items():
        assert paint(stamps=(_ffi.PaintStampC * 2)(stamp_c(), stamp_c(**fields)), count=2) == BT_ERR_INVALID_ARGUMENT, name
    assert paint(h=None) == BT_ERR_INVALID_ARGUMENT
    assert paint(stamps=None) == BT_ERR_INVALID_ARGUMENT
    assert paint(changed=None, cap=4) == BT_ERR_INVALID_ARGUMENT
    assert paint(stamps=(_ffi.PaintStampC * 257)(*[stamp_c()] * 257), count=257) == BT_ERR_INVALID_ARGUMENT
    assert paint(ai=1) == BT_ERR_INVALID_ARGUMENT and paint(lod=3) == BT_ERR_INVALID_ARGUMENT
    assert paint(count=0) == 0 and paint(stamps=None, count=0) == 0
    changed, stats = atlas.paint(0, [])
    assert changed == [] and not any(stats.values())
    heights = planar(device, 16, 2)
    heights_before = Snapshot(heights)
    assert paint(h=heights._h) == BT_ERR_UNSUPPORTED, "paint on an R16 attachment"
    with pytest.raises(bt.BtError) as e:
        heights.paint(0, [P((5.0, 5.0), 2.0, RED)])
    assert e.value.status == BT_ERR_UNSUPPORTED
    odd = {}
    for fmt in (bt.AttachmentFormat.Rgba8, bt.AttachmentFormat.R16):
        cfg = bt.TerrainConfig(lod_count=3, atlas_size=4, path="terrains/paint", model=bt.TerrainModel.planar((0, 0, 0), 1000.0, 0.0, 1.0))
        cfg.add_attachment(bt.AttachmentConfig(name="att", texture_size=17, border_size=2, format=fmt))  # c = 13
        odd[fmt] = bt.TileAtlas.new(cfg, device)
    assert paint(h=odd[bt.AttachmentFormat.Rgba8]._h) == BT_ERR_UNSUPPORTED

    # read_region
    buf = np.full((8, 8, 4), 0xAB, np.uint8)
    missing = C.c_uint32(77)

    def read(h=atlas._h, ai=0, side=0, lod=2, x0=0, y0=0, w=4, hh=4, out=buf.ctypes.data_as(C.c_void_p), pitch=0):
        return L.bt_atlas_read_region(h, ai, side, lod, x0, y0, w, hh, out, pitch, C.byref(missing))

    assert read(h=None) == BT_ERR_INVALID_ARGUMENT and read(out=None) == BT_ERR_INVALID_ARGUMENT
    assert read(ai=1) == BT_ERR_INVALID_ARGUMENT and read(side=1) == BT_ERR_INVALID_ARGUMENT and read(lod=3) == BT_ERR_INVALID_ARGUMENT
    assert read(x0=45) == BT_ERR_INVALID_ARGUMENT and read(y0=45) == BT_ERR_INVALID_ARGUMENT  # 45 + 4 > 48
    assert read(x0=0xFFFFFFFE) == BT_ERR_INVALID_ARGUMENT and read(lod=1, x0=21) == BT_ERR_INVALID_ARGUMENT
    assert read(pitch=15) == BT_ERR_INVALID_ARGUMENT
    for fmt in odd:
        assert read(h=odd[fmt]._h) == BT_ERR_UNSUPPORTED
    for fmt in (bt.AttachmentFormat.Rg16, bt.AttachmentFormat.Rgb8):
        cfg = bt.TerrainConfig(lod_count=3, atlas_size=4, path="terrains/paint", model=bt.TerrainModel.planar((0, 0, 0), 1000.0, 0.0, 1.0))
        cfg.add_attachment(bt.AttachmentConfig(name="att", texture_size=16, border_size=2, format=fmt))
        assert read(h=bt.TileAtlas.new(cfg, device)._h) == BT_ERR_UNSUPPORTED, fmt
    assert read(w=0) == 0 and read(hh=0, out=None) == 0 and read(x0=44, y0=44) == 0  # the last texels of the mosaic are inside
    assert (buf[4:] == 0xAB).all() and (buf[:4].reshape(-1)[64:] == 0xAB).all(), "a refused or empty read wrote something"
    assert np.array_equal(Snapshot(atlas).data, before.data) and np.array_equal(Snapshot(heights).data, heights_before.data), "a refused or empty call wrote something"
    # changed_cap smaller than the count: the list is cut, the count is whole
    stats = _ffi.EditStatsC()
    wide = (_ffi.PaintStampC * 1)(stamp_c(center=(24.0, 24.0), radius=100.0))
    _ffi.check(L.bt_atlas_paint(atlas._h, 0, 2, wide, 1, few, 3, C.byref(stats)))
    assert stats.changed_count == 21 and [t.lod for t in few] == [2, 2, 2, 0]
    _ffi.check(L.bt_atlas_paint(atlas._h, 0, 2, wide, 1, None, 0, None))  # no list, no stats


# ---------------------------------------------------------------------------------------------- 7. read_region

def r16_atlas(device, T=16, b=2, **kw):
    return planar(device, T, b, **kw)


def check_reads(atlas, rects, lod=None, side=0):
    """every rectangle (x0, y0, w, h) against the model's mosaic of the downloaded layers"""
    b, c, _ = geometry(atlas)
    lod = atlas.lod_count - 1 if lod is None else lod
    snap = Snapshot(atlas)
    for x0, y0, w, h in rects:
        got, missing = atlas.read_region(0, x0, y0, w, h, lod, side)
        want, want_missing = PM.read_region(snap.tiles, lod, side, x0, y0, w, h, b)
        assert got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want), (x0, y0, w, h)
        assert missing == want_missing, (x0, y0, w, h, missing, want_missing)
        assert want.any(), "an all-zero rectangle compares nothing"
    return snap


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [R16, RGBA8], ids=["r16", "rgba8"])
@pytest.mark.parametrize("b", [2, 1])
def test_read_region(device, fmt, b):
    """the whole face, one texel, an odd origin with odd sizes across four tiles (R16: half dwords at both ends), LOD 1 and LOD 0, and a row
    pitch larger than the row"""
    atlas = planar(device, 16, b, fmt=fmt) if fmt == R16 else device_atlas(device, "planar_b2" if b == 2 else "planar_b1")
    c = 16 - 2 * b
    n = 4 * c
    snap = check_reads(atlas, [(0, 0, n, n), (c + 1, c + 3, 1, 1), (c - 5, c - 3, 11, 9), (c - 4, 1, 7, 3), (n - 1, n - 1, 1, 1), (1, 0, n - 1, 5)])
    assert (PM.read_region(snap.tiles, 2, 0, 0, 0, n, n, b)[0].reshape(n * n, -1)[:, :3] == 0).all(axis=-1).any(), "no no-data texel in the face"
    check_reads(atlas, [(0, 0, 2 * c, 2 * c), (c - 3, c - 1, 5, 4)], lod=1)
    check_reads(atlas, [(0, 0, c, c), (3, 5, 6, 1)], lod=0)
    # row_pitch: the bytes of a row behind its texels are not touched
    x0, y0, w, h = c - 5, c - 3, 11, 9
    px = 2 if fmt == R16 else 4
    pitch = w * px + 6
    buf = np.full((h, pitch), 0xAB, np.uint8)
    missing = C.c_uint32(9)
    _ffi.check(_ffi.lib().bt_atlas_read_region(atlas._h, 0, 0, 2, x0, y0, w, h, buf.ctypes.data_as(C.c_void_p), pitch, C.byref(missing)))
    want, _ = PM.read_region(snap.tiles, 2, 0, x0, y0, w, h, b)
    assert np.array_equal(buf[:, :w * px], want.view(np.uint8).reshape(h, w * px)) and (buf[:, w * px:] == 0xAB).all() and missing.value == 0
    _ffi.check(_ffi.lib().bt_atlas_read_region(atlas._h, 0, 0, 2, x0, y0, w, h, buf.ctypes.data_as(C.c_void_p), pitch, None))  # tiles_missing may be NULL


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [R16, RGBA8], ids=["r16", "rgba8"])
def test_read_region_over_absent_tiles(device, fmt):
    extent = SPECS["partial"]["extent"]
    atlas = planar(device, 16, 2, fmt=fmt, **extent) if fmt == R16 else device_atlas(device, "partial")
    index = {(c.side, c.lod, c.x, c.y) for c, _ in atlas.tiles()}
    assert (0, 2, 1, 1) in index and (0, 2, 0, 0) not in index
    got, missing = atlas.read_region(0, 0, 0, 48, 48)
    assert missing == 16 - sum(1 for k in index if k[1] == 2) > 0 and not got[:12, :12].any() and got[12:24, 12:24].any()
    check_reads(atlas, [(0, 0, 48, 48), (7, 9, 10, 9), (11, 11, 6, 6)])
    got, missing = atlas.read_region(0, 1, 2, 9, 7)  # absent tiles only: zeros, and a dirty buffer does not show through
    assert missing == 1 and not got.any()


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [R16, RGBA8], ids=["r16", "rgba8"])
def test_read_region_rows_beyond_one_lane_trip(device, fmt):
    """R16 at T = 136 (a row of 132 texels: 67 dwords), Rgba8 at T = 72 (68 dwords), rectangles taller than one row block"""
    if fmt == R16:
        atlas, c = planar(device, 136, 2, src=big_r16(4 * 132)), 132
    else:
        atlas, c = device_atlas(device, "planar_72"), 68
    check_reads(atlas, [(0, 0, 4 * c, 4 * c), (1, 3, 2 * c - 3, 41), (c + 1, c - 7, c - 2, 37)])


@pytest.mark.gpu
def test_read_region_on_a_cube_side(device):
    atlas = device_atlas(device, "cube")
    for side in (3, 4):
        check_reads(atlas, [(0, 0, 24, 24), (9, 7, 7, 9)], side=side)
    a, b = atlas.read_region(0, 0, 0, 24, 24, side=3)[0], atlas.read_region(0, 0, 0, 24, 24, side=4)[0]
    assert not np.array_equal(a, b)


@pytest.mark.gpu
def test_read_region_behind_an_unsynchronised_edit(device):
    atlas = planar(device, 16, 2)
    before = Snapshot(atlas)
    stamps = [EditStamp((12.3, 11.6), 3.5, 0.2)]
    device.synchronize()
    atlas.edit_height(0, stamps)
    got, missing = atlas.read_region(0, 6, 5, 13, 14)
    want, _ = PM.read_region(EM.apply_stamps(before.tiles, 2, stamps, 2), 2, 0, 6, 5, 13, 14, 2)
    assert np.array_equal(got, want) and missing == 0
    assert not np.array_equal(got, PM.read_region(before.tiles, 2, 0, 6, 5, 13, 14, 2)[0]), "the edit changed nothing under the rectangle"


# ---------------------------------------------------------------------------------------------- 8. undo

def clipped_box(stamp, lod, c):
    [(side, x0, y0, x1, y1)] = stamp_boxes([stamp], lod, c)
    return side, x0, y0, x1 - x0 + 1, y1 - y0 + 1


@pytest.mark.gpu
@pytest.mark.parametrize("call", ["paint", "edit_height", "smooth_height"])
def test_undo_is_exact(device, call):
    """read the stamp's clipped box, edit, write the rectangle back: every layer is byte-equal to the snapshot (the box holds no-data texels)"""
    if call == "paint":
        atlas = device_atlas(device, "planar_b2")
        stamp = P((14.5, 8.0), 6.5, RED, opacity=0.9)
        edit = lambda: atlas.paint(0, [stamp])
    elif call == "edit_height":
        atlas = planar(device, 16, 2)  # holes at mosaic rows 15 .. 17 (source rows 20 .. 23), columns 22 .. 25
        stamp = EditStamp((22.5, 14.0), 6.5, 0.2)
        edit = lambda: atlas.edit_height(0, [stamp])
    else:
        atlas = planar(device, 16, 2)
        stamp = SmoothStamp((22.5, 14.0), 6.5, 0.8)
        edit = lambda: atlas.smooth_height(0, [stamp], 2)
    b, c, _ = geometry(atlas)
    snapshot = Snapshot(atlas)
    side, x0, y0, w, h = clipped_box(stamp, 2, c)
    saved, missing = atlas.read_region(0, x0, y0, w, h, side=side)
    assert missing == 0 and (saved.reshape(h * w, -1)[:, :3] == 0).all(axis=-1).any(), "no no-data texel in the box"
    changed, stats = edit()
    edited = Snapshot(atlas)
    assert sum(1 for k in snapshot.tiles if not np.array_equal(snapshot.tiles[k], edited.tiles[k])) >= 3, "the edit changed nothing"
    atlas.write_region(0, saved, x0, y0, side=side)
    assert np.array_equal(Snapshot(atlas).data, snapshot.data)

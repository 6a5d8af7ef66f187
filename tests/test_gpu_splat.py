"""bt_atlas_splat_from_height on the device against the numpy model of its definition (tests/_splat_model.py, held to the header's lines by
tests/test_splat_model.py; propagation is _edit_model.propagate).

The atlases have two attachments: 0 is the Rgba8 target G, 1 the R16 heights H (tests/_splat_cases.py), so every comparison is the one of
tests/test_gpu_edit.py on G (its helpers are imported, not copied): all layers of G downloaded, every existing tile byte-equal to
propagate(apply_splat(before)), every layer outside `changed` byte-equal to before, `changed` inside the allowed set, the stats identities;
and every layer of H byte-equal to before.  test_splat_model.py::test_cases_reach_their_branches asserts, without a GPU, that every case
reaches the branch it is named for; run_case asserts it again on the device's own state."""
import ctypes as C
import importlib.util
import math
import os
import types

import numpy as np
import pytest

import _cases as K
import _edit_model as EM
import _oracle as O
import _render_model as RM
import _splat_cases as SC
import _splat_model as SM
import bevy_terrain_amd as bt
from _splat_cases import G, H, R
from bevy_terrain_amd import EditStamp, _ffi
from test_gpu_edit import ATLAS, Snapshot, ancestors_levels, check_edit, cube_faces, geometry

BT_ERR_INVALID_ARGUMENT, BT_ERR_UNSUPPORTED = -1, -5
INF, NAN = math.inf, math.nan
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def device():
    return bt.Device(0)


def new_atlas(device, spec, mips=1, formats=(bt.AttachmentFormat.Rgba8, bt.AttachmentFormat.R16), sizes=None, atlas_size=None):
    cube = spec["kind"] == "cube"
    cfg = bt.TerrainConfig(lod_count=spec["lods"], atlas_size=atlas_size or (128 if cube else ATLAS), path="terrains/splat", model=SC.models(spec)[0])
    for i, fmt in enumerate(formats):
        T, b = sizes[i] if sizes else (spec["T"], spec["b"])
        cfg.add_attachment(bt.AttachmentConfig(name=f"att{i}", texture_size=T, border_size=b, format=fmt, mip_level_count=mips if i == G else 1))
    return bt.TileAtlas.new(cfg, device)


def device_atlas(device, spec_name, mips=1):
    """the state _splat_cases.oracle_state() describes, on the device"""
    spec = SC.SPECS[spec_name]
    atlas = new_atlas(device, spec, mips)
    server = bt.AssetServer()
    pre = bt.Preprocessor.new().clear_attachment(G, atlas).clear_attachment(H, atlas)
    if spec["kind"] == "cube":
        for name, faces in (("g", SC.target_faces(spec)), ("h", cube_faces(spec["n"]))):
            for s, face in enumerate(faces):
                server.insert(f"{name}{s}", face)
        levels = range(0, spec["lods"])
        pre.preprocess_spherical(bt.SphericalDataset(attachment_index=G, paths=[f"g{s}" for s in range(6)], lod_range=levels), server, atlas)
        pre.preprocess_spherical(bt.SphericalDataset(attachment_index=H, paths=[f"h{s}" for s in range(6)], lod_range=levels), server, atlas)
    else:
        server.insert("g", SC.target_source(spec)).insert("h", SC.heights_source(spec))
        levels, extent = spec.get("lod_range") or range(0, spec["lods"]), spec.get("extent", {})
        pre.preprocess_tile(bt.PreprocessDataset(attachment_index=G, path="g", lod_range=levels, **extent), server, atlas)
        pre.preprocess_tile(bt.PreprocessDataset(attachment_index=H, path="h", lod_range=levels, **extent), server, atlas)
    pre.run(atlas)
    for side, x, y, zeros in SC.hole_rects(spec):
        atlas.write_region(H, zeros, x, y, side=side)
    return atlas


def heights_of(atlas, index):
    data = atlas.download_tiles(H, 0, atlas.atlas_size)
    return data, {k: data[i] for k, i in index.items()}


def splat_and_check(atlas, spec, call, name="", n=0):
    """one call and the comparisons of the module docstring; returns (before, after, changed, stats, what the model reached)"""
    b, c, spherical = geometry(atlas)
    lod, side, rect, mode, rules, fallback = SC.call_arguments(spec, call)
    before = Snapshot(atlas)
    h_data, h_tiles = heights_of(atlas, before.index)
    for tiles in (before.tiles, h_tiles):
        held = EM.propagate(tiles, b, spherical)
        assert all(np.array_equal(held[k], tiles[k]) for k in tiles), "the state before the call is not F of its primary centres"
    changed, stats = atlas.splat_from_height(H, G, rules, mode=mode, fallback=fallback, rect=call["rect"], lod=call["lod"], side=side)
    reached = {}
    expected = SC.model_call(h_tiles, before.tiles, spec, call, reached)
    SC.assert_reached(name, n, spec, call, h_tiles, reached)
    edited = SM.rect_tiles(lod, side, rect, c)
    levels = ancestors_levels(before, edited)
    after = check_edit(atlas, before, expected, changed, stats, edited, levels)
    assert np.array_equal(atlas.download_tiles(H, 0, atlas.atlas_size), h_data), "the call wrote a layer of the heights"
    if atlas.config.attachments[G].mip_level_count == 1:
        assert stats["layers_mipped"] == 0 and stats["launches"] == (1 + levels + 1 if stats["tiles_edited"] else 0)
    # the hole mask of the derived texels is the heights'
    x0, y0, w, h = rect
    for k in edited & set(before.index):
        ox, oy = k[2] * c, k[3] * c
        part = (slice(b + max(y0, oy) - oy, b + min(y0 + h, oy + c) - oy), slice(b + max(x0, ox) - ox, b + min(x0 + w, ox + c) - ox))
        assert np.array_equal((after.tiles[k][part][..., :3] == 0).all(axis=-1), h_tiles[k][part] == 0), (k, "the hole mask is not the heights'")
    return before, after, changed, stats, reached


def run_case(device, name, atlas=None, mips=1):
    spec_name, calls = SC.CASES[name]
    spec = SC.SPECS[spec_name]
    atlas = atlas or device_atlas(device, spec_name, mips)
    results = []
    for n, call in enumerate(calls):
        before, after, changed, stats, reached = splat_and_check(atlas, spec, call, name, n)
        if stats["tiles_edited"]:
            assert sum(1 for k in before.tiles if not np.array_equal(before.tiles[k], after.tiles[k])) >= 1, "the call changed nothing: the comparison would be empty"
        results.append((before, after, changed, stats, reached))
    return atlas, results


# ---------------------------------------------------------------------------------------------- 1. T = 16, b = 2 and b = 1

@pytest.mark.gpu
@pytest.mark.parametrize("name", SC.SMALL)
def test_planar_rectangles_and_rule_sets(device, name):
    atlas, results = run_case(device, name)
    before, after, changed, stats, reached = results[0]
    if name == "whole_face":
        assert stats["tiles_edited"] == 16 and stats["changed_count"] == 21 and stats["tiles_downsampled"] == 5 and stats["tiles_missing"] == 0
    if name == "one_texel":
        assert stats["tiles_edited"] == 1 and stats["tiles_downsampled"] == 2 and stats["launches"] == 4 and stats["tiles_with_children"] == 0
        texel = after.tiles[(0, 2, 1, 1)][2 + 3, 2 + 1]
        assert tuple(texel) == (77, 153, 51, 255)  # enc8 of GRASS: the one rule reaches every data texel with its whole weight
        differing = sum(int((before.tiles[k][2:-2, 2:-2] != after.tiles[k][2:-2, 2:-2]).any(axis=-1).sum()) for k in before.tiles if k[1] == 2)
        assert differing == 1
    if name == "odd_origin_over_four_tiles":
        assert stats["tiles_edited"] == 4
    if name == "one_rule":
        centres = np.concatenate([t[2:-2, 2:-2].reshape(-1, 4) for k, t in after.tiles.items() if k[1] == 2])
        assert set(map(tuple, centres.tolist())) == {(77, 153, 51, 255), (0, 0, 0, 0)}
    if name == "fallback":
        assert reached["fallback"] >= 20


@pytest.mark.gpu
def test_odd_border(device):
    run_case(device, "odd_border")


# ---------------------------------------------------------------------------------------------- 2. beyond one block of the kernel

@pytest.mark.gpu
def test_rows_beyond_one_lane_trip_row_block_and_column_chunk(device):
    atlas, results = run_case(device, "beyond_one_block")
    assert results[0][3]["tiles_edited"] == 16 and results[1][3]["tiles_edited"] == 1


@pytest.mark.gpu
def test_t136_b3(device):
    atlas, results = run_case(device, "t136_b3")
    assert results[0][3]["tiles_edited"] == 6  # columns 0 .. 2 of tile rows 0 and 1


# ---------------------------------------------------------------------------------------------- 3. cube

@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cube_lod_count_2", "cube_lod_count_3"])
def test_cube(device, name):
    """all tiles of all faces compared after every call: the taps of a face's edge texels read aprons that come through project_to_side,
    and the target's seams to the neighbouring faces are re-stitched"""
    atlas, results = run_case(device, name)
    for (before, after, changed, stats, reached), call in zip(results, SC.CASES[name][1]):
        if call["lod"] is None:
            assert {t.side for t in changed} - {call["side"]}, "no tile of a neighbouring face was re-stitched"
        differing = {k[0] for k in before.tiles if not np.array_equal(before.tiles[k][2:-2, 2:-2], after.tiles[k][2:-2, 2:-2])}
        assert differing == {call["side"]}, "a centre texel of another face changed"


# ---------------------------------------------------------------------------------------------- 4. the plan

@pytest.mark.gpu
def test_missing_tiles_are_skipped_and_counted(device):
    atlas, results = run_case(device, "missing_tiles")
    index = set(results[0][0].index)
    assert (0, 2, 1, 1) in index and (0, 2, 0, 0) not in index and len(index) < 21
    held = sum(1 for k in index if k[1] == 2)
    assert results[0][3]["tiles_missing"] == 16 - held > 0 and results[0][3]["tiles_edited"] == held
    assert results[1][3]["tiles_missing"] == 3 and results[1][3]["tiles_edited"] == 1
    before, after, changed, stats, _ = splat_and_check(atlas, SC.SPECS["partial"], SC.Call("one", rect=(1, 2, 9, 7)))  # only an absent tile
    assert stats["tiles_missing"] == 1 and stats["tiles_edited"] == 0 and stats["launches"] == 0 and changed == []


@pytest.mark.gpu
def test_chain_ends_at_a_missing_parent(device):
    atlas, [(before, after, changed, stats, _)] = run_case(device, "missing_parent")
    assert not any(k[1] == 0 for k in before.index)
    assert stats["tiles_edited"] == 4 and stats["tiles_downsampled"] == 4 and all(t.lod >= 1 for t in changed)


@pytest.mark.gpu
def test_below_the_finest_lod_leaves_finer_tiles(device):
    atlas, [(before, after, changed, stats, _)] = run_case(device, "below_the_finest_lod")
    assert stats["tiles_edited"] == 4 and stats["tiles_with_children"] == 4 and stats["tiles_downsampled"] == 1
    assert all(t.lod <= 1 for t in changed)
    assert all(np.array_equal(before.tiles[k], after.tiles[k]) for k in before.tiles if k[1] == 2)


@pytest.mark.gpu
def test_mips_of_the_target_follow(device):
    atlas = device_atlas(device, "planar_b2", mips=3)
    atlas.generate_mipmaps(G)
    mips_before = {i: [atlas.download_mip(G, k, i) for k in (1, 2)] for i in range(ATLAS)}
    before, after, changed, stats, _ = splat_and_check(atlas, SC.SPECS["planar_b2"], SC.Call("colour_eight", rect=(26, 27, 8, 7)))
    layers = {before.index[(t.side, t.lod, t.x, t.y)] for t in changed}
    runs = sum(1 for i in layers if i - 1 not in layers)
    assert stats["layers_mipped"] == len(layers) > 0 and stats["launches"] == 1 + 2 + 1 + 2 * runs
    for i in range(ATLAS):
        got = [atlas.download_mip(G, k, i) for k in (1, 2)]
        if i in layers:
            chain = O.generate_mipmaps(O.FORMAT_RGBA8, after.data[i], 3)
            want = [chain[1024:1280].reshape(8, 8, 4), chain[1280:1344].reshape(4, 4, 4)]
            assert all(np.array_equal(g, w) for g, w in zip(got, want)), f"mips of changed layer {i}"
        else:
            assert all(np.array_equal(g, w) for g, w in zip(got, mips_before[i])), f"mips of untouched layer {i}"


# ---------------------------------------------------------------------------------------------- 5. behind an edit of the heights

@pytest.mark.gpu
def test_rederive_behind_an_unsynchronised_edit_height(device):
    """derive the whole face, raise the ground under a stamp, and re-derive the stamp's box widened by the reach of the taps, all three
    queued without a wait in between: G equals the model of the calls in their order, and that is the model's derivation of the WHOLE face
    from the edited heights: the widened box re-derives everything the edit invalidated"""
    spec = SC.SPECS["planar_b2"]
    b, c, lod = 2, 12, 2
    mode, rules = SC.RULES["colour_eight"]
    stamp = EditStamp((22.0, 14.0), 6.25, 0.3, falloff="hard")
    reach = 16 // (2 * 12) + 2  # REACH of the header: T / (2c) + 2
    x0, y0, x1, y1 = int(math.floor(22.0 - 6.25)) - reach, int(math.floor(14.0 - 6.25)) - reach, int(math.ceil(22.0 + 6.25)) + reach, int(math.ceil(14.0 + 6.25)) + reach
    box = (x0, y0, x1 - x0 + 1, y1 - y0 + 1)
    assert x0 >= 0 and y0 >= 0 and x1 < 48 and y1 < 48
    atlas = device_atlas(device, "planar_b2")
    before = Snapshot(atlas)
    h_data, h_tiles = heights_of(atlas, before.index)
    device.synchronize()
    atlas.splat_from_height(H, G, rules, mode=mode)
    atlas.edit_height(H, [stamp])
    changed, stats = atlas.splat_from_height(H, G, rules, mode=mode, rect=box)
    edited_heights = EM.propagate(EM.apply_stamps(h_tiles, lod, [stamp], b), b, False)
    assert sum(1 for k in h_tiles if not np.array_equal(h_tiles[k], edited_heights[k])) >= 3, "the stamp changed nothing"
    got_h = heights_of(atlas, before.index)[1]
    assert all(np.array_equal(got_h[k], edited_heights[k]) for k in got_h)
    first = SC.model_call(h_tiles, before.tiles, spec, SC.Call("colour_eight"))
    second = SC.model_call(edited_heights, first, spec, SC.Call("colour_eight", rect=box))
    after = Snapshot(atlas)
    assert all(np.array_equal(after.tiles[k], second[k]) for k in second), "the queued calls differ from the model of both"
    whole = SC.model_call(edited_heights, before.tiles, spec, SC.Call("colour_eight"))
    assert sum(1 for k in whole if not np.array_equal(first[k], whole[k])) >= 3, "the edit invalidated nothing"
    assert all(np.array_equal(second[k], whole[k]) for k in whole), "the box widened by the reach left a stale texel"
    assert stats["tiles_edited"] == len(SM.rect_tiles(lod, 0, box, c))


# ---------------------------------------------------------------------------------------------- 6. refusals

def rule_c(**fields):
    values = dict(height_lo=-INF, height_hi=INF, height_fade=0.0, steep_lo=-INF, steep_hi=INF, steep_fade=0.0, weight=1.0, colour=(0.5, 0.5, 0.5))
    values.update(fields)
    colour = values.pop("colour")
    return _ffi.SplatRuleC(colour=(C.c_float * 3)(*colour), **values)


BAD_RULES = {
    "height_lo nan": dict(height_lo=NAN), "steep_hi nan": dict(steep_hi=NAN), "height_fade nan": dict(height_fade=NAN), "weight nan": dict(weight=NAN),
    "colour nan": dict(colour=(0.5, NAN, 0.5)), "colour inf": dict(colour=(INF, 0.5, 0.5)), "height lo > hi": dict(height_lo=2.0, height_hi=1.0),
    "steep lo > hi": dict(steep_lo=0.5, steep_hi=0.25), "height_fade negative": dict(height_fade=-1.0), "steep_fade inf": dict(steep_fade=INF),
    "weight negative": dict(weight=-1.0), "weight inf": dict(weight=INF),
}
SENTINEL = 0xA5A5A5A5


@pytest.mark.gpu
def test_refusals_leave_everything_untouched(device):
    L = _ffi.lib()
    spec = SC.SPECS["planar_b2"]
    atlas = device_atlas(device, "planar_b2")
    before = Snapshot(atlas)
    h_before = atlas.download_tiles(H, 0, ATLAS)
    from bevy_terrain_amd.tile_tree import model_c
    model = model_c(atlas.config.model)
    one = (_ffi.SplatRuleC * 8)(*[rule_c() for _ in range(8)])
    fallback = (C.c_uint8 * 4)(1, 2, 3, 4)

    def call(h=atlas._h, hi=H, gi=G, model=C.byref(model), side=0, lod=2, x0=0, y0=0, w=4, hh=4, mode=_ffi.SPLAT_COLOUR, rules=one, count=1, fallback=fallback, cap=4,
             null_changed=False):
        changed = (_ffi.TileCoordinateC * 4)(*[_ffi.TileCoordinateC(SENTINEL, SENTINEL, SENTINEL, SENTINEL) for _ in range(4)])
        stats = _ffi.EditStatsC(*([7] * 8))
        status = L.bt_atlas_splat_from_height(h, hi, gi, model, side, lod, x0, y0, w, hh, mode, rules, count, fallback, None if null_changed else changed, cap, C.byref(stats))
        if status != 0:
            assert all(t.side == SENTINEL and t.lod == SENTINEL and t.x == SENTINEL and t.y == SENTINEL for t in changed), "a refused call wrote `changed`"
            assert not any(getattr(stats, name) for name, _ in _ffi.EditStatsC._fields_), "a refused call left stats"
        return status

    invalid = dict(
        null_atlas=dict(h=None), null_model=dict(model=None), null_rules=dict(rules=None), null_fallback=dict(fallback=None), null_changed=dict(null_changed=True),
        count_0=dict(count=0), count_9=dict(count=9), weights_count_5=dict(mode=_ffi.SPLAT_WEIGHTS, count=5), mode_2=dict(mode=2),
        same_attachment=dict(hi=G, gi=G), same_attachment_heights=dict(hi=H, gi=H), height_out_of_range=dict(hi=2), target_out_of_range=dict(gi=2),
        model_kind=dict(model=C.byref(_ffi.TerrainModelC(kind=3, a=1000.0))), model_axis=dict(model=C.byref(_ffi.TerrainModelC(kind=0, a=-1.0))),
        side_1_of_a_planar_atlas=dict(side=1), lod_3=dict(lod=3), past_the_right_edge=dict(x0=45), past_the_bottom_edge=dict(y0=45), wraps=dict(x0=0xFFFFFFFE),
        past_the_mosaic_of_lod_1=dict(lod=1, x0=21))
    for name, kw in invalid.items():
        assert call(**kw) == BT_ERR_INVALID_ARGUMENT, name
    for name, fields in BAD_RULES.items():
        assert call(rules=(_ffi.SplatRuleC * 2)(rule_c(), rule_c(**fields)), count=2) == BT_ERR_INVALID_ARGUMENT, name
    # the formats and the shapes
    assert call(hi=G, gi=H) == BT_ERR_UNSUPPORTED, "G not Rgba8 (and H not R16)"
    fmt = bt.AttachmentFormat
    both_colour = new_atlas(device, spec, formats=(fmt.Rgba8, fmt.Rgba8), atlas_size=4)
    assert call(h=both_colour._h) == BT_ERR_UNSUPPORTED, "H not R16"
    both_heights = new_atlas(device, spec, formats=(fmt.R16, fmt.R16), atlas_size=4)
    assert call(h=both_heights._h) == BT_ERR_UNSUPPORTED, "G not Rgba8"
    for sizes, why in ((((16, 2), (20, 2)), "texture_size differs"), (((16, 2), (16, 1)), "border_size differs"), (((16, 0), (16, 0)), "border_size 0"),
                       (((17, 2), (17, 2)), "an odd centre size")):
        assert call(h=new_atlas(device, spec, sizes=sizes, atlas_size=4)._h, w=1, hh=1) == BT_ERR_UNSUPPORTED, why
    huge = new_atlas(device, dict(spec, lods=31), sizes=((16, 2), (16, 2)), atlas_size=4)
    assert call(h=huge._h, lod=30) == BT_ERR_UNSUPPORTED, "a mosaic beyond 2^32 texels"
    with pytest.raises(bt.BtError) as e:
        atlas.splat_from_height(G, H, [R()])
    assert e.value.status == BT_ERR_UNSUPPORTED
    # nothing to do: BT_OK, nothing touched
    assert call(w=0) == 0 and call(hh=0) == 0 and call(w=0, x0=48) == 0 and call(cap=0, null_changed=True, w=0) == 0
    assert np.array_equal(Snapshot(atlas).data, before.data) and np.array_equal(atlas.download_tiles(H, 0, ATLAS), h_before), "a refused or empty call wrote something"
    # the last texels of the mosaic are inside; changed_cap smaller than the count: the list is cut, the count is whole; no list, no stats
    assert call(x0=44, y0=44) == 0
    few = (_ffi.TileCoordinateC * 3)()
    stats = _ffi.EditStatsC()
    _ffi.check(L.bt_atlas_splat_from_height(atlas._h, H, G, C.byref(model), 0, 2, 0, 0, 48, 48, _ffi.SPLAT_COLOUR, one, 8, fallback, few, 3, C.byref(stats)))
    assert stats.changed_count == 21 and stats.tiles_edited == 16 and [t.lod for t in few] == [2, 2, 2]
    _ffi.check(L.bt_atlas_splat_from_height(atlas._h, H, G, C.byref(model), 0, 2, 0, 0, 48, 48, _ffi.SPLAT_WEIGHTS, one, 4, fallback, None, 0, None))
    assert np.array_equal(atlas.download_tiles(H, 0, ATLAS), h_before)


# ---------------------------------------------------------------------------------------------- 7. T = 512

@pytest.mark.gpu
def test_t512_on_the_changed_tiles(device):
    """T = 512, b = 2 (c = 508), lod_count 2: eight column chunks and 32 row blocks per tile; the tiles of `changed` against the model"""
    T, b, lods = 512, 2, 2
    c = T - 2 * b
    spec = dict(kind="planar", T=T, b=b, lods=lods, n=2 * c)
    atlas = new_atlas(device, spec, atlas_size=8)
    heights = K.smooth_raster(2 * c, 2 * c, seed=9, device=device)
    heights[700:720, 300:340] = 0
    server = bt.AssetServer().insert("h", heights)
    pre = bt.Preprocessor.new().clear_attachment(G, atlas).clear_attachment(H, atlas)
    pre.preprocess_tile(bt.PreprocessDataset(attachment_index=H, path="h", lod_range=range(0, lods)), server, atlas).run(atlas)
    index = {(t.side, t.lod, t.x, t.y): i for t, i in atlas.tiles()}
    h_data = atlas.download_tiles(H, 0, 8)
    h_tiles = {k: h_data[i] for k, i in index.items()}
    g_before = atlas.download_tiles(G, 0, 8)
    assert len(index) == 5 and not g_before.any()
    call = SC.Call("colour_eight", rect=(201, 97, 650, 700))
    mode, rules = SC.RULES["colour_eight"]
    changed, stats = atlas.splat_from_height(H, G, rules, mode=mode, rect=call["rect"])
    assert stats["tiles_edited"] == 4 and stats["changed_count"] == 5 and stats["launches"] == 3
    reached = {}
    expected = SC.model_call(h_tiles, {k: g_before[i] for k, i in index.items()}, spec, call, reached)
    assert reached["holes"] >= 100 and reached["mixed"] >= 1000 and reached["data"] > 400000
    g_after = atlas.download_tiles(G, 0, 8)
    for t in changed:
        k = (t.side, t.lod, t.x, t.y)
        assert np.array_equal(g_after[index[k]], expected[k]), (k, np.argwhere((g_after[index[k]] != expected[k]).any(axis=-1))[:4])
    assert np.array_equal(atlas.download_tiles(H, 0, 8), h_data)


# ---------------------------------------------------------------------------------------------- 8. the example

@pytest.mark.gpu
def test_example_picture_is_the_render_model_over_the_model_texture(device):
    """examples/procedural_texture.py at a small size: its albedo attachment is the model's derivation from its heights, and its picture is
    tests/_render_model.py's render of those heights with the MODEL's albedo"""
    spec = importlib.util.spec_from_file_location("procedural_texture", os.path.join(ROOT, "examples", "procedural_texture.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    T, lods = 16, 3
    made = example.run(device, texture_size=T, lod_count=lods, width=24, height=16)
    atlas, b = made.tile_atlas, example.BORDER_SIZE
    assert made.stats["tiles_edited"] == 16 and made.stats["changed_count"] == 21
    index = {(t.side, t.lod, t.x, t.y): i for t, i in atlas.tiles()}
    h_data, g_data = atlas.download_tiles(example.HEIGHT, 0, atlas.atlas_size), atlas.download_tiles(example.ALBEDO, 0, atlas.atlas_size)
    omodel = O.make_model("planar", (0, 0, 0), example.TERRAIN_SIZE, 0.0, example.MIN_HEIGHT, example.MAX_HEIGHT)
    h_tiles = {k: h_data[i] for k, i in index.items()}
    n = (T - 2 * b) << (lods - 1)
    derived = SM.apply_splat(h_tiles, {k: np.zeros((T, T, 4), np.uint8) for k in index}, omodel, lods - 1, 0, (0, 0, n, n), "colour", example.RULES, example.FALLBACK, b)
    model_g = EM.propagate(derived, b, False)
    assert all(np.array_equal(g_data[i], model_g[k]) for k, i in index.items())
    assert len({tuple(t) for t in derived[(0, 2, 1, 1)][b:-b, b:-b].reshape(-1, 4).tolist()}) >= 20, "the texture is one colour"
    # the picture: the oracle's tree with the device tree's entries
    kw = dict(tree_size=4, load_distance=1.2, blend_distance=1.0)
    otree = O.TileTree(omodel, lods, O.make_view_config(**kw))
    otree.update(made.view_position)
    otree.set_entries(made.tile_tree.read()[0])
    approximate_height = made.tile_tree.view_state().approximate_height
    otree.set_approximate_height(approximate_height)
    cam = made.camera
    scene = types.SimpleNamespace(omodel=omodel, otree=otree, approximate_height=approximate_height, T=T, B=b, layers={i: h_data[i] for i in index.values()},
                                  albedo_T=T, albedo_B=b, albedo_layers={i: model_g[k] for k, i in index.items()})
    c = RM.camera(cam.origin, cam.forward, cam.right, cam.up, cam.width, cam.height, cam.t_min, cam.t_max, lighting=cam.lighting, sun=cam.sun, ambient=cam.ambient,
                  background=cam.background, albedo=example.ALBEDO)
    exp = RM.render(scene, c, made.steps, made.refine_rounds)
    assert exp.stats["hit_pixels"] >= 100, exp.stats
    assert made.image["rgba"].tobytes() == exp.rgba.tobytes(), np.argwhere((made.image["rgba"] != exp.rgba).any(axis=-1))[:8]
    assert made.image["stats"] == exp.stats
    assert len({tuple(p) for p in exp.rgba.reshape(-1, 4).tolist()}) >= 30, "the picture is one colour"

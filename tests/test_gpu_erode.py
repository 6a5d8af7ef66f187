"""bt_atlas_erode_height on the device against the numpy model of its definition (tests/_erode_model.py, held to the header's lines by
tests/test_erode_model.py; propagation is _edit_model.propagate).

Every case (tests/_erode_cases.py) writes its texels over its window with write_region, reads them back (the state the model was given),
runs the call and then compares: the window's texels byte for byte and the water and sediment planes bit for bit with the model's; ALL
layers of the attachment with F of those texels by the comparisons of tests/test_gpu_edit.py (its helpers are imported, not copied);
and the whole atlas, `changed` and bt_edit_stats with a twin atlas that received the same texels through write_region.  The model has no
blocks: windows of one block less one, one block, two blocks and one, and a hole on the corner of four blocks show that the result does
not depend on the block size, which is taken from the binding."""
import ctypes as C
import math

import numpy as np
import pytest

import _cases as K
import _edit_model as EM
import _erode_cases as EC
import _erode_model as M
import _oracle as O
import bevy_terrain_amd as bt
from bevy_terrain_amd import ErosionParams, _ffi
from test_gpu_edit import ATLAS, Snapshot, ancestors_levels, check_edit, cube, geometry, planar

BT_ERR_INVALID_ARGUMENT, BT_ERR_UNSUPPORTED = -1, -5
INF, NAN = math.inf, math.nan


@pytest.fixture(scope="module")
def device():
    return bt.Device(0)


def build(device, kind):
    if kind == "t16":
        return planar(device, 16, 2)
    if kind == "t72_l":  # two jobs: x from 0.3 on, then y from 0.3 on: of the finest tiles only (0, 0) stays absent
        atlas = planar(device, 72, 2, top_left=(0.3, 0.0), bottom_right=(1.0, 1.0), then=[(range(0, 3), dict(top_left=(0.0, 0.3), bottom_right=(1.0, 1.0)))])
        index = {(c.side, c.lod, c.x, c.y) for c, _ in atlas.tiles()}
        assert {k for k in EM.region_tiles(2, 0, 0, 0, 272, 272, 68) if k not in index} == set(EC.KINDS[kind]["absent"])
        face, _ = atlas.read_region(0, 0, 0, 272, 272)  # the second job wrote over parts of the first's tiles: a write of the whole face makes the state F again
        atlas.write_region(0, face, 0, 0)
        return atlas
    return cube(device)


@pytest.fixture(scope="module")
def atlases(device):
    """per kind a pair of atlases built alike, made on first use: the one the call runs on and its twin, which gets every texel through write_region"""
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = (build(device, kind), build(device, kind))
        return made[kind]

    return get


def bits(plane):
    return np.ascontiguousarray(plane, dtype=np.float32).view(np.uint32)


def call(atlas, case, weight=None, water=None, sediment=None, **overrides):
    x0, y0, w, h = case["rect"]
    return atlas.erode_height(0, x0, y0, w, h, ErosionParams(**dict(case["params"], **overrides)), weight=weight, water=water, sediment=sediment, side=case["side"])


def same_floats(got, want):
    """bit for bit, a NaN standing for any NaN (the header leaves a NaN's sign and payload open)"""
    return (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))


def run_named(atlases, name):
    return run_case(atlases, EC.CASES[name], EC.texels(name), EC.inputs(name), EC.expected(name)[:5], name)


def run_case(atlases, case, texels, inputs, expected, name=""):
    """the comparisons of the module docstring for one call: case (of _erode_cases.Case), the texels written over the window first, (weight,
    water, sediment) and the model's (raw, tiles_missing, new texels, water, sediment); returns (before, after, changed, stats, water, sediment)"""
    atlas, twin = atlases(case["kind"])
    b, c, spherical = geometry(atlas)
    kind, lod, _ = EC.geometry(case)
    x0, y0, w, h = case["rect"]
    side = case["side"]
    weight, water, sediment = inputs
    raw, missing, new, d, s = expected
    for a in (atlas, twin):
        a.write_region(0, texels, x0, y0, side=side)
    got_raw, got_missing = atlas.read_region(0, x0, y0, w, h, side=side)
    assert np.array_equal(got_raw, raw) and got_missing == missing, "the device atlas is not the state the model was given"
    before = Snapshot(atlas)
    held = EM.propagate(before.tiles, b, spherical)
    assert all(np.array_equal(held[k], before.tiles[k]) for k in before.tiles), "the state before the call is not F of its primary centres"

    changed, stats, water_out, sediment_out = call(atlas, case, weight=weight, water=water, sediment=sediment)

    got_new, _ = atlas.read_region(0, x0, y0, w, h, side=side)
    differ = np.argwhere(got_new != new)
    assert differ.size == 0, (name, len(differ), differ[:5], got_new[tuple(differ[0])], new[tuple(differ[0])], raw[tuple(differ[0])])
    for got, want, given in ((water_out, d, water), (sediment_out, s, sediment)):
        if given is None:
            assert got is None
        else:
            off = np.argwhere(~same_floats(got, want))
            assert off.size == 0, (name, len(off), off[:5], got[tuple(off[0])], want[tuple(off[0])])
    # F of the new texels, over all layers
    expected_tiles = dict(before.tiles)
    expected_tiles.update(EM.propagate(EM.write_region(before.tiles, lod, side, x0, y0, new, b), b, spherical))
    edited = EM.region_tiles(lod, side, x0, y0, w, h, c)
    levels = ancestors_levels(before, edited)
    after = check_edit(atlas, before, expected_tiles, changed, stats["edit"], edited, levels)
    assert stats["edit"]["launches"] == (1 + levels + 1 if stats["edit"]["tiles_edited"] else 0) and stats["edit"]["layers_mipped"] == 0
    assert (stats["cells"], stats["tiles_missing"], stats["steps"], stats["sim_launches"]) == (w * h, missing, case["params"]["steps"], case["params"]["steps"] + 2)
    # the twin: the same texels through write_region
    twin_changed, twin_stats = twin.write_region(0, new, x0, y0, side=side)
    assert np.array_equal(twin.download_tiles(0, 0, twin.atlas_size), after.data), "the atlas differs from one that received the texels through write_region"
    assert [(t.side, t.lod, t.x, t.y) for t in twin_changed] == [(t.side, t.lod, t.x, t.y) for t in changed] and twin_stats == stats["edit"]
    return before, after, changed, stats, water_out, sediment_out


@pytest.mark.gpu
@pytest.mark.parametrize("name", EC.WINDOWS)
def test_windows(device, atlases, name):
    before, after, changed, stats, _, _ = run_named(atlases, name)
    reached = EC.expected(name)[6]
    if reached["written"]:
        assert sum(1 for k in before.tiles if not np.array_equal(before.tiles[k], after.tiles[k])) >= 1, "the call changed nothing: the comparison would be empty"
    if name == "missing_tile_hole_at_block_corner":
        assert stats["tiles_missing"] == 1 and stats["edit"]["tiles_edited"] == 3 and stats["edit"]["tiles_missing"] == 1
    if name == "cube_side_3":
        assert {t.side for t in changed if t.lod == 1} >= {3} and stats["edit"]["tiles_edited"] == 4
        # the same window of another side erodes other heights: the side argument is used
        case = dict(EC.CASES[name], side=1)
        atlas, twin = atlases("cube")
        x0, y0, w, h = case["rect"]
        raw1, _ = atlas.read_region(0, x0, y0, w, h, side=1)
        call(atlas, case)
        twin.write_region(0, M.erode(raw1, case["params"])[0], x0, y0, side=1)
        assert np.array_equal(twin.download_tiles(0, 0, twin.atlas_size), atlas.download_tiles(0, 0, atlas.atlas_size))


@pytest.mark.gpu
@pytest.mark.parametrize("steps", [1, 2, 37])
def test_ping_pong_parity(device, atlases, steps):
    """odd and even step counts end on different sides of the ping-pong: the finish and the state going out read the right one"""
    name = "several_blocks_t16"
    case = EC.CASES[name]
    raw, missing = EC.window(name)
    weight, water, sediment = EC.inputs(name)
    p = dict(case["params"], steps=steps)
    new, d, s, _ = M.erode(raw, p, weight, water, sediment)
    run_case(atlases, dict(case, params=p), EC.texels(name), (weight, water, sediment), (raw, missing, new, d, s), f"{steps} steps")


@pytest.mark.gpu
def test_state_out_and_back_in(device, atlases):
    """five steps, then five more from the water and sediment that came out: each call is the model's, and the two together are not one
    call of ten steps (the fluxes restart at 0, the heights went through the texels)"""
    name = "five_steps_state_out"
    case = EC.CASES[name]
    _, _, _, _, water5, sediment5 = run_named(atlases, name)
    raw, missing, new5, d5, s5 = EC.expected(name)[:5]
    assert np.array_equal(bits(water5), bits(d5)) and (water5 > 0).any() and (sediment5 > 0).any()
    again, d10, s10, _ = M.erode(new5, case["params"], None, water5, sediment5)
    run_case(atlases, case, new5, (None, water5, sediment5), (new5, missing, again, d10, s10), "five more")
    _, d_once, _, _ = M.erode(raw, dict(case["params"], steps=10), None, *EC.inputs(name)[1:])
    assert not np.array_equal(bits(d10), bits(d_once))


@pytest.mark.gpu
def test_subnormal_state(device, atlases):
    """rain = 1e-30: water and fluxes pass through subnormal values (asserted on the model without a GPU); a device that flushed them would differ"""
    assert EC.expected("subnormal")[6]["subnormal"] >= 1
    _, _, _, _, water, _ = run_named(atlases, "subnormal")
    assert (water > 0).any() and water.max() < 1e-29


@pytest.mark.gpu
@pytest.mark.parametrize("name", EC.FIXED_POINTS + ["overflow"])
def test_fixed_points_leave_the_atlas_byte_identical(device, atlases, name):
    before, after, changed, stats, water, sediment = run_named(atlases, name)
    assert np.array_equal(before.data, after.data), "a fixed point moved a texel"
    assert stats["edit"]["tiles_edited"] >= 1 and len(changed) == stats["edit"]["changed_count"] >= stats["edit"]["tiles_edited"]  # listed as for write_region all the same


@pytest.mark.gpu
def test_weight_planes(device, atlases):
    """without a weight plane, with one of 255 everywhere (the same result) and with one of 0 everywhere (nothing moves)"""
    name = "several_blocks_t16"
    case = EC.CASES[name]
    raw, missing = EC.window(name)
    _, water, sediment = EC.inputs(name)
    h, w = raw.shape
    full = M.erode(raw, case["params"], None, water, sediment)
    for weight in (np.full((h, w), 255, np.uint8), np.zeros((h, w), np.uint8)):
        new, d, s, _ = M.erode(raw, case["params"], weight, water, sediment)
        assert np.array_equal(new, full[0] if weight[0, 0] else raw) and np.array_equal(bits(d), bits(full[1]))
        run_case(atlases, case, EC.texels(name), (weight, water, sediment), (raw, missing, new, d, s), f"weight {weight[0, 0]}")


@pytest.mark.gpu
def test_a_window_no_tile_covers(device):
    cfg = bt.TerrainConfig(lod_count=3, atlas_size=4, path="terrains/erode_empty", model=bt.TerrainModel.planar((0, 0, 0), 1000.0, 0.0, 1.0))
    cfg.add_attachment(bt.AttachmentConfig(name="height", texture_size=16, border_size=2, format=bt.AttachmentFormat.R16))
    atlas = bt.TileAtlas.new(cfg, device)
    wet = np.full((20, 30), 0.5, np.float32)
    changed, stats, water, sediment = atlas.erode_height(0, 5, 7, 30, 20, ErosionParams(steps=3), water=wet, sediment=wet)
    assert changed == [] and (water == 0).all() and (sediment == 0).all()
    assert (stats["cells"], stats["tiles_missing"], stats["steps"], stats["sim_launches"]) == (600, 9, 3, 5)
    assert stats["edit"] == dict(tiles_edited=0, tiles_missing=9, tiles_with_children=0, tiles_downsampled=0, tiles_stitched=0, layers_mipped=0, launches=0, changed_count=0)


# ---------------------------------------------------------------------------------------------- refusals

GOOD = dict(M.DEFAULTS, steps=2)


def params_c(p):
    return _ffi.ErosionParamsC(*[float(p[f]) for f, _ in _ffi.ErosionParamsC._fields_[:12]], int(p["steps"]), (C.c_uint32 * 3)(0, 0, 0))


BAD_PARAMS = [
    dict(min_height=-INF), dict(max_height=NAN), dict(min_height=-3e38, max_height=3e38), dict(min_height=5.0, max_height=5.0), dict(min_height=5.0, max_height=4.0),
    dict(cell_size=0.0), dict(cell_size=-1.0), dict(cell_size=INF), dict(cell_size=NAN),
    dict(dt=0.0), dict(dt=-0.05), dict(dt=INF), dict(dt=NAN),
    dict(rain=-0.1), dict(rain=INF), dict(rain=NAN), dict(evaporation=-0.1), dict(evaporation=INF), dict(evaporation=NAN),
    dict(gravity=0.0), dict(gravity=-9.81), dict(gravity=INF), dict(gravity=NAN),
    dict(capacity=-0.1), dict(capacity=INF), dict(capacity=NAN),
    dict(erode=-0.1), dict(erode=1.5), dict(erode=NAN), dict(deposit=-0.1), dict(deposit=1.5), dict(deposit=NAN),
    dict(min_tilt=-0.1), dict(min_tilt=1.5), dict(min_tilt=NAN), dict(min_depth=0.0), dict(min_depth=-0.01), dict(min_depth=INF), dict(min_depth=NAN),
    dict(steps=0), dict(steps=4097),
]


@pytest.mark.gpu
def test_refusals_leave_the_outputs_untouched_and_queue_nothing(device):
    """every refusal: status, outputs untouched, stats zeroed.  The atlas is one of allocated, never-written layers with a fused job queued
    behind: a refused call that had marked a layer written (what queued work does) would take the job's prev_zero_launches away"""
    T, b, lods, W = 128, 2, 3, 496  # source : mosaic = 1.0 -> a fused job (tests/test_gpu_prev_values.py)
    src = K.low_half(K.random_raster(O.FORMAT_R16, W, W, seed=3, holes=0.01), O.FORMAT_R16)
    L = _ffi.lib()
    w, h = 20, 10
    flagged = {}
    for accepted in (False, True):
        cfg = bt.TerrainConfig(lod_count=lods, atlas_size=ATLAS, path="terrains/erode", model=bt.TerrainModel.planar((0, 0, 0), 1000.0, 0.0, 1.0))
        cfg.add_attachment(bt.AttachmentConfig(name="att", texture_size=T, border_size=b, format=bt.AttachmentFormat.R16))
        cfg.add_attachment(bt.AttachmentConfig(name="colour", texture_size=T, border_size=b, format=bt.AttachmentFormat.Rgba8))
        atlas = bt.TileAtlas.new(cfg, device)
        server = bt.AssetServer().insert("src", src)
        pre = bt.Preprocessor.new().clear_attachment(0, atlas).preprocess_tile(bt.PreprocessDataset(attachment_index=0, path="src", lod_range=range(0, lods)), server, atlas)
        assert len(atlas.tiles()) == 21

        def erode(a=atlas._h, ai=0, side=0, lod=2, x0=3, y0=5, width=w, height=h, params=GOOD, null_params=False, water=None, sediment=None, null_changed=False):
            water_out = np.full((h, w), 0.5, np.float32) if water is None else water
            sediment_out = np.full((h, w), 0.25, np.float32) if sediment is None else sediment
            kept = water_out.copy(), sediment_out.copy()
            changed = (_ffi.TileCoordinateC * 32)(*[_ffi.TileCoordinateC(7, 7, 7, 7)] * 32)
            stats = _ffi.ErosionStatsC(9, 9, 9, 9, _ffi.EditStatsC(*([9] * 8)))
            weight = np.full((h, w), 200, np.uint8)
            pc = params_c(params)
            rc = L.bt_atlas_erode_height(a, ai, side, lod, x0, y0, width, height, None if null_params else C.byref(pc), weight.ctypes.data_as(C.POINTER(C.c_uint8)),
                                         water_out.ctypes.data_as(C.POINTER(C.c_float)), sediment_out.ctypes.data_as(C.POINTER(C.c_float)),
                                         None if null_changed else changed, 32, C.byref(stats))
            untouched = np.array_equal(bits(water_out), bits(kept[0])) and np.array_equal(bits(sediment_out), bits(kept[1])) and all(t.side == 7 for t in changed)
            zeroed = all(getattr(stats, f) == 0 for f in ("cells", "tiles_missing", "steps", "sim_launches")) and all(getattr(stats.edit, f) == 0 for f, _ in _ffi.EditStatsC._fields_)
            return rc, untouched, zeroed

        n = 496  # the mosaic of lod 2
        refused = [dict(a=None), dict(ai=2), dict(side=1), dict(lod=3), dict(x0=n - 19), dict(y0=n - 9), dict(x0=n), dict(width=n + 1, x0=0), dict(null_params=True),
                   dict(null_changed=True)] + [dict(params=dict(GOOD, **bad)) for bad in BAD_PARAMS]
        for plane in ("water", "sediment"):
            for value in (-1e-6, -1.0, INF, NAN):
                bad = np.full((h, w), 0.5, np.float32)
                bad[h - 1, w - 1] = value
                refused.append({plane: bad})
        for kw in refused:
            rc, untouched, zeroed = erode(**kw)
            assert rc == BT_ERR_INVALID_ARGUMENT and untouched and zeroed, ({k: v for k, v in kw.items() if k not in ("water", "sediment")}, rc)
        rc, untouched, zeroed = erode(ai=1)  # the Rgba8 attachment
        assert rc == BT_ERR_UNSUPPORTED and untouched and zeroed
        # more than 2^22 cells cannot fit this mosaic (496^2): a wider one, which needs no tile, since the refusal comes first
        wide_cfg = bt.TerrainConfig(lod_count=6, atlas_size=4, path="terrains/erode_limits", model=bt.TerrainModel.planar((0, 0, 0), 1000.0, 0.0, 1.0))
        wide_cfg.add_attachment(bt.AttachmentConfig(name="height", texture_size=72, border_size=2, format=bt.AttachmentFormat.R16))
        wide = bt.TileAtlas.new(wide_cfg, device)
        for kw in (dict(width=2049, height=2048), dict(width=2048, height=2049), dict(width=2176, height=2176)):
            rc, untouched, zeroed = erode(a=wide._h, lod=5, x0=0, y0=0, **kw)
            assert rc == BT_ERR_INVALID_ARGUMENT and untouched and zeroed and b"cells" in L.bt_last_error(), kw
        # an odd centre size
        odd_cfg = bt.TerrainConfig(lod_count=2, atlas_size=4, path="terrains/erode_odd", model=bt.TerrainModel.planar((0, 0, 0), 1000.0, 0.0, 1.0))
        odd_cfg.add_attachment(bt.AttachmentConfig(name="height", texture_size=17, border_size=2, format=bt.AttachmentFormat.R16))
        odd = bt.TileAtlas.new(odd_cfg, device)
        rc, untouched, zeroed = erode(a=odd._h, lod=1, x0=0, y0=0)
        assert rc == BT_ERR_UNSUPPORTED and untouched and zeroed
        # an empty window is BT_OK with nothing touched, whatever the planes hold
        for kw in (dict(width=0), dict(height=0), dict(width=0, height=0)):
            rc, untouched, zeroed = erode(water=np.full((h, w), NAN, np.float32), **kw)
            assert rc == 0 and untouched and zeroed, kw
        # the limits themselves are allowed
        for ok in (dict(rain=0.0), dict(evaporation=0.0), dict(capacity=0.0), dict(erode=0.0, deposit=1.0), dict(min_tilt=0.0), dict(min_tilt=1.0), dict(steps=1)):
            if accepted:
                assert erode(params=dict(GOOD, **ok))[0] == 0, ok
        if accepted:  # the layers hold no data: every cell is a wall, nothing moves, and still the call writes the layers
            rc, untouched, zeroed = erode()
            assert rc == 0 and not untouched and not zeroed
            assert not atlas.download_tiles(0, 0, ATLAS).any()
        pre.run(atlas)
        flagged[accepted] = pre.stats()["prev_zero_launches"]
    assert flagged[False] >= 1 and flagged[True] == 0, flagged


@pytest.mark.gpu
def test_nulls(device, atlases):
    """stats NULL, changed NULL with changed_cap 0, every optional plane NULL: the call only enqueues and the result is the model's"""
    name = "mosaic_edge"
    case = EC.CASES[name]
    atlas, twin = atlases(case["kind"])
    x0, y0, w, h = case["rect"]
    for a in (atlas, twin):
        a.write_region(0, EC.texels(name), x0, y0)
    pc = params_c(case["params"])
    _ffi.check(_ffi.lib().bt_atlas_erode_height(atlas._h, 0, 0, 2, x0, y0, w, h, C.byref(pc), None, None, None, None, 0, None))
    got, _ = atlas.read_region(0, x0, y0, w, h)
    assert np.array_equal(got, EC.expected(name)[2])
    twin.write_region(0, EC.expected(name)[2], x0, y0)
    assert np.array_equal(twin.download_tiles(0, 0, twin.atlas_size), atlas.download_tiles(0, 0, atlas.atlas_size))

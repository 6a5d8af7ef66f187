"""bt_atlas_label_regions on the device against the model of the definition (tests/_regions_model.py, pinned by test_regions_model.py).

Every scene of tests/_regions_cases.py runs on a pair of atlases in one state: the first takes the call, the twin takes the model's baked
texels through bt_atlas_write_region.  Equal with no tolerance and no excluded cell: label_out, id_out, the table, every field of
bt_regions_stats but launches (which is pinned to the documented count); with a bake also `changed`, bt_edit_stats and every layer of
both attachments.  The scenes that read the heights bake into the Rgba8 attachment of the pair; those that read the Rgba8 attachment run
without a bake on a pair nothing writes to, and the bake onto the source attachment has tests of its own.  The model's planes are computed
once per scene (without a GPU, from the CPU oracle's state) and shared; each check first reads the window back with bt_atlas_read_region
and requires the texels the model was given."""
import ctypes as C

import numpy as np
import pytest

import _regions_cases as RC
import _regions_model as M
import bevy_terrain_amd as bt
from _splat_cases import G, H
from bevy_terrain_amd import _ffi
from test_gpu_splat import device_atlas

BT_ERR_INVALID_ARGUMENT, BT_ERR_UNSUPPORTED = -1, -5
LAUNCHES, LAUNCHES_BAKE = 7, 8  # the gather, local, seams, flatten, scan, emit, finish; the gather of a bake's destination
BAKE = dict(attachment=G, channel=2, min_area=2, max_area=40, value=201)  # what the scenes on the heights bake


@pytest.fixture(scope="module")
def device():
    return bt.Device(0)


@pytest.fixture(scope="module")
def pairs(device):
    """two atlases in one state per (spec, use), made on first use.  use: "bake" (the scenes on the heights; G is written), "plant" (the
    scenes that write their own heights first), "read" (the scenes on G: nothing writes)"""
    made = {}

    def get(name):
        scene = RC.SCENES[name]
        key = (scene["spec"], "plant" if scene["plant"] is not None else "bake" if scene["attachment"] == H else "read")
        if key not in made:
            made[key] = (device_atlas(device, key[0]), device_atlas(device, key[0]))
        return made[key]

    return get


def coords(changed):
    return [(t.side, t.lod, t.x, t.y) for t in changed]


def whole(atlas, ai):
    return atlas.download_tiles(ai, 0, atlas.atlas_size).tobytes()


def input_stats(stats):
    return {k: v for k, v in stats.items() if k not in M.SCHEDULE}


def run(atlas, name, **kw):
    scene = RC.SCENES[name]
    x0, y0, w, h = scene["rect"]
    return atlas.label_regions(scene["attachment"], x0, y0, w, h, members=RC.window(name)[2], lod=scene["lod"], side=scene["side"], **RC.rule(name), **kw)


def assert_planes(name, got, want):
    for plane, g, e in zip(("label", "id"), got, want):
        assert g.dtype == e.dtype and g.shape == e.shape, (name, plane)
        differ = np.argwhere(g != e)
        assert differ.size == 0, (name, plane, len(differ), differ[:5], g[tuple(differ[0])], e[tuple(differ[0])])


def assert_table(name, got, want):
    assert got.dtype == want.dtype and len(got) == len(want), (name, len(got), len(want))
    for field in want.dtype.names:
        differ = np.flatnonzero(got[field] != want[field])
        assert differ.size == 0, (name, field, len(differ), differ[:5], got[differ[:5]], want[differ[:5]])


def check_scene(pair, name):
    """the scene on the pair, by the module docstring; returns the device's (label, id, regions, stats)"""
    scene = RC.SCENES[name]
    texels, _, label, id_, regions, stats = RC.expected(name)
    ours, twin = pair
    x0, y0, w, h = scene["rect"]
    where = dict(lod=scene["lod"], side=scene["side"])
    if scene["plant"] is not None:
        for atlas in pair:
            atlas.write_region(H, texels, x0, y0)
    got_texels, missing = ours.read_region(scene["attachment"], x0, y0, w, h, **where)
    assert np.array_equal(got_texels, texels) and missing == stats["tiles_missing"], "the device atlas is not the state the model was given"
    bake = scene["attachment"] == H
    if bake:
        before, _ = twin.read_region(G, x0, y0, w, h, **where)
        baked_texels, baked = M.bake(before, label, regions, BAKE["channel"], BAKE["min_area"], BAKE["max_area"], BAKE["value"])
        changed_m, edit_m = twin.write_region(G, baked_texels, x0, y0, **where)
        *got, table, stats_d, changed = run(ours, name, bake=BAKE)
    else:
        baked = 0
        *got, table, stats_d = run(ours, name)
    assert_planes(name, got, (label, id_))
    assert_table(name, table, regions)
    assert input_stats(stats_d) == dict(stats, baked=baked), (name, stats_d, stats)
    if bake:
        assert stats_d["launches"] == LAUNCHES_BAKE, stats_d
        assert coords(changed) == coords(changed_m) and stats_d["edit"] == edit_m and edit_m["changed_count"] > 0, name
        assert whole(ours, G) == whole(twin, G) and whole(ours, H) == whole(twin, H), name
    else:
        assert stats_d["launches"] == LAUNCHES and not any(stats_d["edit"].values()), stats_d
    return got[0], got[1], table, stats_d


@pytest.mark.gpu
@pytest.mark.parametrize("name", RC.SHAPES)
def test_window_shapes_and_simple_fills(device, pairs, name):
    label, id_, table, stats = check_scene(pairs(name), name)
    if name == "checkerboard_four":
        assert (table["edges"] == 4).all() and stats["regions"] == stats["members"]
    if name in ("all_members", "checkerboard_eight"):
        assert stats["regions"] == 1 and table[0]["label"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", RC.SIZES)
def test_sizes_around_a_block(device, pairs, name):
    check_scene(pairs(name), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", RC.SEAMS)
def test_seams_and_diagonal_links(device, pairs, name):
    check_scene(pairs(name), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", RC.STEPS)
def test_max_step_and_the_values(device, pairs, name):
    _, _, table, stats = check_scene(pairs(name), name)
    if name == "adjacent_not_linked":
        assert table["edges"].tolist() == [4, 4] and table["v_sum"].tolist() == [100, 200]


@pytest.mark.gpu
@pytest.mark.parametrize("name", RC.SOURCES)
def test_formats_channels_flags_and_missing_data(device, pairs, name):
    _, _, _, stats = check_scene(pairs(name), name)
    if name.startswith("missing_tiles"):
        assert stats["tiles_missing"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", RC.OTHER_LAYERS)
def test_other_layers(device, pairs, name):
    label, *_ = check_scene(pairs(name), name)
    if name == "cube_side":  # the same window of another side is another terrain: the side argument is used
        scene = RC.SCENES[name]
        other = pairs(name)[0].label_regions(H, *scene["rect"], lo=scene["lo"], hi=scene["hi"], side=1)
        assert not np.array_equal(other[0], label)


@pytest.mark.gpu
@pytest.mark.parametrize("name", RC.FIELDS)
def test_random_fields(device, pairs, name):
    check_scene(pairs(name), name)


@pytest.mark.gpu
def test_launches_depend_on_the_arguments_alone(device, pairs):
    """one window and one rule over different texels and different member planes: other regions, the same launches"""
    ours, twin = pairs("ramp_step_1")
    x0, y0, w, h = RC.SCENES["ramp_step_1"]["rect"]
    seen = []
    for texels in (RC.ramp(h, w), RC.terrace(h, w), np.full((h, w), 7, np.uint16)):
        ours.write_region(H, texels, x0, y0), twin.write_region(H, texels, x0, y0)  # the pair stays in one state
        *_, stats = ours.label_regions(H, x0, y0, w, h, lo=1, max_step=1)
        seen.append((stats["regions"], stats["launches"]))
    assert len({r for r, _ in seen}) == 3 and {l for _, l in seen} == {LAUNCHES}, seen
    launches = {name: run(ours, name)[3]["launches"] for name in ("serpentine", "spiral", "all_members", "no_members")}
    assert set(launches.values()) == {LAUNCHES}, launches


@pytest.mark.gpu
def test_table_capacity(device, pairs):
    name = "w96_h70_ragged"
    ours, _ = pairs(name)
    scene = RC.SCENES[name]
    _, _, label, id_, regions, stats = RC.expected(name)
    x0, y0, w, h = scene["rect"]
    n = stats["regions"]
    host = RC.window(name)[2]
    rule = _ffi.RegionsRuleC(0, 0, 0, 65535, 0)
    for cap in (0, 1, n - 1, n, n + 5):
        room = np.full(n + 8, 0xAB, np.uint8).repeat(M.REGION_SIZE).view(M.REGION_DTYPE)  # n + 8 records of the byte pattern
        assert room.shape == (n + 8,)
        stats_c = _ffi.RegionsStatsC()
        _ffi.check(_ffi.lib().bt_atlas_label_regions(ours._h, H, 0, 2, x0, y0, w, h, C.byref(rule), host.ctypes.data_as(C.POINTER(C.c_uint8)), None, None,
                                                     room.ctypes.data_as(C.POINTER(_ffi.RegionC)) if cap else None, cap, None, None, 0, C.byref(stats_c)))
        written = min(n, cap)
        assert (stats_c.regions, stats_c.regions_written, stats_c.largest_area, stats_c.largest_label) == (n, written, stats["largest_area"], stats["largest_label"]), cap
        assert_table((name, cap), room[:written], regions[:written])
        assert (room[written:].view(np.uint8) == 0xAB).all(), cap  # the rest of the array is untouched
    # through the wrapper: the ids of the planes do not depend on the capacity
    label_d, id_d, table, stats_d = run(ours, name, region_cap=3)
    assert_planes(name, (label_d, id_d), (label, id_))
    assert_table(name, table, regions[:3])
    assert stats_d["regions_written"] == 3 and stats_d["regions"] == n


@pytest.mark.gpu
def test_each_output_may_be_null_and_two_calls_agree(device, pairs):
    name = "field_59_four"
    ours, _ = pairs(name)
    _, _, label, id_, regions, stats = RC.expected(name)
    for kw in (dict(label=False), dict(id=False), dict(label=False, id=False), dict(region_cap=0), dict(label=False, id=False, region_cap=0)):
        *got, table, stats_d = run(ours, name, **kw)
        for flag, g, e in zip(("label", "id"), got, (label, id_)):
            assert g is None if flag in kw else np.array_equal(g, e), (kw, flag)
        assert_table(name, table, regions[:0] if "region_cap" in kw else regions)
        assert input_stats(stats_d) == dict(stats, baked=0, regions_written=0 if "region_cap" in kw else stats["regions"]) and stats_d["launches"] == LAUNCHES, kw
    a, b = run(ours, name), run(ours, name)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3])) and a[3] == b[3]
    # stats NULL, changed NULL, the planes alone
    scene = RC.SCENES[name]
    x0, y0, w, h = scene["rect"]
    out = np.zeros((h, w), np.uint32)
    host = RC.window(name)[2]
    _ffi.check(_ffi.lib().bt_atlas_label_regions(ours._h, H, 0, 2, x0, y0, w, h, C.byref(_ffi.RegionsRuleC(0, 0, 0, 65535, 0)), host.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                 out.ctypes.data_as(C.POINTER(C.c_uint32)), None, None, 0, None, None, 0, None))
    assert np.array_equal(out, label)


@pytest.mark.gpu
def test_the_call_without_a_bake_is_a_read(device, pairs):
    ours, _ = pairs("rgba_channel_0")
    before = [whole(ours, ai) for ai in (G, H)]
    for name in ("rgba_channel_0", "rgba_channel_3_inverted"):
        *_, stats = run(ours, name)
        assert stats["launches"] == LAUNCHES and not any(stats["edit"].values())
    assert before == [whole(ours, ai) for ai in (G, H)]


@pytest.mark.gpu
def test_scratch_is_reused_and_released_by_trim(device, pairs):
    """the planes stay in the context: a smaller call after a larger one allocates nothing, and bt_ctx_trim gives the bytes back"""
    big, small = "field_45_eight", "w31_h33"
    ours, _ = pairs(big)
    expect = {name: RC.expected(name) for name in (big, small)}

    def same(name):
        label_d, id_d, table, _ = run(ours, name)
        assert_planes(name, (label_d, id_d), expect[name][2:4])
        assert_table(name, table, expect[name][4])

    device.trim()
    same(big)
    large = device.trim()
    cells = 96 * 70
    assert large >= 4 * ((cells * 4 + 255) & ~255) + cells * 80  # P, id, area, rank and the records of a table of `cells` at least
    same(big), same(small), same(big)  # the smaller call in the larger one's buffers
    assert device.trim() == large
    assert device.trim() == 0
    same(small)  # allocated anew, smaller
    assert 0 < device.trim() < large
    same(big)


# ---------------------------------------------------------------------------------------------- the bake

BAKE_RECT = (60, 62, 50, 44)  # of planar_72: across the tile edge at 68 on both axes


@pytest.fixture(scope="module")
def bake_pair(device):
    return device_atlas(device, "planar_72"), device_atlas(device, "planar_72")


def bake_both(pair, source, bake, outputs=True, **rule):
    """the device's bake on the first atlas and the model's on the second, over BAKE_RECT; returns the device's stats and the baked byte"""
    ours, twin = pair
    x0, y0, w, h = BAKE_RECT
    dest, channel, min_area, max_area, value = bake
    texels, _ = twin.read_region(source, x0, y0, w, h)
    member, label, id_, regions, stats = M.solve(texels, channel=rule.get("channel", 0), lo=rule.get("lo"), hi=rule.get("hi"), host=rule.get("members"),
                                                 invert=rule.get("invert", False), max_step=rule.get("max_step", 65535), eight=rule.get("eight", False))
    before, _ = twin.read_region(dest, x0, y0, w, h)
    baked_texels, baked = M.bake(before, label, regions, channel, min_area, max_area, value)
    changed_m, edit_m = twin.write_region(dest, baked_texels, x0, y0)
    label_d, id_d, table, stats_d, changed = ours.label_regions(source, x0, y0, w, h, bake=bake, label=outputs, id=outputs, **rule)
    if outputs:
        assert_planes("bake", (label_d, id_d), (label, id_))
    else:
        assert label_d is None and id_d is None
    assert_table("bake", table, regions)
    assert input_stats(stats_d) == dict(stats, tiles_missing=0, baked=baked) and stats_d["launches"] == LAUNCHES_BAKE
    assert coords(changed) == coords(changed_m) and stats_d["edit"] == edit_m and edit_m["changed_count"] > 0
    assert whole(ours, G) == whole(twin, G) and whole(ours, H) == whole(twin, H)
    after, _ = ours.read_region(dest, x0, y0, w, h)
    assert np.array_equal(after, baked_texels)
    return stats_d, regions, after[:, :, channel], before[:, :, channel], label


@pytest.mark.gpu
@pytest.mark.parametrize("channel", [0, 1, 2, 3])
def test_bake_into_each_channel_of_another_attachment(device, bake_pair, channel):
    stats, regions, byte, before, label = bake_both(bake_pair, H, (G, channel, 3, 200, 17 + channel), lo=33000, hi=36000)
    assert 0 < stats["baked"] < stats["members"]  # some regions lie in the band of areas, some below or above


@pytest.mark.gpu
def test_despeckle_on_the_source_attachment(device, bake_pair):
    """members are a band of the alpha byte; the regions of at most 15 cells are set to 0 in that same byte, which takes them out of
    the band: a second call finds only the regions above 15"""
    stats, regions, byte, before, label = bake_both(bake_pair, G, (G, 3, 0, 15, 0), lo=120, hi=255, channel=3)
    small = int((regions["area"] <= 15).sum())
    assert small > 0 and stats["baked"] == int(regions["area"][regions["area"] <= 15].sum())
    x0, y0, w, h = BAKE_RECT
    *_, table, again = bake_pair[0].label_regions(G, x0, y0, w, h, lo=120, hi=255, channel=3)
    assert again["regions"] == stats["regions"] - small and (table["area"] > 15).all()


@pytest.mark.gpu
def test_bake_with_both_planes_null_from_a_host_plane_under_eight(device, bake_pair):
    stats, *_ = bake_both(bake_pair, H, (G, 1, 1, 1, 255), outputs=False, members=RC.random(0.3, 3)(*BAKE_RECT[:1:-1]), eight=True)
    assert stats["baked"] > 0
    bake_both(bake_pair, H, (G, 0, 0, 0xFFFFFFFF, 9), members=RC.random(0.59, 4)(*BAKE_RECT[:1:-1]), max_step=300)


@pytest.mark.gpu
def test_bake_that_writes_nothing(device, bake_pair):
    stats, *_ = bake_both(bake_pair, H, (G, 3, 5000, 6000, 1), lo=33000, hi=36000)
    assert stats["baked"] == 0
    stats, *_ = bake_both(bake_pair, H, (G, 3, 0, 10, 1), members=RC.nothing(*BAKE_RECT[:1:-1]))
    assert stats["baked"] == 0 and stats["regions"] == 0 and stats["largest_label"] == _ffi.REGIONS_NONE


# ---------------------------------------------------------------------------------------------- refusals

@pytest.mark.gpu
def test_refusals_leave_the_outputs_untouched(device):
    atlas = device_atlas(device, "planar_72")  # its own: the accepted bakes below write
    L = _ffi.lib()
    w, h = 20, 10
    host_plane = np.ones((h, w), np.uint8)
    FT, INV, EIGHT = _ffi.REGIONS_FROM_TEXELS, _ffi.REGIONS_INVERT, _ffi.REGIONS_EIGHT

    def call(a=None, ai=H, side=0, lod=2, x0=3, y0=5, width=w, height=h, rule=(0, 0, 100, 65535, FT), host=False, bake=None, changed_cap=0, null_changed=True, null_rule=False,
             region_cap=8, null_regions=False):
        outs = [np.full((h, w), 77, np.uint32) for _ in range(2)]
        table = np.full(8 * M.REGION_SIZE, 0x4D, np.uint8)
        stats = _ffi.RegionsStatsC(*([9] * 9), (C.c_uint32 * 3)(9, 9, 9), _ffi.EditStatsC(*([9] * 8)))
        changed = (_ffi.TileCoordinateC * 64)()
        rc = L.bt_atlas_label_regions(atlas._h if a is None else a, ai, side, lod, x0, y0, width, height, None if null_rule else C.byref(_ffi.RegionsRuleC(*rule)),
                                      host_plane.ctypes.data_as(C.POINTER(C.c_uint8)) if host else None, outs[0].ctypes.data_as(C.POINTER(C.c_uint32)),
                                      outs[1].ctypes.data_as(C.POINTER(C.c_uint32)), None if null_regions else table.ctypes.data_as(C.POINTER(_ffi.RegionC)), region_cap,
                                      C.byref(_ffi.RegionsBakeC(*bake)) if bake else None, None if null_changed else changed, changed_cap, C.byref(stats))
        untouched = all((o == 77).all() for o in outs) and (table == 0x4D).all()
        zeroed = bytes(stats) == bytes(C.sizeof(stats))
        return rc, untouched, zeroed

    assert call()[0] == 0 and not call()[1] and not call()[2]
    before = [whole(atlas, ai) for ai in (G, H)]
    n = 272  # the mosaic of lod 2
    for kw in (dict(ai=2), dict(side=1), dict(lod=3), dict(x0=n - 19), dict(y0=n - 9), dict(x0=n), dict(width=n + 1, x0=0),  # what region_check refuses
               dict(null_rule=True), dict(rule=(0, 0, 100, 65535, 0)), dict(rule=(0, 0, 100, 65535, INV | EIGHT)),  # neither FROM_TEXELS nor a host plane
               dict(rule=(0, 0, 100, 65535, FT | 8)), dict(rule=(0, 0, 100, 65535, 0x80000000), host=True), dict(rule=(0, 101, 100, 65535, FT)),
               dict(rule=(0, 101, 100, 65535, FT), host=True), dict(rule=(1, 0, 100, 65535, FT)), dict(rule=(4, 0, 100, 65535, FT), ai=G), dict(rule=(0, 0, 65536, 65535, FT)),
               dict(rule=(3, 0, 256, 65535, FT), ai=G), dict(rule=(0, 0, 100, 65536, FT)), dict(rule=(0, 0, 100, 65536, FT), ai=G),
               dict(changed_cap=1), dict(null_regions=True), dict(null_regions=True, region_cap=1),
               dict(bake=(2, 0, 0, 9, 7, 0)), dict(bake=(0xFFFFFFFF, 0, 0, 9, 7, 0)), dict(bake=(G, 4, 0, 9, 7, 0)), dict(bake=(G, 0, 10, 9, 7, 0)), dict(bake=(G, 0, 0, 9, 256, 0)),
               dict(bake=(G, 0, 0, 9, 7, 1)), dict(bake=(G, 0, 0, 9, 7, 0x80000000))):
        rc, untouched, zeroed = call(**kw)
        assert rc == BT_ERR_INVALID_ARGUMENT and untouched and zeroed, (kw, rc, L.bt_last_error())
    for kw in (dict(rule=(0, 0, 65535, 0, FT)), dict(rule=(3, 0, 255, 65535, FT | INV | EIGHT), ai=G), dict(rule=(3, 0, 255, 256, FT), ai=G), dict(rule=(0, 0, 0, 7, INV), host=True),
               dict(rule=(0, 101, 100, 0, 0), host=True), dict(null_regions=True, region_cap=0), dict(bake=(G, 3, 0, 0xFFFFFFFF, 255, 0)), dict(bake=(G, 0, 9, 9, 0, 0)),
               dict(bake=(G, 0, 1, 5, 1, 0), changed_cap=64, null_changed=False)):
        assert call(**kw)[0] == 0, kw
    rc, untouched, zeroed = call(bake=(H, 0, 0, 9, 7, 0))  # the R16 attachment takes no byte
    assert rc == BT_ERR_UNSUPPORTED and untouched and zeroed
    for kw in (dict(width=0), dict(height=0), dict(width=0, height=0), dict(width=0, bake=(G, 0, 0, 9, 7, 0))):  # an empty window is BT_OK with nothing touched
        rc, untouched, zeroed = call(**kw)
        assert rc == 0 and untouched and zeroed, kw
    # an odd centre size (T = 17, b = 2: 13 centre texels); a destination of another texture size, of another border size
    cfg = bt.TerrainConfig(lod_count=2, atlas_size=4, path="terrains/regions_odd", model=bt.TerrainModel.planar((0, 0, 0), 1000.0, 0.0, 1.0))
    cfg.add_attachment(bt.AttachmentConfig(name="height", texture_size=17, border_size=2, format=bt.AttachmentFormat.R16))
    odd = bt.TileAtlas.new(cfg, device)
    rc, untouched, zeroed = call(a=odd._h, ai=0, lod=1, x0=0, y0=0)
    assert rc == BT_ERR_UNSUPPORTED and untouched and zeroed
    cfg = bt.TerrainConfig(lod_count=3, atlas_size=4, path="terrains/regions_mixed", model=bt.TerrainModel.planar((0, 0, 0), 1000.0, 0.0, 1.0))
    cfg.add_attachment(bt.AttachmentConfig(name="height", texture_size=20, border_size=2, format=bt.AttachmentFormat.R16))
    cfg.add_attachment(bt.AttachmentConfig(name="larger", texture_size=24, border_size=2, format=bt.AttachmentFormat.Rgba8))
    cfg.add_attachment(bt.AttachmentConfig(name="thicker", texture_size=20, border_size=4, format=bt.AttachmentFormat.Rgba8))
    cfg.add_attachment(bt.AttachmentConfig(name="alike", texture_size=20, border_size=2, format=bt.AttachmentFormat.Rgba8))
    mixed = bt.TileAtlas.new(cfg, device)
    for dest in (1, 2):
        rc, untouched, zeroed = call(a=mixed._h, ai=0, x0=0, y0=0, bake=(dest, 0, 0, 9, 7, 0))
        assert rc == BT_ERR_UNSUPPORTED and untouched and zeroed, dest
    assert call(a=mixed._h, ai=0, x0=0, y0=0, bake=(3, 0, 0, 9, 7, 0))[0] == 0
    # a side above 8192 and more than 2^22 cells: mosaics wide enough for such windows, which need no tile, since the refusal comes first
    cfg = bt.TerrainConfig(lod_count=10, atlas_size=4, path="terrains/regions_limits", model=bt.TerrainModel.planar((0, 0, 0), 1000.0, 0.0, 1.0))
    cfg.add_attachment(bt.AttachmentConfig(name="height", texture_size=72, border_size=2, format=bt.AttachmentFormat.R16))
    wide = bt.TileAtlas.new(cfg, device)  # 68 << 9 = 34816 across
    for kw, word in ((dict(width=8193, height=1), b"side"), (dict(width=1, height=8193), b"side"), (dict(width=2049, height=2048), b"cells"),
                     (dict(width=2048, height=2049), b"cells"), (dict(width=8192, height=513), b"cells")):
        rc, untouched, zeroed = call(a=wide._h, ai=0, lod=9, x0=0, y0=0, **kw)
        assert rc == BT_ERR_INVALID_ARGUMENT and untouched and zeroed and word in L.bt_last_error(), (kw, L.bt_last_error())
    assert L.bt_atlas_label_regions(None, 0, 0, 0, 0, 0, 0, 0, None, None, None, None, None, 0, None, None, 0, None) == BT_ERR_INVALID_ARGUMENT
    assert [whole(atlas, ai) for ai in (G, H)][1] == before[1]  # the refused calls wrote nothing to the heights (the accepted bakes wrote G)


@pytest.mark.gpu
def test_a_window_no_tile_covers(device):
    cfg = bt.TerrainConfig(lod_count=3, atlas_size=4, path="terrains/regions_empty", model=bt.TerrainModel.planar((0, 0, 0), 1000.0, 0.0, 1.0))
    cfg.add_attachment(bt.AttachmentConfig(name="height", texture_size=16, border_size=2, format=bt.AttachmentFormat.R16))
    atlas = bt.TileAtlas.new(cfg, device)
    label, id_, table, stats = atlas.label_regions(0, 5, 7, 30, 20, hi=0)  # every texel reads 0: one region of every cell (hi alone: from 0)
    assert not label.any() and not id_.any() and len(table) == 1
    assert tuple(table[0]) == (0, 600, 0, 0, 29, 19, 0, 0, 100, 0)
    assert input_stats(stats) == dict(cells=600, members=600, regions=1, regions_written=1, largest_area=600, largest_label=0, tiles_missing=9, baked=0)
    label, id_, table, stats = atlas.label_regions(0, 5, 7, 30, 20, lo=1)  # lo alone: up to 65535
    assert (label == _ffi.REGIONS_NONE).all() and (id_ == _ffi.REGIONS_NONE).all() and len(table) == 0 and stats["regions"] == 0
    assert stats["largest_area"] == 0 and stats["largest_label"] == _ffi.REGIONS_NONE

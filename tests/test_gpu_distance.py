"""bt_atlas_distance_field on the device against the model of the definition (tests/_distance_model.py, pinned by test_distance_model.py).

Both planes are compared over every cell: no tolerance, no excluded cell; so is every field of bt_distance_stats but launches, which is
pinned to the documented count.  The scenes are those of tests/_distance_cases.py; the model's planes are computed once per scene (without
a GPU, from the CPU oracle's state) and shared.  Each check also reads the window back with bt_atlas_read_region and requires the texels
the model was given.  A bake is compared through a second atlas that receives the model's texels by bt_atlas_write_region."""
import ctypes as C

import numpy as np
import pytest

import _distance_cases as DC
import _distance_model as M
import bevy_terrain_amd as bt
from _splat_cases import G, H
from bevy_terrain_amd import _ffi
from test_gpu_splat import device_atlas

BT_ERR_INVALID_ARGUMENT, BT_ERR_UNSUPPORTED = -1, -5
LAUNCHES, LAUNCHES_BAKE = 6, 7  # the gather, the column phase's three, the row phase, the finish; the gather of a bake's destination


@pytest.fixture(scope="module")
def device():
    return bt.Device(0)


@pytest.fixture(scope="module")
def atlases(device):
    """one device atlas per spec, made on first use: the scenes only read"""
    made = {}

    def get(name):
        spec = DC.SCENES[name]["spec"]
        if spec not in made:
            made[spec] = device_atlas(device, spec)
        return made[spec]

    return get


def run(atlas, name, **kw):
    scene = DC.SCENES[name]
    x0, y0, w, h = scene["rect"]
    return atlas.distance_field(scene["attachment"], x0, y0, w, h, lo=scene["lo"], hi=scene["hi"], channel=scene["channel"], seeds=DC.window(name)[2],
                                invert=scene["invert"], lod=scene["lod"], side=scene["side"], **kw)


def input_stats(stats):
    return {k: v for k, v in stats.items() if k not in M.SCHEDULE}


def check_scene(atlas, name):
    scene = DC.SCENES[name]
    texels, _, *want, stats = DC.expected(name)
    x0, y0, w, h = scene["rect"]
    got_texels, missing = atlas.read_region(scene["attachment"], x0, y0, w, h, lod=scene["lod"], side=scene["side"])
    assert np.array_equal(got_texels, texels) and missing == stats["tiles_missing"], "the device atlas is not the state the model was given"
    *got, stats_d = run(atlas, name)
    for plane, g, e in zip(("dist2", "nearest"), got, want):
        assert g.dtype == e.dtype and g.shape == e.shape, (name, plane)
        differ = np.argwhere(g != e)
        assert differ.size == 0, (name, plane, len(differ), differ[:5], g[tuple(differ[0])], e[tuple(differ[0])])
    assert input_stats(stats_d) == stats, name
    assert stats_d["launches"] == LAUNCHES, stats_d
    assert not any(stats_d["edit"].values()) and stats_d["changed"] == []
    return got, stats_d


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["one_cell_seed", "one_cell_empty", "one_row", "one_column", "two_by_two"])
def test_degenerate_windows(device, atlases, name):
    check_scene(atlases(name), name)


@pytest.mark.gpu
def test_no_seed_and_every_cell_a_seed(device, atlases):
    (dist2, nearest), stats = check_scene(atlases("no_seeds"), "no_seeds")
    assert (dist2 == _ffi.DISTANCE_NONE).all() and (nearest == _ffi.DISTANCE_NONE).all() and stats["max_dist2"] == 0 and stats["sum_dist2"] == 0
    (dist2, nearest), stats = check_scene(atlases("all_seeds"), "all_seeds")
    assert not dist2.any() and np.array_equal(nearest.ravel(), np.arange(nearest.size)) and stats["seeds"] == stats["cells"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", DC.CORNERS)
def test_one_seed_at_a_corner(device, atlases, name):
    (dist2, _), stats = check_scene(atlases(name), name)
    h, w = dist2.shape
    assert stats["max_dist2"] == (w - 1) ** 2 + (h - 1) ** 2


@pytest.mark.gpu
@pytest.mark.parametrize("name", DC.SIZES)
def test_sizes_around_the_kernels_units(device, atlases, name):
    check_scene(atlases(name), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["checkerboard", "mirror_row", "mirror_column", "mirror_diagonal", "rows_about_a_band", "two_columns", "stop_rule"])
def test_ties(device, atlases, name):
    (dist2, nearest), _ = check_scene(atlases(name), name)
    w = nearest.shape[1]
    if name == "stop_rule":
        assert dist2[10, 10] == 9 and nearest[10, 10] == 10 * w + 13
    if name == "rows_about_a_band":
        assert (nearest[48] // w == 1).all() and (nearest[49] // w == 95).all()
    if name == "two_columns":
        assert (nearest[:, 12] % w == 4).all() and (nearest[:, 13] % w == 20).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["one_seed_column", "one_seed_row"])
def test_seeds_confined_to_a_line(device, atlases, name):
    check_scene(atlases(name), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", DC.SOURCES)
def test_seed_sources(device, atlases, name):
    _, stats = check_scene(atlases(name), name)
    if name.startswith("missing_tiles"):
        assert stats["tiles_missing"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cube_side", "lod_below_the_top", "no_lod0"])
def test_other_layers(device, atlases, name):
    got, _ = check_scene(atlases(name), name)
    if name == "cube_side":  # the same window of another side is another terrain: the side argument is used
        scene = DC.SCENES[name]
        other = atlases(name).distance_field(H, *scene["rect"], lo=scene["lo"], hi=scene["hi"], side=1)
        assert not np.array_equal(other[0], got[0])


@pytest.mark.gpu
def test_each_output_may_be_null_and_two_calls_agree(device, atlases):
    name = "w65_h66_1in16"
    atlas = atlases(name)
    _, _, *want, stats = DC.expected(name)
    for kw in (dict(dist2=False), dict(nearest=False), dict(dist2=False, nearest=False)):
        *got, stats_d = run(atlas, name, **kw)
        for flag, g, e in zip(("dist2", "nearest"), got, want):
            assert g is None if flag in kw else np.array_equal(g, e), (kw, flag)
        assert input_stats(stats_d) == stats and stats_d["launches"] == LAUNCHES, kw
    a, b = run(atlas, name), run(atlas, name)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:2], b[:2])) and a[2] == b[2]
    # stats NULL, changed NULL
    scene = DC.SCENES[name]
    x0, y0, w, h = scene["rect"]
    out = np.zeros((h, w), np.uint32)
    seeds = _ffi.DistanceSeedsC(0, 0, 0, 0)
    host = DC.window(name)[2]
    _ffi.check(_ffi.lib().bt_atlas_distance_field(atlas._h, H, 0, 2, x0, y0, w, h, C.byref(seeds), host.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                  out.ctypes.data_as(C.POINTER(C.c_uint32)), None, None, None, 0, None))
    assert np.array_equal(out, want[0])


@pytest.mark.gpu
def test_the_call_without_a_bake_is_a_read(device, atlases):
    atlas = atlases("w96_h96_1in16")
    before = [atlas.download_tiles(ai, 0, atlas.atlas_size).copy() for ai in (G, H)]
    check_scene(atlas, "w96_h96_1in16")
    check_scene(atlas, "alpha_band")
    assert all(b.tobytes() == atlas.download_tiles(ai, 0, atlas.atlas_size).tobytes() for ai, b in zip((G, H), before))


@pytest.mark.gpu
def test_scratch_is_reused_and_released_by_trim(device, atlases):
    """the planes stay in the context: a smaller call after a larger one allocates nothing, and bt_ctx_trim gives the bytes back"""
    atlas = atlases("w96_h96_1in16")
    device.trim()
    check_scene(atlas, "w96_h96_1in16")
    large = device.trim()
    cells = 96 * 96
    align = lambda v: (v + 255) & ~255
    assert large >= align(cells * 2) + align(cells) + align(cells * 2) + 2 * align(cells * 4)  # raw, host, r, dist2, nearest at least
    check_scene(atlas, "w96_h96_1in16")
    check_scene(atlas, "two_by_two")  # the smaller calls: in the larger one's buffers, so the same bytes come back
    scene = DC.SCENES["two_by_two"]
    small = atlas.distance_field(H, scene["rect"][0], scene["rect"][1], 3, 3, seeds=DC.points((1, 2))(3, 3))
    assert small[0].tolist() == [[5, 4, 5], [2, 1, 2], [1, 0, 1]] and (small[1] == 7).all()
    check_scene(atlas, "w96_h96_1in16")
    assert device.trim() == large
    assert device.trim() == 0
    check_scene(atlas, "two_by_two")  # allocated anew, smaller
    assert 0 < device.trim() < large


# ---------------------------------------------------------------------------------------------- the bake

BAKE_RECT = (60, 62, 50, 44)  # of planar_72: across the tile edge at 68 on both axes


@pytest.fixture(scope="module")
def bake_pair(device):
    """two atlases in one state: the first takes the device's bakes, the second the model's texels through write_region"""
    return device_atlas(device, "planar_72"), device_atlas(device, "planar_72")


def coords(changed):
    return [(t.side, t.lod, t.x, t.y) for t in changed]


def whole(atlas, ai):
    return atlas.download_tiles(ai, 0, atlas.atlas_size).tobytes()


def bake_both(pair, source, bake, outputs=True, **seeds):
    """the device's bake on the first atlas and the model's on the second, over BAKE_RECT; returns the device's stats"""
    ours, theirs = pair
    x0, y0, w, h = BAKE_RECT
    dest, channel, reach, near = bake
    texels, _ = theirs.read_region(source, x0, y0, w, h)
    seed = M.seed_plane(texels, seeds.get("channel", 0), seeds.get("lo"), seeds.get("hi"), seeds.get("seeds"), seeds.get("invert", False))
    dist2, nearest, stats = M.field(seed)
    before, _ = theirs.read_region(dest, x0, y0, w, h)
    changed_m, edit_m = theirs.write_region(dest, M.bake(before, dist2, channel, reach, near), x0, y0)
    d, n, stats_d = ours.distance_field(source, x0, y0, w, h, bake=bake, dist2=outputs, nearest=outputs, **seeds)
    if outputs:
        assert np.array_equal(d, dist2) and np.array_equal(n, nearest)
    else:
        assert d is None and n is None
    assert input_stats(stats_d) == dict(stats, tiles_missing=0) and stats_d["launches"] == LAUNCHES_BAKE
    assert coords(stats_d["changed"]) == coords(changed_m) and stats_d["edit"] == edit_m and edit_m["changed_count"] > 0
    assert whole(ours, G) == whole(theirs, G) and whole(ours, H) == whole(theirs, H)
    after, _ = ours.read_region(dest, x0, y0, w, h)
    assert np.array_equal(after[:, :, channel], M.bake_plane(dist2, reach, near))
    others = [k for k in range(4) if k != channel]
    assert np.array_equal(after[:, :, others], before[:, :, others])
    return stats_d, after[:, :, channel]


@pytest.mark.gpu
@pytest.mark.parametrize("near", [False, True])
@pytest.mark.parametrize("reach", [1, 7, 255, 65535])
@pytest.mark.parametrize("channel", [0, 1, 2, 3])
def test_bake_into_each_channel(device, bake_pair, channel, reach, near):
    _, byte = bake_both(bake_pair, H, (G, channel, reach, near), lo=33000, hi=36000)
    assert len(np.unique(byte)) > (1 if reach in (7, 255) else 0)


@pytest.mark.gpu
def test_bake_from_one_channel_of_the_destination_into_another(device, bake_pair):
    bake_both(bake_pair, G, (G, 2, 7, True), lo=0, hi=110, channel=0)


@pytest.mark.gpu
def test_bake_with_both_planes_null_and_from_a_host_plane(device, bake_pair):
    bake_both(bake_pair, H, (G, 1, 7, False), outputs=False, seeds=DC.random(64, 3)(*BAKE_RECT[:1:-1]))


@pytest.mark.gpu
def test_bake_without_a_seed(device, bake_pair):
    _, byte = bake_both(bake_pair, H, (G, 3, 7, False), seeds=DC.nothing(*BAKE_RECT[:1:-1]))
    assert (byte == 255).all()
    _, byte = bake_both(bake_pair, H, (G, 3, 7, True), seeds=DC.nothing(*BAKE_RECT[:1:-1]))
    assert (byte == 0).all()


@pytest.mark.gpu
def test_bake_over_missing_tiles(device):
    """on `partial` the rectangle meets tiles the atlas does not hold: they are seeds (lo = hi = 0) and are not written"""
    ours, theirs = device_atlas(device, "partial"), device_atlas(device, "partial")
    x0, y0, w, h = 0, 0, 48, 48
    texels, missing = theirs.read_region(H, x0, y0, w, h)
    dist2, _, stats = M.field(M.seed_plane(texels, lo=0, hi=0))
    before, _ = theirs.read_region(G, x0, y0, w, h)
    changed_m, edit_m = theirs.write_region(G, M.bake(before, dist2, 0, 9), x0, y0)
    _, _, stats_d = ours.distance_field(H, x0, y0, w, h, lo=0, hi=0, bake=dict(attachment=G, channel=0, reach=9))
    assert missing > 0 and input_stats(stats_d) == dict(stats, tiles_missing=missing)
    assert coords(stats_d["changed"]) == coords(changed_m) and stats_d["edit"] == edit_m and edit_m["tiles_missing"] > 0
    assert whole(ours, G) == whole(theirs, G) and whole(ours, H) == whole(theirs, H)


# ---------------------------------------------------------------------------------------------- refusals

@pytest.mark.gpu
def test_refusals_leave_the_outputs_untouched(device):
    atlas = device_atlas(device, "planar_72")  # its own: the accepted bakes below write
    L = _ffi.lib()
    w, h = 20, 10
    host_plane = np.ones((h, w), np.uint8)
    FT, INV = _ffi.DISTANCE_FROM_TEXELS, _ffi.DISTANCE_INVERT

    def call(a=None, ai=H, side=0, lod=2, x0=3, y0=5, width=w, height=h, seeds=(0, 0, 100, FT), host=False, bake=None, changed_cap=0, null_changed=True, null_seeds=False):
        outs = [np.full((h, w), 77, np.uint32) for _ in range(2)]
        stats = _ffi.DistanceStatsC(9, 9, 9, 9, 9, 9, 9, _ffi.EditStatsC(*([9] * 8)))
        changed = (_ffi.TileCoordinateC * 64)()
        rc = L.bt_atlas_distance_field(atlas._h if a is None else a, ai, side, lod, x0, y0, width, height, None if null_seeds else C.byref(_ffi.DistanceSeedsC(*seeds)),
                                       host_plane.ctypes.data_as(C.POINTER(C.c_uint8)) if host else None, outs[0].ctypes.data_as(C.POINTER(C.c_uint32)),
                                       outs[1].ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(_ffi.DistanceBakeC(*bake)) if bake else None,
                                       None if null_changed else changed, changed_cap, C.byref(stats))
        untouched = all((o == 77).all() for o in outs)
        zeroed = bytes(stats) == bytes(C.sizeof(stats))
        return rc, untouched, zeroed

    assert call()[0] == 0 and not call()[1] and not call()[2]
    before = [whole(atlas, ai) for ai in (G, H)]
    n = 272  # the mosaic of lod 2
    for kw in (dict(ai=2), dict(side=1), dict(lod=3), dict(x0=n - 19), dict(y0=n - 9), dict(x0=n), dict(width=n + 1, x0=0),  # what region_check refuses
               dict(null_seeds=True), dict(seeds=(0, 0, 100, 0)), dict(seeds=(0, 0, 100, INV)),  # neither FROM_TEXELS nor a host plane
               dict(seeds=(0, 0, 100, FT | 4)), dict(seeds=(0, 0, 100, 0x80000000), host=True), dict(seeds=(0, 101, 100, FT)), dict(seeds=(0, 101, 100, FT), host=True),
               dict(seeds=(1, 0, 100, FT)), dict(seeds=(4, 0, 100, FT), ai=G), dict(seeds=(0, 0, 65536, FT)), dict(seeds=(3, 0, 256, FT), ai=G),
               dict(changed_cap=1),
               dict(bake=(2, 0, 7, 0)), dict(bake=(0xFFFFFFFF, 0, 7, 0)), dict(bake=(G, 4, 7, 0)), dict(bake=(G, 0, 0, 0)), dict(bake=(G, 0, 65536, 0)), dict(bake=(G, 0, 7, 2))):
        rc, untouched, zeroed = call(**kw)
        assert rc == BT_ERR_INVALID_ARGUMENT and untouched and zeroed, (kw, rc, L.bt_last_error())
    for kw in (dict(seeds=(0, 0, 65535, FT)), dict(seeds=(3, 0, 255, FT | INV), ai=G), dict(seeds=(0, 0, 0, INV), host=True), dict(seeds=(0, 101, 100, 0), host=True),
               dict(bake=(G, 3, 65535, 1)), dict(bake=(G, 0, 1, 0), changed_cap=64, null_changed=False)):
        assert call(**kw)[0] == 0, kw
    rc, untouched, zeroed = call(bake=(H, 0, 7, 0))  # the R16 attachment takes no byte
    assert rc == BT_ERR_UNSUPPORTED and untouched and zeroed
    for kw in (dict(width=0), dict(height=0), dict(width=0, height=0), dict(width=0, bake=(G, 0, 7, 0))):  # an empty window is BT_OK with nothing touched
        rc, untouched, zeroed = call(**kw)
        assert rc == 0 and untouched and zeroed, kw
    # an odd centre size (T = 17, b = 2: 13 centre texels); a destination of another texture size, of another border size
    cfg = bt.TerrainConfig(lod_count=2, atlas_size=4, path="terrains/distance_odd", model=bt.TerrainModel.planar((0, 0, 0), 1000.0, 0.0, 1.0))
    cfg.add_attachment(bt.AttachmentConfig(name="height", texture_size=17, border_size=2, format=bt.AttachmentFormat.R16))
    odd = bt.TileAtlas.new(cfg, device)
    rc, untouched, zeroed = call(a=odd._h, ai=0, lod=1, x0=0, y0=0)
    assert rc == BT_ERR_UNSUPPORTED and untouched and zeroed
    cfg = bt.TerrainConfig(lod_count=3, atlas_size=4, path="terrains/distance_mixed", model=bt.TerrainModel.planar((0, 0, 0), 1000.0, 0.0, 1.0))
    cfg.add_attachment(bt.AttachmentConfig(name="height", texture_size=20, border_size=2, format=bt.AttachmentFormat.R16))
    cfg.add_attachment(bt.AttachmentConfig(name="larger", texture_size=24, border_size=2, format=bt.AttachmentFormat.Rgba8))
    cfg.add_attachment(bt.AttachmentConfig(name="thicker", texture_size=20, border_size=4, format=bt.AttachmentFormat.Rgba8))
    cfg.add_attachment(bt.AttachmentConfig(name="alike", texture_size=20, border_size=2, format=bt.AttachmentFormat.Rgba8))
    mixed = bt.TileAtlas.new(cfg, device)
    for dest in (1, 2):
        rc, untouched, zeroed = call(a=mixed._h, ai=0, x0=0, y0=0, bake=(dest, 0, 7, 0))
        assert rc == BT_ERR_UNSUPPORTED and untouched and zeroed, dest
    assert call(a=mixed._h, ai=0, x0=0, y0=0, bake=(3, 0, 7, 0))[0] == 0
    # a side above 8192 and more than 2^22 cells: mosaics wide enough for such windows, which need no tile, since the refusal comes first
    cfg = bt.TerrainConfig(lod_count=10, atlas_size=4, path="terrains/distance_limits", model=bt.TerrainModel.planar((0, 0, 0), 1000.0, 0.0, 1.0))
    cfg.add_attachment(bt.AttachmentConfig(name="height", texture_size=72, border_size=2, format=bt.AttachmentFormat.R16))
    wide = bt.TileAtlas.new(cfg, device)  # 68 << 9 = 34816 across
    for kw, word in ((dict(width=8193, height=1), b"side"), (dict(width=1, height=8193), b"side"), (dict(width=2049, height=2048), b"cells"),
                     (dict(width=2048, height=2049), b"cells"), (dict(width=8192, height=513), b"cells")):
        rc, untouched, zeroed = call(a=wide._h, ai=0, lod=9, x0=0, y0=0, **kw)
        assert rc == BT_ERR_INVALID_ARGUMENT and untouched and zeroed and word in L.bt_last_error(), (kw, L.bt_last_error())
    assert L.bt_atlas_distance_field(None, 0, 0, 0, 0, 0, 0, 0, None, None, None, None, None, None, 0, None) == BT_ERR_INVALID_ARGUMENT
    assert [whole(atlas, ai) for ai in (G, H)][1] == before[1]  # the refused calls wrote nothing to the heights (the accepted bakes wrote G)


@pytest.mark.gpu
def test_a_window_no_tile_covers(device):
    cfg = bt.TerrainConfig(lod_count=3, atlas_size=4, path="terrains/distance_empty", model=bt.TerrainModel.planar((0, 0, 0), 1000.0, 0.0, 1.0))
    cfg.add_attachment(bt.AttachmentConfig(name="height", texture_size=16, border_size=2, format=bt.AttachmentFormat.R16))
    atlas = bt.TileAtlas.new(cfg, device)
    dist2, nearest, stats = atlas.distance_field(0, 5, 7, 30, 20, hi=0)  # every texel reads 0: every cell a seed (hi alone: from 0)
    assert not dist2.any() and np.array_equal(nearest.ravel(), np.arange(600))
    assert input_stats(stats) == dict(cells=600, seeds=600, tiles_missing=9, max_dist2=0, sum_dist2=0)
    dist2, nearest, stats = atlas.distance_field(0, 5, 7, 30, 20, lo=1)  # lo alone: up to 65535
    assert (dist2 == _ffi.DISTANCE_NONE).all() and (nearest == _ffi.DISTANCE_NONE).all() and stats["seeds"] == 0

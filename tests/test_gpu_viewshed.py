"""bt_atlas_viewshed on the device against the model of the definition (tests/_viewshed_model.py, pinned by test_viewshed_model.py).

All three planes are compared over every cell: no tolerance, no excluded cell; so is every field of bt_viewshed_stats but launches.  The
scenes are those of tests/_viewshed_cases.py; the model's planes are computed once per scene (without a GPU, from the CPU oracle's state)
and shared.  Each check also reads the window back with bt_atlas_read_region and requires the texels the model was given."""
import ctypes as C

import numpy as np
import pytest

import _viewshed_cases as VC
import _viewshed_model as M
import bevy_terrain_amd as bt
from _splat_cases import G, H
from bevy_terrain_amd import _ffi
from test_gpu_splat import device_atlas

BT_ERR_INVALID_ARGUMENT, BT_ERR_UNSUPPORTED = -1, -5
PLANES = ("clearance", "count", "mask")


@pytest.fixture(scope="module")
def device():
    return bt.Device(0)


@pytest.fixture(scope="module")
def atlases(device):
    """two device atlases per spec, made on first use: the one the unplanted scenes read, and the one the planted scenes write their
    window into before their call"""
    made = {}

    def get(name):
        scene = VC.SCENES[name]
        key = (scene["spec"], scene["plant"] is not None)
        if key not in made:
            made[key] = device_atlas(device, scene["spec"])
        if scene["plant"] is not None:
            x0, y0, _, _ = scene["rect"]
            made[key].write_region(H, VC.window(name)[0], x0, y0, side=scene["side"])
        return made[key]

    return get


def run(atlas, scene, **kw):
    x0, y0, w, h = scene["rect"]
    kw = dict(dict(mask=True), **kw)
    return atlas.viewshed(H, x0, y0, w, h, scene["observers"], target_height=scene["target_height"], lod=scene["lod"], side=scene["side"], **kw)


def input_stats(stats):
    return {k: v for k, v in stats.items() if k not in M.SCHEDULE}


def check_scene(atlas, name):
    scene = VC.SCENES[name]
    raw, *want, stats = VC.expected(name)
    x0, y0, w, h = scene["rect"]
    got_raw, missing = atlas.read_region(H, x0, y0, w, h, lod=scene["lod"], side=scene["side"])
    assert np.array_equal(got_raw, raw) and missing == stats["tiles_missing"], "the device atlas is not the state the model was given"
    *got, stats_d = run(atlas, scene)
    for plane, g, e in zip(PLANES, got, want):
        assert g.dtype == e.dtype and g.shape == e.shape, (name, plane)
        differ = np.argwhere(g != e)
        assert differ.size == 0, (name, plane, len(differ), differ[:5], g[tuple(differ[0])], e[tuple(differ[0])])
    assert input_stats(stats_d) == stats, name
    assert stats_d["launches"] == 5, stats_d  # the gather, the transpose, the walk's two, the finish
    return got, stats_d


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["one_cell", "one_row", "one_column", "two_by_two"])
def test_degenerate_windows(device, atlases, name):
    check_scene(atlases(name), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", VC.SIZES)
def test_sizes_around_the_wave(device, atlases, name):
    check_scene(atlases(name), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["eight_octants", "plateau", "plateau_ridge", "tower", "extremes", "extremes_from_below"])
def test_planted_terrains(device, atlases, name):
    (clearance, count, _), _ = check_scene(atlases(name), name)
    if name == "plateau":
        assert not clearance.any() and (count == 2).all()
    if name == "plateau_ridge":
        assert clearance[VC.RIDGE_ROW, 2 + VC.RIDGE_AT + 1:].tolist() == [-(-n // VC.RIDGE_AT) for n in range(VC.RIDGE_AT + 1, 48 - 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["holes", "missing_tiles", "skipped_observers", "all_skipped"])
def test_void_and_missing_ground(device, atlases, name):
    (clearance, count, _), stats = check_scene(atlases(name), name)
    if name == "all_skipped":
        assert (clearance == _ffi.VIEWSHED_NONE).all() and not count.any() and stats["observers_used"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["radii_1_and_5", "radius_beyond"])
def test_radii(device, atlases, name):
    (clearance, _, _), _ = check_scene(atlases(name), name)
    if name == "radii_1_and_5":
        assert clearance[14, 13] != _ffi.VIEWSHED_NONE and clearance[14, 14] == _ffi.VIEWSHED_NONE  # (3, 4) from (10, 10) is inside radius 5


@pytest.mark.gpu
def test_sixty_four_observers(device, atlases):
    (_, count, mask), _ = check_scene(atlases("observers_64"), "observers_64")
    assert all(((mask >> np.uint64(o)) & np.uint64(1)).any() for o in range(64))
    assert np.array_equal(count, sum(((mask >> np.uint64(o)) & np.uint64(1)).astype(np.uint8) for o in range(64)))


@pytest.mark.gpu
def test_one_cell_listed_twice_counts_twice(device, atlases):
    (_, count, mask), _ = check_scene(atlases("one_cell_twice"), "one_cell_twice")
    assert set(np.unique(count)) == {0, 2} and set(np.unique(mask)) == {0, 3}


@pytest.mark.gpu
def test_target_heights(device, atlases):
    planes = [check_scene(atlases(name), name)[0] for name in VC.TARGETS]
    assert all(np.array_equal(p[0], planes[0][0]) for p in planes)
    assert not np.array_equal(planes[0][1], planes[1][1]) and not np.array_equal(planes[1][1], planes[2][1])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cube_side", "lod_below_the_top", "no_lod0"])
def test_other_layers(device, atlases, name):
    got, _ = check_scene(atlases(name), name)
    if name == "cube_side":  # the same window of another side is another terrain: the side argument is used
        other = run(atlases(name), dict(VC.SCENES[name], side=1))
        assert not np.array_equal(other[0], got[0])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["strip_wide", "strip_tall"])
def test_strips(device, atlases, name):
    check_scene(atlases(name), name)


@pytest.mark.gpu
def test_each_output_may_be_null_and_two_calls_agree(device, atlases):
    name = "w65_h66_centre"
    scene, atlas = VC.SCENES[name], atlases(name)
    _, *want, stats = VC.expected(name)
    for off in PLANES + (None,):
        kw = {k: False for k in PLANES} if off is None else {off: False}  # None: stats only
        *got, stats_d = run(atlas, scene, **kw)
        for flag, g, e in zip(PLANES, got, want):
            assert g is None if flag in kw else np.array_equal(g, e), (off, flag)
        assert input_stats(stats_d) == stats, off
    a, b = run(atlas, scene), run(atlas, scene)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3])) and a[3] == b[3]
    # stats NULL
    x0, y0, w, h = scene["rect"]
    out = np.zeros((h, w), np.uint32)
    obs = (_ffi.ViewshedObserverC * 1)(_ffi.ViewshedObserverC(*scene["observers"][0]))
    _ffi.check(_ffi.lib().bt_atlas_viewshed(atlas._h, H, 0, 2, x0, y0, w, h, obs, 1, scene["target_height"], out.ctypes.data_as(C.POINTER(C.c_uint32)), None, None, None))
    assert np.array_equal(out, want[0])


@pytest.mark.gpu
def test_the_call_is_a_read(device, atlases):
    atlas = atlases("w96_h96_centre")
    before = atlas.download_tiles(H, 0, atlas.atlas_size).copy()
    check_scene(atlas, "w96_h96_centre")
    assert before.tobytes() == atlas.download_tiles(H, 0, atlas.atlas_size).tobytes()


@pytest.mark.gpu
def test_scratch_is_reused_and_released_by_trim(device, atlases):
    """the planes stay in the context: a smaller call after a larger one allocates nothing, and bt_ctx_trim gives the bytes back"""
    atlas = atlases("w96_h96_centre")
    device.trim()
    check_scene(atlas, "w96_h96_centre")
    large = device.trim()
    cells = 96 * 96
    align = lambda v: (v + 255) & ~255
    assert large >= align(cells * 2) + align(cells * 4) + align(cells) + align(cells * 8)  # raw, clearance, count, mask at least; read_region's besides
    check_scene(atlas, "w96_h96_centre")
    check_scene(atlases("w63_h66_corner"), "w63_h66_corner")  # the smaller call: in the larger one's buffers, so the same bytes come back
    assert device.trim() == large
    assert device.trim() == 0
    check_scene(atlases("w63_h66_corner"), "w63_h66_corner")  # allocated anew, smaller
    assert 0 < device.trim() < large


@pytest.mark.gpu
def test_refusals_leave_the_outputs_untouched(device, atlases):
    atlas = atlases("w63_h66_corner")
    L = _ffi.lib()
    w, h = 20, 10

    def call(a=None, ai=H, side=0, lod=2, x0=3, y0=5, width=w, height=h, observers=((4, 5, 10, 0),), count=None, target_height=3, null_observers=False):
        outs = [np.full((h, w), 77, t) for t in (np.uint32, np.uint8, np.uint64)]
        stats = _ffi.ViewshedStatsC(*([9] * 10), (C.c_uint32 * 5)(9, 9, 9, 9, 9))
        arr = (_ffi.ViewshedObserverC * max(len(observers), 1))(*[_ffi.ViewshedObserverC(*o) for o in observers])
        rc = L.bt_atlas_viewshed(atlas._h if a is None else a, ai, side, lod, x0, y0, width, height, None if null_observers else arr,
                                 len(observers) if count is None else count, target_height, outs[0].ctypes.data_as(C.POINTER(C.c_uint32)),
                                 outs[1].ctypes.data_as(C.POINTER(C.c_uint8)), outs[2].ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(stats))
        untouched = all((o == 77).all() for o in outs)
        zeroed = all(getattr(stats, f) == 0 for f, _ in _ffi.ViewshedStatsC._fields_[:10]) and not any(stats._padding)
        return rc, untouched, zeroed

    assert call()[0] == 0 and not call()[1] and not call()[2]
    n = 272  # the mosaic of lod 2
    many = tuple((i % w, i % h, 1, 0) for i in range(65))
    for kw in (dict(ai=2), dict(side=1), dict(lod=3), dict(x0=n - 19), dict(y0=n - 9), dict(x0=n), dict(width=n + 1, x0=0),  # what region_check refuses
               dict(null_observers=True), dict(count=0), dict(observers=many), dict(observers=many[:64], count=65),
               dict(observers=((w, 5, 0, 0),)), dict(observers=((4, h, 0, 0),)), dict(observers=((4, 5, 0, 0), (0xFFFFFFFF, 0, 0, 0))),  # outside the window
               dict(observers=((4, 5, 65536, 0),)), dict(target_height=65536)):
        rc, untouched, zeroed = call(**kw)
        assert rc == BT_ERR_INVALID_ARGUMENT and untouched and zeroed, (kw, rc)
    assert call(observers=many[:64])[0] == 0 and call(observers=((4, 5, 65535, 0xFFFFFFFF),), target_height=65535)[0] == 0
    rc, untouched, zeroed = call(ai=G)  # the Rgba8 attachment
    assert rc == BT_ERR_UNSUPPORTED and untouched and zeroed
    for kw in (dict(width=0), dict(height=0), dict(width=0, height=0)):  # an empty window is BT_OK with nothing touched
        rc, untouched, zeroed = call(**kw)
        assert rc == 0 and untouched and zeroed, kw
    # an odd centre size (T = 17, b = 2: 13 centre texels)
    cfg = bt.TerrainConfig(lod_count=2, atlas_size=4, path="terrains/viewshed_odd", model=bt.TerrainModel.planar((0, 0, 0), 1000.0, 0.0, 1.0))
    cfg.add_attachment(bt.AttachmentConfig(name="height", texture_size=17, border_size=2, format=bt.AttachmentFormat.R16))
    odd = bt.TileAtlas.new(cfg, device)
    rc, untouched, zeroed = call(a=odd._h, ai=0, lod=1, x0=0, y0=0)
    assert rc == BT_ERR_UNSUPPORTED and untouched and zeroed
    # a side above 32768 and more than 2^22 cells: mosaics wide enough for such windows, which need no tile, since the refusal comes first
    cfg = bt.TerrainConfig(lod_count=10, atlas_size=4, path="terrains/viewshed_limits", model=bt.TerrainModel.planar((0, 0, 0), 1000.0, 0.0, 1.0))
    cfg.add_attachment(bt.AttachmentConfig(name="height", texture_size=72, border_size=2, format=bt.AttachmentFormat.R16))
    wide = bt.TileAtlas.new(cfg, device)  # 68 << 9 = 34816 across
    for kw, word in ((dict(width=32769, height=1), b"side"), (dict(width=1, height=32769), b"side"), (dict(width=2049, height=2048), b"cells"),
                     (dict(width=2048, height=2049), b"cells"), (dict(width=32768, height=129), b"cells")):
        rc, untouched, zeroed = call(a=wide._h, ai=0, lod=9, x0=0, y0=0, observers=((0, 0, 0, 0),), **kw)
        assert rc == BT_ERR_INVALID_ARGUMENT and untouched and zeroed and word in L.bt_last_error(), (kw, L.bt_last_error())
    assert L.bt_atlas_viewshed(None, 0, 0, 0, 0, 0, 0, 0, None, 0, 0, None, None, None, None) == BT_ERR_INVALID_ARGUMENT


@pytest.mark.gpu
def test_a_window_no_tile_covers_is_all_void(device):
    cfg = bt.TerrainConfig(lod_count=3, atlas_size=4, path="terrains/viewshed_empty", model=bt.TerrainModel.planar((0, 0, 0), 1000.0, 0.0, 1.0))
    cfg.add_attachment(bt.AttachmentConfig(name="height", texture_size=16, border_size=2, format=bt.AttachmentFormat.R16))
    atlas = bt.TileAtlas.new(cfg, device)
    clearance, count, mask, stats = atlas.viewshed(0, 5, 7, 30, 20, [(3, 3, 10), (29, 19, 0, 4)], mask=True)
    assert (clearance == _ffi.VIEWSHED_NONE).all() and not count.any() and not mask.any()
    assert input_stats(stats) == dict(cells=600, voids=600, tiles_missing=9, observers_used=0, observers_skipped=2, covered=0, visible=0, max_clearance=0, samples=0)

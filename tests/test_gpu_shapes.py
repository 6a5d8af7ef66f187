"""bt_atlas_rasterize_shapes on the device against the model of the definition (tests/_shapes_model.py, pinned by test_shapes_model.py).

The scenes are those of tests/_shapes_cases.py.  Each runs on a pair of atlases in one state: the first takes the device's call, the second
the model's texels through bt_atlas_write_region over U.  count, last, the texels and every field of bt_shapes_stats but launches are
compared with no tolerance and no excluded cell; `changed`, stats->edit and every layer of both attachments are compared after the write.
launches is pinned to the documented count."""
import ctypes as C

import numpy as np
import pytest

import _shapes_cases as SC
import _shapes_model as M
import bevy_terrain_amd as bt
from _splat_cases import G, H
from bevy_terrain_amd import _ffi
from test_gpu_splat import device_atlas

BT_ERR_INVALID_ARGUMENT, BT_ERR_UNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def device():
    return bt.Device(0)


@pytest.fixture(scope="module")
def pairs(device):
    """two device atlases per spec, made on first use; every scene leaves them in one state again"""
    made = {}

    def get(spec):
        if spec not in made:
            made[spec] = (device_atlas(device, spec), device_atlas(device, spec))
        return made[spec]

    return get


def api_shapes(shapes):
    """the model's shapes as TileAtlas.rasterize_shapes takes them with fixed=True"""
    return [dict(polygon=s["contours"], nonzero=s["nonzero"], op=s["op"], value=s["value"]) if "contours" in s
            else dict(stroke=s["points"], half_width=s["r"], closed=s["closed"], op=s["op"], value=s["value"]) for s in shapes]


def coords(changed):
    return [(t.side, t.lod, t.x, t.y) for t in changed]


def whole(atlas):
    return [atlas.download_tiles(ai, 0, atlas.atlas_size).tobytes() for ai in (G, H)]


def input_stats(stats):
    return {k: v for k, v in stats.items() if k not in M.SCHEDULE + ("edit", "changed")}


def expect(theirs, scene, shapes=None, write=True):
    """the model's planes, texels and stats for a scene from the state of `theirs`; with write: its texels go into `theirs` over U"""
    x0, y0, w, h = scene["rect"]
    where = dict(lod=scene["lod"], side=scene["side"])
    ai = scene["attachment"]
    texels, _ = theirs.read_region(ai, x0, y0, w, h, **where)
    count, last, out, stats = M.raster(texels, scene["shapes"] if shapes is None else shapes, scene["channel"])
    u = stats["box"]
    changed, edit, stats["tiles_missing"] = [], {name: 0 for name, _ in _ffi.EditStatsC._fields_}, 0
    if u != M.EMPTY:
        stats["tiles_missing"] = theirs.read_region(ai, x0 + u[0], y0 + u[1], u[2] - u[0] + 1, u[3] - u[1] + 1, **where)[1]
        if write:
            changed, edit = theirs.write_region(ai, np.ascontiguousarray(out[u[1]:u[3] + 1, u[0]:u[2] + 1]), x0 + u[0], y0 + u[1], **where)
    return texels, count, last, out, stats, changed, edit


def run(ours, scene, shapes=None, **kw):
    x0, y0, w, h = scene["rect"]
    return ours.rasterize_shapes(scene["attachment"], x0, y0, w, h, api_shapes(scene["shapes"] if shapes is None else shapes), channel=scene["channel"], lod=scene["lod"],
                                 side=scene["side"], fixed=True, **kw)


def check_scene(pair, name, shapes=None):
    ours, theirs = pair
    scene = SC.SCENES[name]
    texels, count, last, out, stats, changed, edit = expect(theirs, scene, shapes)
    count_d, last_d, stats_d = run(ours, scene, shapes)
    for plane, g, e in (("count", count_d, count), ("last", last_d, last)):
        assert g.dtype == e.dtype and g.shape == e.shape, (name, plane)
        differ = np.argwhere(g != e)
        assert differ.size == 0, (name, plane, len(differ), differ[:5], g[tuple(differ[0])], e[tuple(differ[0])])
    assert input_stats(stats_d) == stats, name
    assert stats_d["launches"] == (0 if stats["box"] == M.EMPTY else 2), stats_d
    assert coords(stats_d["changed"]) == coords(changed) and stats_d["edit"] == edit, name
    x0, y0, w, h = scene["rect"]
    after, _ = ours.read_region(scene["attachment"], x0, y0, w, h, lod=scene["lod"], side=scene["side"])
    assert np.array_equal(after, theirs.read_region(scene["attachment"], x0, y0, w, h, lod=scene["lod"], side=scene["side"])[0]), name
    if not stats["tiles_missing"]:  # (a tile the atlas does not hold reads 0 whatever was folded)
        assert np.array_equal(after, out), name
    assert whole(ours) == whole(theirs), name
    return count_d, last_d, stats_d, texels, after


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["one_cell", "one_cell_missed", "one_row", "one_column"])
def test_degenerate_windows(device, pairs, name):
    check_scene(pairs(SC.SCENES[name]["spec"]), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SC.BLOCKS)
def test_windows_about_the_kernels_block(device, pairs, name):
    _, _, stats, _, _ = check_scene(pairs("planar_72"), name)
    w, h = SC.SCENES[name]["rect"][2:]
    assert stats["box"] == (0, 0, w - 1, h - 1) and stats["covered"] == w * h


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["square_ccw", "square_cw", "vertex_on_a_sample_row", "horizontal_edge_on_a_sample_row", "pentagram_even_odd", "pentagram_nonzero", "line_45",
                                  "line_half", "three_four_five", "three_four_five_less_one"])
def test_boundary_rules(device, pairs, name):
    count, _, stats, _, _ = check_scene(pairs("planar_72"), name)
    want = {"square_ccw": 16, "square_cw": 16, "pentagram_even_odd": 65, "pentagram_nonzero": 95, "line_45": 11, "line_half": 11}.get(name)
    assert want is None or stats["covered"] == want
    if name.startswith("square"):
        assert np.array_equal(np.argwhere(count), [[y, x] for y in range(2, 6) for x in range(2, 6)])


@pytest.mark.gpu
@pytest.mark.parametrize("name", SC.HOLES)
def test_a_polygon_with_a_hole(device, pairs, name):
    count, _, _, _, _ = check_scene(pairs("planar_72"), name)
    assert count[4, 5] == 1 and count[9, 10] == ("hole_filled" in SC.SCENES[name]["reach"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["larger_than_the_window", "all_outside", "partly_outside"])
def test_shapes_and_the_window(device, pairs, name):
    pair = pairs("planar_72")
    before = whole(pair[0])
    count, last, stats, _, _ = check_scene(pair, name)
    if name == "all_outside":
        assert stats["shapes_culled"] == stats["shapes"] == 3 and stats["box"] == M.EMPTY and not count.any() and (last == M.NONE).all()
        assert stats["covered"] == stats["written"] == 0 and not any(stats["edit"].values()) and whole(pair[0]) == before
    if name == "partly_outside":
        assert stats["shapes_culled"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["chunk_straddle", "long_segment", "duplicates_disc_closed"])
def test_chunks_wide_products_and_degenerate_vertices(device, pairs, name):
    _, _, stats, _, _ = check_scene(pairs("planar_72"), name)
    assert name != "long_segment" or stats["covered"] == 845


@pytest.mark.gpu
@pytest.mark.parametrize("name", SC.OPS + [f"channel_{c}" for c in range(4)])
def test_every_op_in_both_formats_and_each_channel(device, pairs, name):
    _, _, stats, texels, after = check_scene(pairs("planar_72"), name)
    assert stats["covered"] > 0
    if texels.ndim == 3:
        c = SC.SCENES[name]["channel"]
        others = [k for k in range(4) if k != c]
        assert np.array_equal(after[:, :, others], texels[:, :, others])
    else:
        assert after.min() >= 1


@pytest.mark.gpu
def test_r16_holes_stay_and_results_clamp_to_one(device, pairs):
    _, _, stats, texels, after = check_scene(pairs("planar_b2"), "r16_holes")
    assert (texels == 0).any() and np.array_equal(after == 0, texels == 0)
    assert (after == 1).any() and stats["written"] > 0  # the SUB of 65535 along the stroke


@pytest.mark.gpu
def test_order_matters(device, pairs):
    pair = pairs("planar_72")
    *_, a = check_scene(pair, "set_then_add")
    *_, b = check_scene(pair, "add_then_set")
    assert (a[8, 8, 0], b[8, 8, 0]) == (45, 40)


@pytest.mark.gpu
def test_count_saturates_and_the_most_shapes(device, pairs):
    pair = pairs("planar_72")
    count, last, _, _, _ = check_scene(pair, "count_saturates")
    assert count.max() == 255 and last[6, 7] == 299
    count, last, stats, _, _ = check_scene(pair, "max_shapes")
    assert stats["shapes"] == M.MAX_SHAPES and last[last != M.NONE].max() == M.MAX_SHAPES - 1 and (last == M.NONE).any()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["missing_tiles", "missing_tiles_r16", "cube_side", "lod_below_the_top"])
def test_other_layers(device, pairs, name):
    _, _, stats, _, _ = check_scene(pairs(SC.SCENES[name]["spec"]), name)
    if name.startswith("missing_tiles"):
        assert stats["tiles_missing"] > 0 and stats["edit"]["tiles_missing"] > 0


@pytest.mark.gpu
def test_dry_run_is_a_read_and_each_output_may_be_null_and_two_calls_agree(device, pairs):
    ours, theirs = pairs("planar_72")
    name = "partly_outside"
    scene = SC.SCENES[name]
    before = whole(ours)
    _, count, last, _, stats, _, _ = expect(theirs, scene, write=False)
    for kw in (dict(), dict(count=False), dict(last=False), dict(count=False, last=False)):
        count_d, last_d, stats_d = run(ours, scene, dry_run=True, **kw)
        assert (count_d is None if "count" in kw else np.array_equal(count_d, count)) and (last_d is None if "last" in kw else np.array_equal(last_d, last)), kw
        assert input_stats(stats_d) == stats and stats_d["launches"] == 2 and not any(stats_d["edit"].values()) and stats_d["changed"] == [], kw
    assert whole(ours) == before == whole(theirs)
    # `changed` is not written, stats may be NULL, changed may be NULL
    x0, y0, w, h = scene["rect"]
    vertices, entries = bt.TileAtlas.pack_shapes(api_shapes(scene["shapes"]), fixed=True)
    changed = (_ffi.TileCoordinateC * 8)(*[_ffi.TileCoordinateC(7, 7, 7, 7)] * 8)
    out = np.zeros((h, w), np.uint8)
    args = (ours._h, G, 0, 2, x0, y0, w, h, 0, vertices.ctypes.data_as(C.POINTER(_ffi.ShapeVertexC)), len(vertices), entries.ctypes.data_as(C.POINTER(_ffi.ShapeC)), len(entries))
    _ffi.check(_ffi.lib().bt_atlas_rasterize_shapes(*args, _ffi.SHAPES_DRY_RUN, out.ctypes.data_as(C.POINTER(C.c_uint8)), None, changed, 8, None))
    assert np.array_equal(out, count) and all((t.side, t.lod, t.x, t.y) == (7, 7, 7, 7) for t in changed)
    _ffi.check(_ffi.lib().bt_atlas_rasterize_shapes(*args, _ffi.SHAPES_DRY_RUN, None, None, None, 0, None))
    assert whole(ours) == before
    a, b = run(ours, scene, dry_run=True), run(ours, scene, dry_run=True)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]
    # two writes: the second folds into the first one's texels, on both atlases alike
    first = check_scene((ours, theirs), "lod_below_the_top")
    second = check_scene((ours, theirs), "lod_below_the_top")
    assert first[0].tobytes() == second[0].tobytes() and first[4].tobytes() != second[4].tobytes()


@pytest.mark.gpu
def test_scratch_is_reused_and_released_by_trim(device, pairs):
    pair = pairs("planar_72")
    device.trim()
    check_scene(pair, "block_200x100")
    large = device.trim()
    assert large >= 200 * 100 * (4 + 1 + 2)  # U's texels and its two planes at least
    check_scene(pair, "block_200x100")
    check_scene(pair, "square_ccw")  # the smaller call: in the larger one's buffers, so the same bytes come back
    check_scene(pair, "block_200x100")
    assert device.trim() == large
    assert device.trim() == 0
    check_scene(pair, "square_ccw")
    assert 0 < device.trim() < large


@pytest.mark.gpu
def test_refusals_leave_the_outputs_untouched(device):
    atlas = device_atlas(device, "planar_72")
    L = _ffi.lib()
    w, h = 20, 10
    good = [M.polygon([SC.square(1, 5), SC.square(2, 4)], nonzero=True, op=M.ADD, value=3), M.stroke(SC.cells((1, 1), (3, 3)), 100, closed=True)]
    good_vertices, good_entries = M.pack(good)
    made = {}

    def call(a=None, ai=G, side=0, lod=2, x0=3, y0=5, width=w, height=h, channel=0, flags=0, entry=None, vertex=None, null_vertices=False, null_shapes=False, entry_count=None,
             changed_cap=0, null_changed=True):
        vertices, entries = good_vertices.copy(), good_entries.copy()
        if entry:
            entries[entry[0], entry[1]] = entry[2]
        if vertex:
            vertices[vertex[0]] = vertex[1:]
        made["expected_entry"] = M.validate(vertices, entries, width, height)[1]
        count, last = np.full((h, w), 77, np.uint8), np.full((h, w), 77, np.uint16)
        stats = _ffi.ShapesStatsC(9, 9, 9, 9, 9, 9, _ffi.ShapeBoxC(9, 9, 9, 9), 9, 9, _ffi.EditStatsC(*([9] * 8)))
        changed = (_ffi.TileCoordinateC * 64)()
        rc = L.bt_atlas_rasterize_shapes(atlas._h if a is None else a, ai, side, lod, x0, y0, width, height, channel,
                                         None if null_vertices else vertices.ctypes.data_as(C.POINTER(_ffi.ShapeVertexC)), len(vertices),
                                         None if null_shapes else entries.ctypes.data_as(C.POINTER(_ffi.ShapeC)), len(entries) if entry_count is None else entry_count, flags,
                                         count.ctypes.data_as(C.POINTER(C.c_uint8)), last.ctypes.data_as(C.POINTER(C.c_uint16)), None if null_changed else changed, changed_cap,
                                         C.byref(stats))
        return rc, bool((count == 77).all() and (last == 77).all()), bytes(stats) == bytes(C.sizeof(stats))

    assert call(flags=1)[0] == 0 and not call(flags=1)[1] and not call(flags=1)[2]
    before = whole(atlas)
    n = 272
    KIND, FLAGS, FIRST, COUNT, R, OP, VALUE, PAD = range(8)
    for kw in (dict(ai=2), dict(side=1), dict(lod=3), dict(x0=n - 19), dict(y0=n - 9), dict(x0=n), dict(width=n + 1, x0=0),  # what the read refuses
               dict(null_vertices=True), dict(null_shapes=True), dict(channel=4), dict(channel=1, ai=H), dict(flags=2), dict(flags=0x80000001), dict(changed_cap=1),
               dict(entry=(0, KIND, 2)), dict(entry=(0, FLAGS, 7)), dict(entry=(2, FLAGS, M.MORE)), dict(entry=(2, FLAGS, M.NONZERO)), dict(entry=(1, OP, 5)), dict(entry=(2, VALUE, 256)),
               dict(entry=(2, VALUE, 65536), ai=H), dict(entry=(1, PAD, 1)), dict(entry=(0, R, 1)), dict(entry=(2, R, M.MAX_HALF_WIDTH + 1)), dict(entry=(0, COUNT, 2)),
               dict(entry=(2, COUNT, 0)), dict(entry=(2, COUNT, 3)), dict(entry=(2, FIRST, 0xFFFFFFFF)), dict(vertex=(5, M.MAX_COORD + 1, 0)), dict(vertex=(9, 0, -M.MAX_COORD - 1)),
               dict(entry=(1, OP, M.SET)), dict(entry=(1, VALUE, 4)), dict(entry=(1, FLAGS, 0)), dict(entry=(1, FLAGS, M.NONZERO | M.MORE)), dict(entry_count=1)):
        rc, untouched, zeroed = call(**kw)
        assert rc == BT_ERR_INVALID_ARGUMENT and untouched and zeroed, (kw, rc, L.bt_last_error())
        if "entry" in kw and not (kw["entry"][1] == VALUE and kw["entry"][2] == 256):  # the message names the entry the model names (the format's top: this call's own rule)
            assert made["expected_entry"] != M.NO_ENTRY and b"entry %d:" % made["expected_entry"] in L.bt_last_error(), (kw, L.bt_last_error())
    for kw in (dict(entry=(2, VALUE, 255)), dict(entry=(2, VALUE, 65535), ai=H), dict(channel=3), dict(changed_cap=64, null_changed=False), dict(vertex=(5, M.MAX_COORD, -M.MAX_COORD))):
        assert call(flags=1, **kw)[0] == 0, kw  # (dry runs: the atlas stays as it is)
    for kw in (dict(width=0), dict(height=0), dict(entry_count=0), dict(entry_count=0, null_shapes=True)):  # nothing to do: BT_OK with nothing touched
        rc, untouched, zeroed = call(**kw)
        assert rc == 0 and untouched and zeroed, kw
    assert whole(atlas)[1] == before[1]
    # an odd centre size
    cfg = bt.TerrainConfig(lod_count=2, atlas_size=4, path="terrains/shapes_odd", model=bt.TerrainModel.planar((0, 0, 0), 1000.0, 0.0, 1.0))
    cfg.add_attachment(bt.AttachmentConfig(name="height", texture_size=17, border_size=2, format=bt.AttachmentFormat.R16))
    odd = bt.TileAtlas.new(cfg, device)
    rc, untouched, zeroed = call(a=odd._h, ai=0, lod=1, x0=0, y0=0)
    assert rc == BT_ERR_UNSUPPORTED and untouched and zeroed
    # a side above 8192 and more than 2^22 cells: a mosaic wide enough for such windows, which needs no tile, since the refusal comes first
    cfg = bt.TerrainConfig(lod_count=10, atlas_size=4, path="terrains/shapes_limits", model=bt.TerrainModel.planar((0, 0, 0), 1000.0, 0.0, 1.0))
    cfg.add_attachment(bt.AttachmentConfig(name="height", texture_size=72, border_size=2, format=bt.AttachmentFormat.R16))
    wide = bt.TileAtlas.new(cfg, device)
    for kw, word in ((dict(width=8193, height=1), b"side"), (dict(width=1, height=8193), b"side"), (dict(width=2049, height=2048), b"cells"), (dict(width=8192, height=513), b"cells")):
        rc, untouched, zeroed = call(a=wide._h, ai=0, lod=9, x0=0, y0=0, **kw)
        assert rc == BT_ERR_INVALID_ARGUMENT and untouched and zeroed and word in L.bt_last_error(), (kw, L.bt_last_error())
    assert L.bt_atlas_rasterize_shapes(None, 0, 0, 0, 0, 0, 0, 0, 0, None, 0, None, 0, 0, None, None, None, 0, None) == BT_ERR_INVALID_ARGUMENT


@pytest.mark.gpu
def test_a_window_no_tile_covers(device):
    cfg = bt.TerrainConfig(lod_count=3, atlas_size=4, path="terrains/shapes_empty", model=bt.TerrainModel.planar((0, 0, 0), 1000.0, 0.0, 1.0))
    cfg.add_attachment(bt.AttachmentConfig(name="height", texture_size=16, border_size=2, format=bt.AttachmentFormat.R16))
    atlas = bt.TileAtlas.new(cfg, device)
    count, last, stats = atlas.rasterize_shapes(0, 5, 7, 30, 20, [dict(polygon=[(2, 2), (20, 3), (10, 15)], value=500)])
    shape = M.polygon([(512, 512), (5120, 768), (2560, 3840)], value=500)
    assert np.array_equal(count, M.cover(shape, 30, 20).astype(np.uint8)) and stats["covered"] == int(count.sum()) and stats["written"] == 0
    assert stats["tiles_missing"] > 0 and stats["edit"]["changed_count"] == 0

"""bt_tile_tree_tile_geometry and bt_tile_tree_build_geometry on the device: every admissible vertex equal to the CPU model of the
definition (tests/_geometry_model.py), field by field and bit for bit, no tolerance.

The scenes are tests/_geometry_cases.py's (test_geometry_model.py asserts without a GPU that they reach every branch): terrains of
lod_count 4, tree_size 4, T = 32, b = 2 preprocessed here from 128 x 128 sources, saved, and streamed back with the files of chosen tiles
removed; planar, sphere (centred away from the origin) and ellipsoid; grids 4, 5, 12, 16 (a second trip of the 256-thread workgroup) and
32 (the cap); three views each (morph ratio 0, between, 1; blend ratio 0 and above; coordinate_change_lod both ways); trees with some tiles
loaded and with none; tiles on all six sides; both layouts and both NO_* flags.  The device's best-tile table and layers must equal the
ones the model is given.

The two log2 of the definition are OCML's on the device and libm's in the model, at most an ulp of a double apart: the model flags a
vertex inadmissible when a log2 two doubles away on either side would change one of its bits, and only those vertices are skipped
(test_geometry_model.py caps them at 1 in 1000; the count is printed).

Then the device form after bt_tiling_prepass_run (equal to the host form on the list bt_tiling_prepass_read returns, slot for slot; a
capacity one vertex short leaves the last tile's slots untouched), the refusals, count == 0, and both calls as reads of the atlas."""
import ctypes as C
import os

import numpy as np
import pytest

import _geometry_cases as GC
import _geometry_model as GM
import _oracle as O
import bevy_terrain_amd as bt
from bevy_terrain_amd import _ffi
from test_gpu_sample_shapes import preprocess_and_save, stream_one_frame
from test_tile_tree_host import struct_bytes

pytestmark = pytest.mark.gpu
BT_ERR_INVALID_ARGUMENT, BT_ERR_UNSUPPORTED = -1, -5
FLAG_KW = lambda flags: dict(grid=bool(flags & GM.GRID), morph=not flags & GM.NO_MORPH, blend=not flags & GM.NO_BLEND)


@pytest.fixture(scope="module")
def device():
    return bt.Device(0)


@pytest.fixture(scope="module")
def terrains(device, tmp_path_factory):
    """terrains(kind) -> the streamed atlas of that kind, once per module, checked against what the model is given: the request list, the
    device's best-tile table == table(kind)'s, the loaded layers == the CPU oracle's tiles"""
    cache = {}

    def get(kind):
        if kind in cache:
            return cache[kind]
        model = GC.MODELS[kind][0]
        root = str(tmp_path_factory.mktemp("geometry_" + kind) / "assets")
        path = preprocess_and_save(device, root, model, GC.LODS, GC.T, GC.B, *GC.rasters(kind))
        for side, lod, x, y in GC.missing(kind):
            for name in ("height", "albedo"):
                os.remove(os.path.join(root, path, "data", name, f"{side}_{lod}_{x}_{y}.bin"))
        atlas, tree, requested, loaded, failed = stream_one_frame(device, root, path, model, GC.LODS, GC.T, GC.B, GC.atlas_size(kind), GC.view_config(4)[0],
                                                                  GC.SPECS[kind]["tree_view"])
        exp_requested, exp_loaded, exp_entries, exp_coords = GC.table(kind)
        assert requested == exp_requested and loaded == 2 * len(exp_loaded) and failed > 0
        entries, _, coords, _ = tree.read()
        assert np.array_equal(coords, exp_coords) and np.array_equal(entries, exp_entries)
        pyramid = GC.oracle_tiles(kind)
        for c, index in exp_loaded.items():
            assert np.array_equal(atlas.download_tile(0, index), pyramid[c]), c
        cache[kind] = atlas
        return atlas

    return get


@pytest.fixture(scope="module")
def trees(terrains):
    """trees(kind, grid, loaded) -> (atlas, a tile tree of that grid size on it after one update at the scene's tree view and, when loaded,
    adjust_to_tile_atlas); its table is the scene's"""
    cache = {}

    def get(kind, grid, loaded=True):
        key = (kind, grid, loaded)
        if key not in cache:
            atlas = terrains(kind)
            tree = bt.TileTree.new(atlas, GC.view_config(grid)[0])
            tree.update(GC.SPECS[kind]["tree_view"])  # (its requests are not applied: the atlas stays as streamed)
            if loaded:
                tree.adjust_to_tile_atlas()
            assert np.array_equal(tree.read()[0], GC.scene(kind, grid, loaded).entries)
            cache[key] = (atlas, tree)
        return cache[key]

    return get


def library_view(kind, grid, position):
    """the library's bt_view_state of a position, which must be the oracle's the model is given"""
    v = bt.view_state_from_config(GC.MODELS[kind][0], GC.view_config(grid)[0], position, GC.approximate_height(kind))
    assert struct_bytes(v) == struct_bytes(O.view_state_from_config(GC.MODELS[kind][1], GC.view_config(grid)[1], position, GC.approximate_height(kind)))
    return v


def assert_vertices_equal(got, exp, admissible, what):
    """field by field, bit for bit, every admissible vertex"""
    assert got.shape == exp.shape and got.dtype.itemsize == 48, (what, got.shape, exp.shape)
    for name in GM.FIELDS:
        a = np.ascontiguousarray(got[name]).view(np.uint32).reshape(got.shape + (-1,))
        b = np.ascontiguousarray(exp[name]).view(np.uint32).reshape(exp.shape + (-1,))
        bad = (a != b).any(axis=-1) & admissible
        assert not bad.any(), (what, name, int(bad.sum()), np.argwhere(bad)[:6].tolist(), got[name][bad][:3], exp[name][bad][:3])


# ---- 1. the host form against the model --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,grid,loaded,flags", GC.COMPARED)
def test_tile_geometry_equals_the_model(trees, kind, grid, loaded, flags):
    atlas, tree = trees(kind, grid, loaded)
    c = GC.scene(kind, grid, loaded)
    skipped = total = 0
    for n, position in enumerate(GC.SPECS[kind]["views"]):
        exp, trace, admissible = GC.expected(kind, grid, loaded, n, flags)
        got = tree.tile_geometry(0, c.tiles, library_view(kind, grid, position), **FLAG_KW(flags))
        assert got.shape == (len(c.tiles), tree.vertices_per_tile(bool(flags & GM.GRID)))
        assert_vertices_equal(got, exp, admissible, (kind, grid, loaded, flags, n))
        skipped, total = skipped + int((~admissible).sum()), total + admissible.size
    print(kind, grid, loaded, flags, "vertices", total, "skipped as inadmissible", skipped)
    assert skipped * 1000 <= total


def test_default_view_is_the_trees_own(trees):
    """view == NULL: bt_tile_tree_view_state, for both forms' host wrappers"""
    atlas, tree = trees("planar", 4)
    tiles = GC.tiles("planar")[:6]
    assert tree.tile_geometry(0, tiles).tobytes() == tree.tile_geometry(0, tiles, tree.view_state()).tobytes()
    exp, _, admissible = GM.geometry(O.view_state_from_config(GC.MODELS["planar"][1], GC.view_config(4)[1], GC.SPECS["planar"]["tree_view"], GC.approximate_height("planar")),
                                     GC.scene("planar", 4).P, GC.scene("planar", 4).entries, GC.scene("planar", 4).layers, GC.T, GC.B, tiles)
    assert_vertices_equal(tree.tile_geometry(0, tiles), exp, admissible, "the tree's own view")


# ---- 2. the device form ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,grid,flags", [("planar", 4, 0), ("sphere", 5, GM.GRID), ("ellipsoid", 16, 0)])
def test_build_geometry_equals_the_host_form_on_the_prepass_list(device, trees, kind, grid, flags):
    atlas, tree = trees(kind, grid)
    view = library_view(kind, grid, GC.SPECS[kind]["views"][0])
    prepass = bt.TilingPrepass(device, 4096)
    prepass.run(view)
    tiles, indirect = prepass.read()
    slots = tree.vertices_per_tile(bool(flags & GM.GRID))
    assert len(tiles) >= 16 and len(set(tiles[:, 1].tolist())) >= 2 and tiles[:, 1].max() < GC.LODS  # (the near view: the list mixes LODs)
    assert indirect[0] == len(tiles) * tree.vertices_per_tile() == len(tiles) * view.vertices_per_tile
    host = tree.tile_geometry(0, tiles, view, **FLAG_KW(flags))
    built = tree.build_geometry(prepass, 0, view, **FLAG_KW(flags))
    assert built.shape == host.shape == (len(tiles), slots) and built.tobytes() == host.tobytes()
    assert np.array_equal(built["tile_index"], np.repeat(np.arange(len(tiles), dtype=np.uint32)[:, None], slots, axis=1))
    c = GC.scene(kind, grid)
    exp, _, admissible = GM.geometry(c.views[0], c.P, c.entries, c.layers, GC.T, GC.B, tiles, flags)
    assert_vertices_equal(built, exp, admissible, (kind, grid, flags))
    # a capacity one vertex short of the need: the last tile's slots keep the sentinel, everything before them is what it was
    need = len(tiles) * slots
    sentinel = np.full((need + slots) * 48, 0xA5, np.uint8)  # (a tile's worth of guard behind the list)
    ptr = device.upload(sentinel)
    try:
        assert tree.build_geometry(prepass, 0, view, vertices=ptr, vertex_capacity=need - 1, **FLAG_KW(flags)) is None
        short = device.download(ptr, (need + slots) * 48, np.uint8)
        assert short[:(need - slots) * 48].tobytes() == host[:-1].tobytes() and (short[(need - slots) * 48:] == 0xA5).all()
        tree.build_geometry(prepass, 0, view, vertices=ptr, vertex_capacity=need + slots, **FLAG_KW(flags))  # room to spare: the list, and no more
        whole = device.download(ptr, (need + slots) * 48, np.uint8)
        assert whole[:need * 48].tobytes() == host.tobytes() and (whole[need * 48:] == 0xA5).all()
        # vertex_capacity == 0 touches nothing
        _ffi.check(_ffi.lib().bt_tile_tree_build_geometry(tree._h, atlas._h, 0, C.byref(view), prepass._h, 0, C.c_void_p(ptr), 0))
        _ffi.check(_ffi.lib().bt_tile_tree_build_geometry(tree._h, atlas._h, 0, C.byref(view), prepass._h, 0, None, 0))
        assert device.download(ptr, (need + slots) * 48, np.uint8).tobytes() == whole.tobytes()
    finally:
        device.free(ptr)


# ---- 3. refusals, count == 0 -------------------------------------------------------------------------------------------------------------

def test_refusals_and_empty_calls(device, terrains, trees):
    L = _ffi.lib()
    atlas, tree = trees("planar", 4)
    view = library_view("planar", 4, GC.SPECS["planar"]["views"][0])
    tiles = np.ascontiguousarray(GC.tiles("planar")[:3])
    tp = tiles.ctypes.data_as(C.POINTER(_ffi.TileCoordinateC))
    out = np.full(3 * 48 * 48, 0x77, np.uint8)  # three tiles of 48 strip slots
    op = out.ctypes.data_as(C.POINTER(_ffi.TerrainVertexC))
    prepass = bt.TilingPrepass(device, 64)
    prepass.run(view)
    buffer = device.upload(np.full(48 * 48 * 64, 0x5A, np.uint8))
    vp = C.c_void_p(buffer)

    def host(tree_h=tree._h, atlas_h=atlas._h, ai=0, v=C.byref(view), t=tp, count=3, flags=0, o=op, nbytes=out.nbytes):
        return L.bt_tile_tree_tile_geometry(tree_h, atlas_h, ai, v, t, count, flags, o, nbytes)

    def dev(tree_h=tree._h, atlas_h=atlas._h, ai=0, v=C.byref(view), p=prepass._h, flags=0, o=vp, capacity=48 * 64):
        return L.bt_tile_tree_build_geometry(tree_h, atlas_h, ai, v, p, flags, o, capacity)

    try:
        # NULL handles and arrays, the attachment index, the flags
        for call in (host, dev):
            assert call(tree_h=None) == BT_ERR_INVALID_ARGUMENT and L.bt_last_error()
            assert call(atlas_h=None) == BT_ERR_INVALID_ARGUMENT
            assert call(ai=2) == BT_ERR_INVALID_ARGUMENT and b"attachment" in L.bt_last_error()
            assert call(flags=8) == BT_ERR_INVALID_ARGUMENT
            assert call(ai=1) == BT_ERR_UNSUPPORTED and b"R16" in L.bt_last_error()  # the Rgba8 attachment
            assert call(o=None) == BT_ERR_INVALID_ARGUMENT
        assert host(t=None) == BT_ERR_INVALID_ARGUMENT
        assert host(nbytes=out.nbytes - 1) == BT_ERR_INVALID_ARGUMENT and b"out_bytes" in L.bt_last_error()
        assert host(flags=GM.GRID) == _ffi.BT_OK  # 25 vertices a tile fit where 48 do
        out[:] = 0x77
        assert dev(p=None) == BT_ERR_INVALID_ARGUMENT
        assert dev(o=C.c_void_p(buffer + 4)) == BT_ERR_INVALID_ARGUMENT and b"aligned" in L.bt_last_error()
        for bad in ((1, 0, 0, 0), (0, GC.LODS, 0, 0), (0, 1, 2, 0), (0, 2, 0, 4)):  # side, lod, x, y
            t = np.ascontiguousarray(np.vstack([tiles[:2], [bad]]).astype(np.uint32))
            assert host(t=t.ctypes.data_as(C.POINTER(_ffi.TileCoordinateC))) == BT_ERR_INVALID_ARGUMENT, bad
        # a view of the other kind of model
        other_view = library_view("sphere", 4, GC.SPECS["sphere"]["views"][0])
        assert host(v=C.byref(other_view)) == BT_ERR_INVALID_ARGUMENT and dev(v=C.byref(other_view)) == BT_ERR_INVALID_ARGUMENT
        # grid_size 33 (and 0), a range that is not > 0 while its stage is on
        for kw, status, flags_ok in ((dict(grid_size=33), BT_ERR_UNSUPPORTED, None), (dict(grid_size=0), BT_ERR_UNSUPPORTED, None),
                                     (dict(morph_range=0.0), BT_ERR_INVALID_ARGUMENT, GM.NO_MORPH), (dict(blend_range=float("inf")), BT_ERR_INVALID_ARGUMENT, GM.NO_BLEND),
                                     (dict(morph_range=float("nan")), BT_ERR_INVALID_ARGUMENT, GM.NO_MORPH), (dict(blend_range=-0.2), BT_ERR_INVALID_ARGUMENT, GM.NO_BLEND)):
            odd = bt.TileTree.new(atlas, bt.TerrainViewConfig(**dict(dict(tree_size=GC.TREE, grid_size=4), **kw)))
            odd.update(GC.SPECS["planar"]["tree_view"])
            assert host(tree_h=odd._h) == status and L.bt_last_error(), kw
            assert dev(tree_h=odd._h) == status, kw
            if flags_ok is not None:  # with the stage off its range is not read
                assert host(tree_h=odd._h, flags=flags_ok) == _ffi.BT_OK, kw
                out[:] = 0x77
        # count == 0: BT_OK, whatever the arrays
        assert host(count=0) == _ffi.BT_OK and host(t=None, count=0, o=None, nbytes=0) == _ffi.BT_OK
        assert dev(capacity=0) == _ffi.BT_OK
        # nothing was touched by any refusal or empty call
        assert (out == 0x77).all()
        assert (device.download(buffer, 48 * 48 * 64, np.uint8) == 0x5A).all()
        # the scratch stays in the context until bt_ctx_trim, and the call works again after it
        first = tree.tile_geometry(0, tiles, view)
        assert device.trim() > 0
        assert tree.tile_geometry(0, tiles, view).tobytes() == first.tobytes()
    finally:
        device.free(buffer)


# ---- 4. reads ----------------------------------------------------------------------------------------------------------------------------

def test_both_calls_are_reads(device, trees):
    """as test_gpu_normals.test_both_calls_are_reads: on an atlas nothing has written, neither call marks a layer written, so the job with
    no-data texels that follows takes prev_zero as often as without them; on a loaded atlas every layer's bytes are unchanged"""
    from test_gpu_tile_bounds import holed_job
    counts = []
    for read_first in (False, True):
        atlas, pre = holed_job(device)
        if read_first:
            tree = bt.TileTree.new(atlas, bt.TerrainViewConfig(tree_size=4, grid_size=4, refinement_count=2))
            model = atlas.config.model
            p = np.array(model.translation, dtype=np.float64) + [3.0, float(model.max_height) + 10.0, -2.0]
            tree.update(tuple(p))
            got = tree.tile_geometry(0, [(0, 0, 0, 0), (0, 1, 1, 0)])
            assert float(model.min_height) == 0.0 and (got["height"] == 0.0).all()  # (mix(0, 1, 0) and any blend of zeros: exactly 0)
            prepass = bt.TilingPrepass(device, 256)
            prepass.run(tree.view_state())
            assert (tree.build_geometry(prepass)["height"] == 0.0).all()
        pre.run(atlas)
        counts.append(pre.stats()["prev_zero_launches"])
    assert counts[0] > 0 and counts[1] == counts[0], counts
    atlas, tree = trees("planar", 4)
    used = max(GC.table("planar")[1].values()) + 1
    before = atlas.download_tiles(0, 0, used).copy()
    view = library_view("planar", 4, GC.SPECS["planar"]["views"][0])
    tree.tile_geometry(0, GC.tiles("planar"), view)
    prepass = bt.TilingPrepass(device, 1024)
    prepass.run(view)
    tree.build_geometry(prepass, 0, view)
    assert np.array_equal(atlas.download_tiles(0, 0, used), before)

"""bt_tile_tree_tile_geometry_hp and bt_tile_tree_build_geometry_hp on the device: every admissible vertex equal to the CPU model of the
definition (tests/_hp_model.py), field by field and bit for bit, no tolerance.

The scenes are tests/_hp_cases.py's (test_hp_model.py asserts without a GPU that they reach hp / not hp and every direction of
coordinate_change_lod to origin_lod, hp vertices on all six sides, hp and other vertices in one wave): _geometry_cases' terrains, sphere and
ellipsoid, grids 4, 5, 16 (a second trip of the 256-thread workgroup) and 32 (the LDS cap), thresholds 10.0 (every vertex hp) and 0.05
(split tiles), origin_lod 3 and 10, both layouts, NO_MORPH, NO_BLEND, VIEW_RELATIVE on and off; a deep scene (lod_count 16, LOD 15 tiles
under a view 2 m above the ground, default threshold) where the coordinate goes DOWN to origin_lod.  Threshold 0 must give the bytes of the
existing bt_tile_tree_tile_geometry.  Then the device form against the host form on the prepass's list with the capacity edge, the tree's
own approximation, and every refusal — flag 8 still refused by the two plain calls."""
import ctypes as C

import numpy as np
import pytest

import _geometry_cases as GC
import _geometry_model as GM
import _hp_cases as HC
import _hp_model as HM
import _oracle as O
import bevy_terrain_amd as bt
from bevy_terrain_amd import _ffi
from test_gpu_geometry import assert_vertices_equal, device, terrains, trees  # noqa: F401 (module-scoped fixtures of the geometry tests)
from test_tile_tree_host import struct_bytes

pytestmark = pytest.mark.gpu
BT_ERR_INVALID_ARGUMENT, BT_ERR_UNSUPPORTED = -1, -5
FLAG_KW = lambda flags: dict(grid=bool(flags & GM.GRID), morph=not flags & GM.NO_MORPH, blend=not flags & GM.NO_BLEND, view_relative=bool(flags & HM.VIEW_RELATIVE))


def library_pair(kind, grid, threshold, origin_lod, n):
    """the library's view and approximation of view n, which must be the oracle's view and the model's approximation"""
    model, position = GC.MODELS[kind][0], GC.SPECS[kind]["views"][n]
    vc = HC.view_config(grid, threshold, origin_lod)[0]
    view = bt.view_state_from_config(model, vc, position, GC.approximate_height(kind))
    assert struct_bytes(view) == struct_bytes(HC.view_of(kind, grid, threshold, origin_lod, n))
    approximation = bt.model_approximation_from_config(model, vc, position)
    assert struct_bytes(approximation) == HM.approximation_bytes(HC.approximation_of(kind, grid, threshold, origin_lod, n))
    return view, approximation


@pytest.mark.parametrize("kind,grid,threshold,origin_lod,flags,views", HC.COMPARED)
def test_tile_geometry_hp_equals_the_model(trees, kind, grid, threshold, origin_lod, flags, views):
    atlas, tree = trees(kind, grid, True)
    c = GC.scene(kind, grid, True)
    skipped = total = 0
    for n in views:
        exp, trace, admissible = HC.expected(kind, grid, threshold, origin_lod, flags, n)
        view, approximation = library_pair(kind, grid, threshold, origin_lod, n)
        got = tree.tile_geometry(0, c.tiles, view, approximation=approximation, **FLAG_KW(flags))
        assert got.shape == (len(c.tiles), tree.vertices_per_tile(bool(flags & GM.GRID)))
        assert_vertices_equal(got, exp, admissible, (kind, grid, threshold, origin_lod, flags, n))
        skipped, total = skipped + int((~admissible).sum()), total + admissible.size
        print(kind, grid, threshold, origin_lod, flags, n, "vertices", admissible.size, "hp", int(trace["hp"].sum()), "inadmissible", int((~admissible).sum()))
    assert skipped * 1000 <= total


@pytest.mark.parametrize("kind", HC.KINDS)
def test_deep_scene_goes_down_to_origin_lod(terrains, kind):
    """lod_count 16 on the streamed atlas: the tree was never adjusted, so no entry names a tile and no layer is read"""
    c = HC.deep_scene(kind)
    tree = bt.TileTree(terrains(kind), c.model, HC.DEEP_LODS, c.view_config)
    view = bt.view_state_from_config(c.model, c.view_config, c.position, 0.0)
    assert struct_bytes(view) == struct_bytes(c.view)
    approximation = bt.model_approximation_from_config(c.model, c.view_config, c.position)
    assert struct_bytes(approximation) == HM.approximation_bytes(c.approximation)
    for flags in (0, HM.VIEW_RELATIVE):
        exp, trace, admissible = HC.deep_expected(kind, flags)
        assert (trace["dir_origin"] == GM.DOWN).all() and trace["hp"].any() and not trace["hp"].all()
        got = tree.tile_geometry(0, c.tiles, view, approximation=approximation, **FLAG_KW(flags))
        assert_vertices_equal(got, exp, admissible, (kind, "deep", flags))
        assert (~admissible).sum() * 1000 <= admissible.size
    # bt_tile_tree_model_approximation: the tree's last view position, like bt_tile_tree_view_state
    tree.update(c.position)
    assert struct_bytes(tree.model_approximation()) == struct_bytes(approximation)
    own = tree.tile_geometry(0, c.tiles, approximation=tree.model_approximation(), view_relative=True)
    assert own.tobytes() == tree.tile_geometry(0, c.tiles, tree.view_state(), approximation=approximation, view_relative=True).tobytes()
    tree.close()


@pytest.mark.parametrize("kind,grid", [("sphere", 16), ("ellipsoid", 4), ("sphere", 5)])
def test_threshold_zero_is_the_existing_call_byte_for_byte(trees, kind, grid):
    atlas, tree = trees(kind, grid, True)
    tiles = GC.tiles(kind)
    for n in range(3):
        view, approximation = library_pair(kind, grid, 0.0, 10, n)
        assert approximation.precision_threshold_distance == 0.0
        for flags in (0, GM.GRID | GM.NO_MORPH, GM.NO_BLEND):
            kw = FLAG_KW(flags)
            plain = tree.tile_geometry(0, tiles, view, **dict(kw, view_relative=False))
            assert tree.tile_geometry(0, tiles, view, approximation=approximation, **kw).tobytes() == plain.tobytes(), (kind, grid, n, flags)


@pytest.mark.parametrize("kind,grid,flags", [("sphere", 5, GM.GRID | HM.VIEW_RELATIVE), ("ellipsoid", 16, 0)])
def test_build_geometry_hp_equals_the_host_form_on_the_prepass_list(device, trees, kind, grid, flags):
    atlas, tree = trees(kind, grid)
    view, approximation = library_pair(kind, grid, HC.DEVICE, 3, HC.NEAR)
    prepass = bt.TilingPrepass(device, 4096)
    prepass.run(view)
    tiles, indirect = prepass.read()
    slots = tree.vertices_per_tile(bool(flags & GM.GRID))
    assert len(tiles) >= 16 and len(set(tiles[:, 1].tolist())) >= 2 and tiles[:, 1].max() < GC.LODS
    kw = dict(FLAG_KW(flags), approximation=approximation)
    host = tree.tile_geometry(0, tiles, view, **kw)
    built = tree.build_geometry(prepass, 0, view, **kw)
    assert built.shape == host.shape == (len(tiles), slots) and built.tobytes() == host.tobytes()
    c = GC.scene(kind, grid)
    exp, trace, admissible = HM.geometry(HC.view_of(kind, grid, HC.DEVICE, 3, HC.NEAR), HC.approximation_of(kind, grid, HC.DEVICE, 3, HC.NEAR), c.P, c.entries, c.layers, GC.T, GC.B, tiles, flags)
    assert trace["hp"].sum() * 10 > trace["hp"].size and not trace["hp"].all()
    assert_vertices_equal(built, exp, admissible, (kind, grid, flags))
    # a capacity one vertex short of the need: the last tile's slots keep the sentinel, everything before them is what it was
    need = len(tiles) * slots
    sentinel = np.full((need + slots) * 48, 0xA5, np.uint8)  # (a tile's worth of guard behind the list)
    ptr = device.upload(sentinel)
    try:
        assert tree.build_geometry(prepass, 0, view, vertices=ptr, vertex_capacity=need - 1, **kw) is None
        short = device.download(ptr, (need + slots) * 48, np.uint8)
        assert short[:(need - slots) * 48].tobytes() == host[:-1].tobytes() and (short[(need - slots) * 48:] == 0xA5).all()
        tree.build_geometry(prepass, 0, view, vertices=ptr, vertex_capacity=need + slots, **kw)  # room to spare: the list, and no more
        whole = device.download(ptr, (need + slots) * 48, np.uint8)
        assert whole[:need * 48].tobytes() == host.tobytes() and (whole[need * 48:] == 0xA5).all()
        # vertex_capacity == 0 touches nothing
        L = _ffi.lib()
        _ffi.check(L.bt_tile_tree_build_geometry_hp(tree._h, atlas._h, 0, C.byref(view), C.byref(approximation), prepass._h, flags, C.c_void_p(ptr), 0))
        _ffi.check(L.bt_tile_tree_build_geometry_hp(tree._h, atlas._h, 0, C.byref(view), C.byref(approximation), prepass._h, flags, None, 0))
        assert device.download(ptr, (need + slots) * 48, np.uint8).tobytes() == whole.tobytes()
    finally:
        device.free(ptr)


def test_refusals_and_empty_calls(device, terrains, trees):
    L = _ffi.lib()
    atlas, tree = trees("sphere", 4)
    view, approximation = library_pair("sphere", 4, HC.SPLIT, 3, HC.NEAR)
    tiles = np.ascontiguousarray(GC.tiles("sphere")[:3])
    tp = tiles.ctypes.data_as(C.POINTER(_ffi.TileCoordinateC))
    out = np.full(3 * 48 * 48, 0x77, np.uint8)  # three tiles of 48 strip slots
    op = out.ctypes.data_as(C.POINTER(_ffi.TerrainVertexC))
    prepass = bt.TilingPrepass(device, 64)
    prepass.run(view)
    buffer = device.upload(np.full(48 * 48 * 64, 0x5A, np.uint8))
    vp = C.c_void_p(buffer)

    def host(tree_h=tree._h, atlas_h=atlas._h, ai=0, v=C.byref(view), a=C.byref(approximation), t=tp, count=3, flags=0, o=op, nbytes=out.nbytes):
        return L.bt_tile_tree_tile_geometry_hp(tree_h, atlas_h, ai, v, a, t, count, flags, o, nbytes)

    def dev(tree_h=tree._h, atlas_h=atlas._h, ai=0, v=C.byref(view), a=C.byref(approximation), p=prepass._h, flags=0, o=vp, capacity=48 * 64):
        return L.bt_tile_tree_build_geometry_hp(tree_h, atlas_h, ai, v, a, p, flags, o, capacity)

    def altered(**kw):
        a = _ffi.ModelApproximationC.from_buffer_copy(struct_bytes(approximation))
        for k, value in kw.items():
            setattr(a, k, value)
        return a

    try:
        # the plain calls' refusals
        for call in (host, dev):
            assert call(tree_h=None) == BT_ERR_INVALID_ARGUMENT and L.bt_last_error()
            assert call(atlas_h=None) == BT_ERR_INVALID_ARGUMENT
            assert call(ai=2) == BT_ERR_INVALID_ARGUMENT and b"attachment" in L.bt_last_error()
            assert call(flags=16) == BT_ERR_INVALID_ARGUMENT and b"flags" in L.bt_last_error()
            assert call(ai=1) == BT_ERR_UNSUPPORTED and b"R16" in L.bt_last_error()  # the Rgba8 attachment
            assert call(o=None) == BT_ERR_INVALID_ARGUMENT
        assert host(t=None) == BT_ERR_INVALID_ARGUMENT
        assert host(nbytes=out.nbytes - 1) == BT_ERR_INVALID_ARGUMENT and b"out_bytes" in L.bt_last_error()
        assert dev(p=None) == BT_ERR_INVALID_ARGUMENT
        assert dev(o=C.c_void_p(buffer + 4)) == BT_ERR_INVALID_ARGUMENT and b"aligned" in L.bt_last_error()
        for bad in ((6, 0, 0, 0), (0, GC.LODS, 0, 0), (0, 1, 2, 0), (0, 2, 0, 4)):  # side, lod, x, y
            t = np.ascontiguousarray(np.vstack([tiles[:2], [bad]]).astype(np.uint32))
            assert host(t=t.ctypes.data_as(C.POINTER(_ffi.TileCoordinateC))) == BT_ERR_INVALID_ARGUMENT, bad
        planar_view = bt.view_state_from_config(GC.MODELS["planar"][0], GC.view_config(4)[0], GC.SPECS["planar"]["views"][0], 0.0)
        assert host(v=C.byref(planar_view)) == BT_ERR_INVALID_ARGUMENT and dev(v=C.byref(planar_view)) == BT_ERR_INVALID_ARGUMENT
        for kw, status in ((dict(grid_size=33), BT_ERR_UNSUPPORTED), (dict(morph_range=0.0), BT_ERR_INVALID_ARGUMENT), (dict(blend_range=float("nan")), BT_ERR_INVALID_ARGUMENT)):
            odd = bt.TileTree.new(atlas, bt.TerrainViewConfig(**dict(dict(tree_size=GC.TREE, grid_size=4), **kw)))
            assert host(tree_h=odd._h) == status and dev(tree_h=odd._h) == status, kw
        # the approximation: NULL, another origin_lod than the view's, a threshold that is not finite or is negative
        for call in (host, dev):
            assert call(a=None) == BT_ERR_INVALID_ARGUMENT and b"approximation" in L.bt_last_error()
            assert call(a=C.byref(altered(origin_lod=4))) == BT_ERR_INVALID_ARGUMENT and b"origin_lod" in L.bt_last_error()
            for threshold in (float("nan"), float("inf"), -1.0, -float("inf")):
                assert call(a=C.byref(altered(precision_threshold_distance=threshold))) == BT_ERR_INVALID_ARGUMENT, threshold
        # a planar tree
        planar_atlas, planar_tree = trees("planar", 4)
        ptiles = np.ascontiguousarray(GC.tiles("planar")[:3])
        ptp = ptiles.ctypes.data_as(C.POINTER(_ffi.TileCoordinateC))
        planar_approximation = altered(origin_lod=planar_view.origin_lod)
        assert host(tree_h=planar_tree._h, atlas_h=planar_atlas._h, v=C.byref(planar_view), a=C.byref(planar_approximation), t=ptp) == BT_ERR_UNSUPPORTED and b"planar" in L.bt_last_error()
        assert dev(tree_h=planar_tree._h, atlas_h=planar_atlas._h, v=C.byref(planar_view), a=C.byref(planar_approximation)) == BT_ERR_UNSUPPORTED
        with pytest.raises(_ffi.BtError):
            planar_tree.model_approximation()
        # flag 8 belongs to the new calls alone
        assert L.bt_tile_tree_tile_geometry(tree._h, atlas._h, 0, C.byref(view), tp, 3, 8, op, out.nbytes) == BT_ERR_INVALID_ARGUMENT
        assert L.bt_tile_tree_build_geometry(tree._h, atlas._h, 0, C.byref(view), prepass._h, 8, vp, 48 * 64) == BT_ERR_INVALID_ARGUMENT
        with pytest.raises(ValueError):
            tree.tile_geometry(0, tiles, view, view_relative=True)
        # count == 0: BT_OK, whatever the arrays
        assert host(count=0) == _ffi.BT_OK and host(t=None, count=0, o=None, nbytes=0) == _ffi.BT_OK
        assert dev(capacity=0) == _ffi.BT_OK
        # nothing was touched by any refusal or empty call
        assert (out == 0x77).all()
        assert (device.download(buffer, 48 * 48 * 64, np.uint8) == 0x5A).all()
        assert host(flags=8) == _ffi.BT_OK and not (out == 0x77).all()
        zero = altered(precision_threshold_distance=-0.0)  # -0.0 is not negative: accepted, and no vertex is hp
        assert host(a=C.byref(zero)) == _ffi.BT_OK and dev(a=C.byref(zero)) == _ffi.BT_OK
    finally:
        device.free(buffer)

"""Where a tile's vertices go: the geometry kernel's workgroup loop beyond its first trip, the host form's launches of 32 MiB each, and the
capacity cut away from the list's end.  test_gpu_geometry.py and test_gpu_hp_geometry.py pin every vertex's arithmetic on lists of 37 and 52
tiles, which one launch of as many workgroups takes in one trip each; here the lists are long (tests/_geometry_cases.py, LONG and
deep_scene; tests/_hp_cases.py, LONG and long_device_scene; test_geometry_model.py and test_hp_model.py assert without a GPU that they reach
what they claim) and every admissible vertex is again compared bit for bit with the CPU model.

A launch has min(count, 1024) workgroups (host form) or 1024 (device form), and workgroup w takes tiles w, w + 1024, w + 2048, ...: the
lists put tiles of different LOD or side one and two trips apart, so a tile read or written with the workgroup's index in place of the
tile's differs from the expected one in its positions.  The host form makes one launch per 32 MiB of vertices, max(1, (32 << 20) // (slots *
48)) tiles, with tile_index going on from the chunk's first tile; the lists' first tile differs from the first of every later chunk.  Bytes of
the output array beyond count * slots * 48 stay as they were.

The device form runs on the prepass's list of a 9-LOD tree that was never adjusted (every height is mix(min, max, 0): what is pinned is
addressing, distance, morph and blend ratio), 1416 tiles on the sphere and 1415 on the ellipsoid, and is cut at capacities that end in a
second trip, at every workgroup's second trip, between the trips and nowhere.

Not claimed: the barrier that closes a trip.  Without it a later trip races with the copy-out of the one before, which a run may or may
not show."""
import ctypes as C

import numpy as np
import pytest

import _geometry_cases as GC
import _geometry_model as GM
import _hp_cases as HC
import _hp_model as HM
import bevy_terrain_amd as bt
from bevy_terrain_amd import _ffi
from test_gpu_geometry import assert_vertices_equal, device, library_view, terrains, trees  # noqa: F401 (module-scoped fixtures of the geometry tests)
from test_gpu_hp_geometry import library_pair
from test_tile_tree_host import struct_bytes

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5


def host_form(tree, tiles, view, flags, approximation=None):
    """bt_tile_tree_tile_geometry(_hp) with the exact out_bytes, into the head of a larger array filled with a sentinel -> the vertices
    (count, slots); whatever lies beyond them must be untouched"""
    tiles = np.ascontiguousarray(tiles, np.uint32).reshape(-1, 4)
    count, slots = len(tiles), tree.vertices_per_tile(bool(flags & GM.GRID))
    nbytes = count * slots * GC.VERTEX_BYTES
    out = np.full(nbytes + slots * GC.VERTEX_BYTES + 64, SENTINEL, np.uint8)  # (a tile's worth of guard and a little more)
    head = (tree._h, tree.atlas._h, 0, C.byref(view))
    tail = (tiles.ctypes.data_as(C.POINTER(_ffi.TileCoordinateC)), count, flags, out.ctypes.data_as(C.POINTER(_ffi.TerrainVertexC)), nbytes)
    if approximation is None:
        _ffi.check(_ffi.lib().bt_tile_tree_tile_geometry(*head, *tail))
    else:
        _ffi.check(_ffi.lib().bt_tile_tree_tile_geometry_hp(*head, C.byref(approximation), *tail))
    assert (out[nbytes:] == SENTINEL).all(), ("bytes beyond count * slots * 48 were written", int((out[nbytes:] != SENTINEL).sum()))
    return out[:nbytes].view(GM.VERTEX_DTYPE).reshape(count, slots)


def assert_tile_index_counts_on(got):
    """stated on its own, so that a wrong tile_base reads as one"""
    rows = np.arange(len(got), dtype=np.uint32)[:, None]
    bad = np.flatnonzero((got["tile_index"] != rows).any(axis=1))
    assert not len(bad), ("tile_index is not the tile's place in the list", len(bad), bad[:4].tolist(), got["tile_index"][bad[:4], 0].tolist())


def assert_long_list(got, exp, admissible, what):
    assert_tile_index_counts_on(got)
    assert_vertices_equal(got, exp, admissible, what)
    skipped = int((~admissible).sum())
    print(*what, "vertices", admissible.size, "skipped as inadmissible", skipped)
    assert skipped * 1000 <= admissible.size


# ---- 1. the host form: later trips and chunk boundaries ----------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,grid,flags,count,launches", GC.LONG)
def test_tile_geometry_on_long_lists(trees, kind, grid, flags, count, launches):
    atlas, tree = trees(kind, grid)
    assert launches == GC.launches_of(grid, flags, count) and tree.vertices_per_tile(bool(flags & GM.GRID)) == GC.slots_of(grid, flags)
    exp, admissible = GC.long_expected(kind, grid, 0, flags, count)
    got = host_form(tree, GC.long_tiles(kind, count), library_view(kind, grid, GC.SPECS[kind]["views"][0]), flags)
    assert_long_list(got, exp, admissible, (kind, grid, flags, count, launches))


@pytest.mark.parametrize("kind,grid,threshold,origin_lod,flags,n,count,launches", HC.LONG)
def test_tile_geometry_hp_on_long_lists(trees, kind, grid, threshold, origin_lod, flags, n, count, launches):
    atlas, tree = trees(kind, grid)
    assert launches == GC.launches_of(grid, flags, count)
    exp, admissible, hp = HC.long_expected(kind, grid, threshold, origin_lod, flags, n, count)
    view, approximation = library_pair(kind, grid, threshold, origin_lod, n)
    got = host_form(tree, GC.long_tiles(kind, count), view, flags, approximation)
    print("hp vertices", int(hp[GC.long_index(kind, count)].sum()))
    assert_long_list(got, exp, admissible, (kind, grid, threshold, origin_lod, flags, n, count, launches))


# ---- 2. the host form's scratch: regrown, kept, trimmed ----------------------------------------------------------------------------------

def test_scratch_regrows_and_comes_back_after_trim():
    """on a context of its own, so that the order of the requests is this test's: a small one, a large one (the scratch is regrown), the
    small one in the large scratch, bt_ctx_trim, the large one in a scratch allocated anew.  Nothing is loaded (a tree that was never
    updated: every entry invalid), which the scratch does not care about"""
    kind, count = "ellipsoid", 1300
    fresh = bt.Device(0)
    model = GC.MODELS[kind][0]
    cfg = bt.TerrainConfig(lod_count=GC.LODS, atlas_size=8, path="terrains/none", model=model)
    cfg.add_attachment(bt.AttachmentConfig(name="height", texture_size=GC.T, border_size=GC.B))
    atlas = bt.TileAtlas.new(cfg, fresh)
    small, large = bt.TileTree.new(atlas, GC.view_config(4)[0]), bt.TileTree.new(atlas, GC.view_config(16)[0])
    try:
        for tree in (small, large):
            assert (tree.read()[0] == GM.INVALID).all()
        few, many = GC.tiles(kind)[:3], GC.long_tiles(kind, count)
        view4, view16 = library_view(kind, 4, GC.SPECS[kind]["views"][0]), library_view(kind, 16, GC.SPECS[kind]["views"][0])
        first = host_form(small, few, view4, 0).tobytes()
        second = host_form(large, many, view16, 0)
        exp, _, admissible = GC.expected(kind, 16, False, 0, 0)
        assert_long_list(second, *GC.gather((exp, None, admissible), GC.long_index(kind, count)), (kind, 16, "nothing loaded", count))
        exp, _, admissible = GC.expected(kind, 4, False, 0, 0)
        assert_vertices_equal(np.frombuffer(first, GM.VERTEX_DTYPE).reshape(3, -1), exp[:3], admissible[:3], (kind, 4, "nothing loaded", 3))
        assert host_form(small, few, view4, 0).tobytes() == first
        assert fresh.trim() >= GC.chunk_tiles(16, 0) * 576 * GC.VERTEX_BYTES  # (the scratch held one launch's vertices: 1213 tiles)
        assert host_form(large, many, view16, 0).tobytes() == second.tobytes()
        assert host_form(small, few, view4, 0).tobytes() == first
    finally:
        small.close()
        large.close()
        atlas.close()
        fresh.close()


# ---- 3. the device form on a prepass list longer than 1024 ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def deep(device, terrains):
    """deep(kind, hp) -> (scene, tree, prepass after its run, view, approximation or None): a tree of 9 LODs on the streamed atlas, never
    adjusted; the prepass's list at the near view is the oracle's"""
    cache = {}

    def get(kind, hp=False):
        if (kind, hp) not in cache:
            c = HC.long_device_scene(kind) if hp else GC.deep_scene(kind)
            tree = bt.TileTree(terrains(kind), c.model, GC.DEEP_LODS, c.view_config)
            assert (tree.read()[0] == GM.INVALID).all() and tree.read()[0].shape == c.entries.shape
            view = bt.view_state_from_config(c.model, c.view_config, c.position, GC.approximate_height(kind))
            assert struct_bytes(view) == struct_bytes(c.view)
            approximation = None
            if hp:
                approximation = bt.model_approximation_from_config(c.model, c.view_config, c.position)
                assert struct_bytes(approximation) == HM.approximation_bytes(c.approximation)
            prepass = bt.TilingPrepass(device, GC.DEEP_KW["geometry_tile_count"])
            prepass.run(view)
            tiles, indirect = prepass.read()
            print(kind, "prepass list", len(tiles), "tiles, the oracle's", len(c.tiles))
            assert np.array_equal(tiles, c.tiles) and list(indirect) == c.indirect and GC.TRIP < len(tiles) <= 2 * GC.TRIP
            cache[(kind, hp)] = (c, tree, prepass, view, approximation)
        return cache[(kind, hp)]

    return get


def test_build_geometry_on_a_list_longer_than_1024(deep):
    c, tree, prepass, view, _ = deep("sphere")
    exp, _, admissible = GC.deep_expected("sphere", 0)
    host = host_form(tree, c.tiles, view, 0)
    built = tree.build_geometry(prepass, 0, view)
    assert built.shape == host.shape == (len(c.tiles), 48)
    assert_long_list(built, exp, admissible, ("sphere", "device form", len(c.tiles)))
    assert_long_list(host, exp, admissible, ("sphere", "host form", len(c.tiles)))
    assert built.tobytes() == host.tobytes()


def test_build_geometry_hp_on_a_list_longer_than_1024(deep):
    flags = GM.GRID | HM.VIEW_RELATIVE
    c, tree, prepass, view, approximation = deep("ellipsoid", True)
    exp, trace, admissible = HC.long_device_expected("ellipsoid", flags)
    share = trace["hp"].mean()
    print("hp share %.3f" % share)
    assert 0.1 < share < 1
    host = host_form(tree, c.tiles, view, flags, approximation)
    built = tree.build_geometry(prepass, 0, view, grid=True, approximation=approximation, view_relative=True)
    assert built.shape == host.shape == (len(c.tiles), 25)
    assert_long_list(built, exp, admissible, ("ellipsoid", "hp device form", len(c.tiles)))
    assert_long_list(host, exp, admissible, ("ellipsoid", "hp host form", len(c.tiles)))
    assert built.tobytes() == host.tobytes()


def test_capacity_cut_in_later_trips(device, deep):
    """a tile whose last slot would fall beyond vertex_capacity is skipped whole, and so is every tile behind it, whichever workgroup and trip
    they are; everything before it is written"""
    c, tree, prepass, view, _ = deep("sphere")
    n, slots = len(c.tiles), 48
    host = host_form(tree, c.tiles, view, 0)
    sentinel = np.full((n + 1) * slots * GC.VERTEX_BYTES, SENTINEL, np.uint8)  # (a tile's worth of guard behind the list)
    ptr = device.upload(sentinel)
    try:
        for capacity, cut in GC.cuts(n, slots):
            _ffi.check(_ffi.lib().bt_memcpy_h2d(device._h, C.c_void_p(ptr), sentinel.ctypes.data_as(C.c_void_p), sentinel.nbytes))
            assert tree.build_geometry(prepass, 0, view, vertices=ptr, vertex_capacity=capacity) is None
            got = device.download(ptr, sentinel.nbytes, np.uint8)
            kept = cut * slots * GC.VERTEX_BYTES
            written = got[:kept].view(GM.VERTEX_DTYPE).reshape(cut, slots)
            untouched = (got[kept:].reshape(-1, slots * GC.VERTEX_BYTES) == SENTINEL).all(axis=1)
            assert untouched.all(), (capacity, cut, "tiles written behind the cut", (cut + np.flatnonzero(~untouched))[:6].tolist())
            missing = np.flatnonzero((written.view(np.uint8).reshape(cut, -1) == SENTINEL).all(axis=1))
            assert not len(missing), (capacity, cut, "tiles before the cut left out", missing[:6].tolist())
            assert written.tobytes() == host[:cut].tobytes(), (capacity, cut)
    finally:
        device.free(ptr)

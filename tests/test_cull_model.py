"""The culling definition (include/bevy_terrain_amd.h) on the CPU: bt_cull_planes against culling_bind_group.rs, the numpy model's cull
test against visibility sampled in float64 (it may never drop a tile a sample of which is inside the frustum), the culled list against
the unculled one, and the rules of the height-bounds table.  The kernels are held to this model bit for bit by test_gpu_culling.py."""
import ctypes as C

import numpy as np
import pytest

import _cull_model as M
import _refine_model as R
import bevy_terrain_amd as bt
from bevy_terrain_amd import _ffi

VIEWS = 20


def models(kind):
    if kind == "planar":
        return bt.TerrainModel.planar((0.0, 0.0, 0.0), 1000.0, 0.0, 250.0), 1, (0.0, 250.0)
    return bt.TerrainModel.sphere((0.0, 0.0, 0.0), 6371000.0, -12000.0, 9000.0), 6, (-12000.0, 9000.0)


def synthetic_table(rng, sides, levels=5):
    """random nested ranges: a child's range lies inside its parent's, as after bt_height_bounds_build"""
    table = M.Table(sides, levels)
    for lod in range(1, levels):
        for side in range(sides):
            for y in range(1 << lod):
                for x in range(1 << lod):
                    lo, hi = (int(v) for v in table.data[table.index(side, lod - 1, x >> 1, y >> 1)])
                    a, b = sorted(int(v) for v in rng.integers(lo, hi + 1, 2))
                    table.data[table.index(side, lod, x, y)] = (a, b)
    return table


def visited_tiles(view):
    """every tile the unculled prepass visits, in id order"""
    out = []
    current = np.array([[s, 0, 0, 0] for s in range(6 if view.spherical else 1)], np.uint32)
    for _ in range(view.refinement_count + 1):
        if len(current) == 0:
            break
        out.append(current)
        parents = current[R.should_be_divided(view, current)[0]]
        i = np.tile(np.arange(4, dtype=np.uint32), len(parents))
        rep = np.repeat(parents, 4, axis=0)
        current = np.stack([rep[:, 0], rep[:, 1] + 1, (rep[:, 2] << 1) + (i & 1), (rep[:, 3] << 1) + ((i >> 1) & 1)], axis=1).astype(np.uint32).reshape(-1, 4)
    return np.concatenate(out)


def visible(view, tiles, cull, table):
    """a sample of the tile's volume — a 9 x 9 x 3 grid of (uv, h) — lies strictly inside every plane, in float64"""
    vmin, vmax = M.raw_range(tiles, table)
    lo, hi = M.heights(cull, vmin).astype(np.float64), M.heights(cull, vmax).astype(np.float64)
    planes = cull.planes.astype(np.float64)
    seen = np.zeros(len(tiles), bool)
    for v in np.linspace(0.0, 1.0, 9):
        for u in np.linspace(0.0, 1.0, 9):
            world, normal = M.surface(view, tiles, (u, v), np.float64)
            for h in (lo, 0.5 * (lo + hi), hi):
                p = world + h[:, None] * normal
                seen |= np.all(p @ planes[:, :3].T + planes[:, 3] > 0.0, axis=1)
    return seen


def test_cull_planes_equal_the_reference_function_bit_for_bit():
    rng = np.random.default_rng(5)
    for k in range(200):
        m = (rng.normal(size=(4, 4)) * 10.0 ** rng.uniform(-3, 6)).astype(np.float32)
        if k % 7 == 0:
            m[rng.integers(0, 4), rng.integers(0, 4)] = [np.inf, -0.0, 0.0, np.float32(1e-42)][k % 4]
        ours, expected = bt.cull_planes(m), M.planes_from_matrix(m)
        assert np.array_equal(ours.view(np.uint32), expected.view(np.uint32)), k
    # perspective_infinite_reverse_rh(90 degrees, aspect 1, near 1), camera at the origin looking down -z: x = +-z, y = +-z, z = -1
    clip = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1], [0, 0, -1, 0]], np.float32)
    assert np.array_equal(bt.cull_planes(clip), np.array([[1, 0, -1, 0], [-1, 0, -1, 0], [0, 1, -1, 0], [0, -1, -1, 0], [0, 0, -1, -1]], np.float32))
    assert np.allclose(M.clip_from_world((0, 0, 0), (0, 0, -1), np.pi / 2, 1.0, near=1.0), clip, atol=1e-15)
    inside, outside = np.array([0.5, -0.5, -2.0, 1.0]), np.array([3.0, 0.0, -2.0, 1.0])
    assert np.all(bt.cull_planes(clip) @ inside >= 0) and np.any(bt.cull_planes(clip) @ outside < 0)


def test_cull_view_layout():
    assert C.sizeof(_ffi.CullViewC) == 96 and _ffi.CullViewC.plane_count.offset == 80 and _ffi.CullViewC.max_height.offset == 92


def test_point_is_the_divide_tests_point():
    """point(tile, uv, h) with the view's uv and approximate_height gives the distance _refine_model.should_be_divided compares"""
    for kind in ("planar", "sphere"):
        model, _, _ = models(kind)
        eye, _ = M.random_camera(np.random.default_rng(3), kind)
        view = bt.make_view_state(model, bt.TerrainViewConfig(), tuple(eye))
        tiles = visited_tiles(view)
        uv = np.empty((len(tiles), 2), np.float32)
        for s in np.unique(tiles[:, 0]):
            m = tiles[:, 0] == s
            p = view.sides[int(s)]
            vxy, vuv = R._change_lod((p.view_xy[0], p.view_xy[1]), (p.view_uv[0], p.view_uv[1]), view.origin_lod, tiles[m, 1])
            off = vxy.astype(np.int64) - tiles[m, 2:4].astype(np.int64)
            uv[m] = np.where(off < 0, np.float32(0), np.where(off > 0, np.float32(1), vuv))
        d = M.point(view, tiles, uv, view.approximate_height) - np.array(list(view.world_position), np.float32)
        assert np.array_equal(M.length3(d.astype(np.float32)), R.should_be_divided(view, tiles)[1])


@pytest.mark.parametrize("kind", ["planar", "sphere"])
def test_culling_is_conservative_and_not_vacuous(kind):
    """Over VIEWS random views: no tile with a sample strictly inside the frustum is culled (a count of zero, with margin 0, with and
    without a table), and the culled prepass keeps fewer than 0.75 of the unculled final tiles."""
    model, sides, (min_height, max_height) = models(kind)
    rng = np.random.default_rng(2024 if kind == "planar" else 2025)
    table = synthetic_table(rng, sides)
    kept = {False: 0, True: 0}
    unculled = visited_total = 0
    for k in range(VIEWS):
        eye, clip = M.random_camera(rng, kind)
        view = bt.make_view_state(model, bt.TerrainViewConfig(), tuple(eye))
        cull = M.CullView(bt.cull_planes(clip), 0.0, min_height, max_height)
        tiles = visited_tiles(view)
        visited_total += len(tiles)
        unculled += len(R.refine(view)[0])
        for with_table in (False, True):
            t = table if with_table else None
            out = M.culled(view, tiles, cull, t)
            lost = int(visible(view, tiles[out], cull, t).sum())
            print(kind, "view", k, "table" if with_table else "no table", "visited", len(tiles), "culled", int(out.sum()), "visible and culled", lost)
            assert lost == 0, (kind, k, with_table, lost)
            kept[with_table] += len(M.refine_culled(view, cull, t)[0])
    print(kind, "visited", visited_total, "final tiles", unculled, "kept", kept)
    assert visited_total > 5000
    assert kept[False] < 0.75 * unculled and kept[True] < 0.75 * unculled


@pytest.mark.parametrize("kind", ["planar", "sphere"])
def test_culled_list_is_the_unculled_list_without_culled_subtrees(kind):
    model, sides, (min_height, max_height) = models(kind)
    rng = np.random.default_rng(77)
    table = synthetic_table(rng, sides, levels=3)
    for k in range(6):
        eye, clip = M.random_camera(rng, kind)
        view = bt.make_view_state(model, bt.TerrainViewConfig(), tuple(eye))
        final, dropped, _ = R.refine(view)
        assert len(dropped) == 0
        none = M.CullView(np.zeros((0, 4), np.float32), 0.0, min_height, max_height)
        got, n_culled, n_visited = M.refine_culled(view, none, table)
        assert np.array_equal(got, final) and n_culled == 0 and n_visited == len(visited_tiles(view))
        cull = M.CullView(bt.cull_planes(clip), 3.0 if k % 2 else 0.0, min_height, max_height)
        passes = []
        got, n_culled, n_visited = M.refine_culled(view, cull, table, passes)
        # a final tile stays unless it or one of its ancestors is culled
        keep = np.ones(len(final), bool)
        chain = final.copy()
        while True:
            keep &= ~M.culled(view, chain, cull, table)
            up = chain[:, 1] > 0
            if not up.any():
                break
            chain = np.where(up[:, None], np.stack([chain[:, 0], chain[:, 1] - 1, chain[:, 2] >> 1, chain[:, 3] >> 1], axis=1), chain).astype(np.uint32)
        assert np.array_equal(got, final[keep]), (kind, k)
        assert sum(v for v, _ in passes) == n_visited and n_culled > 0
        assert not M.overflows(passes, len(got), 1 << 20) and M.overflows(passes, len(got), max(v for v, _ in passes) - 1)
    # NaN planes cull nothing
    nan = M.CullView(np.full((5, 4), np.nan, np.float32), 0.0, min_height, max_height)
    assert np.array_equal(M.refine_culled(view, nan)[0], final)


def layer(lo, hi, T=8):
    out = np.full((T, T), lo, np.uint16)
    out[0, T - 1] = hi  # (a border texel: the border counts)
    return out


def test_table_rules_on_hand_made_atlases():
    # a held leaf, a missing tile filled from its parent, a parent narrower than its children
    held = {(0, 0, 0, 0): layer(100, 200), (0, 1, 0, 0): layer(50, 120), (0, 1, 1, 0): layer(150, 400), (0, 1, 0, 1): layer(110, 190),
            (0, 2, 0, 0): layer(40, 60)}
    t = M.build_table(1, 3, held)
    e = lambda lod, x, y: tuple(int(v) for v in t.data[t.index(0, lod, x, y)])
    assert e(2, 0, 0) == (40, 60)                 # a held leaf: its own layer
    assert e(2, 1, 0) == (50, 120)                # missing: own of its parent (0, 1, 0, 0), not the parent's union
    assert e(2, 3, 3) == (100, 200)               # missing under a missing parent: the root's own, handed down twice
    assert e(1, 1, 1) == (100, 200)               # missing: the root's own
    assert e(1, 0, 0) == (40, 120)                # own (50, 120) united with its children (40, 60), (50, 120) x 3
    assert e(1, 1, 0) == (150, 400)
    assert e(0, 0, 0) == (40, 400)                # the root is narrower than its children: the union holds for every LOD below it
    assert np.all(t.data[:, 0] <= t.data[:, 1])
    # a missing root is the whole range, and so is everything below it that is not held
    t = M.build_table(6, 2, {(2, 1, 1, 1): layer(7, 9)})
    assert tuple(t.data[t.index(2, 1, 1, 1)]) == (7, 9) and tuple(t.data[t.index(2, 1, 0, 1)]) == (0, 65535)
    assert tuple(t.data[t.index(2, 0, 0, 0)]) == (0, 65535) and tuple(t.data[t.index(3, 0, 0, 0)]) == (0, 65535)
    # tiles of LODs the table does not have are left out of it, and read their ancestor at the last level
    t = M.build_table(1, 2, {(0, 0, 0, 0): layer(10, 20), (0, 1, 1, 0): layer(12, 18), (0, 2, 2, 0): layer(1, 60000)})
    assert tuple(t.data[t.index(0, 1, 1, 0)]) == (12, 18) and tuple(t.data[t.index(0, 0, 0, 0)]) == (10, 20)
    tiles = np.array([[0, 1, 1, 0], [0, 2, 2, 1], [0, 5, 16 + 7, 3], [0, 5, 3, 16 + 1], [0, 0, 0, 0]], np.uint32)
    vmin, vmax = M.raw_range(tiles, t)
    assert list(zip(vmin.tolist(), vmax.tolist())) == [(12, 18), (12, 18), (12, 18), (10, 20), (10, 20)]
    assert M.raw_range(tiles, None)[1].tolist() == [65535] * 5
    cull = M.CullView(np.zeros((0, 4)), 0.0, -100.0, 300.0)
    h = M.heights(cull, np.array([0, 65535, 13107], np.uint16))
    assert h[0] == np.float32(-100.0) and h[1] == np.float32(300.0) and h[2] == np.float32(-100.0) + np.float32(400.0) * (np.float32(13107) / np.float32(65535))

"""bt_atlas_path_field on the device against the heapq model of the definition (tests/_path_model.py, pinned by test_path_model.py).

D is compared as uint32 bit patterns and next byte for byte, over every cell: no tolerance, no excluded cell.  The scenes are those of
tests/_path_cases.py; the model's planes are computed once per scene (without a GPU, from the CPU oracle's state) and shared.  Each test
also reads the window back with bt_atlas_read_region and requires the texels the model was given."""
import ctypes as C
import math

import numpy as np
import pytest

import _path_cases as PC
import _path_model as M
import bevy_terrain_amd as bt
from _splat_cases import G, H
from bevy_terrain_amd import PathCost, _ffi
from test_gpu_splat import device_atlas

BT_ERR_INVALID_ARGUMENT, BT_ERR_UNSUPPORTED = -1, -5
INF, NAN = math.inf, math.nan
SCHEDULE = ("sweeps", "launches")  # the fields of bt_path_stats that describe the schedule, not the input


@pytest.fixture(scope="module")
def device():
    return bt.Device(0)


@pytest.fixture(scope="module")
def atlases(device):
    """one device atlas per (spec, planted walls) of the scenes, made on first use, and one per spec for the scenes that plant whole texels"""
    made = {}

    def get(name):
        scene = PC.SCENES[name]
        walls = [p for p in scene["plants"] if p[2].dtype == bool]
        key = (scene["spec"], name if walls else "texels" if scene["plants"] else None)
        x0, y0, _, _ = scene["rect"]
        if key not in made:
            atlas = device_atlas(device, scene["spec"])
            for x, y, wall in walls:  # a wall is a no-data texel: the region is read, cut and written back
                h, w = wall.shape
                part, _ = atlas.read_region(H, x0 + x, y0 + y, w, h, side=scene["side"])
                part[wall] = 0
                atlas.write_region(H, part, x0 + x, y0 + y, side=scene["side"])
            made[key] = atlas
        for x, y, texels in scene["plants"]:  # whole texels: the scenes that plant them share one atlas and write theirs before their call
            if texels.dtype != bool:
                made[key].write_region(H, texels, x0 + x, y0 + y, side=scene["side"])
        return made[key]

    return get


def bits(plane):
    return np.ascontiguousarray(plane, dtype=np.float32).view(np.uint32)


def run(atlas, scene, **kw):
    x0, y0, w, h = scene["rect"]
    return atlas.path_field(H, x0, y0, w, h, PathCost(**scene["cost"]), scene["goals"], blocked=scene["mask"], lod=scene["lod"], side=scene["side"], **kw)


def check_scene(atlas, name):
    scene = PC.SCENES[name]
    raw, D, nxt, stats, _ = PC.expected(name)
    x0, y0, w, h = scene["rect"]
    got_raw, missing = atlas.read_region(H, x0, y0, w, h, lod=scene["lod"], side=scene["side"])
    assert np.array_equal(got_raw, raw) and missing == stats["tiles_missing"], "the device atlas is not the state the model was given"
    cost, nxt_d, stats_d = run(atlas, scene)
    differ = np.argwhere(bits(cost) != bits(D))
    assert differ.size == 0, (name, len(differ), differ[:5], cost[tuple(differ[0])], D[tuple(differ[0])])
    assert np.array_equal(nxt_d, nxt), (name, np.argwhere(nxt_d != nxt)[:5])
    assert {k: v for k, v in stats_d.items() if k not in SCHEDULE} == stats, name
    assert 1 <= stats_d["sweeps"] <= stats["cells"] and stats_d["launches"] == stats_d["sweeps"] + 3, (name, stats_d)
    return cost, nxt_d, stats_d


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["one_cell", "one_row", "one_column"])
def test_degenerate_windows(device, atlases, name):
    check_scene(atlases(name), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", PC.WIDTHS)
def test_widths_around_the_block_size_with_three_goals(device, atlases, name):
    check_scene(atlases(name), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["pure_distance_through_a_block_corner", "grade_unlimited", "grade_tight"])
def test_weights_and_grades(device, atlases, name):
    check_scene(atlases(name), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["missing_tiles", "missing_tiles_odd_window"])
def test_missing_tiles_are_blocked_and_counted(device, atlases, name):
    check_scene(atlases(name), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mask_alone", "mask_and_holes"])
def test_host_mask(device, atlases, name):
    check_scene(atlases(name), name)


@pytest.mark.gpu
def test_maze_needs_several_batches(device, atlases):
    """the maze is the path field's long walk: a route of 72 x 64 cells along rows, which a wave walks in lockstep, one cell a round and 64
    rounds a sweep; only a row's end, where the route changes rows and may change waves, can carry the news further in a round.  More than
    4 + 8 + 16 = 28 sweeps means that batches of kBatchMax = 32 ran, whose count comes back from the last of the 32 counters (the schedule
    model's fastest block order needs 97: tests/test_relax_model.py)"""
    _, _, stats = check_scene(atlases("maze"), "maze")
    assert stats["sweeps"] > 4 + 8 + 16, stats


@pytest.mark.gpu
@pytest.mark.parametrize("name", PC.CROSSING_SCENES)
def test_a_late_crossing_wakes_a_block_that_went_quiet(device, atlases, name):
    """more than 4 x 64 cells of corridor lie between the goal and the one step into the next block: the field crosses after the first
    batch of 4 sweeps, into a block that the one flag bit of the scene's name wakes.  At a corner the step is diagonal between two
    pillars, free cells too steep to step on, which keep the rule against cutting corners satisfied and carry nothing themselves"""
    _, nxt, stats = check_scene(atlases(name), name)
    assert stats["sweeps"] > 4, stats
    if name != "crossing_up":
        assert (nxt == _ffi.PATH_UNREACHABLE).sum() == 2


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["goal_in_a_corner", "goal_on_an_edge"])
def test_a_goal_walled_in_within_its_block_leaves_through_the_next(device, atlases, name):
    """the goal changes nothing in its own block, which therefore flags nothing: the blocks around it run because path_prepare_kernel
    flagged all 3 x 3"""
    cost, _, _ = check_scene(atlases(name), name)
    assert np.isfinite(cost).sum() >= 8


@pytest.mark.gpu
def test_cube_face(device, atlases):
    check_scene(atlases("cube_face"), "cube_face")
    # the same window of another side is another field: the side argument is used
    scene = dict(PC.SCENES["cube_face"], side=1)
    other, _, _ = run(atlases("cube_face"), scene)
    assert not np.array_equal(bits(other), bits(PC.expected("cube_face")[1]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["w65", "mask_and_holes", "maze"])
def test_two_calls_agree_and_routes_fold_to_their_cost(device, atlases, name):
    scene = PC.SCENES[name]
    atlas = atlases(name)
    raw, D, nxt, _, _ = PC.expected(name)
    cost_a, next_a, _ = run(atlas, scene)
    cost_b, next_b, _ = run(atlas, scene)
    assert cost_a.tobytes() == cost_b.tobytes() and next_a.tobytes() == next_b.tobytes()
    goal_costs, _ = M.usable_goals(raw, scene["mask"], scene["goals"])
    h, w = raw.shape
    rng = np.random.default_rng(9)
    starts = [PC.farthest(D)] + [(int(rng.integers(w)), int(rng.integers(h))) for _ in range(8)]
    for start in starts:
        cells, status = bt.trace_path(next_a, start)
        want, want_status = M.trace(nxt, start)
        cells = [tuple(int(v) for v in xy) for xy in cells]
        assert cells == want and status == want_status, (name, start)
        if status == "ok":  # the fold of w along the device's route, re-evaluated in numpy, is the device's cost at the start
            assert bits(M.fold_along(raw, scene["cost"], cells, goal_costs[cells[-1]])) == bits(cost_a[start[1], start[0]]), (name, start)


@pytest.mark.gpu
def test_each_output_may_be_null(device, atlases):
    scene = PC.SCENES["w33"]
    atlas = atlases("w33")
    _, D, nxt, stats, _ = PC.expected("w33")
    cost, none, s1 = run(atlas, scene, want_next=False)
    assert none is None and np.array_equal(bits(cost), bits(D))
    none, nxt_d, s2 = run(atlas, scene, want_cost=False)
    assert none is None and np.array_equal(nxt_d, nxt)
    none_a, none_b, s3 = run(atlas, scene, want_cost=False, want_next=False)
    assert none_a is None and none_b is None
    for s in (s1, s2, s3):
        assert {k: v for k, v in s.items() if k not in SCHEDULE} == stats
    # stats NULL
    x0, y0, w, h = scene["rect"]
    out = np.zeros((h, w), np.float32)
    goals = (_ffi.PathGoalC * 1)(_ffi.PathGoalC(20, 20, 0.5))
    cost_c = PathCost(**scene["cost"])._c()
    _ffi.check(_ffi.lib().bt_atlas_path_field(atlas._h, H, 0, 2, x0, y0, w, h, C.byref(cost_c), goals, 1, None, out.ctypes.data_as(C.POINTER(C.c_float)), None, None))
    assert np.isfinite(out).any()


@pytest.mark.gpu
def test_minus_zero_cost0_is_zero(device, atlases):
    scene = dict(PC.SCENES["w31"], goals=[(20, 20, -0.0)])
    cost, nxt, _ = run(atlases("w31"), scene)
    raw = PC.expected("w31")[0]
    D, want_next, _ = M.field(raw, None, scene["cost"], [(20, 20, 0.0)])
    assert np.array_equal(bits(cost), bits(D)) and np.array_equal(nxt, want_next) and bits(cost[20:21, 20:21])[0, 0] == 0


@pytest.mark.gpu
def test_refusals_leave_the_outputs_untouched(device, atlases):
    atlas = atlases("w31")
    L = _ffi.lib()
    w, h = 20, 10
    good_cost = dict(min_height=0.0, max_height=1.0, cell_size=1.0, max_grade=INF, grade_weight=0.0, climb_weight=0.0, descend_weight=0.0)

    def call(a=None, ai=H, side=0, lod=2, x0=3, y0=5, width=w, height=h, cost=good_cost, goals=((1, 1, 0.0),), goal_count=None, null_cost=False, null_goals=False):
        cost_out = np.full((h, w), 7.5, np.float32)
        next_out = np.full((h, w), 77, np.uint8)
        stats = _ffi.PathStatsC(*([9] * 8))
        arr = (_ffi.PathGoalC * max(len(goals), 1))(*[_ffi.PathGoalC(*g) for g in goals])
        cost_c = _ffi.PathCostC(*[cost[f] for f, _ in _ffi.PathCostC._fields_[:7]], 0)
        rc = L.bt_atlas_path_field(atlas._h if a is None else a, ai, side, lod, x0, y0, width, height, None if null_cost else C.byref(cost_c), None if null_goals else arr,
                                   len(goals) if goal_count is None else goal_count, None, cost_out.ctypes.data_as(C.POINTER(C.c_float)),
                                   next_out.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(stats))
        untouched = (cost_out == 7.5).all() and (next_out == 77).all()
        zeroed = all(getattr(stats, f) == 0 for f, _ in _ffi.PathStatsC._fields_)
        return rc, untouched, zeroed

    assert call()[0] == 0 and not call()[1]
    n = 272  # the mosaic of lod 2
    refused = [
        dict(ai=2), dict(side=1), dict(lod=3), dict(x0=n - 19), dict(y0=n - 9), dict(x0=n), dict(width=n + 1, x0=0),
        dict(null_cost=True), dict(null_goals=True), dict(goal_count=0), dict(goals=tuple((1, 1, 0.0) for _ in range(4097))),
        dict(width=2049, height=2049, x0=0, y0=0, lod=2),
        dict(goals=((w, 1, 0.0),)), dict(goals=((1, h, 0.0),)), dict(goals=((1, 1, 0.0), (1, 1, -1.0))), dict(goals=((1, 1, INF),)), dict(goals=((1, 1, NAN),)),
        dict(cost=dict(good_cost, cell_size=0.0)), dict(cost=dict(good_cost, cell_size=-1.0)), dict(cost=dict(good_cost, cell_size=INF)), dict(cost=dict(good_cost, cell_size=NAN)),
        dict(cost=dict(good_cost, grade_weight=-1.0)), dict(cost=dict(good_cost, climb_weight=INF)), dict(cost=dict(good_cost, descend_weight=NAN)),
        dict(cost=dict(good_cost, max_grade=NAN)), dict(cost=dict(good_cost, max_grade=-0.5)),
        dict(cost=dict(good_cost, min_height=-INF)), dict(cost=dict(good_cost, max_height=NAN)), dict(cost=dict(good_cost, min_height=-3e38, max_height=3e38)),
    ]
    for kw in refused:
        rc, untouched, zeroed = call(**kw)
        assert rc == BT_ERR_INVALID_ARGUMENT and untouched and zeroed, (kw if len(kw.get("goals", ())) < 10 else "4097 goals", rc)
    rc, untouched, zeroed = call(ai=G)  # the Rgba8 attachment
    assert rc == BT_ERR_UNSUPPORTED and untouched and zeroed
    # an empty window is BT_OK with nothing touched; max_grade +inf and 0 are allowed
    for kw in (dict(width=0), dict(height=0), dict(width=0, height=0)):
        rc, untouched, zeroed = call(**kw)
        assert rc == 0 and untouched and zeroed, kw
    assert call(cost=dict(good_cost, max_grade=0.0))[0] == 0
    # more than 2^22 cells: a mosaic wide enough for such a window (68 << 5 = 2176), which needs no tile, since the refusal comes first
    cfg = bt.TerrainConfig(lod_count=6, atlas_size=4, path="terrains/path_limits", model=bt.TerrainModel.planar((0, 0, 0), 1000.0, 0.0, 1.0))
    cfg.add_attachment(bt.AttachmentConfig(name="height", texture_size=72, border_size=2, format=bt.AttachmentFormat.R16))
    wide = bt.TileAtlas.new(cfg, device)
    for kw in (dict(width=2049, height=2048), dict(width=2048, height=2049), dict(width=2176, height=2176)):
        rc, untouched, zeroed = call(a=wide._h, ai=0, lod=5, x0=0, y0=0, **kw)
        assert rc == BT_ERR_INVALID_ARGUMENT and untouched and zeroed and b"cells" in _ffi.lib().bt_last_error(), kw


@pytest.mark.gpu
def test_a_window_no_tile_covers_is_all_blocked(device):
    cfg = bt.TerrainConfig(lod_count=3, atlas_size=4, path="terrains/path_empty", model=bt.TerrainModel.planar((0, 0, 0), 1000.0, 0.0, 1.0))
    cfg.add_attachment(bt.AttachmentConfig(name="height", texture_size=16, border_size=2, format=bt.AttachmentFormat.R16))
    atlas = bt.TileAtlas.new(cfg, device)
    cost, nxt, stats = atlas.path_field(0, 5, 7, 30, 20, PathCost(), [(3, 3), (4, 4, 1.0)])
    assert np.isinf(cost).all() and (nxt == _ffi.PATH_BLOCKED).all()
    assert {k: v for k, v in stats.items() if k not in SCHEDULE} == dict(cells=600, blocked=600, reachable=0, goals_used=0, goals_blocked=2, tiles_missing=9)

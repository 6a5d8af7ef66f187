"""The cases of tests/_prepass_cases.py reach the kernel and the branch each is there for — asserted from the numpy model alone, no GPU —
and the model's list is the sequential oracle's for every one of them.  The numbers are the model's at the commit that added the cases:
exact where the case depends on them (a pass of exactly 2048 tiles), lower bounds elsewhere.  test_gpu_prepass_shapes.py runs the same
cases on the device.

No test claims: the in-place evaluation of an ancestor outside its window in tiling_collect_kernel (the count is 0 for every window tile
of every case at every radius, see test_no_window_tile_has_an_ancestor_outside_its_window), and the barriers of the ordered kernel."""
import os
import re

import numpy as np
import pytest

import _cull_model as M
import _oracle as O
import _prepass_cases as P
import _refine_model as R
from test_refine_model import oracle_view

SOURCE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "bevy_terrain_amd", "csrc", "bt_refine.hip")
ASSISTED = [c for c in P.CASES if c.kernel == "assisted"]


def test_the_constants_are_the_kernels():
    """a change to one of them un-aims the cases: fail here, loudly"""
    text = open(SOURCE).read()
    for name, value in (("kWinK", P.WIN_K), ("kFrontierCap", P.FRONTIER_CAP), ("kThreads", P.THREADS), ("kMaxLods", P.MAX_LODS)):
        found = re.findall(r"constexpr\s+(?:int|uint32_t)\s+%s\s*=\s*(\d+)\s*;" % name, text)
        assert found == [str(value)], (name, found)
    assert re.findall(r"form == 0u && lods < (\d+)u", text) == [str(P.ASSIST_MIN_LODS)]
    assert "min(v.origin_lod, 30u)" in text  # window_origin's clamp of the view's tile, restated in _prepass_cases.window_origin


@pytest.mark.parametrize("case", P.CASES, ids=repr)
def test_the_model_is_the_oracle_and_the_estimate_picks_the_kernel(case):
    t = P.case_trace(case.name)
    v = case.view(max(t.n_min, 8))
    exp, indirect, passes = O.refine(oracle_view(v))
    assert np.array_equal(exp, t.final)
    assert passes[:len(t.passes)] == [p[0] for p in t.passes] and not any(passes[len(t.passes):])
    assert indirect == [v.vertices_per_tile * len(exp), 1, 0, 0]
    final, dropped, _ = R.refine(v)
    assert np.array_equal(final, t.final) and np.array_equal(dropped, t.dropped)
    # n_min is the edge of _cull_model.overflows (a pass needs its parents and their children, the final list its tiles)
    assert not M.overflows(t.passes, len(t.final), t.n_min) and M.overflows(t.passes, len(t.final), t.n_min - 1)
    # the restated estimate, with the margins that make it the host's whatever its log2f rounds to
    assert P.estimate_margin(v) >= 0.05
    assert t.lods >= 13 if case.kernel == "assisted" else t.lods <= 10
    assert t.deep == 0  # a direct call's estimate covers the tree: only bt_frame_update's stale height leaves LODs without bits


def numbers(name, radius=0):
    t = P.case_trace(name, radius)
    return t, [v for v, _ in t.passes]


def test_exact_cap():
    t, sizes = numbers("exact-cap")
    assert t.lods == 15 and sizes[6:11] == [1484, 2044, 2048, 2036, 2008]
    assert max(sizes) == P.FRONTIER_CAP and set(t.source) == {"lds"}  # a pass exactly at the cap, read from LDS
    assert 8 in t.second_sweep_children  # ... and its second sweep appends children


def test_around_cap():
    t, sizes = numbers("around-cap")
    assert t.lods == 16 and sizes[5:12] == [1024, 2056, 2044, 2060, 2052, 2032, 2012]
    assert t.sweeps[5] == 1 and t.sweeps[6] == 3  # one exactly full sweep; 2056 tiles take a third
    assert t.source[5:11] == ["lds", "global", "lds", "global", "global", "lds"]
    assert t.transitions == [("lds", "global"), ("global", "lds"), ("lds", "global"), ("global", "lds")]


def test_second_sweep():
    t, sizes = numbers("second-sweep")
    assert t.lods == 14 and sizes[6:10] == [988, 1140, 1108, 1096] and max(sizes) <= P.FRONTIER_CAP
    assert t.second_sweep_children == [7] and len(t.final) == t.n_min == 5230  # (the final list decides the capacity)


def test_outside_window():
    t, sizes = numbers("outside-window")
    assert t.lods == 14 and len(t.final) == 17197
    assert t.outside >= 16000 and t.outside_divide >= 800 and t.outside_divide_above_cap >= 600 and max(sizes) == 4052


def test_deep():
    t, sizes = numbers("deep")
    assert t.lods == 30 and t.deepest_lod == 27 and len(t.final) == 18724 and max(sizes) == 1140
    assert t.second_sweep_children == [13]
    assert int(t.final[:, 2:].max()) > 1 << 24  # float(tile.x) rounds


@pytest.mark.parametrize("name,lods", [("on-surface-30", 31), ("on-surface-31", 32), ("on-surface-origin-31", 31)])
def test_on_surface(name, lods):
    t, sizes = numbers(name)
    assert P.log2_ratio(P.BY_NAME[name].view()) is None  # clearance 0: the estimate falls through to 32
    assert t.lods == lods and t.deepest_lod == 30 and len(t.final) == 22051 and sizes[-1] == 1800 and len(t.dropped) == 0
    assert t.second_sweep_children == [13]
    # window_origin clamps the view's tile with min(origin_lod, 30): at origin_lod 31 the windows sit in the wrong place (time, not result)
    assert t.outside == (19756 if name == "on-surface-origin-31" else 450)
    assert t.outside_divide == (4632 if name == "on-surface-origin-31" else 0)


def test_sphere_deep():
    t, sizes = numbers("sphere-deep")
    assert t.lods == 31 and t.deepest_lod == 30 and len(t.final) == 40962 and sizes[-1] == 3360
    assert t.outside == 2649 and t.outside_divide >= 90 and t.transitions == [("lds", "global")] and len(t.second_sweep_children) >= 20


def test_corner():
    t, sizes = numbers("corner")
    assert t.lods == 30 and len(t.final) == 32076 and t.outside == 20355 and t.outside_divide >= 4600  # (the cube-sphere warp)
    assert t.transitions == [("lds", "global"), ("global", "lds")]


def test_shallow_and_pass_decides():
    for name, passes, dropped in (("shallow-planar", [(1, 1)], 1), ("shallow-sphere", [(6, 6), (24, 24)], 24)):
        t = P.case_trace(name)
        assert t.passes == passes and len(t.final) == 0 and len(t.dropped) == dropped
    t = P.case_trace("pass-decides")
    assert t.passes[-1] == (256, 244) and len(t.final) == 12 and t.n_min == 256 + 4 * 244  # a pass decides the capacity, not the list


def test_dividing_tiles_outside_their_windows_at_the_default_radius():
    """the assisted kernel's in-place fallback and the walk of the unordered form at radius 28"""
    hits = {c.name: P.case_trace(c.name).outside_divide for c in ASSISTED}
    assert {n for n, v in hits.items() if v > 0} >= {"outside-window", "corner", "sphere-deep", "on-surface-origin-31"}
    for name in ("outside-window", "corner", "sphere-deep"):
        assert P.case_trace(name).walk_roots > 0 and P.case_trace(name).climbs > 0


@pytest.mark.parametrize("radius", [9, 2])
def test_walks_descend_three_levels_and_climb(radius):
    deepest = {c.name: P.case_trace(c.name, radius) for c in P.CASES}
    assert any(t.walk_depth >= 3 and t.climbs > 0 and t.climbs_multi > 0 for t in deepest.values())
    assert deepest["corner"].walk_depth >= 13 and deepest["corner"].climbs_multi >= 1000
    if radius == 2:  # a walk that stops at refinement_count: its last descent is from LOD refinement_count - 1
        assert deepest["pass-decides"].walk_last_descent == 39 and deepest["on-surface-30"].walk_last_descent >= 400


def test_no_window_tile_has_an_ancestor_outside_its_window():
    """Windows nest: a tile within radius r of the view's tile (clamped into the face) has its parent within r of the view's parent, for
    every r >= 1.  So the in-place evaluation in tiling_collect_kernel's ancestor loop is reached by no thread: no test claims it."""
    for case in P.CASES:
        for radius in P.RADII:
            assert P.case_trace(case.name, radius).ancestor_outside == 0, (case, radius)
    for name in P.CULL:
        for radius in P.RADII:
            assert P.culled_trace(name, radius).ancestor_outside == 0


@pytest.mark.parametrize("name", sorted(P.CULL))
def test_the_culled_cases_cull_tiles_the_walk_tests_in_place(name):
    case, cull = P.BY_NAME[name], P.case_cull(name)
    t = P.culled_trace(name)
    final, n_culled, n_visited = M.refine_culled(case.view(), cull)
    assert np.array_equal(final, t.final) and (n_visited, n_culled) == (t.visited, t.culled)
    assert 0 < len(t.final) < len(P.case_trace(name).final)
    for radius in P.RADII:
        assert P.culled_trace(name, radius).uncovered_culled > 0, radius


def test_a_stale_estimate_leaves_lods_without_bits():
    """bt_frame_update estimates from the host's height, one frame old: after a teleport onto ground 8 m higher the tree is deeper than
    the LODs that got bits (the model of test_gpu_prepass_shapes.test_stale_height_through_frame_update, with nominal heights)"""
    case = P.Case("stale", P.PLANAR, (3.3, 108.25, -7.7), "assisted")
    config = P.bt.TerrainViewConfig(**case.config)
    stale = P.bt.make_view_state(case.model(), config, case.position, approximate_height=100.0)
    fresh = P.bt.make_view_state(case.model(), config, case.position, approximate_height=108.0)
    lods = P.estimate_lods(stale)
    t = P.trace(fresh, lods)
    assert lods == 14 and P.estimate_lods(fresh) >= 17 and t.deepest_lod == 16
    assert t.deep > 1000 and t.deep_divide > 100 and t.outside == 0 and t.uncovered == t.deep

"""tests/_path_model.py against the PATH FIELD definition of include/bevy_terrain_amd.h, without a GPU: Dijkstra against a plain whole-grid
Jacobi iteration bit for bit, against closed forms, and every scene of tests/_path_cases.py against what it is named for.  bt_path_trace,
which is host code, is held against the model's trace here as well."""
import ctypes as C

import numpy as np
import pytest

import _path_cases as PC
import _path_model as M
from bevy_terrain_amd import _ffi

F = np.float32


def bits(plane):
    return np.ascontiguousarray(plane, dtype=np.float32).view(np.uint32)


def flat(h, w, value=1000):
    return np.full((h, w), value, dtype=np.uint16)


@pytest.mark.parametrize("name", sorted(PC.SCENES))
def test_dijkstra_is_the_jacobi_fixed_point_bit_for_bit(name):
    scene = PC.SCENES[name]
    raw, D, nxt, stats, _ = PC.expected(name)
    W = M.edge_weights(raw, scene["mask"], scene["cost"])
    goal_costs, _ = M.usable_goals(raw, scene["mask"], scene["goals"])
    J, iterations = M.jacobi(W, goal_costs)
    assert np.array_equal(bits(J), bits(D)), name
    assert iterations <= raw.size - 1 or raw.size == 1


def test_random_heights_and_random_order_relaxation_agree():
    """the property the device relies on: relaxing cells in a random order, from +inf, reaches the same bits"""
    rng = np.random.default_rng(11)
    raw = rng.integers(1, 65536, size=(23, 29)).astype(np.uint16)
    raw[rng.random(raw.shape) < 0.1] = 0
    c = M.cost(min_height=-20.0, max_height=80.0, cell_size=3.0, max_grade=9.0, grade_weight=1.5, climb_weight=2.0, descend_weight=0.25)
    goals = [(4, 4, 0.0), (20, 15, 3.0), (10, 10, 0.125)]
    raw[4, 4] = raw[15, 20] = raw[10, 10] = 30000
    D, _, _ = M.field(raw, None, c, goals)
    W = M.edge_weights(raw, None, c)
    goal_costs, _ = M.usable_goals(raw, None, goals)
    X = np.full(raw.shape, M.INF, dtype=F)
    for (x, y), c0 in goal_costs.items():
        X[y, x] = c0
    h, w = raw.shape
    for _ in range(h * w):
        moved = False
        for i in rng.permutation(h * w):
            y, x = divmod(int(i), w)
            for k, (dx, dy) in enumerate(M.NEIGHBOURS):
                bx, by = x + dx, y + dy
                if 0 <= bx < w and 0 <= by < h and X[by, bx] + W[k, y, x] < X[y, x]:
                    X[y, x] = X[by, bx] + W[k, y, x]
                    moved = True
        if not moved:
            break
    assert np.array_equal(bits(X), bits(D))


def test_flat_window_is_the_octile_distance():
    cell = 2.0  # a power of two: n * cell is exact
    c = M.cost(cell_size=cell)
    gx, gy = 9, 6
    D, nxt, stats = M.field(flat(17, 25), None, c, [(gx, gy, 0.0)])
    ys, xs = np.mgrid[0:17, 0:25]
    dx, dy = np.abs(xs - gx), np.abs(ys - gy)
    assert np.array_equal(D[gy, :], (np.abs(np.arange(25) - gx) * cell).astype(F))
    assert np.array_equal(D[:, gx], (np.abs(np.arange(17) - gy) * cell).astype(F))
    diag = float(F(cell) * F(1.41421356))
    octile = (np.maximum(dx, dy) - np.minimum(dx, dy)) * cell + np.minimum(dx, dy) * diag
    assert np.allclose(D.astype(np.float64), octile, rtol=1e-6, atol=0.0)
    assert nxt[gy, gx] == M.GOAL and nxt[gy, gx + 3] == 4 and nxt[gy + 2, gx] == 6 and nxt[gy + 2, gx + 2] == 5
    assert stats == dict(cells=17 * 25, blocked=0, reachable=17 * 25, goals_used=1, goals_blocked=0)


def test_a_wall_with_one_gap_forces_the_route_through_the_gap():
    raw = flat(12, 21)
    raw[:, 10] = 0
    raw[3, 10] = 1000
    D, nxt, _ = M.field(raw, None, M.cost(), [(2, 9, 0.0)])
    cells, status = M.trace(nxt, (18, 9))
    assert status == M.TRACE_OK and (10, 3) in cells and cells[-1] == (2, 9)
    # no corner cutting: the cells diagonally beside the gap step straight, so the route holds (11, 3) and (9, 3) too
    assert (11, 3) in cells and (9, 3) in cells
    raw[3, 10] = 0
    D, nxt, stats = M.field(raw, None, M.cost(), [(2, 9, 0.0)])
    assert np.isinf(D[:, 11:]).all() and (nxt[:, 11:] == M.UNREACHABLE).all() and (nxt[:, 10] == M.BLOCKED).all()
    assert stats["reachable"] == 12 * 10 and stats["blocked"] == 12
    assert M.trace(nxt, (18, 9)) == ([(18, 9)], M.TRACE_UNREACHABLE) and M.trace(nxt, (10, 5)) == ([(10, 5)], M.TRACE_BLOCKED)


def test_max_grade_cuts_a_cliff():
    raw = flat(8, 16, 1000)
    raw[:, 8:] = 60000
    c = dict(min_height=0.0, max_height=100.0, cell_size=1.0)
    D, _, _ = M.field(raw, None, M.cost(**c, max_grade=5.0), [(1, 1, 0.0)])
    assert np.isfinite(D[:, :8]).all() and np.isinf(D[:, 8:]).all()
    D, _, _ = M.field(raw, None, M.cost(**c), [(1, 1, 0.0)])
    assert np.isfinite(D).all()


def test_climb_and_descend_weights_make_the_field_asymmetric():
    raw = np.tile((1000 + 3000 * np.arange(16)).astype(np.uint16), (5, 1))  # a ramp that rises with x
    c = M.cost(min_height=0.0, max_height=100.0, cell_size=1.0, climb_weight=3.0, descend_weight=0.0)
    down, _, _ = M.field(raw, None, c, [(0, 2, 0.0)])  # towards the foot: travelling from x = 15 descends
    up, _, _ = M.field(raw, None, c, [(15, 2, 0.0)])   # towards the top: travelling from x = 0 climbs
    assert down[2, 15] == F(15.0)
    assert up[2, 0] > down[2, 15] + F(100.0)
    level = M.cost(min_height=0.0, max_height=100.0, cell_size=1.0, climb_weight=1.0, descend_weight=1.0)
    a, _, _ = M.field(raw, None, level, [(0, 2, 0.0)])
    b, _, _ = M.field(raw, None, level, [(15, 2, 0.0)])
    assert abs(float(a[2, 15]) - float(b[2, 0])) <= 1e-5 * float(a[2, 15])


@pytest.mark.parametrize("name", sorted(PC.SCENES))
def test_every_scene_reaches_what_it_is_named_for(name):
    scene = PC.SCENES[name]
    raw, D, nxt, stats, reached = PC.expected(name)
    for want in scene["reach"]:
        assert reached.get(want, 0) >= 1, (name, want, reached)
    assert stats["goals_used"] >= 1, name
    # the fold of w along the route from the farthest cell is that cell's cost
    start = PC.farthest(D)
    cells, status = M.trace(nxt, start)
    assert status == M.TRACE_OK
    goal_costs, _ = M.usable_goals(raw, scene["mask"], scene["goals"])
    assert bits(M.fold_along(raw, scene["cost"], cells, goal_costs[cells[-1]])) == bits(D[start[1], start[0]]), name


def test_the_scenes_together_reach_the_definition():
    reached = {}
    for name in PC.SCENES:
        for k, v in PC.expected(name)[4].items():
            reached[k] = reached.get(k, 0) + int(v)
    for want in ("unreachable", "dominated_goals", "corner_cut", "long_route", "grade_cut", "goals_blocked", "tiles_missing", "mask_only", "holes_and_mask", "block_corner"):
        assert reached.get(want, 0) >= 1, (want, reached)
    raw, D, nxt, _, _ = PC.expected("maze")
    assert raw.shape == (96, 96)
    cells, status = M.trace(nxt, PC.farthest(D))
    assert status == M.TRACE_OK and len(cells) >= 2000


# ---------------------------------------------------------------------------------------------- bt_path_trace (host code)

def lib_trace(nxt, start, cap=None):
    L = _ffi.lib()
    nxt = np.ascontiguousarray(nxt, dtype=np.uint8)
    h, w = nxt.shape
    count, status = C.c_uint32(77), C.c_uint32(77)
    n = h * w + 1 if cap is None else cap
    out = np.full((n + 1, 2), 0xABCD, dtype=np.uint32)
    rc = L.bt_path_trace(nxt.ctypes.data_as(C.POINTER(C.c_uint8)), w, h, start[0], start[1], out.ctypes.data_as(C.POINTER(C.c_uint32)), n, C.byref(count), C.byref(status))
    assert (out[n:] == 0xABCD).all() and (out[min(count.value, n):] == 0xABCD).all(), "wrote past what it may"
    return rc, [tuple(int(v) for v in xy) for xy in out[:min(count.value, n)]], count.value, status.value


STATUS = {0: M.TRACE_OK, 1: M.TRACE_BLOCKED, 2: M.TRACE_UNREACHABLE, 3: M.TRACE_LOOP}


@pytest.mark.parametrize("name", ["maze", "mask_and_holes", "w65", "one_cell"])
def test_trace_follows_the_model(name):
    import bevy_terrain_amd as bt
    raw, D, nxt, _, _ = PC.expected(name)
    h, w = nxt.shape
    rng = np.random.default_rng(5)
    starts = [PC.farthest(D)] + [(int(rng.integers(w)), int(rng.integers(h))) for _ in range(12)]
    for start in starts:
        want, want_status = M.trace(nxt, start)
        rc, got, count, status = lib_trace(nxt, start)
        assert rc == 0 and got == want and count == len(want) and STATUS[status] == want_status, (name, start)
        cells, text = bt.trace_path(nxt, start)
        assert [tuple(int(v) for v in xy) for xy in cells] == want and text == want_status
    # a cap below the count: the first `cap` cells, the full count
    want, _ = M.trace(nxt, starts[0])
    rc, got, count, status = lib_trace(nxt, starts[0], cap=min(3, len(want)))
    assert rc == 0 and got == want[:3] and count == len(want) and status == 0


def test_trace_loops_bad_bytes_and_refusals():
    L = _ffi.lib()
    two = np.array([[0, 4]], dtype=np.uint8)  # two cells that point at each other
    rc, got, count, status = lib_trace(two, (0, 0))
    assert rc == 0 and STATUS[status] == M.TRACE_LOOP and count == 3 and M.trace(two, (0, 0)) == (got, M.TRACE_LOOP)
    for bad, start in ((np.array([[4, 8]], dtype=np.uint8), (0, 0)),       # points out of the window to the left
                       (np.array([[6, 8]], dtype=np.uint8), (0, 0)),       # ... above
                       (np.array([[0, 1]], dtype=np.uint8), (0, 0)),       # ... below, from the second cell
                       (np.array([[0, 9], [8, 8]], dtype=np.uint8), (0, 0)),    # a byte that is no direction
                       (np.array([[0, 255], [8, 8]], dtype=np.uint8), (0, 0)),  # walks onto a blocked cell
                       (np.array([[0, 254], [8, 8]], dtype=np.uint8), (0, 0))):
        rc, got, count, status = lib_trace(bad, start)
        want, want_status = M.trace(bad, start)
        assert rc == 0 and STATUS[status] == M.TRACE_LOOP == want_status and got == want, bad
    ok = np.array([[8]], dtype=np.uint8)
    p = ok.ctypes.data_as(C.POINTER(C.c_uint8))
    count, status, xy = C.c_uint32(5), C.c_uint32(5), (C.c_uint32 * 2)(9, 9)
    for args in ((None, 1, 1, 0, 0, xy, 1, C.byref(count), C.byref(status)), (p, 1, 1, 0, 0, xy, 1, C.byref(count), None), (p, 1, 1, 0, 0, None, 1, C.byref(count), C.byref(status)),
                 (p, 0, 1, 0, 0, xy, 1, C.byref(count), C.byref(status)), (p, 1, 0, 0, 0, xy, 1, C.byref(count), C.byref(status)),
                 (p, 1, 1, 1, 0, xy, 1, C.byref(count), C.byref(status)), (p, 1, 1, 0, 1, xy, 1, C.byref(count), C.byref(status))):
        status.value = 5
        assert L.bt_path_trace(*args) == -1 and status.value == 5 and tuple(xy) == (9, 9)
    assert L.bt_path_trace(p, 1, 1, 0, 0, None, 0, None, C.byref(status)) == 0 and status.value == 0


def test_field_refusals_without_an_atlas():
    L = _ffi.lib()
    stats = _ffi.PathStatsC(*([7] * 8))
    cost_c = _ffi.PathCostC(0.0, 1.0, 1.0, np.inf, 0.0, 0.0, 0.0, 0)
    goal = (_ffi.PathGoalC * 1)(_ffi.PathGoalC(0, 0, 0.0))
    assert L.bt_atlas_path_field(None, 0, 0, 0, 0, 0, 1, 1, C.byref(cost_c), goal, 1, None, None, None, C.byref(stats)) == -1
    assert all(getattr(stats, f) == 0 for f, _ in _ffi.PathStatsC._fields_)
    assert L.bt_atlas_path_field(None, 0, 0, 0, 0, 0, 0, 0, None, None, 0, None, None, None, None) == -1
    assert C.sizeof(_ffi.PathCostC) == 32 and C.sizeof(_ffi.PathGoalC) == 12 and C.sizeof(_ffi.PathStatsC) == 32

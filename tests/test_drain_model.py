"""The model of bt_atlas_drainage (tests/_drain_model.py) without a GPU: against a brute-force restatement of the header's DRAINAGE section
on small windows, against hand-worked answers, and its invariants on every scene of tests/_drain_cases.py, each of which must also reach
what its name claims."""
import numpy as np
import pytest

import _drain_cases as DC
import _drain_model as M
import bevy_terrain_amd as bt

INF = 1 << 40


def brute(raw, void=None, weight=None):
    """the header restated as fixed points: W by relaxation from above, F and A by repeated passes until nothing moves"""
    h, w = raw.shape
    is_void = M.void_cells(raw, void)
    z = raw.astype(np.int64)
    cells = [(x, y) for y in range(h) for x in range(w) if not is_void[y, x]]

    def nb(x, y):
        return [(k, x + dx, y + dy) if 0 <= x + dx < w and 0 <= y + dy < h and not is_void[y + dy, x + dx] else (k, None, None) for k, (dx, dy) in enumerate(M.NEIGHBOURS)]

    outlet = {c for c in cells if any(nx is None for _, nx, _ in nb(*c))}
    W = {c: int(z[c[1], c[0]]) if c in outlet else INF for c in cells}
    moved = True
    while moved:
        moved = False
        for c in cells:
            if c in outlet:
                continue
            v = max(int(z[c[1], c[0]]), min(W[(nx, ny)] for _, nx, ny in nb(*c)))
            if v < W[c]:
                W[c], moved = v, True
    drain = {c for c in cells if c in outlet or any(W[(nx, ny)] < W[c] for _, nx, ny in nb(*c) if nx is not None)}
    F = {c: 0 if c in drain else INF for c in cells}
    moved = True
    while moved:
        moved = False
        for c in cells:
            if c in drain:
                continue
            v = 1 + min([F[(nx, ny)] for _, nx, ny in nb(*c) if W[(nx, ny)] == W[c]], default=INF)
            if v < F[c]:
                F[c], moved = v, True
    direction = np.full((h, w), M.VOID, np.uint8)
    for c in cells:
        if c in outlet:
            k = M.OUTLET
        elif any(W[(nx, ny)] < W[c] for _, nx, ny in nb(*c)):
            scores = [((W[c] - W[(nx, ny)]) ** 2 * (1 if k & 1 else 2), -k) for k, nx, ny in nb(*c) if W[(nx, ny)] < W[c]]
            k = -max(scores)[1]
        else:
            k = min(k for k, nx, ny in nb(*c) if W[(nx, ny)] == W[c] and F[(nx, ny)] == F[c] - 1)
        direction[c[1], c[0]] = k
    wt = {c: 1 if weight is None else int(weight[c[1], c[0]]) for c in cells}
    donors = {c: [] for c in cells}
    for c, r in M.receivers(direction).items():
        donors[r].append(c)
    A = dict(wt)
    moved = True
    while moved:
        moved = False
        for c in cells:
            v = wt[c] + sum(A[d] for d in donors[c])
            if v != A[c]:
                A[c], moved = v, True
    plane = lambda values, dtype: np.array([[values.get((x, y), 0) for x in range(w)] for y in range(h)], dtype=dtype)
    return plane(W, np.uint16), plane(F, np.uint32), direction, plane(A, np.uint32)


@pytest.mark.parametrize("seed", range(24))
def test_model_equals_the_brute_force_restatement(seed):
    rng = np.random.default_rng(seed)
    h, w = int(rng.integers(1, 13)), int(rng.integers(1, 13))
    levels = [3, 12, 65535][seed % 3]  # few levels: flats and ties everywhere
    raw = rng.integers(1, levels + 1, (h, w)).astype(np.uint16)
    raw[rng.random((h, w)) < [0.0, 0.05, 0.3][(seed // 3) % 3]] = 0
    void = (rng.random((h, w)) < 0.1).astype(np.uint8) if seed % 4 == 1 else None
    weight = rng.integers(0, 256, (h, w)).astype(np.uint8) if seed % 2 else None
    got = M.drainage(raw, void, weight)
    for g, b, what in zip(got, brute(raw, void, weight), "WFdA"):
        assert np.array_equal(g, b), (seed, what)


def test_bowl_by_hand():
    raw = np.array([[9, 9, 9, 9, 9],
                    [9, 5, 5, 5, 9],
                    [9, 5, 1, 5, 7],
                    [9, 5, 5, 5, 9],
                    [9, 9, 9, 9, 9]], np.uint16)
    W, F, d, A, stats = M.drainage(raw)
    # the rim's lowest cell is the 7 at the edge: the 3 x 3 fills to 7; (3, 1..3) see it lower than nothing (7 == 7): the level area is
    # the 3 x 3 plus that outlet, and the distance counts from the outlet
    assert W.tolist() == [[9, 9, 9, 9, 9], [9, 7, 7, 7, 9], [9, 7, 7, 7, 7], [9, 7, 7, 7, 9], [9, 9, 9, 9, 9]]
    assert F.tolist() == [[0] * 5, [0, 3, 2, 1, 0], [0, 3, 2, 1, 0], [0, 3, 2, 1, 0], [0] * 5]
    # towards (4, 2): from column 3 k = 1, 0, 7; further in the smallest k with F one less: k = 0 where it exists, else the diagonal
    assert d.tolist() == [[8] * 5, [8, 0, 0, 1, 8], [8, 0, 0, 0, 8], [8, 0, 0, 7, 8], [8] * 5]
    assert A.tolist() == [[1] * 5, [1, 1, 2, 3, 1], [1, 1, 2, 3, 10], [1, 1, 2, 3, 1], [1] * 5]
    assert stats == dict(cells=25, voids=0, outlets=16, filled=9, flats=9, max_flat_distance=3, max_accumulation=10, outflow=25)


def test_row_by_hand():
    raw = np.array([[5, 3, 0, 4, 4, 9]], np.uint16)
    W, F, d, A, stats = M.drainage(raw, weight=np.array([[2, 3, 7, 0, 255, 1]], np.uint8))
    assert W.tolist() == [[5, 3, 0, 4, 4, 9]] and F.tolist() == [[0] * 6] and d.tolist() == [[8, 8, 255, 8, 8, 8]] and A.tolist() == [[2, 3, 0, 0, 255, 1]]
    assert stats == dict(cells=6, voids=1, outlets=5, filled=0, flats=0, max_flat_distance=0, max_accumulation=255, outflow=261)


def test_two_pit_cells_fill_to_the_rim_not_below():
    """the fixed point that is wanted is the one from above: the two pit cells could hold each other at any level from 2 to 6"""
    raw = np.array([[9, 9, 9, 9], [9, 1, 2, 6], [9, 9, 9, 9]], np.uint16)
    W = M.drainage(raw)[0]
    assert W[1].tolist() == [9, 6, 6, 6]


@pytest.mark.parametrize("name", sorted(DC.SCENES))
def test_scene_invariants_and_reach(name):
    scene = DC.SCENES[name]
    raw, W, F, direction, A, stats = DC.expected(name)
    h, w = raw.shape
    active = direction != M.VOID
    assert stats["cells"] == h * w and stats["voids"] == int((~active).sum())
    assert ((W >= raw) | ~active).all() and not W[~active].any() and not F[~active].any() and not A[~active].any()
    # the receiver is strictly smaller in (W, F)
    for (x, y), (rx, ry) in M.receivers(direction).items():
        assert (int(W[ry, rx]), int(F[ry, rx])) < (int(W[y, x]), int(F[y, x])), (name, x, y)
    # what rains on the window leaves it
    weight = np.ones((h, w), np.int64) if scene["weight"] is None else scene["weight"].astype(np.int64)
    assert stats["outflow"] == int(weight[active].sum()) == int(A[direction == M.OUTLET].astype(np.int64).sum())
    reaches = DC.scene_reaches(name)
    for want in scene["reach"]:
        assert reaches.get(want), (name, want, stats)


@pytest.mark.parametrize("name", ["bowl_with_island_lake", "serpentine", "all_three_voids", "w33_h33_quantised"])
def test_path_trace_follows_the_directions_to_an_outlet(name):
    """BT_DRAIN_OUTLET == BT_PATH_GOAL and BT_DRAIN_VOID == BT_PATH_BLOCKED: bt_path_trace (host code) ends OK from every active cell, after
    as many cells as the model's own walk"""
    direction = DC.expected(name)[3]
    assert M.OUTLET == bt._ffi.PATH_GOAL == bt._ffi.DRAIN_OUTLET and M.VOID == bt._ffi.PATH_BLOCKED == bt._ffi.DRAIN_VOID
    for y, x in np.argwhere(direction != M.VOID):
        cells, status = bt.trace_path(direction, (int(x), int(y)))
        assert status == "ok" and len(cells) == M.chain_length(direction, (int(x), int(y))), (name, x, y)
    voids = np.argwhere(direction == M.VOID)
    if len(voids):
        assert bt.trace_path(direction, (int(voids[0][1]), int(voids[0][0])))[1] == "blocked"

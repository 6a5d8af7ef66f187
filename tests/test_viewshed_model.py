"""The model of bt_atlas_viewshed (tests/_viewshed_model.py) without a GPU: against an independent restatement in fractions on small
windows, against answers worked by hand, the symmetry of intervisibility, and the reach of every scene of tests/_viewshed_cases.py, each
of which must hold what its name claims.  And the declaration: the header, and the binding that mirrors it."""
import ctypes as C
import math
import re
from fractions import Fraction

import numpy as np
import pytest

import _viewshed_cases as VC
import _viewshed_model as M
from bevy_terrain_amd import _ffi


def ground(z, ox, oy, tx, ty, j):
    """the interpolated ground under P_j of the line from (ox, oy) to (tx, ty), a Fraction"""
    dx, dy = tx - ox, ty - oy
    n = max(abs(dx), abs(dy))
    px, py = ox + Fraction(dx * j, n), oy + Fraction(dy * j, n)
    fx, fy = math.floor(px), math.floor(py)  # one of the two is the coordinate itself
    if px != fx:
        return z[fy][fx] * (1 - (px - fx)) + z[fy][fx + 1] * (px - fx)
    if py != fy:
        return z[fy][fx] * (1 - (py - fy)) + z[fy + 1][fx] * (py - fy)
    return Fraction(z[fy][fx])


def clearance_by_raising(z, ox, oy, eye_height, tx, ty):
    """the smallest whole t for which the straight line from the eye to t above the ground at the target clears the ground at every P_j"""
    n = max(abs(tx - ox), abs(ty - oy))
    E = z[oy][ox] + eye_height
    t = 0
    while not all(E + Fraction((z[ty][tx] + t - E) * j, n) >= ground(z, ox, oy, tx, ty, j) for j in range(1, n)):
        t += 1
    return t


@pytest.mark.parametrize("seed", range(12))
def test_model_equals_the_restatement_in_fractions(seed):
    rng = np.random.default_rng(seed)
    h, w = (9, 11) if seed == 0 else (int(rng.integers(1, 10)), int(rng.integers(1, 12)))
    raw = rng.integers(1, [4, 25, 60][seed % 3], (h, w)).astype(np.uint16)
    raw[rng.random((h, w)) < [0.0, 0.1, 0.3][(seed // 3) % 3]] = 0
    z = raw.astype(int).tolist()
    for _ in range(3):
        ox, oy, eye = int(rng.integers(0, w)), int(rng.integers(0, h)), int(rng.integers(0, 12))
        if raw[oy, ox] == 0:
            continue
        C_o, _ = M.observer_clearance(raw, ox, oy, eye)
        for ty in range(h):
            for tx in range(w):
                assert int(C_o[ty, tx]) == clearance_by_raising(z, ox, oy, eye, tx, ty), (seed, (ox, oy, eye), (tx, ty))


@pytest.mark.parametrize("seed", range(6))
def test_planes_and_stats_follow_the_observers(seed):
    """clearance, count, mask and the stats, from per-observer clearances put together cell by cell in Python integers"""
    rng = np.random.default_rng(100 + seed)
    h, w = int(rng.integers(2, 10)), int(rng.integers(2, 12))
    raw = rng.integers(1, 30, (h, w)).astype(np.uint16)
    raw[rng.random((h, w)) < 0.15] = 0
    observers = [(int(rng.integers(0, w)), int(rng.integers(0, h)), int(rng.integers(0, 9)), int(rng.integers(0, 6))) for _ in range(5)]
    t = int(rng.integers(0, 4))
    clearance, count, mask, stats = M.viewshed(raw, observers, t)
    used = [(o, ob) for o, ob in enumerate(observers) if raw[ob[1], ob[0]]]
    samples = 0
    for y in range(h):
        for x in range(w):
            each = {o: clearance_by_raising(raw.astype(int).tolist(), ox, oy, e, x, y) for o, (ox, oy, e, r) in used
                    if raw[y, x] and (r == 0 or (x - ox) ** 2 + (y - oy) ** 2 <= r * r)}
            samples += sum(max(max(abs(x - observers[o][0]), abs(y - observers[o][1])) - 1, 0) for o in each)
            assert clearance[y, x] == (min(each.values()) if each else M.NONE)
            assert count[y, x] == sum(c <= t for c in each.values()) and int(mask[y, x]) == sum(1 << o for o, c in each.items() if c <= t)
    assert stats["observers_used"] == len(used) and stats["observers_skipped"] == 5 - len(used) and stats["samples"] == samples
    assert stats["voids"] == int((raw == 0).sum()) and stats["covered"] == int((clearance != M.NONE).sum()) and stats["visible"] == int((count > 0).sum())


def test_plateau_by_hand():
    raw = np.full((7, 9), 500, np.uint16)
    clearance, count, mask, stats = M.viewshed(raw, [(4, 3, 0), (0, 0, 10)])
    assert not clearance.any() and (count == 2).all() and (mask == 3).all()
    assert stats == dict(cells=63, voids=0, observers_used=2, observers_skipped=0, covered=63, visible=63, max_clearance=0,
                         samples=sum(max(max(abs(x - ox), abs(y - oy)) - 1, 0) for ox, oy in ((4, 3), (0, 0)) for y in range(7) for x in range(9)))


@pytest.mark.parametrize("d", [1, 2, 3, 7])
def test_ridge_by_hand(d):
    """level ground, the observer with eye_height 0 at (1, 2), one cell one unit higher d cells to its right: behind the ridge, n cells
    from the observer along the row, the line must rise by n / d, rounded up; up to the ridge and on it everything is seen"""
    raw = np.full((5, 24), 100, np.uint16)
    raw[2, 1 + d] = 101
    clearance = M.viewshed(raw, [(1, 2, 0)])[0]
    assert clearance[2, :2 + d].tolist() == [0] * (2 + d)
    assert clearance[2, 2 + d:].tolist() == [-(-n // d) for n in range(d + 1, 23)]


@pytest.mark.parametrize("h", [0, 3])
def test_intervisibility_is_symmetric(h):
    """with eye_height = target_height = h: O sees T iff T sees O, over all pairs of a small random window"""
    rng = np.random.default_rng(5)
    raw = rng.integers(1, 12, (7, 8)).astype(np.uint16)
    sees = {}
    for oy in range(7):
        for ox in range(8):
            sees[(ox, oy)] = M.viewshed(raw, [(ox, oy, h)], h)[1]
    differ = [(o, (tx, ty)) for o in sees for ty in range(7) for tx in range(8) if sees[o][ty, tx] != sees[(tx, ty)][o[1], o[0]]]
    assert not differ, differ[:5]
    assert 0 < sum(int(s.sum()) for s in sees.values()) < 56 * 56  # some pairs see each other and some do not


@pytest.mark.parametrize("name", sorted(VC.SCENES))
def test_scene_reach(name):
    scene = VC.SCENES[name]
    raw, clearance, count, mask, stats = VC.expected(name)
    h, w = raw.shape
    assert stats["cells"] == h * w and stats["observers_used"] + stats["observers_skipped"] == len(scene["observers"])
    assert (clearance[raw == 0] == M.NONE).all() and not count[raw == 0].any() and not mask[raw == 0].any()
    assert ((count > 0) <= (clearance <= scene["target_height"])).all() and stats["visible"] <= stats["covered"]
    reaches = VC.scene_reaches(name)
    for want in scene["reach"]:
        assert reaches.get(want), (name, want, stats)


def test_target_height_moves_count_and_mask_only():
    planes = [VC.expected(name) for name in VC.TARGETS]
    assert all(np.array_equal(p[1], planes[0][1]) for p in planes)
    assert planes[0][4]["visible"] < planes[1][4]["visible"] < planes[2][4]["visible"] == planes[2][4]["covered"]


def test_header_and_binding_declare_the_call():
    with open(_ffi.HEADER_PATH) as f:
        header = f.read()
    assert "bt_atlas_viewshed" in _ffi.header_symbols() and "bt_atlas_viewshed" in _ffi.PROTOTYPES
    values = {name: int(value.rstrip("u"), 0) if "<<" not in value else 1 << int(re.search(r"<<\s*(\d+)", value).group(1))
              for name, value in re.findall(r"#define (BT_VIEWSHED_\w+) (\(?[0-9a-fA-Fx]+u?(?: << \d+\))?)", header)}
    assert values == dict(BT_VIEWSHED_NONE=0xFFFFFFFF, BT_VIEWSHED_MAX_OBSERVERS=64, BT_VIEWSHED_MAX_SIDE=32768, BT_VIEWSHED_MAX_CELLS=1 << 22)
    assert (_ffi.VIEWSHED_NONE, _ffi.VIEWSHED_MAX_OBSERVERS, _ffi.VIEWSHED_MAX_SIDE, _ffi.VIEWSHED_MAX_CELLS) == (0xFFFFFFFF, 64, 32768, 1 << 22)
    assert (M.NONE, M.MAX_OBSERVERS, M.MAX_SIDE, M.MAX_CELLS) == (0xFFFFFFFF, 64, 32768, 1 << 22)
    assert C.sizeof(_ffi.ViewshedObserverC) == 16 and C.sizeof(_ffi.ViewshedStatsC) == 64 and _ffi.ViewshedStatsC.samples.offset == 32
    assert re.search(r"\}\s*bt_viewshed_observer;\s*/\* 16 bytes \*/", header) and re.search(r"\}\s*bt_viewshed_stats;\s*/\* 64 bytes \*/", header)

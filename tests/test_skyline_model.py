"""The model of bt_atlas_skyline (tests/_skyline_model.py) against the header's hull reading restated, answers worked by hand, the
invariants of the digital lines, bt_skyline_line_count and TileAtlas.sun_directions; and every scene of tests/_skyline_cases.py against
what it is named for.  No GPU."""
import ctypes as C
import math
import re
from pathlib import Path

import numpy as np
import pytest

import _skyline_cases as SC
import _skyline_model as M
import bevy_terrain_amd as bt
from bevy_terrain_amd import _ffi

ROOT = Path(__file__).resolve().parents[1]
VECTORS = [(dx, dy) for dx in range(-7, 8) for dy in range(-7, 8) if dx or dy]


@pytest.mark.parametrize("levels", [2, 4, 400])
def test_the_hull_reading_is_the_definition(levels):
    """random windows with heavy ties, every direction with components up to 7"""
    rng = np.random.default_rng(levels)
    for _ in range(120):
        h, w = rng.integers(1, 13, 2)
        z = (rng.integers(0, levels, (h, w)) * (65535 // (levels - 1))).astype(np.uint16)
        dx, dy = VECTORS[rng.integers(len(VECTORS))]
        steps, rise = M.horizon(z, dx, dy)
        steps_h, rise_h, _ = M.hull(z, dx, dy)
        assert np.array_equal(steps, steps_h) and np.array_equal(rise, rise_h), (z, dx, dy)


@pytest.mark.parametrize("name", sorted(SC.SCENES))
def test_the_hull_reading_on_every_scene(name):
    raw, steps, rise, *_ = SC.expected(name)
    for k, (dx, dy, _, _) in enumerate(SC.SCENES[name]["directions"][:17]):
        steps_h, rise_h, _ = M.hull(raw, dx, dy)
        assert np.array_equal(steps[k], steps_h) and np.array_equal(rise[k], rise_h), (name, k)


def test_a_row_by_hand():
    z = np.array([[10, 20, 30, 5, 40, 0]], np.uint16)
    steps, rise, mask, count, stats = M.skyline(z, [(1, 0, 10, 1), (-1, 0, 0, 1), (1, 0, 9, 1)])
    assert steps[0].tolist() == [[1, 1, 2, 1, 1, 0]] and rise[0].tolist() == [[10, 10, 10, 35, -40, 0]]  # from x = 0: 10 / 1 = 20 / 2, the nearest
    assert steps[1].tolist() == [[0, 1, 1, 1, 2, 1]] and rise[1].tolist() == [[0, -10, -10, 25, -10, 40]]
    assert mask.tolist() == [[0b011, 0b011, 0b111, 0b000, 0b111, 0b101]] and count.tolist() == [[2, 2, 3, 0, 3, 2]]
    assert stats == dict(cells=6, voids=1, directions=3, lines=3, longest_line=6, max_steps=2, lit=12, sum_steps=18)


def test_a_diagonal_and_an_oblique_by_hand():
    z = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9]], np.uint16)
    steps, rise = M.horizon(z, 1, 1)
    assert steps.tolist() == [[1, 1, 0], [1, 1, 0], [0, 0, 0]] and rise.tolist() == [[4, 4, 0], [4, 4, 0], [0, 0, 0]]
    assert M.line_counts(3, 3, 1, 1) == (5, 3) and M.line_counts(3, 3, -1, 1) == (5, 3) and M.line_counts(3, 3, 1, 0) == (3, 3)
    # (2, 1): off(x) = floor((2 x + 2) / 4) = 0, 1, 1: the line of (0, 0) goes on through (1, 1) and (2, 1)
    j, x_major = M.line_index(3, 3, 2, 1)
    assert x_major and j.tolist() == [[0, -1, -1], [1, 0, 0], [2, 1, 1]]
    steps, rise = M.horizon(z, 2, 1)
    assert (steps[0, 0], rise[0, 0]) == (1, 4) and (steps[1, 1], rise[1, 1]) == (1, 1) and steps[1, 2] == 0
    # the true floor: with m = -1, off(x) = floor((2 - 2 x) / 4) runs 0, 0, -1
    assert M.line_index(3, 3, 2, -1)[0].tolist() == [[0, 0, 1], [1, 1, 2], [2, 2, 3]]


def test_the_bake_byte():
    count = np.array([[0, 1, 2, 3]], np.uint8)
    assert M.bake_plane(count, 3).tolist() == [[0, 85, 170, 255]] and M.bake_plane(count, 3, shade=True).tolist() == [[255, 170, 85, 0]]
    assert M.bake_plane(count[:, :2], 1).tolist() == [[0, 255]]
    assert M.bake_plane(np.array([[63, 64]], np.uint8), 64).tolist() == [[251, 255]]
    before = np.arange(16, dtype=np.uint8).reshape(1, 4, 4)
    after = M.bake(before, count, 3, 2)
    assert after[0, :, 2].tolist() == [0, 85, 170, 255] and np.array_equal(np.delete(after, 2, 2), np.delete(before, 2, 2))


@pytest.mark.parametrize("h,w", [(1, 1), (1, 9), (9, 1), (5, 8), (13, 6)])
def test_the_lines_partition_the_window_in_contiguous_ranges(h, w):
    for dx, dy in VECTORS + [(1024, 1023), (-1023, 1024), (1024, -1), (1, 1024)]:
        j, x_major = M.line_index(h, w, dx, dy)
        lines, _ = M.lines_of(h, w, dx, dy)
        assert sorted(c for line in lines for c in line) == sorted((x, y) for y in range(h) for x in range(w))  # every cell on exactly one line
        for line in lines:
            major = [c[0] if x_major else c[1] for c in line]
            assert sorted(major) == list(range(min(major), max(major) + 1))  # a contiguous range, each coordinate once
            minor = [c[1] if x_major else c[0] for c in line]
            assert all(abs(a - b) <= 1 for a, b in zip(minor, minor[1:]))
        assert set(np.unique(j)) == set(range(int(j.min()), int(j.max()) + 1))
        assert np.array_equal(j, M.line_index(h, w, 3 * dx, 3 * dy)[0]) if max(abs(dx), abs(dy)) * 3 <= 1024 else True  # scaling
        assert np.array_equal(j, M.line_index(h, w, -dx, -dy)[0])  # reversal: the same lines
    for d in (1, 5):  # an exact diagonal: the same lines on either axis
        for sx, sy in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
            jx, _ = M.line_index(h, w, sx * d, sy * d)
            ys, xs = np.mgrid[0:h, 0:w]
            jy = xs - (ys if sx * sy > 0 else -ys)  # the y-major reading: m = sx * sy, n = 1, off(y) = floor((2 y m + 1) / 2) = y m
            assert len({(a, b) for a, b in zip(jx.ravel().tolist(), jy.ravel().tolist())}) == len(np.unique(jx)) == len(np.unique(jy))


def test_lit_is_monotone_in_the_sun():
    raw, steps, rise, *_ = SC.expected("sixteen_ways")
    before = np.zeros(steps[2].shape, bool)
    for num in (0, 1, 7, 50, 200, 398, 399, 400, 1 << 20, (1 << 31) - 1):
        lit = M.lit_plane(steps[2], rise[2], num, 3)
        assert not (before & ~lit).any()
        before = lit
    assert before.all() and bool((~M.lit_plane(steps[2], rise[2], 0, 65535)).any())
    assert np.array_equal(M.lit_plane(steps[2], rise[2], 14, 6), M.lit_plane(steps[2], rise[2], 7, 3))


def line_count(w, h, dx, dy):
    lines, longest = C.c_uint32(7), C.c_uint32(7)
    rc = _ffi.lib().bt_skyline_line_count(w, h, dx, dy, C.byref(lines), C.byref(longest))
    return rc, lines.value, longest.value


@pytest.mark.parametrize("name", sorted(SC.SCENES))
def test_line_count_on_the_scenes(name):
    scene = SC.SCENES[name]
    w, h = scene["rect"][2:]
    total = longest = 0
    for dx, dy, _, _ in scene["directions"]:
        rc, a, b = line_count(w, h, dx, dy)
        assert rc == 0 and (a, b) == M.line_counts(h, w, dx, dy), (name, dx, dy)
        total, longest = total + a, max(longest, b)
    stats = SC.expected(name)[5]
    assert (total, longest) == (stats["lines"], stats["longest_line"])


def test_line_count_on_random_arguments_and_its_refusals():
    rng = np.random.default_rng(5)
    for _ in range(300):
        w, h = (int(v) for v in rng.integers(1, 60, 2))
        dx, dy = (int(v) for v in rng.integers(-1024, 1025, 2)) if rng.integers(2) else VECTORS[rng.integers(len(VECTORS))]
        if dx == 0 and dy == 0:
            continue
        assert line_count(w, h, dx, dy) == (0, *M.line_counts(h, w, dx, dy)), (w, h, dx, dy)
    # the largest arguments: off(32767) = floor((2 * 32767 * 1023 + 1024) / 2048) = 32735; floor((1024 - 2 * 32767) / 2048) = -32
    assert line_count(32768, 128, 1024, 1023) == (0, *M.line_counts(128, 32768, 1024, 1023)) and line_count(32768, 128, 1024, 1023)[1] == 128 + 32735
    assert line_count(128, 32768, -1, 1024) == (0, 128 + 32, 32768) == (0, *M.line_counts(32768, 128, -1, 1024))
    assert line_count(0, 5, 1, 0) == (0, 0, 0) and line_count(5, 0, 1, 0) == (0, 0, 0)
    for bad in ((5, 5, 0, 0), (5, 5, 1025, 0), (5, 5, 0, -1025), (32769, 1, 1, 0), (1, 32769, 1, 0)):
        assert line_count(*bad) == (-1, 0, 0), bad
    assert _ffi.lib().bt_skyline_line_count(5, 4, 1, 1, None, None) == 0


def test_sun_directions_against_closed_forms():
    rows = bt.TileAtlas.sun_directions([0, 45, 90, 180, 270], 45, cell_size=1.0, raw_unit=1.0)
    assert rows[:, :2].tolist() == [[64, 0], [45, 45], [0, 64], [-64, 0], [0, -64]]
    # tan 45 = 1 per cell; a diagonal step is sqrt(2) cells long
    assert rows[:, 2].tolist() == [4096, math.floor(4096 * math.sqrt(2)), 4096, 4096, 4096] and (rows[:, 3] == 4096).all()
    rows = bt.TileAtlas.sun_directions(0, [0, 90, math.degrees(math.atan(0.5))], cell_size=30.0, raw_unit=0.25, resolution=1024)
    assert rows.tolist() == [[1024, 0, 0, 4096], [1024, 0, (1 << 31) - 1, 4096], [1024, 0, 4096 * 60, 4096]]  # 0.5 * 30 / 0.25 = 60 raw units a cell
    rows = bt.TileAtlas.sun_directions(30, 10, cell_size=2.0, raw_unit=0.5, resolution=64)
    dx, dy, num, den = rows[0].tolist()
    assert (dx, dy, den) == (55, 32, 4096)
    exact = math.tan(math.radians(10)) * 2.0 * math.hypot(55, 32) / 55 / 0.5
    assert num <= exact * 4096 * (1 + 1e-9) < num + 1 + 1e-3  # the floor
    for bad in (dict(elevation_deg=-1), dict(elevation_deg=91), dict(cell_size=0.0), dict(resolution=0), dict(resolution=1025)):
        with pytest.raises(ValueError):
            bt.TileAtlas.sun_directions(**dict(dict(azimuth_deg=0, elevation_deg=10, cell_size=1.0, raw_unit=1.0), **bad))


@pytest.mark.parametrize("name", sorted(SC.SCENES))
def test_every_scene_reaches_what_it_is_named_for(name):
    reaches = SC.scene_reaches(name)
    missing = [r for r in SC.SCENES[name]["reach"] if not reaches.get(r)]
    assert not missing, (name, missing)


def test_the_scene_sets():
    names = set(SC.SCENES)
    assert {"one_cell", "one_row", "one_column", "two_by_two", "sixteen_ways", "plateau", "ramp", "collinear_by_hand", "dome", "bowl", "dome_then_spike", "extremes",
            "holes", "missing_tiles", "grazing", "suns_64", "one_direction"} <= names and set(SC.SIZES) <= names
    shapes = {SC.SCENES[n]["rect"][2:] for n in SC.SIZES}
    assert {s for shape in shapes for s in shape} >= {SC.WAVE - 1, SC.WAVE, SC.WAVE + 1, 96}
    assert all(SC.SCENES[n]["rect"][2:] in ((272, 3), (3, 272)) for n in ("dome", "dome_tall", "bowl", "bowl_tall", "dome_then_spike", "dome_then_spike_tall"))
    # no scene's cell count reaches a second batch: the launch formula at 2^22 cells is the plan's own
    assert all(M.launches(*SC.SCENES[n]["rect"][:1:-1], len(SC.SCENES[n]["directions"])) == 4 for n in names)
    assert M.launches(2048, 2048, 64) == 2 + 2 * 4 and M.launches(2048, 2048, 16) == 4 and M.launches(2048, 2048, 17, bake=True) == 7 and M.launches(4096, 512, 33) == 6


def test_the_mirror_has_the_headers_constants():
    header = (ROOT / "include" / "bevy_terrain_amd.h").read_text()

    def define(name):
        return int(re.search(rf"^#define {name} (\w+)$", header, flags=re.M).group(1).rstrip("u"), 0)

    assert define("BT_SKYLINE_MAX_DIRECTIONS") == _ffi.SKYLINE_MAX_DIRECTIONS == M.MAX_DIRECTIONS and define("BT_SKYLINE_MAX_COMPONENT") == _ffi.SKYLINE_MAX_COMPONENT
    assert define("BT_SKYLINE_MAX_SIDE") == _ffi.SKYLINE_MAX_SIDE
    assert "#define BT_SKYLINE_MAX_CELLS (1u << 22)" in header and _ffi.SKYLINE_MAX_CELLS == 1 << 22
    assert "#define BT_SKYLINE_STACK_BUDGET (256ull << 20)" in header and _ffi.SKYLINE_STACK_BUDGET == M.STACK_BUDGET == 256 << 20
    assert "enum { BT_SKYLINE_BAKE_SHADE = 1 };" in header and _ffi.SKYLINE_BAKE_SHADE == 1
    for struct, ctype in (("bt_skyline_direction", _ffi.SkylineDirectionC), ("bt_skyline_bake", _ffi.SkylineBakeC), ("bt_skyline_stats", _ffi.SkylineStatsC)):
        stated = int(re.search(rf"\}} {struct}; /\* (\d+) bytes \*/", header).group(1))
        assert stated == C.sizeof(ctype) and stated % 8 == 0, struct

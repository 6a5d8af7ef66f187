"""The scenes of bt_atlas_skyline shared by tests/test_skyline_model.py (no GPU: every scene reaches what it is named for, on the model
alone) and tests/test_gpu_skyline.py (the device against the model).

TEST INFRASTRUCTURE ONLY.  The atlases are those of tests/_splat_cases.py (attachment 1 = H, the R16 heights, with its planted no-data
texels).  A scene is a window of H, a list of directions (dx, dy, sun_num, sun_den) and optionally a `plant`: a function from the
window's texels as the jobs left them to the texels the scene wants, which the GPU test writes over the whole window with write_region
before the call (so planted scenes share one atlas per spec, kept apart from the one the unplanted scenes read).  Without a GPU the
window's texels come from the CPU oracle's state of the same jobs through the model of bt_atlas_read_region.  No window exceeds 96 x 96,
but for the strips of 272 x 3 and 3 x 272.

The stack shapes are named for the terrain.  Over a dome (concave) the nearest cell ahead is always the steepest, so nothing ever pops
and the stack grows to the length of the line; over a bowl (convex, z = x^2 scaled) the farthest is, so every arrival pops."""
import functools

import numpy as np

import _paint_model as PM
import _skyline_model as M
import _splat_cases as SC

WAVE = 64  # lines of one wave of the walk


def Scene(spec, rect, directions, plant=None, side=0, lod=None, reach=()):
    """rect (x0, y0, w, h) in mosaic texels; plant: raw (h, w) uint16 -> texels (h, w) uint16 (finest LOD only); reach: names of
    scene_reaches() that must hold"""
    w, h = rect[2:]
    assert (w <= 96 and h <= 96) or (max(w, h) <= 272 and min(w, h) <= 3)
    assert plant is None or lod is None
    assert 1 <= len(directions) <= M.MAX_DIRECTIONS
    return dict(spec=spec, rect=rect, directions=[M.direction(d) for d in directions], plant=plant, side=side, lod=lod, reach=set(reach))


# ---------------------------------------------------------------------------------------------- directions

AXES = [(1, 0), (-1, 0), (0, 1), (0, -1)]
DIAGONALS = [(1, 1), (-1, 1), (1, -1), (-1, -1)]
OBLIQUES = [(3, 1), (2, 5), (-5, 7), (-4, 1), (-3, -2), (-1, -6), (2, -7), (7, -3)]  # one in each octant
STEEPEST = [(1024, 1023)]


def with_suns(vectors, step=23, den=1):
    """sun k rises step * k / den per step of the major axis"""
    return [(dx, dy, step * k, den) for k, (dx, dy) in enumerate(vectors)]


WAYS = with_suns(AXES + DIAGONALS + OBLIQUES + STEEPEST)
A_FEW = with_suns([(1, 0), (0, -1), (3, -2), (-1, -1)], step=40)
ROUND_64 = [(int(np.floor(64 * np.cos(a) + 0.5)), int(np.floor(64 * np.sin(a) + 0.5)), 5 * k, 1) for k, a in enumerate(np.arange(64) * 2 * np.pi / 64)]

# ---------------------------------------------------------------------------------------------- plants


def random_hills(raw):
    """heights in [1000, 1400), independent from cell to cell"""
    return np.random.default_rng(31).integers(1000, 1400, raw.shape).astype(np.uint16)


def heavy_ties(raw):
    """four heights only: equal rationals on most lines"""
    return (1000 + 100 * np.random.default_rng(32).integers(0, 4, raw.shape)).astype(np.uint16)


def level(raw):
    return np.full(raw.shape, 30000, np.uint16)


def ramp(raw):
    """a plane: collinear along every axis and diagonal"""
    ys, xs = np.mgrid[0:raw.shape[0], 0:raw.shape[1]]
    return (1000 + 10 * xs + 3 * ys).astype(np.uint16)


BY_HAND_ROW = 1  # the row of collinear_by_hand that holds 10, 20, 30 from x = 0


def by_hand(raw):
    z = np.full(raw.shape, 5, np.uint16)
    z[BY_HAND_ROW, :3] = (10, 20, 30)  # from (0, row) towards +x: 10 / 1 and 20 / 2 tie; the nearest is the answer
    return z


RIDGE_AT, RIDGE_ROW, RIDGE_UP = 3, 5, 7  # the ridge of grazing: RIDGE_AT cells right of the cell (2, RIDGE_ROW), RIDGE_UP above the plateau


def level_with_ridge(raw):
    z = level(raw)
    z[RIDGE_ROW, 2 + RIDGE_AT] += RIDGE_UP
    return z


def along(raw):
    """the coordinate along the strip's long axis, as a plane"""
    h, w = raw.shape
    return np.arange(w)[None, :].repeat(h, 0) if w >= h else np.arange(h)[:, None].repeat(w, 1)


def dome(raw):
    return (40000 - along(raw) ** 2 // 4).astype(np.uint16)  # gentle enough for the spike below to see past all of it


def bowl(raw):
    a = along(raw)
    return (a * (a + 1) // 2 + 1).astype(np.uint16)  # strictly convex: x^2 / 2 rounded so that no three cells are collinear


def dome_then_spike(raw):
    """the dome, and at the long axis' origin of the middle line a spike: walking towards the origin, that lane pops its whole stack there"""
    z = dome(raw)
    if raw.shape[1] >= raw.shape[0]:
        z[1, 0] = 65535
    else:
        z[0, 1] = 65535
    return z


def stripes(raw):
    """columns of 0 and 65535 by turns, three wide, and two rows of the other value"""
    z = np.where((np.arange(raw.shape[1]) // 3) % 2 == 0, 0, 65535)[None, :].repeat(raw.shape[0], 0)
    z[7] = 65535 - z[7]
    z[20] = 65535 - z[20]
    return z.astype(np.uint16)


# ---------------------------------------------------------------------------------------------- the scenes

HILLS = ("planar_72", (70, 71, 90, 75))  # across the tile edges at 136 on both axes; 75 and 90 lines and more, no multiple of 64
SMALL = ("planar_72", (70, 71, 12, 9))
STRIP_WIDE, STRIP_TALL = ("planar_72", (0, 100, 272, 3)), ("planar_72", (100, 0, 3, 272))
GRAZING_SUNS = [(1, 0, RIDGE_UP, RIDGE_AT), (1, 0, RIDGE_UP - 1, RIDGE_AT), (1, 0, 2 * RIDGE_UP, 2 * RIDGE_AT), (1, 0, 2 * RIDGE_UP - 1, 2 * RIDGE_AT)]
SCENES = {
    "one_cell": Scene("planar_b2", (13, 15, 1, 1), A_FEW, reach={"nothing_ahead"}),
    "one_row": Scene("planar_b2", (5, 27, 9, 1), WAYS),
    "one_column": Scene("planar_b2", (27, 25, 1, 9), WAYS),
    "two_by_two": Scene("planar_b2", (30, 30, 2, 2), WAYS),
    "sixteen_ways": Scene(*HILLS, WAYS, plant=random_hills, reach={"every_octant", "length_one_lines", "lines_past_a_wave", "lines_wrap_a_lane"}),
    "sixteen_ways_tied": Scene(*HILLS, WAYS, plant=heavy_ties, reach={"ties_1000"}),
    "scaled_and_reversed": Scene(*HILLS, [(1, 2), (2, 4), (-1, -2), (3, 1), (300, 100), (-3, -1), (5, -5), (-1, 1)], plant=heavy_ties, reach={"scaled_equal", "reversed"}),
    "plateau": Scene(*HILLS, WAYS, plant=level, reach={"steps_all_one"}),
    "ramp": Scene(*HILLS, with_suns(AXES + DIAGONALS, step=3), plant=ramp, reach={"ramp"}),
    "collinear_by_hand": Scene(*SMALL, [(1, 0, 10, 1), (1, 0, 9, 1)], plant=by_hand, reach={"tie_by_hand"}),
    "dome": Scene(*STRIP_WIDE, [(1, 0, 0, 1), (-1, 0, 100, 1)], plant=dome, reach={"never_pops", "depth_256"}),
    "dome_tall": Scene(*STRIP_TALL, [(0, 1, 0, 1), (0, -1, 100, 1)], plant=dome, reach={"never_pops", "depth_256"}),
    "bowl": Scene(*STRIP_WIDE, [(1, 0, 300, 1), (-1, 0, 0, 1)], plant=bowl, reach={"every_step_pops"}),
    "bowl_tall": Scene(*STRIP_TALL, [(0, 1, 300, 1), (0, -1, 0, 1)], plant=bowl, reach={"every_step_pops"}),
    "dome_then_spike": Scene(*STRIP_WIDE, [(1, 0, 0, 1), (136, 1, 0, 1)], plant=dome_then_spike, reach={"one_lane_pops_256"}),
    "dome_then_spike_tall": Scene(*STRIP_TALL, [(0, 1, 0, 1), (1, 136, 0, 1)], plant=dome_then_spike, reach={"one_lane_pops_256"}),
    "strip_oblique": Scene(*STRIP_WIDE, with_suns(OBLIQUES + STEEPEST + DIAGONALS), plant=random_hills, reach={"length_one_lines", "lines_past_a_wave"}),
    "extremes": Scene(*HILLS, WAYS, plant=stripes, reach={"extremes"}),
    # void and missing ground: the planted HOLES lie at x 14..17, y 5..8; (3, 20); x 21, y 12..17
    "holes": Scene("planar_b2", (0, 0, 48, 40), WAYS, reach={"voids"}),
    "missing_tiles": Scene("partial", (0, 0, 48, 48), WAYS, reach={"voids", "tiles_missing"}),
    # suns
    "grazing": Scene(*HILLS, GRAZING_SUNS, plant=level_with_ridge, reach={"grazing"}),
    "suns_64": Scene(*HILLS, ROUND_64, plant=random_hills, reach={"every_mask_bit", "every_octant"}),
    "one_direction": Scene(*HILLS, [(-5, 7, 150, 1)], plant=random_hills, reach={"lit_and_shadow"}),
    # other layers: a cube face's window at the face's edge (the mosaic is 48 across), a coarser LOD, an atlas without LOD 0
    "cube_side": Scene("cube_3", (8, 3, 40, 37), A_FEW, side=4),
    "lod_below_the_top": Scene("planar_72", (5, 6, 60, 50), A_FEW, lod=1),
    "no_lod0": Scene("no_lod0", (0, 0, 48, 40), A_FEW),
}
SIZES = []  # 63, 64, 65 and 96 lines and lanes on each axis
for _w, _h in [(s, 66) for s in (63, 64, 65, 96)] + [(67, s) for s in (63, 64, 65, 96)] + [(96, 96)]:
    SCENES[f"w{_w}_h{_h}"] = Scene("planar_72", (3, 5, _w, _h), with_suns([(1, 0), (0, 1), (-3, 1), (1, -3), (1, 1)], step=2))
    SIZES.append(f"w{_w}_h{_h}")
PLANTED = [n for n, s in SCENES.items() if s["plant"] is not None]


def geometry(scene):
    spec = SC.SPECS[scene["spec"]]
    lod = spec["lods"] - 1 if scene["lod"] is None else scene["lod"]
    return spec, lod


@functools.lru_cache(maxsize=None)
def window(name):
    """the scene's raw texels (h, w) uint16 and the number of tiles of the window the atlas does not hold, without a GPU"""
    scene = SCENES[name]
    spec, lod = geometry(scene)
    tiles = SC.oracle_state(scene["spec"])[0]
    x0, y0, w, h = scene["rect"]
    raw, missing = PM.read_region(tiles, lod, scene["side"], x0, y0, w, h, spec["b"])
    if scene["plant"] is not None:
        raw = scene["plant"](raw)
        assert raw.shape == (h, w) and raw.dtype == np.uint16
    return raw, missing


@functools.lru_cache(maxsize=None)
def expected(name):
    """(raw, steps, rise, mask, count, stats) of the model: computed once, shared, not to be written to"""
    scene = SCENES[name]
    raw, missing = window(name)
    steps, rise, mask, count, stats = M.skyline(raw, scene["directions"])
    stats["tiles_missing"] = missing
    for plane in (raw, steps, rise, mask, count):
        plane.setflags(write=False)
    return raw, steps, rise, mask, count, stats


def octant(dx, dy):
    """0..7 for a vector off the axes and diagonals, None on them"""
    if dx == 0 or dy == 0 or abs(dx) == abs(dy):
        return None
    return (dx > 0) * 4 + (dy > 0) * 2 + (abs(dx) > abs(dy))


def line_brute(zs):
    """(steps, rise) along one line given in the order of the direction: the definition on a sequence"""
    out = []
    for a in range(len(zs)):
        best = (0, 0)
        for b in range(a + 1, len(zs)):
            t, r = b - a, zs[b] - zs[a]
            if best[0] == 0 or r * best[0] > best[1] * t:
                best = (t, r)
        out.append(best)
    return out


def scene_reaches(name):
    """what a scene's planes reach, by name"""
    scene = SCENES[name]
    raw, steps, rise, mask, count, stats = expected(name)
    h, w = raw.shape
    dirs = scene["directions"]
    z = raw.astype(np.int64)
    out = {"tiles_missing": stats["tiles_missing"] > 0, "voids": 0 < stats["voids"] < stats["cells"]}
    out["nothing_ahead"] = not steps.any() and not rise.any() and bool((count == len(dirs)).all())
    out["every_octant"] = {octant(dx, dy) for dx, dy, _, _ in dirs} >= set(range(8)) and {(np.sign(dx), np.sign(dy)) for dx, dy, _, _ in dirs if octant(dx, dy) is None} >= \
        {(1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1)}
    counts = [np.unique(M.line_index(h, w, dx, dy)[0], return_counts=True)[1] for dx, dy, _, _ in dirs]
    out["length_one_lines"] = any(int((c == 1).sum()) >= 2 for c in counts)
    out["lines_past_a_wave"] = any(len(c) > WAVE and len(c) % WAVE for c in counts)
    # more lines than the minor axis is long: a lane of the walk takes a second line after its first
    out["lines_wrap_a_lane"] = any(len(c) > (h if abs(dx) >= abs(dy) else w) for c, (dx, dy, _, _) in zip(counts, dirs))
    if "ties_1000" in scene["reach"]:
        out["ties_1000"] = sum(int((M.hull(raw, dx, dy, strict=False)[0] != steps[k]).sum()) for k, (dx, dy, _, _) in enumerate(dirs[:4])) >= 1000
    if name == "scaled_and_reversed":
        out["scaled_equal"] = all(np.array_equal(steps[a], steps[b]) and np.array_equal(rise[a], rise[b]) for a, b in ((0, 1), (3, 4))) and not np.array_equal(steps[0], steps[3])
        ok = True
        for fwd, back in ((0, 2), (3, 5), (6, 7)):
            lines_f, _ = M.lines_of(h, w, *dirs[fwd][:2])
            lines_b, _ = M.lines_of(h, w, *dirs[back][:2])
            ok &= [l[::-1] for l in lines_f] == lines_b
            for cells in lines_f:  # walking order is against the direction: as given it is the order of the reversed direction
                for (x, y), (t, r) in zip(cells, line_brute([int(z[y, x]) for x, y in cells])):
                    ok &= int(steps[back][y, x]) == t and int(rise[back][y, x]) == r
        out["reversed"] = bool(ok) and not np.array_equal(steps[0], steps[2])
    if name in ("plateau", "ramp"):
        ahead = np.stack([M.horizon(np.arange(h * w, dtype=np.uint16).reshape(h, w), dx, dy)[0] > 0 for dx, dy, _, _ in dirs])  # any plane: is a cell ahead
        out["steps_all_one"] = bool((steps[ahead] == 1).all()) and not steps[~ahead].any() and not rise.any() and stats["lit"] == stats["cells"] * len(dirs)
    if name == "ramp":
        out["ramp"] = bool((steps[ahead] == 1).all()) and all(len(np.unique(rise[k][ahead[k]])) == 1 for k in range(len(dirs))) and \
            {int(rise[k][ahead[k]][0]) for k in range(len(dirs))} == {10, -10, 3, -3, 13, -7, 7, -13}
    if name == "collinear_by_hand":
        loose = M.hull(raw, 1, 0, strict=False)
        out["tie_by_hand"] = (int(steps[0][BY_HAND_ROW, 0]), int(rise[0][BY_HAND_ROW, 0])) == (1, 10) and (int(loose[0][BY_HAND_ROW, 0]), int(loose[1][BY_HAND_ROW, 0])) == (2, 20) \
            and int(mask[BY_HAND_ROW, 0]) == 0b01 and int(mask[BY_HAND_ROW, 2]) == 0b11
    if scene["reach"] & {"never_pops", "depth_256", "every_step_pops", "one_lane_pops_256"}:
        popped = [M.pops(raw, dx, dy) for dx, dy, _, _ in dirs]
        depth = [M.hull(raw, dx, dy)[2] for dx, dy, _, _ in dirs]
        out["never_pops"] = not any(p.any() for p in popped)
        out["depth_256"] = min(depth) >= 256 and min(depth) == max(h, w)
        long_axis = 1 if w >= h else 0
        out["every_step_pops"] = all(int((p == 1).sum()) == (max(h, w) - 2) * min(h, w) and int(p.sum()) == int((p == 1).sum()) for p in popped)
        spike = (1, 0) if long_axis else (0, 1)
        out["one_lane_pops_256"] = int(popped[0][spike]) >= 256 and int(popped[0].sum()) == int(popped[0][spike]) and max(depth) >= 256
    both = bool((raw == 0).any()) and bool((raw == 65535).any()) and not ((raw != 0) & (raw != 65535)).any()
    out["extremes"] = both and int(rise.max()) == 65535 and int(rise.min()) == -65535 and int((steps > 1).sum()) > 100
    if name == "grazing":
        at = (RIDGE_ROW, 2)
        out["grazing"] = (int(steps[0][at]), int(rise[0][at])) == (RIDGE_AT, RIDGE_UP) and int(mask[at]) == 0b0101 and int(count[at]) == 2 and \
            int(mask[RIDGE_ROW, 2 + RIDGE_AT]) == 0b1111
    out["every_mask_bit"] = len(dirs) == 64 and all(0 < int(((mask >> np.uint64(k)) & np.uint64(1)).sum()) < h * w for k in range(64)) and int(count.max()) > 32
    out["lit_and_shadow"] = len(dirs) == 1 and set(np.unique(count)) == {0, 1} and set(np.unique(mask)) == {0, 1}
    return out

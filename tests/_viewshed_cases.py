"""The scenes of bt_atlas_viewshed shared by tests/test_viewshed_model.py (no GPU: every scene reaches what it is named for, on the model
alone) and tests/test_gpu_viewshed.py (the device against the model).

TEST INFRASTRUCTURE ONLY.  The atlases are those of tests/_splat_cases.py (attachment 1 = H, the R16 heights, with its planted no-data
texels).  A scene is a window of H, a list of observers (x, y, eye_height, radius), a target height and optionally a `plant`: a function
from the window's texels as the jobs left them to the texels the scene wants, which the GPU test writes over the whole window with
write_region before the call (so planted scenes share one atlas per spec, kept apart from the one the unplanted scenes read).  Without a
GPU the window's texels come from the CPU oracle's state of the same jobs through the model of bt_atlas_read_region.  No window exceeds
96 x 96, but for the strips of 272 x 3 and 3 x 272."""
import functools

import numpy as np

import _paint_model as PM
import _splat_cases as SC
import _viewshed_model as M

WAVE = 64  # targets of one wave along the minor axis of a line


def Scene(spec, rect, observers, target_height=0, plant=None, side=0, lod=None, reach=()):
    """rect (x0, y0, w, h) in mosaic texels; plant: raw (h, w) uint16 -> texels (h, w) uint16 (finest LOD only); reach: names of
    scene_reaches() that must hold"""
    w, h = rect[2:]
    assert (w <= 96 and h <= 96) or (max(w, h) <= 272 and min(w, h) <= 4)
    assert plant is None or lod is None
    return dict(spec=spec, rect=rect, observers=[M.observer(o) for o in observers], target_height=target_height, plant=plant, side=side, lod=lod, reach=set(reach))


# ---------------------------------------------------------------------------------------------- plants

def random_hills(raw):
    """heights in [1000, 1400), independent from cell to cell; this seed puts 1384 under the observer of eight_octants at (24, 20), high
    enough to see some cells in every octant"""
    return np.random.default_rng(29).integers(1000, 1400, raw.shape).astype(np.uint16)


def level(raw):
    return np.full(raw.shape, 30000, np.uint16)


RIDGE_AT, RIDGE_ROW = 3, 5  # the ridge cell of plateau_ridge: RIDGE_AT cells right of the observer at (2, RIDGE_ROW)


def level_with_ridge(raw):
    z = level(raw)
    z[RIDGE_ROW, 2 + RIDGE_AT] += 1
    return z


def stripes(raw):
    """columns of 1 and 65535 by turns, three wide, and two rows of the other value"""
    z = np.where((np.arange(raw.shape[1]) // 3) % 2 == 0, 1, 65535)[None, :].repeat(raw.shape[0], 0)
    z[7] = 65535 - z[7] + 1
    z[20] = 65535 - z[20] + 1
    return z.astype(np.uint16)


# ---------------------------------------------------------------------------------------------- the scenes

HILLS = ("planar_72", (70, 71, 48, 40))
SCENES = {
    "one_cell": Scene("planar_b2", (13, 15, 1, 1), [(0, 0, 5)]),
    "one_row": Scene("planar_b2", (5, 27, 9, 1), [(0, 0, 5), (4, 0, 0)], target_height=3),
    "one_column": Scene("planar_b2", (27, 25, 1, 9), [(0, 8, 5), (0, 4, 0)], target_height=3),
    "two_by_two": Scene("planar_b2", (30, 30, 2, 2), [(1, 1, 2)]),
    "eight_octants": Scene(*HILLS, [(24, 20, 30)], target_height=30, plant=random_hills, reach={"eight_octants"}),
    "plateau": Scene(*HILLS, [(24, 20, 0), (0, 0, 0)], plant=level, reach={"all_seen", "grazings_5000"}),
    "plateau_ridge": Scene(*HILLS, [(2, RIDGE_ROW, 0)], plant=level_with_ridge, reach={"ridge_by_hand", "grazings_5000"}),
    "tower": Scene(*HILLS, [(24, 20, 3000)], plant=random_hills, reach={"tower"}),
    "extremes": Scene(*HILLS, [(1, 1, 65535), (46, 38, 65535), (4, 1, 65535)], target_height=65535, plant=stripes, reach={"extremes"}),
    "extremes_from_below": Scene(*HILLS, [(1, 1, 0)], target_height=65535, plant=stripes, reach={"clearance_past_2_20"}),
    # void and missing ground: the planted HOLES lie at x 14..17, y 5..8; (3, 20); x 21, y 12..17
    "holes": Scene("planar_b2", (0, 0, 48, 40), [(10, 7, 12), (30, 30, 40)], target_height=20, reach={"void_targets", "void_on_lines"}),
    "missing_tiles": Scene("partial", (0, 0, 48, 48), [(30, 30, 25), (47, 20, 3)], target_height=10, reach={"tiles_missing", "void_on_lines"}),
    "skipped_observers": Scene("partial", (0, 0, 48, 48), [(21, 14, 9), (30, 30, 25), (2, 2, 9)], target_height=10, reach={"skips_hole_and_missing_tile"}),
    "all_skipped": Scene("partial", (0, 0, 48, 48), [(21, 14, 9), (2, 2, 9)], reach={"nothing_used"}),
    # radii
    "radii_1_and_5": Scene("planar_72", (3, 5, 40, 33), [(10, 10, 20, 5), (30, 20, 20, 1)], target_height=10, reach={"disc_5", "disjoint_discs"}),
    "radius_beyond": Scene("planar_72", (3, 5, 40, 33), [(10, 10, 20, 1000), (39, 32, 5, 0xFFFFFFFF)], target_height=10, reach={"all_covered"}),
    # observers
    "observers_64": Scene("planar_72", (3, 5, 40, 33), [(1 + 5 * (i % 8), (4, 8, 12, 14, 20, 24, 28, 32)[i // 8], 5 + i, 0 if i % 3 else 9) for i in range(64)], target_height=4,
                          reach={"every_mask_bit"}),
    "one_cell_twice": Scene("planar_72", (3, 5, 40, 33), [(10, 10, 50), (10, 10, 50)], target_height=10, reach={"counts_of_two"}),
    # other layers: a cube face's window at the face's edge (the mosaic is 48 across), a coarser LOD, an atlas without LOD 0
    "cube_side": Scene("cube_3", (8, 3, 40, 37), [(20, 18, 15), (39, 0, 2)], target_height=5, side=4),
    "lod_below_the_top": Scene("planar_72", (5, 6, 60, 50), [(30, 25, 300)], target_height=100, lod=1),
    "no_lod0": Scene("no_lod0", (0, 0, 48, 40), [(24, 20, 30), (40, 3, 30)], target_height=5),
    # strips across four tiles of 68: the longest lines
    "strip_wide": Scene("planar_72", (0, 100, 272, 3), [(0, 1, 200), (271, 0, 200), (136, 2, 50)], target_height=50, reach={"n_200"}),
    "strip_tall": Scene("planar_72", (100, 0, 3, 272), [(1, 0, 200), (0, 271, 200), (2, 136, 50)], target_height=50, reach={"n_200"}),
}
for _t in (0, 7, 65535):
    SCENES[f"target_{_t}"] = Scene("planar_72", (3, 5, 40, 33), [(10, 10, 20), (35, 30, 0)], target_height=_t)
TARGETS = ["target_0", "target_7", "target_65535"]
SIZES = []  # 63, 64, 65 and 96 on each axis, the observer at a corner, at an edge midpoint and at the centre
for _w, _h in [(s, 66) for s in (63, 64, 65, 96)] + [(67, s) for s in (63, 64, 65, 96)] + [(96, 96)]:
    for _where, _o in (("corner", (0, 0)), ("edge", (_w // 2, _h - 1)), ("centre", (_w // 2, _h // 2))):
        SCENES[f"w{_w}_h{_h}_{_where}"] = Scene("planar_72", (3, 5, _w, _h), [(*_o, 40)], target_height=10)
        SIZES.append(f"w{_w}_h{_h}_{_where}")
# the cases that hold a full run of 64 targets of one n in one line and a run the window's edge cuts
RUNS = ["w96_h66_corner", "w67_h96_corner", "w96_h96_corner", "w96_h96_edge", "w65_h66_corner", "w67_h65_corner"]
for _name in RUNS:
    SCENES[_name]["reach"] |= {"run_of_64", "cut_run"}


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
    """(raw, clearance, count, mask, stats) of the model: computed once, shared, not to be written to"""
    scene = SCENES[name]
    raw, missing = window(name)
    clearance, count, mask, stats = M.viewshed(raw, scene["observers"], scene["target_height"])
    stats["tiles_missing"] = missing
    for plane in (raw, clearance, count, mask):
        plane.setflags(write=False)
    return raw, clearance, count, mask, stats


def runs(w, h, ox, oy):
    """(full, cut): is there a wave of 64 lanes in the window that all walk for the observer at (ox, oy), and one that walks with fewer
    than 64 lanes inside the window; over both classes (x-major: a column and 64 consecutive y; y-major: a row and 64 consecutive x)"""
    dx, dy, n, x_major, _, _ = M.geometry(h, w, ox, oy)
    full = cut = False
    for mine, axis in ((x_major & (n > 1), 0), (~x_major & (n > 1), 1)):  # axis: the one the 64 lanes lie along
        length = mine.shape[axis]
        for c in range(0, length, WAVE):
            lanes = mine[c:c + WAVE] if axis == 0 else mine[:, c:c + WAVE]
            inside = lanes.shape[axis]
            walking = lanes.sum(axis=axis)
            full |= bool((walking == WAVE).any())
            cut |= inside < WAVE and bool((walking > 0).any())
    return full, cut


def scene_reaches(name):
    """what a scene's planes reach, by name"""
    scene = SCENES[name]
    raw, clearance, count, mask, stats = expected(name)
    h, w = raw.shape
    obs, t = scene["observers"], scene["target_height"]
    ox, oy, eye, radius = obs[0]
    z = raw.astype(np.int64)
    dx, dy, n, x_major, _, _ = M.geometry(h, w, ox, oy)
    seen, active = count > 0, raw != 0
    out = {"tiles_missing": stats["tiles_missing"] > 0}
    # the eight open octants and the eight axis and diagonal rays from the first observer
    parts = []
    for sx in (-1, 1):
        for sy in (-1, 1):
            parts += [(np.sign(dx) == sx) & (np.sign(dy) == sy) & (np.abs(dx) > np.abs(dy)), (np.sign(dx) == sx) & (np.sign(dy) == sy) & (np.abs(dx) < np.abs(dy)),
                      (np.sign(dx) == sx) & (np.sign(dy) == sy) & (np.abs(dx) == np.abs(dy))]
        parts += [(np.sign(dx) == sx) & (dy == 0), (np.sign(dy) == sx) & (dx == 0)]
    out["eight_octants"] = len(parts) == 16 and all(bool((p & seen).any()) and bool((p & ~seen & active).any()) for p in parts)
    out["all_seen"] = bool(seen.all()) and not clearance.any()
    out["grazings_5000"] = sum(M.grazings(raw, x, y, e, t) for x, y, e, _ in obs if raw[y, x]) >= 5000
    if name == "plateau_ridge":
        behind = np.arange(RIDGE_AT + 1, w - ox)
        out["ridge_by_hand"] = clearance[oy, ox + behind].tolist() == [-(-int(k) // RIDGE_AT) for k in behind] and not clearance[oy, :ox + RIDGE_AT + 1].any()
    if name == "tower":
        Sb, jb = M.line_maxima(raw, ox, oy, eye)
        walked = jb > 0
        out["tower"] = bool((Sb[walked] < 0).all()) and int((Sb[walked] % jb[walked] != 0).sum()) > 500 and int((clearance[walked] > 0).sum()) > 50
    both = bool((raw == 1).any()) and bool((raw == 65535).any()) and not ((raw != 1) & (raw != 65535)).any()
    out["extremes"] = both and {int(raw[y, x]) for x, y, _, _ in obs} == {1, 65535} and stats["max_clearance"] > 60000 and t == eye == 65535
    out["clearance_past_2_20"] = both and stats["max_clearance"] > 1 << 20 and 0 < stats["visible"] < stats["cells"]
    out["void_targets"] = bool((~active & (n > 0)).any()) and bool((clearance[~active] == M.NONE).all()) and not count[~active].any()
    # a void cell half-way between a used observer and an active target: that line's middle sample is no-data ground, with r = 0
    def behind(x, y, vx, vy):
        return 0 <= 2 * vx - x < w and 0 <= 2 * vy - y < h and bool(active[2 * vy - y, 2 * vx - x])
    out["void_on_lines"] = any(raw[y, x] and behind(x, y, int(vx), int(vy)) for x, y, _, _ in obs for vy, vx in np.argwhere(~active))
    if name == "skipped_observers":  # the first observer on a planted hole of a tile the atlas holds, the third on a tile it does not hold
        spec, lod = geometry(scene)
        tiles = SC.oracle_state(scene["spec"])[0]
        held = [PM.read_region(tiles, lod, scene["side"], scene["rect"][0] + x, scene["rect"][1] + y, 1, 1, spec["b"])[1] == 0 for x, y, _, _ in obs]
        out["skips_hole_and_missing_tile"] = stats["observers_skipped"] == 2 and stats["observers_used"] == 1 and held == [True, True, False] and \
            [int(raw[y, x] != 0) for x, y, _, _ in obs] == [0, 1, 0]
    out["nothing_used"] = stats["observers_used"] == 0 and stats["observers_skipped"] == len(obs) and bool((clearance == M.NONE).all()) and not count.any() \
        and stats["covered"] == 0 and stats["samples"] == 0
    if len(obs) >= 2:
        c0, c1 = (M.covers(h, w, x, y, r) for x, y, _, r in obs[:2])
        out["disc_5"] = radius == 5 and oy + 4 < h and ox + 4 < w and bool(c0[oy + 4, ox + 3]) and not c0[oy + 4, ox + 4] and int(c0.sum()) == 81 and int(c1.sum()) == 5
        out["disjoint_discs"] = not (c0 & c1).any() and bool((clearance[~(c0 | c1)] == M.NONE).all()) and stats["covered"] == int(((c0 | c1) & active).sum())
    out["all_covered"] = stats["covered"] == int(active.sum()) and all(r >= max(w, h) * 2 for _, _, _, r in obs)
    out["every_mask_bit"] = len(obs) == 64 and all(bool((mask >> np.uint64(o) & np.uint64(1)).any()) for o in range(64)) and int(count.max()) > 8
    out["counts_of_two"] = len(obs) == 2 and obs[0] == obs[1] and set(np.unique(count)) == {0, 2} and set(np.unique(mask)) == {0, 3}
    out["n_200"] = int(max(M.geometry(h, w, x, y)[2].max() for x, y, _, _ in obs)) >= 200
    full, cut = zip(*(runs(w, h, x, y) for x, y, _, _ in obs))
    out["run_of_64"], out["cut_run"] = any(full), any(cut)
    return out

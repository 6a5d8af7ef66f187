"""The scenes of bt_atlas_distance_field shared by tests/test_distance_model.py (no GPU: every scene reaches what it is named for, on the
model alone) and tests/test_gpu_distance.py (the device against the model).

TEST INFRASTRUCTURE ONLY.  The atlases are those of tests/_splat_cases.py (attachment 0 = G, Rgba8; attachment 1 = H, the R16 heights with
its planted no-data texels), as the jobs left them: no scene writes.  A scene is a window of one attachment and what makes a cell a seed:
a band of texel values (lo, hi, channel), a host plane (a function of the window's (h, w)), or both, and INVERT.  The geometric scenes take
their seeds from the host plane alone, so their texels do not matter; they still run on a real window.  Without a GPU the window's texels
come from the CPU oracle's state of the same jobs through the model of bt_atlas_read_region.  No window exceeds 96 x 96, but for the strips
of up to 272 x 3 and 3 x 272."""
import functools

import numpy as np

import _distance_model as M
import _paint_model as PM
import _splat_cases as SC
from _splat_cases import G, H
from bevy_terrain_amd import _ffi

BAND = _ffi.DISTANCE_BAND                  # rows of a band of the column phase
THREADS = _ffi.DISTANCE_THREADS            # columns of a workgroup of the column phase; the stride of a row's cells in the row phase
FINISH_CELLS = _ffi.DISTANCE_FINISH_CELLS  # cells of a workgroup of the finish launch


def Scene(rect, host=None, lo=None, hi=None, channel=0, invert=False, spec="planar_72", attachment=H, side=0, lod=None, reach=()):
    """rect (x0, y0, w, h) in mosaic texels; host: (h, w) -> the uint8 seed plane; reach: names of scene_reaches() that must hold"""
    w, h = rect[2:]
    assert (w <= 96 and h <= 96) or (max(w, h) <= 272 and min(w, h) <= 3)
    assert host is not None or lo is not None
    return dict(spec=spec, rect=rect, attachment=attachment, lo=lo, hi=hi, channel=channel, host=host, invert=invert, side=side, lod=lod, reach=set(reach))


# ---------------------------------------------------------------------------------------------- host planes

def points(*cells):
    def make(h, w):
        plane = np.zeros((h, w), np.uint8)
        for x, y in cells:
            plane[y, x] = 1
        return plane
    return make


def random(one_in, seed, only_column=None, only_row=None):
    """a seed with probability 1 / one_in per cell; at least one; values 1..255, since any non-zero byte is a seed"""
    def make(h, w):
        rng = np.random.default_rng(seed)
        plane = (rng.integers(0, one_in, (h, w)) == 0) * rng.integers(1, 256, (h, w))
        if only_column is not None:
            plane[:, np.arange(w) != only_column] = 0
        if only_row is not None:
            plane[np.arange(h) != only_row, :] = 0
        if not plane.any():
            plane[(h - 1) if only_row is None else only_row, (w // 2) if only_column is None else only_column] = 200
        return plane.astype(np.uint8)
    return make


def rows(*ys):
    def make(h, w):
        plane = np.zeros((h, w), np.uint8)
        plane[list(ys)] = 1
        return plane
    return make


def columns(*xs):
    def make(h, w):
        plane = np.zeros((h, w), np.uint8)
        plane[:, list(xs)] = 1
        return plane
    return make


def checkerboard(h, w):
    return ((np.add.outer(np.arange(h), np.arange(w)) % 2) == 0).astype(np.uint8)


def nothing(h, w):
    return np.zeros((h, w), np.uint8)


def everything(h, w):
    return np.full((h, w), 255, np.uint8)


# ---------------------------------------------------------------------------------------------- the scenes

AT = (3, 5)  # where the geometric windows lie in the mosaic of planar_72 (272 across): across tile edges (68)
SCENES = {
    "one_cell_seed": Scene((13, 15, 1, 1), everything),
    "one_cell_empty": Scene((13, 15, 1, 1), nothing, reach={"no_seeds"}),
    "one_row": Scene((5, 27, 9, 1), points((2, 0), (7, 0))),
    "one_column": Scene((27, 25, 1, 9), points((0, 1), (0, 6))),
    "two_by_two": Scene((30, 30, 2, 2), points((1, 0))),
    "no_seeds": Scene((*AT, 40, 33), nothing, reach={"no_seeds"}),
    "all_seeds": Scene((*AT, 40, 33), everything, reach={"all_seeds"}),
    # ties
    "checkerboard": Scene((*AT, 24, 21), checkerboard, reach={"ties"}),
    "mirror_row": Scene((*AT, 20, 13), points((5, 2), (5, 10)), reach={"ties", "tie_line_row_6"}),
    "mirror_column": Scene((*AT, 20, 13), points((2, 5), (12, 5)), reach={"ties", "tie_line_column_7"}),
    "mirror_diagonal": Scene((*AT, 20, 13), points((3, 8), (8, 3)), reach={"ties", "tie_line_diagonal"}),
    "rows_about_a_band": Scene((*AT, 40, 96), rows(1, 95), reach={"ties", "upper_row_wins", "an_empty_band"}),
    "two_columns": Scene((*AT, 25, 30), columns(4, 20), reach={"ties", "smaller_x_wins"}),
    "stop_rule": Scene((*AT, 30, 20), points((10, 13), (13, 10)), reach={"ties", "tie_at_dx2_equal_best"}),
    "one_seed_column": Scene((*AT, 40, 70), random(2, 5, only_column=7), reach={"one_column_of_seeds"}),
    "one_seed_row": Scene((*AT, 70, 40), random(2, 6, only_row=33), reach={"one_row_of_seeds"}),
    # seed sources; the planted no-data texels of H lie at x 14..17, y 5..8; (3, 20); x 21, y 12..17
    "height_band": Scene((70, 71, 48, 40), lo=33000, hi=36000, reach={"some_seeds"}),
    "holes": Scene((0, 0, 48, 40), lo=0, hi=0, spec="planar_b2", reach={"seeds_are_the_zeros"}),
    "missing_tiles": Scene((0, 0, 48, 48), lo=0, hi=0, spec="partial", reach={"seeds_are_the_zeros", "tiles_missing"}),
    "alpha_band": Scene((70, 71, 48, 40), lo=100, hi=140, channel=3, attachment=G, reach={"some_seeds"}),
    "host_alone": Scene((70, 71, 48, 40), random(16, 7), reach={"some_seeds"}),
    "host_or_texels": Scene((70, 71, 48, 40), random(16, 7), lo=40000, hi=65535, reach={"some_seeds", "both_sources"}),
    "green_or_host": Scene((70, 71, 48, 40), random(16, 8), lo=0, hi=60, channel=1, attachment=G, reach={"some_seeds", "both_sources"}),
    # other layers: a cube face's window at the face's edge (the mosaic is 48 across), a coarser LOD, an atlas without LOD 0
    "cube_side": Scene((8, 3, 40, 37), lo=30000, hi=34000, spec="cube_3", side=4, reach={"some_seeds"}),
    "lod_below_the_top": Scene((5, 6, 60, 50), lo=0, hi=22000, lod=1, reach={"some_seeds"}),
    "no_lod0": Scene((0, 0, 48, 40), lo=40000, hi=65535, spec="no_lod0", reach={"some_seeds"}),
}
SOURCES = ["height_band", "holes", "missing_tiles", "alpha_band", "host_alone", "host_or_texels", "green_or_host"]
for _name in list(SOURCES):
    SCENES[_name + "_inverted"] = dict(SCENES[_name], invert=True, reach=SCENES[_name]["reach"] - {"seeds_are_the_zeros"} | {"inverted"})
    SOURCES.append(_name + "_inverted")
# one seed at each corner in turn: the farthest cell of a strip is 271^2 + 2^2 away, the longest outward search
CORNERS = []
for _w, _h in ((96, 96), (272, 3), (3, 272)):
    for _k, (_x, _y) in enumerate(((0, 0), (_w - 1, 0), (0, _h - 1), (_w - 1, _h - 1))):
        SCENES[f"corner_{_w}x{_h}_{_k}"] = Scene((0, 100, _w, _h) if _w > _h else (100, 0, _w, _h), points((_x, _y)), reach={"one_seed", "farthest_is_the_diagonal"})
        CORNERS.append(f"corner_{_w}x{_h}_{_k}")
# sizes around the kernels' units, at three densities
SIZES = []
_shapes = [(s, 66) for s in (63, 64, 65, 96)] + [(67, s) for s in (63, 64, 65, 96)] + [(96, 96)] + [(40, s) for s in (BAND - 1, BAND, BAND + 1, 2 * BAND, 2 * BAND + 1)] + \
    [(s, 3) for s in (THREADS - 1, THREADS, THREADS + 1)] + [(3, s) for s in (THREADS - 1, THREADS, THREADS + 1)] + \
    [(33, 31), (32, 32), (41, 25)]  # FINISH_CELLS - 1, FINISH_CELLS, FINISH_CELLS + 1 cells
assert [w * h for w, h in _shapes[-3:]] == [FINISH_CELLS - 1, FINISH_CELLS, FINISH_CELLS + 1]
for _w, _h in _shapes:
    for _one_in in (256, 16, 2):
        _rect = (*AT, _w, _h) if max(_w, _h) <= 96 else ((0, 100, _w, _h) if _w > _h else (100, 0, _w, _h))
        SCENES[f"w{_w}_h{_h}_1in{_one_in}"] = Scene(_rect, random(_one_in, _w * 1000 + _h + _one_in), reach={"some_seeds"})
        SIZES.append(f"w{_w}_h{_h}_1in{_one_in}")


def geometry(scene):
    spec = SC.SPECS[scene["spec"]]
    lod = spec["lods"] - 1 if scene["lod"] is None else scene["lod"]
    return spec, lod


@functools.lru_cache(maxsize=None)
def window(name):
    """the scene's texels ((h, w) uint16 or (h, w, 4) uint8), the number of tiles of the window the atlas does not hold and the host plane
    (or None), without a GPU"""
    scene = SCENES[name]
    spec, lod = geometry(scene)
    tiles = SC.oracle_state(scene["spec"])[0 if scene["attachment"] == H else 1]
    x0, y0, w, h = scene["rect"]
    texels, missing = PM.read_region(tiles, lod, scene["side"], x0, y0, w, h, spec["b"])
    host = None if scene["host"] is None else scene["host"](h, w)
    assert host is None or (host.shape == (h, w) and host.dtype == np.uint8)
    return texels, missing, host


@functools.lru_cache(maxsize=None)
def expected(name):
    """(texels, seed, dist2, nearest, stats) of the model: computed once, shared, not to be written to"""
    scene = SCENES[name]
    texels, missing, host = window(name)
    seed = M.seed_plane(texels, scene["channel"], scene["lo"], scene["hi"], host, scene["invert"])
    dist2, nearest, stats = M.field(seed)
    stats["tiles_missing"] = missing
    for plane in (texels, seed, dist2, nearest):
        plane.setflags(write=False)
    return texels, seed, dist2, nearest, stats


def scene_reaches(name):
    """what a scene's planes reach, by name"""
    scene = SCENES[name]
    texels, seed, dist2, nearest, stats = expected(name)
    _, _, host = window(name)
    h, w = seed.shape
    ys, xs = np.mgrid[0:h, 0:w]
    ny, nx = nearest // w, nearest % w
    out = {"tiles_missing": stats["tiles_missing"] > 0}
    out["no_seeds"] = stats["seeds"] == 0 and bool((dist2 == M.NONE).all()) and bool((nearest == M.NONE).all()) and stats["max_dist2"] == 0 and stats["sum_dist2"] == 0
    out["all_seeds"] = stats["seeds"] == h * w and not dist2.any() and np.array_equal(nearest, ys * w + xs)
    out["one_seed"] = stats["seeds"] == 1
    out["some_seeds"] = 0 < stats["seeds"] < h * w
    if stats["seeds"]:
        sy, sx = np.nonzero(seed)
        d_all = (xs[..., None] - sx) ** 2 + (ys[..., None] - sy) ** 2 if h * w * len(sy) <= 1 << 22 else None
        if d_all is not None:  # a cell has a tie when two seeds attain its minimum
            out["ties"] = bool(((d_all == dist2[..., None]).sum(axis=2) > 1).any())
        out["farthest_is_the_diagonal"] = stats["seeds"] == 1 and stats["max_dist2"] == (w - 1) ** 2 + (h - 1) ** 2
    if name == "mirror_row":  # every cell of row 6 is as far from (5, 2) as from (5, 10): the upper seed
        out["tie_line_row_6"] = bool((nearest[6] == 2 * w + 5).all()) and bool((nearest[7] == 10 * w + 5).all())
    if name == "mirror_column":
        out["tie_line_column_7"] = bool((nearest[:, 7] == 5 * w + 2).all()) and bool((nearest[:, 8] == 5 * w + 12).all())
    if name == "mirror_diagonal":  # the cells with x == y: the seed of the smaller row, (8, 3)
        out["tie_line_diagonal"] = all(nearest[k, k] == 3 * w + 8 for k in range(min(h, w))) and nearest[12, 0] == 8 * w + 3
    if name == "rows_about_a_band":
        out["upper_row_wins"] = bool((ny[48] == 1).all()) and bool((ny[49] == 95).all()) and bool((nx == xs).all())
        out["an_empty_band"] = not seed[BAND:2 * BAND].any() and bool(seed[:BAND].any()) and bool(seed[2 * BAND:].any())
    if name == "two_columns":
        out["smaller_x_wins"] = bool((nx[:, 12] == 4).all()) and bool((nx[:, 13] == 20).all()) and bool((ny == ys).all())
    if name == "stop_rule":  # cell (10, 10): its own column's seed is 3 below, the seed 3 to the right has the smaller index
        out["tie_at_dx2_equal_best"] = bool(seed[13, 10]) and bool(seed[10, 13]) and dist2[10, 10] == 9 and nearest[10, 10] == 10 * w + 13
    out["one_column_of_seeds"] = stats["seeds"] > 1 and len(set(np.nonzero(seed)[1])) == 1
    out["one_row_of_seeds"] = stats["seeds"] > 1 and len(set(np.nonzero(seed)[0])) == 1
    plain = texels if texels.ndim == 2 else texels[:, :, scene["channel"]]
    out["seeds_are_the_zeros"] = not scene["invert"] and stats["seeds"] > 0 and np.array_equal(seed, plain == 0)
    if scene["lo"] is not None and host is not None:
        from_texels = (scene["lo"] <= plain) & (plain <= scene["hi"])
        out["both_sources"] = bool((from_texels & (host == 0)).any()) and bool((~from_texels & (host != 0)).any()) and bool((from_texels & (host != 0)).any())
    out["inverted"] = scene["invert"] and np.array_equal(seed, ~M.seed_plane(texels, scene["channel"], scene["lo"], scene["hi"], host, False))
    return out

"""The cases of bt_atlas_erode_height shared by tests/test_erode_model.py (no GPU: every case reaches what it is named for, on the model alone)
and tests/test_gpu_erode.py (the device against the model).

TEST INFRASTRUCTURE ONLY.  A case names an atlas kind and a window; its texels are made here (a sinusoid plus noise with planted no-data
texels) and the GPU test writes them over the window with write_region before the call, so the window's state is known without a GPU: the
texels, zeroed where the atlas kind holds no tile.  The atlas kinds (tests/test_gpu_erode.py builds them; heights are attachment 0):
    t16     planar, T = 16, b = 2 (c = 12), lod_count 3: a mosaic of 48, every tile present
    t72_l   planar, T = 72, b = 2 (c = 68), lod_count 3: a mosaic of 272; two jobs fill an L, tile (0, 2, 0, 0) is absent
    cube    T = 16, b = 2, lod_count 2: a mosaic of 24 per face
"""
import functools

import numpy as np

import _erode_model as M
from bevy_terrain_amd import _ffi

BLOCK = _ffi.ERODE_BLOCK  # the workgroup's block of cells: the window sizes below are made from it

KINDS = {
    "t16": dict(T=16, b=2, lods=3, cube=False, absent=()),
    "t72_l": dict(T=72, b=2, lods=3, cube=False, absent=((0, 2, 0, 0),)),
    "cube": dict(T=16, b=2, lods=2, cube=True, absent=()),
}


def terrain(h, w, seed, holes=(), flat=None, plateau=None):
    """(h, w) uint16 in [1, 65535]: a sinusoid plus noise (or the constant `flat`); plateau: a (y, x, hh, ww) rectangle of one height; holes:
    (y, x, hh, ww) rectangles of zeros"""
    if flat is not None:
        raw = np.full((h, w), flat, dtype=np.uint16)
    else:
        y, x = np.mgrid[0:h, 0:w]
        rng = np.random.default_rng(seed)
        z = 0.5 + 0.3 * np.sin(x / 4.0 + 0.3 * seed) * np.cos(y / 5.0) + 0.04 * rng.standard_normal((h, w))
        raw = np.clip(np.round(z * 65535.0), 1, 65535).astype(np.uint16)
    if plateau is not None:
        y0, x0, hh, ww = plateau
        raw[y0:y0 + hh, x0:x0 + ww] = 40000
    for y0, x0, hh, ww in holes:
        raw[y0:y0 + hh, x0:x0 + ww] = 0
    return raw


def round_weight(h, w):
    """a round brush: 255 in the middle, falling to 0 at the window's edge, with a patch where 0 and 255 alternate cell by cell"""
    y, x = np.mgrid[0:h, 0:w]
    r = np.hypot((x - (w - 1) / 2.0) / max(w / 2.0, 1.0), (y - (h - 1) / 2.0) / max(h / 2.0, 1.0))
    wt = np.clip(np.round(255.0 * (1.0 - r) * 1.6), 0, 255).astype(np.uint8)
    ph, pw = min(4, h), min(6, w)
    wt[:ph, :pw] = np.where((x[:ph, :pw] + y[:ph, :pw]) % 2 == 0, 0, 255)
    return wt


def start_plane(h, w, seed, scale):
    """an initial water or sediment plane: finite, >= 0, zero on a third of the cells"""
    rng = np.random.default_rng(seed)
    plane = (rng.random((h, w)) * scale).astype(np.float32)
    plane[rng.random((h, w)) < 0.33] = 0.0
    return plane


def Case(kind, rect, steps, seed=1, side=0, holes=(), flat=None, plateau=None, weight=False, water=None, sediment=None, reach=(), **overrides):
    """rect (x0, y0, w, h) in mosaic texels of the finest LOD; holes and plateau in cells of the window; water / sediment: None (NULL), 0.0 (a plane of zeros
    goes in and the state comes out) or a scale (start_plane); reach: counters of _erode_model that must be >= 1"""
    return dict(kind=kind, rect=rect, side=side, seed=seed, holes=tuple(holes), flat=flat, plateau=plateau, weight=weight, water=water, sediment=sediment, reach=set(reach),
                params=M.params(steps=steps, **overrides))


FULL = {"k_limited", "erodes", "deposits_something", "at_min_tilt", "above_min_tilt", "at_min_depth", "above_min_depth", "d2_clamped", "written"}
B = BLOCK

CASES = {
    # the windows.  The large ones have a plateau (cells at min_tilt) and a min_depth above rain_dt / 2 (cells at min_depth)
    "one_cell": Case("t16", (13, 15, 1, 1), 2, reach={"wall_neighbours", "at_min_tilt", "kept_same_bits"}),
    "one_column": Case("t16", (5, 7, 1, 7), 37, seed=2, reach={"k_limited", "erodes", "written"}),
    "one_row": Case("t16", (5, 7, 7, 1), 37, seed=3, reach={"k_limited", "erodes", "written"}),
    "block_minus_1": Case("t72_l", (100, 90, B - 1, B - 1), 37, seed=4, plateau=(20, 3, 8, 9), min_depth=0.02, reach=FULL),
    "one_block": Case("t72_l", (100, 90, B, B), 2, seed=5, reach={"k_limited", "erodes", "written"}),
    "two_blocks_plus_1": Case("t72_l", (100, 90, 2 * B + 1, 2 * B + 1), 37, seed=6, plateau=(40, 28, 9, 8), min_depth=0.02, weight=True, reach=FULL | {"kept_weight_0"}),
    # tiles (0..1, 0..1) of the L: (0, 0) is absent; no-data texels on the corner of four blocks (cells 31..32 on both axes) and elsewhere
    "missing_tile_hole_at_block_corner": Case("t72_l", (40, 40, 60, 60), 37, seed=7, holes=[(B - 1, B - 1, 2, 2), (50, 40, 1, 1), (35, 44, 6, 1)], plateau=(40, 48, 8, 8), min_depth=0.02,
                                              weight=True, water=0.4, sediment=0.05, reach=FULL | {"kept_wall", "wall_neighbours"}),
    "mosaic_edge": Case("t16", (40, 30, 8, 18), 1, seed=8, reach={"k_limited", "written"}),
    "several_blocks_t16": Case("t16", (5, 7, 40, 33), 2, seed=9, holes=[(10, 12, 3, 3)], water=0.0, sediment=0.0, reach={"k_limited", "erodes", "written", "kept_wall"}),
    "cube_side_3": Case("cube", (3, 2, 20, 21), 2, seed=10, side=3, holes=[(4, 5, 2, 2)], reach={"k_limited", "erodes", "written"}),
    # the state goes out and comes back: five steps, and (test_gpu_erode.py) five more from what came out
    "five_steps_state_out": Case("t16", (5, 7, 40, 33), 5, seed=11, water=0.3, sediment=0.02, reach={"k_limited", "erodes", "deposits_something", "written"}),
    # the issue's prototype cut to 24 x 24 with next to no rain and everything evaporating: subnormal water and fluxes within 8 steps
    "subnormal": Case("t16", (0, 0, 24, 24), 8, seed=33, holes=[(9, 9, 2, 3)], water=0.0, sediment=0.0, rain=1e-30, evaporation=15.0, reach={"subnormal"}),
    # the fixed points
    "flat": Case("t16", (5, 7, 40, 33), 37, flat=30000, water=0.0, sediment=0.0),
    "no_water": Case("t16", (5, 7, 40, 33), 37, seed=13, holes=[(10, 12, 3, 3)], rain=0.0, water=0.0, sediment=0.0),
    "capacity_0": Case("t16", (5, 7, 40, 33), 37, seed=14, capacity=0.0, water=0.0, sediment=0.0, reach={"k_limited"}),
    # a dt and depths that overflow the fluxes (inf, then inf * 0 = NaN under the K limit): heights that are not finite cannot reach the atlas
    "overflow": Case("t16", (5, 7, 20, 13), 3, seed=15, dt=3e37, rain=0.0, water=1e30, sediment=0.0, reach={"kept_not_finite"}),
}
FIXED_POINTS = ["flat", "no_water", "capacity_0"]
WINDOWS = ["one_cell", "one_column", "one_row", "block_minus_1", "one_block", "two_blocks_plus_1", "missing_tile_hole_at_block_corner", "mosaic_edge", "several_blocks_t16",
           "cube_side_3"]


def geometry(case):
    kind = KINDS[case["kind"]]
    return kind, kind["lods"] - 1, kind["T"] - 2 * kind["b"]


def texels(name):
    """what the GPU test writes over the window before the call"""
    case = CASES[name]
    _, _, w, h = case["rect"]
    return terrain(h, w, case["seed"], case["holes"], case["flat"], case["plateau"])


def window(name):
    """(raw, tiles_missing): the window's texels as the call finds them (zeros where the atlas kind holds no tile)"""
    case = CASES[name]
    kind, lod, c = geometry(case)
    x0, y0, w, h = case["rect"]
    raw = texels(name)
    missing = 0
    for side, l, tx, ty in kind["absent"]:
        xa, xb, ya, yb = max(x0, tx * c), min(x0 + w, (tx + 1) * c), max(y0, ty * c), min(y0 + h, (ty + 1) * c)
        if side == case["side"] and l == lod and xa < xb and ya < yb:
            raw[ya - y0:yb - y0, xa - x0:xb - x0] = 0
            missing += 1
    return raw, missing


def inputs(name):
    """(weight, water, sediment) of the call: arrays or None"""
    case = CASES[name]
    _, _, w, h = case["rect"]

    def plane(scale, seed):
        return None if scale is None else np.zeros((h, w), np.float32) if scale == 0.0 else start_plane(h, w, seed, scale)

    return (round_weight(h, w) if case["weight"] else None), plane(case["water"], 100 + case["seed"]), plane(case["sediment"], 200 + case["seed"])


@functools.lru_cache(maxsize=None)
def expected(name):
    """(raw, tiles_missing, new texels, water, sediment, bT, reached) of the model: computed once, shared, not to be written to"""
    raw, missing = window(name)
    weight, water, sediment = inputs(name)
    reached = {}
    new, d, s, bT = M.erode(raw, CASES[name]["params"], weight, water, sediment, reached)
    for plane in (raw, new, d, s, bT):
        plane.setflags(write=False)
    return raw, missing, new, d, s, bT, reached

"""The cases of bt_atlas_scatter_instances shared by tests/test_scatter_model.py (no GPU: every case reaches the branch it is named for, on
the states the CPU oracle makes) and tests/test_gpu_scatter.py (the device against the model).

TEST INFRASTRUCTURE ONLY.  The states are those of tests/_splat_cases.py (SPECS / oracle_state): attachment 1 is H, the R16 heights with
their planted holes, attachment 0 an Rgba8 attachment that, after a weights splat from H, serves as the mask M.

The kernels' constants (bevy_terrain_amd/csrc/bt_scatter.hip), which the shapes below are chosen against: ROWS = 16 rows of a tile per
workgroup, LANES = 64 cells of a row per trip, CHUNK_TILES = 1024 listed tiles per chunk of launches, SCAN_ITEMS = 256 row blocks per trip
of the scan, MAX_HALO = 8 (a wider halo is not staged in LDS)."""
import functools
import math

import numpy as np

import _scatter_model as M
import _splat_cases as SC
from bevy_terrain_amd import ScatterRule as R

INF = math.inf
ROWS, LANES, CHUNK_TILES, SCAN_ITEMS, MAX_HALO = 16, 64, 1024, 256, 8

RULES = {
    # trees on gentle low ground, rocks on steep ground, shrubs high up: all with fades, every rule places somewhere
    "three": [R(height=(-INF, 260.0), height_fade=30.0, slope=(0.0, 30.0), slope_fade=0.05, density=0.35, scale=(0.8, 1.6)),
              R(slope=(20.0, 90.0), slope_fade=0.05, density=0.5, scale=(0.3, 0.9)),
              R(height=(200.0, INF), height_fade=20.0, density=0.1, scale=(0.5, 0.5))],
    # the first rule takes every cell below 250: the second, which passes everywhere, stands behind a sum of 1 there and places only above
    "starved": [R(height=(-INF, 250.0), density=1.0), R(density=0.5, scale=(1.0, 2.0))],
    # hard bands (fade 0) beside the same bands with a fade: both forms of band()
    "hard_and_faded": [R(height=(120.0, 220.0), slope=(0.0, 35.0), density=0.4), R(height=(120.0, 220.0), height_fade=25.0, slope=(0.0, 35.0), slope_fade=0.1, density=0.4)],
    # eight rules: the loop's full length
    "eight": [R(height=(-INF if k == 0 else 60.0 + 40.0 * k, 100.0 + 40.0 * k), height_fade=10.0, density=0.1 + 0.05 * k, scale=(1.0, 1.0 + k)) for k in range(8)],
    # bytes 0 and 3 of the mask M
    "masked": [R(density=0.9, mask_channel=0, scale=(1.0, 2.0)), R(density=0.9, mask_channel="a"), R(slope=(30.0, 90.0), density=0.2)],
    "all_pass_quarter": [R(density=0.25)],
    "nothing": [R(density=0.0), R(density=0.0, height=(100.0, 200.0), height_fade=5.0)],
    "everything": [R(density=1.0)],
}
# (seed, mosaic texel of lod 2) whose selection number f(r_0) is exactly 0: with density 0 the sum stays 0 and `u < A` must not place
ZERO_DRAWS = [(2, (0, 0)), (4329, (22, 44))]
# the splat call that makes attachment 0 the mask of the "masked" rules: _splat_cases.Call on the whole finest level
MASK_SPLAT = SC.Call("weights_alpha_dominant")


def tiles_of(spec_name, lod=None, side=None):
    """the coordinates the state holds, in (side, lod, x, y) order, optionally of one lod / side"""
    h, _ = SC.oracle_state(spec_name)
    return sorted(k for k in h if (lod is None or k[1] == lod) and (side is None or k[0] == side))


def Case(spec, rules, coords, seed=0, jitter=1.0, masked=False, reach=()):
    """coords: a list of coordinates, or a function of the spec name that returns one"""
    return dict(spec=spec, rules=rules, coords=coords, seed=seed, jitter=jitter, masked=masked, reach=set(reach))


ALL_RULES_3 = {"rule_0", "rule_1", "rule_2"}
CASES = {
    # T = 16, b = 2 (c = 12): a row is a fifth of a wave, one partial row block.  Tile (1, 1) holds the column piece of HOLES
    "one_tile": Case("planar_b2", "three", [(0, 2, 1, 1)], seed=1, reach=ALL_RULES_3 | {"centre_hole", "pair_hole"}),
    "finest_level": Case("planar_b2", "three", lambda s: tiles_of(s, lod=2), seed=2, reach=ALL_RULES_3 | {"centre_hole", "pair_hole"}),
    "coarser_lod": Case("planar_b2", "three", lambda s: tiles_of(s, lod=1) + tiles_of(s, lod=0), seed=3, reach=ALL_RULES_3),
    "no_jitter": Case("planar_b2", "three", lambda s: tiles_of(s, lod=2), seed=4, jitter=0.0, reach=ALL_RULES_3),
    "half_jitter": Case("planar_b2", "eight", lambda s: tiles_of(s, lod=2), seed=5, jitter=0.5, reach={f"rule_{k}" for k in range(8)}),
    "starved_by_the_sum": Case("planar_b2", "starved", lambda s: tiles_of(s, lod=2), seed=6, reach={"starved", "rule_0", "rule_1"}),
    "hard_and_faded_bands": Case("planar_b2", "hard_and_faded", lambda s: tiles_of(s, lod=2), seed=7, reach={"rule_0", "rule_1"}),
    "masked": Case("planar_b2", "masked", lambda s: tiles_of(s, lod=2), seed=8, masked=True, reach=ALL_RULES_3 | {"mask_0", "mask_255"}),
    # b = 1 is below the taps' reach: the taps of an edge cell are clamped at the layer's edge, where the kernel's window is cut
    "edge_clamp": Case("planar_b1", "three", lambda s: tiles_of(s, lod=2), seed=9, reach=ALL_RULES_3 | {"clamped"}),
    # T = 72, b = 2 (c = 68): a second lane trip of four cells, five row blocks of which the last has four rows; tile (0, 0) holds HOLES
    "planar_72": Case("planar_72", "three", [(0, 2, 0, 0), (0, 2, 3, 1), (0, 1, 1, 0), (0, 0, 0, 0)], seed=10, reach=ALL_RULES_3 | {"centre_hole", "pair_hole"}),
    # T = 136, b = 3 (c = 130): a third lane trip, nine row blocks
    "planar_136": Case("planar_136", "three", [(0, 2, 0, 0), (0, 2, 2, 3), (0, 1, 1, 1)], seed=11, reach=ALL_RULES_3 | {"centre_hole", "pair_hole"}),
    # the cube: tiles on all six sides, at face edges and corners and inside; the normal's three face_up pairs
    "cube_3": Case("cube_3", "three", lambda s: [(side,) + t for side in range(6) for t in ((2, 0, 0), (2, 3, 1), (2, 1, 2), (1, 1, 1), (0, 0, 0))], seed=12,
                   reach=ALL_RULES_3 | {"centre_hole", "pair_hole"}),
}


def case_arguments(name):
    """(spec name, coords, rules, seed, jitter, masked)"""
    case = CASES[name]
    coords = case["coords"](case["spec"]) if callable(case["coords"]) else list(case["coords"])
    return case["spec"], coords, RULES[case["rules"]], case["seed"], case["jitter"], case["masked"]


@functools.lru_cache(maxsize=None)
def mask_tiles(spec_name):
    """attachment 0 after MASK_SPLAT, by the splat model: the mask M of the masked cases"""
    h, g = SC.oracle_state(spec_name)
    return SC.model_call(h, g, SC.SPECS[spec_name], MASK_SPLAT)


def model_scatter(spec_name, coords, rules, seed=0, jitter=1.0, masked=False, cache=None, reached=None):
    """the model's (instances, first, stats) of one call on the state of spec_name"""
    spec = SC.SPECS[spec_name]
    h, _ = SC.oracle_state(spec_name)
    return M.scatter(SC.models(spec)[1], h, spec["b"], coords, rules, seed, jitter, mask_tiles(spec_name) if masked else None, cache, reached)


@functools.lru_cache(maxsize=None)
def model_case(name):
    """(instances, first, stats, reached) of a case, computed once and shared: treat as read-only"""
    spec_name, coords, rules, seed, jitter, masked = case_arguments(name)
    reached = {}
    instances, first, stats = model_scatter(spec_name, coords, rules, seed, jitter, masked, reached=reached)
    instances.setflags(write=False)
    first.setflags(write=False)
    return instances, first, stats, reached


def window_fallbacks(spec, coord, seed, jitter):
    """how many cells of a tile fail the decide kernel's window test (all their texels are then fetched from HBM): the window of a cell is
    the rows of its block of ROWS and the columns of its trip of LANES plus halo = T / (2c) + 2 texels on every side, cut to the layer"""
    T, b = spec["T"], spec["b"]
    c = T - 2 * b
    halo = T // (2 * c) + 2
    if halo > MAX_HALO:
        return c * c
    cl = M.cells(coord, c, seed, jitter)
    lo_x, hi_x, lo_y, hi_y = [np.clip(v, 0, T - 1) for v in M.tap_extent(T, b, cl["uv"])]
    y_begin = cl["j"] // ROWS * ROWS
    y_end = np.minimum(y_begin + ROWS - 1, c - 1)
    chunk = b + cl["i"] // LANES * LANES
    chunk_last = np.minimum(chunk + LANES - 1, b + c - 1)
    wy0, wy1 = np.where(b + y_begin > halo, b + y_begin - halo, 0), np.minimum(b + y_end + halo, T - 1)
    wx0, wx1 = np.where(chunk > halo, chunk - halo, 0), np.minimum(chunk_last + halo, T - 1)
    inside = (lo_x >= wx0) & (hi_x <= wx1) & (lo_y >= wy0) & (hi_y <= wy1)
    return int((~inside).sum())

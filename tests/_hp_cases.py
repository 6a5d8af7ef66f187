"""The scenes of the high-precision geometry tests, shared by test_hp_model.py (no GPU) and test_gpu_hp_geometry.py.

The shallow scenes are _geometry_cases' (lod_count 4, tree_size 4, T = 32, sphere and ellipsoid, the tree's table with some tiles loaded)
with a precision_threshold_distance and an origin_lod of their own: 10.0 (x the model's scale) makes every vertex of every view hp, on all
six sides; 0.05 with the near view (0.02 scales above the ground) splits tiles, and waves, into hp and other vertices; origin_lod 3 sends
coordinate_change_lod UP (tile LODs 0 .. 2) and nowhere (LOD 3), origin_lod 10 UP.

The deep scene sends it DOWN and is the one the accuracy is measured on: lod_count 16, nothing loaded, min_height 0 (every height is
exactly 0, so `position` is the surface point itself), grid 16, LOD 15 tiles (about 300 m) under and around a view 2 m above the ground, out
to the default threshold (0.001 scales, about 6.4 km) and just beyond it, the reference's default view configuration otherwise.

At the end, for test_gpu_geometry_trips.py: _geometry_cases' long lists with a threshold and an origin_lod (LONG, long_device_scene)."""
import functools
import types

import numpy as np

import _geometry_cases as GC
import _geometry_model as GM
import _hp_model as HM
import _oracle as O
import bevy_terrain_amd as bt

KINDS = ("sphere", "ellipsoid")
ALL, SPLIT = 10.0, 0.05  # precision_threshold_distance: every vertex hp / hp and other vertices in one tile (near view)
DEVICE = 0.4  # the device-form test's: about a quarter of the vertices of the near view's prepass list (none nearer than 0.14 scales) are hp
NEAR, MIDDLE, FAR = 0, 1, 2


def view_config(grid, threshold, origin_lod):
    """_geometry_cases.view_config with the two fields the approximation reads"""
    kw = dict(tree_size=GC.TREE, load_distance=GC.LOAD_DISTANCE, morph_distance=1.0, blend_distance=1.0, grid_size=grid, refinement_count=GC.LODS - 1,
              precision_threshold_distance=threshold, origin_lod=origin_lod)
    return bt.TerrainViewConfig(**kw), O.make_view_config(**kw)


# (kind, grid, threshold, origin_lod, flags, views): compared with the model on the GPU, every admissible vertex bit for bit
COMPARED = [
    ("sphere", 4, ALL, 3, 0, (NEAR, MIDDLE, FAR)),
    ("ellipsoid", 5, ALL, 10, HM.VIEW_RELATIVE, (NEAR, MIDDLE, FAR)),
    ("sphere", 16, SPLIT, 3, GM.GRID, (NEAR,)),
    ("ellipsoid", 32, SPLIT, 3, HM.VIEW_RELATIVE | GM.NO_MORPH, (NEAR,)),
    ("sphere", 5, SPLIT, 10, GM.GRID | GM.NO_BLEND | HM.VIEW_RELATIVE, (NEAR, MIDDLE)),
    ("ellipsoid", 4, ALL, 3, GM.NO_MORPH | GM.NO_BLEND, (MIDDLE,)),
    ("ellipsoid", 16, SPLIT, 3, 0, (NEAR,)),
    ("sphere", 32, ALL, 10, HM.VIEW_RELATIVE, (MIDDLE,)),
]


def view_of(kind, grid, threshold, origin_lod, n):
    """the oracle's bt_view_state of view n of the shallow scene (the library's is asserted equal to it on the GPU side)"""
    return O.view_state_from_config(GC.MODELS[kind][1], view_config(grid, threshold, origin_lod)[1], GC.SPECS[kind]["views"][n], GC.approximate_height(kind))


def approximation_of(kind, grid, threshold, origin_lod, n):
    return HM.approximation(GC.MODELS[kind][0], view_config(grid, threshold, origin_lod)[0], GC.SPECS[kind]["views"][n])


@functools.lru_cache(maxsize=None)
def expected(kind, grid, threshold, origin_lod, flags, n):
    """the model's answer for view n of a shallow scene: (vertices, trace, admissible)"""
    c = GC.scene(kind, grid, True)
    return HM.geometry(view_of(kind, grid, threshold, origin_lod, n), approximation_of(kind, grid, threshold, origin_lod, n), c.P, c.entries, c.layers, GC.T, GC.B, c.tiles, flags)


# ---- the deep scene ----------------------------------------------------------------------------------------------------------------------
DEEP_LODS, DEEP_GRID, DEEP_LOD = 16, 16, 15
DEEP_MODELS = {
    "sphere": (bt.TerrainModel.sphere(GC.CENTRE, GC.R, 0.0, 9000.0), O.make_model("spherical", GC.CENTRE, GC.R, 0.0, 0.0, 9000.0)),
    "ellipsoid": (bt.TerrainModel.ellipsoid((100.0, 200.0, -300.0), 6378137.0, GC.MINOR, 0.0, 9000.0),
                  O.make_model("ellipsoidal", (100.0, 200.0, -300.0), 6378137.0, GC.MINOR, 0.0, 9000.0)),
}
# the point under the view (side, uv of the face) and the LOD 15 tiles, as offsets from the view's tile: under it, next to it, on the way
# out, at the default threshold (20 tiles of ~305 m straight, 14 diagonally) and beyond it
DEEP_UNDER = {"sphere": (3, (0.537, 0.4621)), "ellipsoid": (2, (0.3108, 0.6442))}
DEEP_OFFSETS = [(0, 0), (1, 0), (0, -1), (-1, 1), (7, -5), (-12, 9), (20, 0), (0, -20), (14, 14), (-15, -14), (22, 3)]


def deep_view_config():
    """the reference's defaults (threshold 0.001, origin_lod 10, morph 16, blend 2) on a small tree"""
    kw = dict(tree_size=GC.TREE, grid_size=DEEP_GRID)
    return bt.TerrainViewConfig(**kw), O.make_view_config(**kw)


@functools.lru_cache(maxsize=None)
def deep_scene(kind):
    c = types.SimpleNamespace(kind=kind)
    c.model, c.omodel = DEEP_MODELS[kind]
    c.view_config, c.oview_config = deep_view_config()
    side, uv = DEEP_UNDER[kind]
    c.position = tuple(float(v) for v in HM.tree_model(c.model).world_position(side, np.array(uv, np.float64), 2.0))  # 2 m above the ground
    x, y = (int(v * (1 << DEEP_LOD)) for v in uv)
    c.tiles = np.array([(side, DEEP_LOD, x + dx, y + dy) for dx, dy in DEEP_OFFSETS], np.uint32)
    c.P = GM.params(c.model, c.view_config, DEEP_LODS)
    c.view = O.view_state_from_config(c.omodel, c.oview_config, c.position, 0.0)
    c.approximation = HM.approximation(c.model, c.view_config, c.position)
    c.entries = np.full((6 * DEEP_LODS * GC.TREE * GC.TREE, 2), GM.INVALID, np.uint32)  # a tree that was never updated
    return c


@functools.lru_cache(maxsize=None)
def deep_expected(kind, flags):
    c = deep_scene(kind)
    return HM.geometry(c.view, c.approximation, c.P, c.entries, {}, GC.T, GC.B, c.tiles, flags)


# ---- long lists (test_gpu_geometry_trips.py): _geometry_cases' long lists through the kHighPrecision instantiation --------------------------
# (kind, grid, threshold, origin_lod, flags, view, count, launches)
LONG = [
    ("sphere", 4, SPLIT, 3, 0, NEAR, 2060, (2060,)),                         # later trips, hp and other vertices mixed
    ("ellipsoid", 32, ALL, 10, HM.VIEW_RELATIVE, MIDDLE, 330, (321, 9)),  # the hp form across a chunk boundary
]


def long_expected(kind, grid, threshold, origin_lod, flags, n, count, seed=3):
    """(vertices, admissible) of the long list, (hp per vertex) of the scene's own tiles"""
    e = expected(kind, grid, threshold, origin_lod, flags, n)
    return GC.gather(e, GC.long_index(kind, count, seed)) + (e[1]["hp"],)


# the device form on _geometry_cases.deep_scene's list (more than 1024 tiles of LODs 2 .. 8 in that order, nothing loaded).  Chosen from the
# model's trace: the nearest vertex of the near view's list is 0.026 scales away and the median 0.25; at 0.1 scales a quarter of the vertices
# are hp, 4 in 100 of the first 1024 tiles' and 86 in 100 of the later tiles', which are the workgroups' second trip, and some forty tiles
# of that trip hold both kinds.  The hp vertices belong to tiles of LODs 7 and 8: with origin_lod 7 coordinate_change_lod goes nowhere and DOWN
LONG_DEVICE_THRESHOLD, LONG_DEVICE_ORIGIN = 0.1, 7


def long_device_view_config():
    return GC.deep_view_config(precision_threshold_distance=LONG_DEVICE_THRESHOLD, origin_lod=LONG_DEVICE_ORIGIN)


@functools.lru_cache(maxsize=None)
def long_device_scene(kind):
    """_geometry_cases.deep_scene with the threshold and origin_lod above: its view, approximation and the oracle's prepass list"""
    c = types.SimpleNamespace(**vars(GC.deep_scene(kind)))
    c.view_config, c.oview_config = long_device_view_config()
    c.view = O.view_state_from_config(c.omodel, c.oview_config, c.position, GC.approximate_height(kind))
    c.approximation = HM.approximation(c.model, c.view_config, c.position)
    c.tiles, c.indirect, _ = O.refine(c.view)
    return c


@functools.lru_cache(maxsize=None)
def long_device_expected(kind, flags):
    c = long_device_scene(kind)
    return HM.geometry(c.view, c.approximation, c.P, c.entries, {}, GC.T, GC.B, c.tiles, flags)

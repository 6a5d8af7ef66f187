"""The scenes of the terrain geometry tests, shared by test_geometry_model.py (no GPU) and test_gpu_geometry.py.

A scene is a small terrain (lod_count 4, tree_size 4, T = 32, b = 2, an R16 height attachment and an Rgba8 one preprocessed from 128 x 128
synthetic sources), a tile tree after one frame with the files of chosen tiles missing (region by region the best loaded tile of a node is
its own, an ancestor's, or none: _sample_cases.centre_layout) or with nothing loaded at all, a grid size, a list of tiles of every LOD on
every side, and three explicit views (near, middle, far) that put those tiles at morph ratio 0, between and 1 and at blend ratio 0 and
above.  The tree's table is derived on the CPU from the second models (_second_models.TileTreeModel / StreamModel), the tiles by the CPU
oracle; the GPU test streams the same terrain and asserts that the device's table and layers are these.

scene(kind, grid, loaded) computes once per process: the parameters, the views, the tiles, the entries and the layers.

At the end, for test_gpu_geometry_trips.py: the scenes' tiles as lists longer than one launch's 1024 workgroups and than the host form's
32 MiB launches (long_tiles, LONG), and a 9-LOD tree whose prepass list is longer than 1024 (deep_scene)."""
import functools
import types

import numpy as np

import _cases as K
import _geometry_model as GM
import _oracle as O
import _sample_cases as SC
import _second_models as S
import bevy_terrain_amd as bt

LODS, TREE, T, B = 4, 4, 32, 2
SOURCE = 128  # the synthetic sources are SOURCE x SOURCE
GRIDS = (4, 5, 12, 16, 32)
LOAD_DISTANCE = 20.0  # every node of every window is requested
R, MINOR = 6371000.0, 6356752.314245
CENTRE = (2.0e6, -1.0e6, 3.0e6)  # the sphere is centred away from the origin

MODELS = {
    "planar": (bt.TerrainModel.planar((10.0, -5.0, 3.0), 1000.0, 0.0, 250.0), O.make_model("planar", (10.0, -5.0, 3.0), 1000.0, 0.0, 0.0, 250.0)),
    "sphere": (bt.TerrainModel.sphere(CENTRE, R, -12000.0, 9000.0), O.make_model("spherical", CENTRE, R, 0.0, -12000.0, 9000.0)),
    "ellipsoid": (bt.TerrainModel.ellipsoid((100.0, 200.0, -300.0), 6378137.0, MINOR, -12000.0, 9000.0),
                  O.make_model("ellipsoidal", (100.0, 200.0, -300.0), 6378137.0, MINOR, -12000.0, 9000.0)),
}

_unit = SC.unit
# the tree's view (what the table is built around), the face it looks at, and the explicit views of the geometry: near, middle, far.  The
# middle view stands straight over the centre of its face at 0.23 blend distances: the root tile's centre vertex sits inside the blend ring
# of LOD 2 there, so its second lookup goes UP (to LOD 1 from LOD 0)
SPECS = {
    "planar": dict(side=0, tree_view=(10.0 + 1000.0 * 9 / 1024, 120.0, 3.0 - 1000.0 * 13 / 1024), root_missing=True,
                   views=[(40.0, 150.0, -20.0), (10.0, 235.0, 3.0), (300.0, 2600.0, -250.0)]),
    "sphere": dict(side=3, tree_view=tuple(np.array(CENTRE) + _unit((1.0, 0.012, -0.017)) * (R + 500.0)), root_missing=False,
                   views=[tuple(np.array(CENTRE) + _unit((1.0, 0.05, -0.03)) * (R + 0.02 * R)), tuple(np.array(CENTRE) + np.array((1.0, 0.0, 0.0)) * (R + 0.23 * R)),
                          tuple(np.array(CENTRE) + _unit((0.8, 0.5, 0.3)) * (R + 4.0 * R))]),
    "ellipsoid": dict(side=2, tree_view=tuple(np.array((100.0, 200.0, -300.0)) + _unit((0.015, 1.0, -0.011)) * (MINOR + 500.0)), root_missing=False,
                      views=[tuple(np.array((100.0, 200.0, -300.0)) + _unit((0.04, 1.0, 0.02)) * (MINOR + 0.02 * R)),
                             tuple(np.array((100.0, 200.0, -300.0)) + np.array((0.0, 1.0, 0.0)) * (MINOR + 0.23 * (6378137.0 + MINOR) / 2.0)),
                             tuple(np.array((100.0, 200.0, -300.0)) + _unit((0.4, 0.8, -0.5)) * (MINOR + 4.0 * R))]),
}


def missing(kind):
    """the tiles whose files are missing: centre_layout around the view's face; on a cube one more face without any tile"""
    spec = SPECS[kind]
    out = SC.centre_layout(spec["side"], spec["root_missing"])
    if kind != "planar":
        out |= SC.descendants((spec["side"] + 1) % 6, 0, 0, 0)
    return out


def view_config(grid):
    """morph_distance 1 and blend_distance 1 (x the model's scale): the rings of LODs 0 .. 3 lie inside the terrain"""
    kw = dict(tree_size=TREE, load_distance=LOAD_DISTANCE, morph_distance=1.0, blend_distance=1.0, grid_size=grid, refinement_count=LODS - 1)
    return bt.TerrainViewConfig(**kw), O.make_view_config(**kw)


def rasters(kind):
    faces = 1 if kind == "planar" else 6
    return [K.smooth_raster(SOURCE, SOURCE, seed=3 + s) for s in range(faces)], [K.random_raster(O.FORMAT_RGBA8, SOURCE, SOURCE, seed=60 + s) for s in range(faces)]


def atlas_size(kind):
    return 64 if kind == "planar" else 256


@functools.lru_cache(maxsize=None)
def oracle_tiles(kind):
    """{(side, lod, x, y): the R16 tile} of the whole pyramid, by the CPU oracle"""
    heights, _ = rasters(kind)
    atlas = O.OracleAtlas(LODS, 6 * 100, kind != "planar", [(T, B, 1, O.FORMAT_R16)])
    atlas.clear_attachment(0)
    if kind == "planar":
        atlas.preprocess_tile(0, heights[0], (0, LODS))
    else:
        atlas.preprocess_spherical(0, heights, (0, LODS))
    atlas.run(4)
    return {coord: atlas.tile(0, i) for coord, i in atlas.tiles()}


@functools.lru_cache(maxsize=None)
def table(kind):
    """the state one frame at the tree's view leaves (update -> requests -> loads, the missing ones failing -> adjust_to_tile_atlas), from
    the second models -> (requested tiles in order, {coordinate: atlas index} of the loaded tiles, entries (nodes, 2), node coordinates)"""
    model = MODELS[kind][0]
    tm = S.TileTreeModel(kind, model.translation, model.scale_vec, model.min_height, model.max_height, LODS, TREE, LOAD_DISTANCE)
    tm.project = O.project_point_ellipsoid
    existing = set(oracle_tiles(kind))
    released, requested = tm.update(SPECS[kind]["tree_view"])
    assert released == []
    stream = S.StreamModel(atlas_size(kind), 2, existing=existing)
    for c in requested:
        stream.request_tile(c)
    loaded = dict(stream.finish_loads(stream.pending_loads(), missing=missing(kind)))
    coords, _ = tm.node_tables()
    entries = np.array([stream.get_best_tile(tuple(int(v) for v in c)) if c[1] != GM.INVALID else (GM.INVALID, GM.INVALID) for c in coords], np.uint32)
    return requested, loaded, entries, coords


def approximate_height(kind):
    """TileTree::new's, which a tree that never sampled its height keeps"""
    model = MODELS[kind][0]
    return float((np.float32(model.min_height) + np.float32(model.max_height)) / np.float32(2.0))


def views(kind, grid):
    """the explicit views, as the oracle derives a bt_view_state (the library's bt_view_state_from_config is tested against it)"""
    return [O.view_state_from_config(MODELS[kind][1], view_config(grid)[1], v, approximate_height(kind)) for v in SPECS[kind]["views"]]


def tiles(kind):
    """every tile of LODs 0 .. 2 of the face the views look at, the LOD 3 tiles around its centre, and on a cube the roots, one LOD 1 and
    one LOD 3 tile of every face: (n, 4) uint32"""
    side = SPECS[kind]["side"]
    out = [(side, lod, x, y) for lod in range(3) for x in range(1 << lod) for y in range(1 << lod)]
    out += [(side, 3, x, y) for x in range(2, 6) for y in range(2, 6)]
    if kind != "planar":
        for s in range(6):
            if s != side:
                out += [(s, 0, 0, 0), (s, 1, s & 1, 1), (s, 3, 2 + s, 7 - s)]
    return np.array(out, np.uint32)


@functools.lru_cache(maxsize=None)
def scene(kind, grid, loaded=True):
    """loaded: the table of table(kind) and its layers; not loaded: a tree that was updated and found nothing (every entry invalid)"""
    c = types.SimpleNamespace(kind=kind, grid=grid, loaded=loaded)
    c.model, c.omodel = MODELS[kind]
    c.view_config, c.oview_config = view_config(grid)
    c.P = GM.params(c.model, c.view_config, LODS)
    c.views, c.tiles = views(kind, grid), tiles(kind)
    _, held, entries, coords = table(kind)
    c.coords = coords
    if loaded:
        pyramid = oracle_tiles(kind)
        c.entries, c.layers = entries, {index: pyramid[coord] for coord, index in held.items()}
    else:
        c.entries, c.layers = np.full_like(entries, GM.INVALID), {}
    return c


@functools.lru_cache(maxsize=None)
def expected(kind, grid, loaded, view, flags):
    """the model's answer for one view of a scene: (vertices, trace, admissible)"""
    c = scene(kind, grid, loaded)
    return GM.geometry(c.views[view], c.P, c.entries, c.layers, T, B, c.tiles, flags)


# the scenes the GPU test compares, every one with all three views: (kind, grid, loaded, flags)
COMPARED = ([(kind, 4, True, 0) for kind in MODELS] + [("planar", 5, True, 0), ("sphere", 12, True, 0), ("ellipsoid", 16, True, 0), ("planar", 32, True, 0)]
            + [("sphere", 5, True, GM.GRID), ("planar", 12, True, GM.GRID | GM.NO_MORPH), ("ellipsoid", 4, True, GM.NO_BLEND), ("planar", 16, True, GM.NO_MORPH | GM.NO_BLEND)]
            + [("planar", 4, False, 0), ("sphere", 4, False, GM.GRID)])


# ---- long lists: later trips of the workgroup loop, the host form's chunks, the capacity cut ------------------------------------------------
# (test_gpu_geometry_trips.py; test_geometry_model.py asserts without a GPU that they reach what they claim)
TRIP = 1024  # workgroups of one launch: tile k and tile k + TRIP are the same workgroup's, one trip apart
VERTEX_BYTES = 48
LONG_MAX = 2060  # the longest list: the shorter ones are its head


def slots_of(grid, flags):
    return (grid + 1) ** 2 if flags & GM.GRID else 2 * grid * (grid + 2)


def chunk_tiles(grid, flags):
    """tiles per launch of the host form, from the header's rule (one launch per 32 MiB of vertices, at least one tile)"""
    return max(1, (32 << 20) // (slots_of(grid, flags) * VERTEX_BYTES))


@functools.lru_cache(maxsize=None)
def long_rows(kind, seed):
    """rows of tiles(kind) for a list of LONG_MAX tiles: the scene over and over, each round in a permuted order of its own, such that
    positions k and k + 1024, and k and k + 2048, hold tiles of different LOD or side, and positions k and k + 1 different tiles.
    (One order repeated cannot do it: on the planar scene 32 of the 37 tiles are of two LODs, and the three positions of a workgroup that
    takes three trips need a third LOD each.)  Every round is drawn from `seed`; then, while a pair clashes, one of its two positions
    changes places with another of its round, and the exchange is kept unless it adds clashes"""
    t = tiles(kind)
    m = len(t)
    cls = t[:, 0].astype(np.int64) * 64 + t[:, 1]
    rng = np.random.default_rng(seed)
    k1, k2 = np.arange(LONG_MAX - TRIP), np.arange(LONG_MAX - 2 * TRIP)

    def clashing(r):
        c = cls[r]
        one, two = k1[c[k1] == c[k1 + TRIP]], k2[c[k2] == c[k2 + 2 * TRIP]]
        return np.concatenate([one, one + TRIP, two, two + 2 * TRIP, np.flatnonzero(r[1:] == r[:-1])])

    for attempt in range(32):  # (a draw whose repair comes to rest on a few clashes is drawn again)
        rows = np.concatenate([rng.permutation(m) for _ in range(-(-LONG_MAX // m))])[:LONG_MAX]
        bad = clashing(rows)
        for _ in range(4000):
            if not len(bad):
                return rows
            i = int(bad[rng.integers(len(bad))])
            j = min(i // m * m + int(rng.integers(m)), LONG_MAX - 1)
            rows[i], rows[j] = rows[j], rows[i]
            after = clashing(rows)
            if len(after) <= len(bad):
                bad = after
            else:
                rows[i], rows[j] = rows[j], rows[i]
    raise AssertionError((kind, seed, len(bad)))


def long_index(kind, count, seed=3):
    """row of tiles(kind) that position k of the long list holds"""
    assert count <= LONG_MAX
    return long_rows(kind, seed)[:count]


def long_tiles(kind, count, seed=3):
    """tiles(kind) in a fixed permuted order, round after round until `count`: every tile of the scene the same number of times +- 1"""
    return np.ascontiguousarray(tiles(kind)[long_index(kind, count, seed)])


def gather(expectation, index):
    """a model's (vertices, trace, admissible) of the scene's tiles -> (vertices, admissible) of the long list: the rows gathered to list
    order, tile_index the list's own"""
    vertices, _, admissible = expectation
    vertices = vertices[index].copy()
    vertices["tile_index"] = np.arange(len(index), dtype=np.uint32)[:, None]
    return vertices, admissible[index]


def long_expected(kind, grid, view, flags, count, seed=3):
    return gather(expected(kind, grid, True, view, flags), long_index(kind, count, seed))


# the host form's long calls, near view, loaded scenes: (kind, grid, flags, count, launches).  launches: the tiles of each launch, by the
# header's rule; more than 1024 in one launch is a later trip of the workgroup loop
LONG = [
    ("planar", 4, 0, 2060, (2060,)),                    # second and third trip; 12 workgroups take three
    ("sphere", 4, GM.GRID | GM.NO_MORPH, 1025, (1025,)),  # exactly one workgroup takes a second trip
    ("planar", 4, 0, 1024, (1024,)),                    # the boundary: nobody takes a second trip
    ("ellipsoid", 16, 0, 1300, (1213, 87)),             # a second trip inside chunk 0 (289 grid vertices: the thread loop's second trip too)
    ("planar", 32, 0, 330, (321, 9)),                   # a chunk boundary at the LDS cap
    ("sphere", 32, GM.GRID, 1290, (641, 641, 8)),       # three chunks: the scratch reused twice
]


def launches_of(grid, flags, count):
    chunk = chunk_tiles(grid, flags)
    return tuple(min(chunk, count - first) for first in range(0, count, chunk))


# ---- the device form on a list longer than 1024: a deeper tree on the same atlas, never adjusted (every entry invalid) ---------------------
DEEP_LODS = 9
DEEP_KW = dict(tree_size=4, morph_distance=6.0, blend_distance=1.0, grid_size=4, refinement_count=8, geometry_tile_count=4096)


def deep_view_config(**more):
    kw = dict(DEEP_KW, **more)
    return bt.TerrainViewConfig(**kw), O.make_view_config(**kw)


@functools.lru_cache(maxsize=None)
def deep_scene(kind):
    """the near view over a tree of DEEP_LODS LODs: the oracle's prepass list (measured: 1416 tiles on the sphere, 1415 on the ellipsoid, LODs
    2 .. 8), the parameters and the all-invalid table"""
    c = types.SimpleNamespace(kind=kind)
    c.model, c.omodel = MODELS[kind]
    c.view_config, c.oview_config = deep_view_config()
    c.position = SPECS[kind]["views"][0]
    c.view = O.view_state_from_config(c.omodel, c.oview_config, c.position, approximate_height(kind))
    c.tiles, c.indirect, _ = O.refine(c.view)
    c.P = GM.params(c.model, c.view_config, DEEP_LODS)
    c.entries = np.full(((1 if kind == "planar" else 6) * DEEP_LODS * DEEP_KW["tree_size"] ** 2, 2), GM.INVALID, np.uint32)
    return c


@functools.lru_cache(maxsize=None)
def deep_expected(kind, flags):
    c = deep_scene(kind)
    return GM.geometry(c.view, c.P, c.entries, {}, T, B, c.tiles, flags)


def cuts(n, slots):
    """(vertex_capacity, the first tile left out) of the capacity-cut test on a list of n tiles: in a second trip with tiles behind it;
    no partial tile and every second trip cut (24 workgroups already at their first: tiles 1000 .. 1023); the first trip whole and the
    second cut whole; everything"""
    return [(1100 * slots + slots - 1, 1100), (1000 * slots, 1000), (1024 * slots + 1, 1024), (n * slots, n)]

"""The case table of the sampling path (sample_surface of bt_tile_tree_device.hpp: compute_blend, lookup_tile at lod and lod - 1, the tile
samples, their blend), shared by test_sample_model.py (no GPU) and test_gpu_sample_shapes.py.

A case is a small terrain (lod_count 4, tree_size 4, an R16 and an Rgba8 attachment from different rasters), a view, a set of tiles whose
files are missing, and a batch of 1000 world positions.  Nothing is left to luck:

  * the loaded set is chosen so that, region by region around the view, the best loaded tile of a node is its own, its parent, its
    grandparent, or none at all (centre_layout, edge_layout); the best-tile table comes from the second models (TileTreeModel.update for the nodes and the
    requests, StreamModel for the atlas slots, a load of a missing tile left Loading);
  * the positions are crafted branch by branch (crafted_positions: by bisection on the second model's own log2, so ratio == 1, the blend
    range, lod 0 and the lod cap are all met on every bearing from the view; outside the planar terrain on all four sides; on every cube
    face, on its edges and corners), then padded with random ones;
  * compute_blend's f64 log2 is the platform's (OCML on the device, libm here), at most 1 ulp apart: a position is kept only if a log2 two
    representable doubles away on either side gives the same sample (S.blend_is_admissible); one that is not is replaced by the next draw,
    never left out of a comparison, and `replaced` counts them.

case(name) computes, once per process: the positions, the second model's values, heights and trace, and the oracle's values and heights
(an oracle tile tree given the same table).  reach_counts(case) turns the trace into the counts MINIMUM asks for."""
import functools
import math
import types

import numpy as np

import _cases as K
import _oracle as O
import _second_models as S
import bevy_terrain_amd as bt

LODS, TREE = 4, 4
COUNT = 1000  # positions per case
INVALID = 0xFFFFFFFF

MODELS = {
    "planar": (bt.TerrainModel.planar((10.0, -5.0, 3.0), 1000.0, 0.0, 250.0), O.make_model("planar", (10.0, -5.0, 3.0), 1000.0, 0.0, 0.0, 250.0)),
    "sphere": (bt.TerrainModel.sphere((0.0, 0.0, 0.0), 6371000.0, -12000.0, 9000.0), O.make_model("spherical", (0, 0, 0), 6371000.0, 0.0, -12000.0, 9000.0)),
    "ellipsoid": (bt.TerrainModel.ellipsoid((100.0, 200.0, -300.0), 6378137.0, 6356752.314245, -12000.0, 9000.0),
                  O.make_model("ellipsoidal", (100.0, 200.0, -300.0), 6378137.0, 6356752.314245, -12000.0, 9000.0)),
}


def descendants(side, lod, x, y):
    """the tile and every tile below it"""
    out = set()
    for l in range(lod, LODS):
        n = 1 << (l - lod)
        out |= {(side, l, (x << (l - lod)) + i, (y << (l - lod)) + j) for i in range(n) for j in range(n)}
    return out


def centre_layout(side, root_missing):
    """around the centre of a face, by quadrant of LOD 1: (0, 0) everything loaded; (1, 0) LOD 3 missing: a LOD 3 node is served by its
    parent; (0, 1) LODs 3 and 2 missing: by its grandparent; (1, 1) LODs 3, 2 and 1 missing: by the root, or (root_missing) by nothing"""
    missing = descendants(side, 1, 1, 1)
    missing |= {(side, 3, x, y) for x in range(4, 8) for y in range(0, 4)}
    missing |= {(side, 3, x, y) for x in range(0, 4) for y in range(4, 8)} | {(side, 2, x, y) for x in range(0, 2) for y in range(2, 4)}
    return missing | ({(side, 0, 0, 0)} if root_missing else set())


def edge_layout():
    """planar, around uv (0.5, 0.06) at the terrain's edge: the four LOD 3 tiles there are (3, 0) loaded; (4, 0) and (4, 1) missing under a
    loaded parent; (3, 1) missing under a missing parent: its grandparent.  The far quadrant and the root are missing: nothing."""
    return descendants(0, 1, 1, 1) | {(0, 0, 0, 0), (0, 2, 1, 0), (0, 3, 3, 1), (0, 3, 4, 0), (0, 3, 4, 1)}


def unit(v):
    v = np.asarray(v, np.float64)
    return v / math.sqrt(float(v @ v))


# kind, T, b, the view's blend_distance setting, the view position, the missing tiles
R, B = 6371000.0, 6356752.314245  # the sphere's radius, the ellipsoid's minor axis
SPECS = {
    # the view ON the surface (y = -5 + 125) and a round trip through the local frame that is exact: its own surface point is at distance 0
    "planar": dict(kind="planar", T=32, b=2, blend=1.0, view=(10.0 + 1000.0 * 9 / 1024, 120.0, 3.0 - 1000.0 * 13 / 1024), missing=centre_layout(0, True)),
    "planar_b1": dict(kind="planar", T=20, b=1, blend=2.0, view=(14.0, 130.0, 3.0 - 500.0 + 60.0), missing=edge_layout()),
    # above the centre of face 3 (+x), 2 km over the surface; face 4 has no tile at all
    "sphere": dict(kind="sphere", T=32, b=2, blend=1.0, view=tuple(unit((1.0, 0.012, -0.017)) * (R - 1500.0 + 2000.0)),
                   missing=centre_layout(3, False) | descendants(4, 0, 0, 0)),
    # above the centre of face 2 (+y, the pole); face 3 has no tile at all
    "ellipsoid": dict(kind="ellipsoid", T=32, b=2, blend=1.0, view=tuple(np.array((100.0, 200.0, -300.0)) + unit((0.015, 1.0, -0.011)) * (B + 500.0)),
                      missing=centre_layout(2, False) | descendants(3, 0, 0, 0)),
}
LOAD_DISTANCE = 20.0  # every node of every window is requested
BLEND_RANGE = 0.2

R16, RGBA8 = O.FORMAT_R16, O.FORMAT_RGBA8
CASES = {
    "planar_r16": ("planar", R16), "planar_rgba8": ("planar", RGBA8), "planar_b1_rgba8": ("planar_b1", RGBA8),
    "sphere_r16": ("sphere", R16), "sphere_rgba8": ("sphere", RGBA8), "ellipsoid_r16": ("ellipsoid", R16),
}

# what every case reaches, counted from the second model's trace (reach_counts)
MINIMUM = {"ratio_between": 32, "ratio_one": 8, "lod_zero": 8, "lod_cap": 8, "depth_0": 16, "depth_1": 16, "depth_2": 16, "no_ancestor": 8,
           "blend_depths_differ": 8, "wrapped_slot": 8}
MINIMUM_PLANAR = {"outside_x_low": 8, "outside_x_high": 8, "outside_z_low": 8, "outside_z_high": 8}
MINIMUM_CUBE = dict({f"face_{s}": 8 for s in range(6)}, face_edge=8)


def view_config(spec_name):
    spec = SPECS[spec_name]
    kw = dict(tree_size=TREE, load_distance=LOAD_DISTANCE, blend_distance=spec["blend"])
    return bt.TerrainViewConfig(**kw), O.make_view_config(**kw)


def raster_width(spec):
    return 2 ** (LODS - 1) * (spec["T"] - 2 * spec["b"]) + 13


def rasters(spec_name):
    """(the R16 sources, the Rgba8 sources): one each for the planar terrain, one per face for the others"""
    spec = SPECS[spec_name]
    w, faces = raster_width(spec), 1 if spec["kind"] == "planar" else 6
    return [K.smooth_raster(w, w, seed=3 + s) for s in range(faces)], [K.random_raster(RGBA8, w, w, seed=60 + s) for s in range(faces)]


def atlas_size(spec_name):
    return 64 if SPECS[spec_name]["kind"] == "planar" else 256


@functools.lru_cache(maxsize=None)
def oracle_tiles(spec_name):
    """{(side, lod, x, y): (R16 tile, Rgba8 tile)} of the whole pyramid, by the CPU oracle"""
    spec = SPECS[spec_name]
    heights, colours = rasters(spec_name)
    atlas = O.OracleAtlas(LODS, 6 * 100, spec["kind"] != "planar", [(spec["T"], spec["b"], 1, R16), (spec["T"], spec["b"], 1, RGBA8)])
    atlas.clear_attachment(0).clear_attachment(1)
    if spec["kind"] == "planar":
        atlas.preprocess_tile(0, heights[0], (0, LODS)).preprocess_tile(1, colours[0], (0, LODS))
    else:
        atlas.preprocess_spherical(0, heights, (0, LODS)).preprocess_spherical(1, colours, (0, LODS))
    atlas.run(4)
    return {coord: (atlas.tile(0, i), atlas.tile(1, i)) for coord, i in atlas.tiles()}


def tree_model(spec_name):
    spec = SPECS[spec_name]
    model = MODELS[spec["kind"]][0]
    tm = S.TileTreeModel(spec["kind"], model.translation, model.scale_vec, model.min_height, model.max_height, LODS, TREE, LOAD_DISTANCE)
    tm.project = O.project_point_ellipsoid  # (used by the ellipsoid only: the one step the second model does not restate)
    return tm


def blend_distance(spec_name):
    spec = SPECS[spec_name]
    model = MODELS[spec["kind"]][0]
    scale = float(model.scale_vec[0]) / 2.0 if spec["kind"] == "planar" else (float(model.scale_vec[0]) + float(model.scale_vec[1])) / 2.0
    return spec["blend"] * scale


@functools.lru_cache(maxsize=None)
def table(spec_name):
    """the state one frame leaves (update -> requests -> loads, those of SPECS[...]["missing"] failing -> adjust_to_tile_atlas), from the second
    models alone -> (TileTreeModel, requested tiles in order, {coordinate: atlas index} of the loaded tiles, entries (nodes, 2) u32,
    node coordinates (nodes, 4) u32)"""
    spec = SPECS[spec_name]
    existing = set(oracle_tiles(spec_name))
    assert spec["missing"] <= existing
    tm = tree_model(spec_name)
    released, requested = tm.update(spec["view"])
    assert released == []
    stream = S.StreamModel(atlas_size(spec_name), 2, existing=existing)
    for c in requested:
        stream.request_tile(c)
    done = stream.finish_loads(stream.pending_loads(), missing=spec["missing"])
    loaded = {c: index for c, index in done}
    coords, _ = tm.node_tables()
    entries = np.array([stream.get_best_tile(tuple(int(v) for v in c)) if c[1] != INVALID else (INVALID, INVALID) for c in coords], np.uint32)
    return tm, requested, loaded, entries, coords


def nearest_loaded_ancestor(coords, loaded):
    """the table once more, from the loaded set alone: every node's entry is its nearest loaded ancestor-or-self"""
    out = np.full((len(coords), 2), INVALID, np.uint32)
    for n, (side, lod, x, y) in enumerate(coords.tolist()):
        while lod != INVALID:
            if (side, lod, x, y) in loaded:
                out[n] = (loaded[(side, lod, x, y)], lod)
                break
            if lod == 0:
                break
            lod, x, y = lod - 1, x >> 1, y >> 1
    return out


# ---------------------------------------------------------------------------------------------- positions

TARGETS = ([1.0, 2.0, 3.0] + [k + f for k in (1, 2, 3) for f in (0.03, 0.08, 0.13, 0.18)] + [k + f for k in (0, 1, 2, 3) for f in (0.3, 0.6, 0.9)]
           + [3.995, 4.2, 5.0, 6.5, 9.0] + [-0.05, -0.2, -0.4])
BEARINGS = 16


def crafted_positions(spec_name, tm, height):
    """positions whose log2(blend_distance / view_distance), by the second model's arithmetic, is each of TARGETS on each of BEARINGS bearings
    from the view (found by bisection along the bearing; an integer target is met when its f32 IS that integer: ratio == 1); the view itself
    and the point under it; then per model the positions the blend does not steer: outside the terrain / every face, its edges and corners"""
    spec = SPECS[spec_name]
    view = np.asarray(spec["view"], np.float64)
    D = blend_distance(spec_name)
    rng = np.random.default_rng(5)
    centre = np.asarray(tm.t, np.float64)
    if spec["kind"] == "planar":
        reach = 1500.0
        along = lambda theta, s: view + s * np.array([math.cos(theta), 0.3, math.sin(theta)])
    else:
        n0 = unit(view - centre)
        e1 = unit(np.cross(n0, (0.0, 0.0, 1.0)))
        e2 = np.cross(n0, e1)
        radius = float(np.linalg.norm(view - centre))
        reach = math.pi  # s: the angle from the view's direction
        along = lambda theta, s: centre + (math.cos(s) * n0 + math.sin(s) * (math.cos(theta) * e1 + math.sin(theta) * e2)) * radius * (1.0 + 0.2 * math.sin(7.0 * theta))
    log2_at = lambda p: S.blend_log2(view, D, S.surface_position(tm, p, height))
    out = [view, along(0.0, 0.0) + (0.0, 77.0, 0.0) if spec["kind"] == "planar" else centre + (view - centre) * 1.5]
    for k in range(BEARINGS):
        theta = (k + 0.37) * 2.0 * math.pi / BEARINGS
        for target in TARGETS:
            lo, hi = 0.0, reach  # log2_at falls along the bearing
            exact = target == int(target)
            for _ in range(200):
                mid = 0.5 * (lo + hi)
                l2 = log2_at(along(theta, mid))
                if (np.float32(l2) == np.float32(target)) if exact else abs(l2 - target) < 1e-9:
                    out.append(along(theta, mid))
                    break
                lo, hi = (mid, hi) if l2 > target else (lo, mid)
    if spec["kind"] == "planar":
        half = 500.0
        for axis, sign in ((0, -1), (0, 1), (2, -1), (2, 1)):  # beyond each of the four sides, by 1 mm .. 10 km, all along the side and past its ends
            for k, beyond in enumerate((1e-3, 0.5, 3.0, 20.0, 45.0, 80.0, 150.0, 400.0, 2500.0, 1e4)):
                p = centre + (0.0, rng.uniform(0.0, 300.0), 0.0)
                p[axis] += sign * (half + beyond)
                p[2 - axis] += (k - 4.5) * 125.0 + (view[2 - axis] - centre[2 - axis] if k in (4, 5) else 0.0)
                out.append(p)
        for sx in (-1, 1):  # the four corners, exactly and inside
            for sz in (-1, 1):
                out += [centre + (sx * half, 10.0, sz * half), centre + (sx * (half - 7.0), 40.0, sz * (half - 31.0)), centre + (sx * (half - 60.0), 0.0, sz * (half - 2.0))]
    else:
        scale = float(tm.scale[0])
        axes = [np.array(v, np.float64) for v in ((-1, 0, 0), (0, 0, 1), (0, 1, 0), (1, 0, 0), (0, 0, -1), (0, -1, 0))]  # the centres of faces 0 .. 5
        for axis in axes:  # every face: its centre, and nine directions across it
            out.append(centre + axis * scale * 1.25)
            out += [centre + unit(axis + rng.uniform(-0.8, 0.8, 3) * (1.0 - np.abs(axis))) * scale * rng.uniform(0.5, 3.0) for _ in range(9)]
        for i in range(3):  # the twelve edges: exactly on them (two components tie) and a hair off; the eight corners
            for si in (-1.0, 1.0):
                for sj in (-1.0, 1.0):
                    d = np.zeros(3)
                    d[i], d[(i + 1) % 3], d[(i + 2) % 3] = si, sj, rng.uniform(-0.9, 0.9)
                    out.append(centre + d * scale * 0.9)
                    d[i] *= 1.0 - 1e-9
                    out.append(centre + d * scale * 1.1)
                    # ... and the two positions next to each other on either side of that edge as the MODEL sees it (an ellipsoid's edges are
                    # not where two components of the position tie): bisection on the side of the coordinate
                    across = lambda s: centre + np.where(np.arange(3) == i, d * (1.0 + s), d) * scale * 1.05
                    side_of = lambda p: tm.view_coordinate(S.surface_position(tm, p, height))[0]
                    lo, hi = -1e-3, 1e-3
                    if side_of(across(lo)) != side_of(across(hi)):
                        for _ in range(60):
                            mid = 0.5 * (lo + hi)
                            lo, hi = (mid, hi) if side_of(across(mid)) == side_of(across(lo)) else (lo, mid)
                        out += [across(lo), across(hi)]
        out += [centre + np.array((sx, sy, sz)) * scale * 0.7 for sx in (-1.0, 1.0) for sy in (-1.0, 1.0) for sz in (-1.0, 1.0)]
    return [np.asarray(p, np.float64) for p in out]


def random_positions(spec_name, tm, seed):
    """an endless stream of draws: near the view (all LODs) and anywhere"""
    spec = SPECS[spec_name]
    rng = np.random.default_rng(seed)
    view, centre = np.asarray(spec["view"], np.float64), np.asarray(tm.t, np.float64)
    D = blend_distance(spec_name)
    while True:
        if spec["kind"] == "planar":
            near = view + rng.normal(size=3) * (0.3 * D, 100.0, 0.3 * D)
            yield near if rng.random() < 0.8 else centre + rng.uniform(-620.0, 620.0, 3) * (1.0, 0.5, 1.0)
        else:
            scale = float(tm.scale[0])
            near = view + rng.normal(size=3) * 0.25 * D
            yield near if rng.random() < 0.5 else centre + unit(rng.normal(size=3)) * scale * rng.uniform(0.6, 2.0)


@functools.lru_cache(maxsize=None)
def positions(spec_name):
    """-> ((COUNT, 3) f64 positions, draws, replaced): the crafted positions, then random draws up to COUNT, every inadmissible draw replaced by
    the next one"""
    tm = table(spec_name)[0]
    height = float(tm.approximate_height)
    view, D = np.asarray(SPECS[spec_name]["view"], np.float64), blend_distance(spec_name)
    kept, draws, replaced = [], 0, 0
    stream = random_positions(spec_name, tm, seed=31)
    crafted = crafted_positions(spec_name, tm, height)
    assert len(crafted) <= COUNT - 200, len(crafted)
    while len(kept) < COUNT:
        p = crafted[draws] if draws < len(crafted) else next(stream)
        draws += 1
        if S.blend_is_admissible(S.blend_log2(view, D, S.surface_position(tm, p, height)), LODS, BLEND_RANGE):
            kept.append(p)
        else:
            replaced += 1
    return np.array(kept), draws, replaced


@functools.lru_cache(maxsize=None)
def case(name):
    """everything the tests of one case share, computed once: the positions, the second model's answer and trace, the oracle's answer"""
    spec_name, fmt = CASES[name]
    spec = SPECS[spec_name]
    tm, requested, loaded, entries, coords = table(spec_name)
    tiles = oracle_tiles(spec_name)
    c = types.SimpleNamespace()
    c.name, c.spec_name, c.spec, c.fmt, c.attachment = name, spec_name, spec, fmt, 0 if fmt == R16 else 1
    c.entries, c.coords, c.loaded = entries, coords, loaded
    c.layers = {index: tiles[coord][c.attachment] for coord, index in loaded.items()}
    c.positions, c.draws, c.replaced = positions(spec_name)
    c.model_values, c.model_heights, c.trace = S.sample_attachment(
        fmt, tm, spec["view"], tm.approximate_height, blend_distance(spec_name), BLEND_RANGE, LODS, entries.reshape(tm.sides, LODS, TREE, TREE, 2),
        c.layers, spec["T"], spec["b"], c.positions)
    otree = O.TileTree(MODELS[spec["kind"]][1], LODS, view_config(spec_name)[1])
    otree.update(spec["view"])
    otree.set_entries(entries)
    c.oracle_nodes = otree.read()[2]
    c.oracle_values, c.oracle_heights = otree.sample_attachment(fmt, spec["T"], spec["b"], c.layers, c.positions)
    return c


def reach_counts(c):
    """the counts MINIMUM (+ MINIMUM_PLANAR / MINIMUM_CUBE) names, from the second model's trace and the positions"""
    n = {k: 0 for k in list(MINIMUM) + list(MINIMUM_PLANAR if c.spec["kind"] == "planar" else MINIMUM_CUBE)}
    cap = np.float32(float(LODS) - 0.00001)
    centre = np.asarray(MODELS[c.spec["kind"]][0].translation, np.float64)
    for p, t in zip(c.positions, c.trace):
        first = t.lookups[0]
        n["ratio_between"] += 0.0 < t.ratio < 1.0
        n["ratio_one"] += t.ratio == 1.0
        n["lod_zero"] += t.lod == 0
        n["lod_cap"] += t.target_lod == cap
        for depth in (0, 1, 2):
            n[f"depth_{depth}"] += first.depth == depth
        n["no_ancestor"] += first.depth is None and (len(t.lookups) == 1 or t.lookups[1].depth is None)
        n["blend_depths_differ"] += len(t.lookups) == 2 and None not in (first.depth, t.lookups[1].depth) and first.depth != t.lookups[1].depth
        n["wrapped_slot"] += any((l.slot_x, l.slot_y) != (l.tile_x, l.tile_y) and l.depth is not None for l in t.lookups)
        if c.spec["kind"] == "planar":
            assert t.clamped == bool(abs(p[0] - centre[0]) > 500.0 or abs(p[2] - centre[2]) > 500.0)
            n["outside_x_low"] += p[0] - centre[0] < -500.0
            n["outside_x_high"] += p[0] - centre[0] > 500.0
            n["outside_z_low"] += p[2] - centre[2] < -500.0
            n["outside_z_high"] += p[2] - centre[2] > 500.0
        else:
            n[f"face_{t.side}"] += 1
            n["face_edge"] += min(t.uv[0], 1.0 - t.uv[0], t.uv[1], 1.0 - t.uv[1]) <= 1e-6
    return {k: int(v) for k, v in n.items()}


def minimum(c):
    return dict(MINIMUM, **(MINIMUM_PLANAR if c.spec["kind"] == "planar" else MINIMUM_CUBE))

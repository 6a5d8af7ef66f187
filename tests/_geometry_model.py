"""The definition of the terrain geometry (include/bevy_terrain_amd.h, TERRAIN GEOMETRY) written once more on the CPU in numpy, binary32
where the header says binary32, every operation in the header's order, whole arrays of vertices at a time.  TEST INFRASTRUCTURE ONLY.

Written from the header, not from the kernel.  What the definition takes over from elsewhere comes from the models of those parts: POINT's
pair from _cull_model.surface (the culling test's), the bilinear tail of the tile sample from _normal_model.tap (the normals').  numpy's
float32 +, -, *, /, sqrt are IEEE and unfused, one rounding per written operation, like the kernels' (-ffp-contract=off).

The two log2 are f64 and the platform's (libm here, OCML on the device), which may differ in the last place of a double.  geometry()
therefore also returns, per vertex, whether it is ADMISSIBLE: false when a log2 moved two representable doubles either way would change
any bit of the vertex.  Those are the only vertices a comparison with the device may skip."""
import math
import types

import numpy as np

import _cull_model as CM
import _normal_model as NM

F = np.float32
INVALID = 0xFFFFFFFF
GRID, NO_MORPH, NO_BLEND = 1, 2, 4

VERTEX_DTYPE = np.dtype([("position", np.float32, 3), ("height", np.float32), ("normal", np.float32, 3), ("tile_index", np.uint32),
                         ("coordinate_uv", np.float32, 2), ("view_distance", np.float32), ("blend_ratio", np.float32)])
FIELDS = ("position", "height", "normal", "tile_index", "coordinate_uv", "view_distance", "blend_ratio")

UP, NONE, DOWN = 1, 0, -1          # trace: which way coordinate_change_lod went (to a finer LOD, not at all, to a coarser one)
OWN, ANCESTOR, NO_ENTRY = 0, 1, 2  # trace: the entry a lookup found (its own LOD's tile, an ancestor's, BT_INVALID_LOD)
MORPH_ZERO, MORPH_BETWEEN, MORPH_ONE = 0, 1, 2


def params(model, view_config, lod_count):
    """what the definition takes from the tree: bt.TerrainModel, bt.TerrainViewConfig -> a namespace; the distances are
    f32(view_config value * TerrainModel::scale()), the scale in f64"""
    return types.SimpleNamespace(
        grid_size=int(view_config.grid_size), tree_size=int(view_config.tree_size), lod_count=int(lod_count),
        morph_distance=F(float(view_config.morph_distance) * NM.model_scale(_kind(model))), blend_distance=F(float(view_config.blend_distance) * NM.model_scale(_kind(model))),
        morph_range=F(view_config.morph_range), blend_range=F(view_config.blend_range), min_height=F(model.min_height), max_height=F(model.max_height))


def _kind(model):
    """a bt.TerrainModel as _normal_model.model_scale reads one (kind, a, b)"""
    kind = {"planar": 0, "spherical": 1, "ellipsoidal": 2}[model.kind]
    a = model.side_length if kind == 0 else (model.radius if kind == 1 else model.major_axis)
    return types.SimpleNamespace(kind=kind, a=a, b=model.minor_axis if kind == 2 else 0.0)


def strip_map(g):
    """slot gi of a tile's strip -> (cx, cy): compute_tile_uv's index arithmetic"""
    vpr = 2 * (g + 2)
    gi = np.arange(g * vpr)
    r = np.clip(gi % vpr, 1, vpr - 2) - 1
    col = gi // vpr
    return col + (r & 1), r >> 1


def slot_vertices(g, grid):
    """slot -> index cy * (g + 1) + cx of the grid vertex it holds, for either layout"""
    if grid:
        return np.arange((g + 1) ** 2)
    cx, cy = strip_map(g)
    return cy * (g + 1) + cx


def mix(a, b, t):
    return (a * (F(1.0) - t) + b * t).astype(F)


def sat(x):
    with np.errstate(invalid="ignore"):
        return np.where(x < 0, F(0.0), np.where(x > 1, F(1.0), x)).astype(F)


def log2_f64(x):
    """the platform's f64 log2 of an f32 array (libm through math.log2; the values libm's refuses, from numpy)"""
    x = x.astype(np.float64)
    with np.errstate(all="ignore"):
        out = np.log2(x)
    ok = np.isfinite(x) & (x > 0)
    out[ok] = [math.log2(v) for v in x[ok]]
    return out


def step_doubles(x, steps):
    """x moved `steps` representable doubles (towards +inf when positive)"""
    out = x.copy()
    for _ in range(abs(steps)):
        out = np.nextafter(out, np.inf if steps > 0 else -np.inf)
    return out


def change_lod(lod, x, y, u, v, new_lod):
    """coordinate_change_lod (functions.wgsl:164-188) of arrays of coordinates to arrays of LODs -> (x, y, u, v, direction)"""
    d = new_lod.astype(np.int64) - lod.astype(np.int64)
    count = np.uint64(1) << np.abs(d).astype(np.uint64)
    size = np.ldexp(F(1.0), d.astype(np.int32)).astype(F)
    out = []
    for xy, uv in ((x, u), (y, v)):
        xy = xy.astype(np.uint64)
        scaled = (uv * size).astype(F)
        whole = np.trunc(scaled)
        up_xy = (xy * count + whole.astype(np.uint64)) & np.uint64(0xFFFFFFFF)
        up_uv = (scaled - whole).astype(F)
        down_xy = xy >> np.abs(d).astype(np.uint64)
        down_uv = (((xy & (count - np.uint64(1))).astype(F) + uv).astype(F) * size).astype(F)
        out.append((np.where(d > 0, up_xy, np.where(d < 0, down_xy, xy)).astype(np.uint32), np.where(d > 0, up_uv, np.where(d < 0, down_uv, uv)).astype(F)))
    return out[0][0], out[1][0], out[0][1], out[1][1], np.sign(d).astype(np.int8)


def lookup(P, entries, stack, T, b, side, lod, x, y, u, v, lookup_lod):
    """lookup(o) of step 5 from L = bl - o on -> (h_o, the first change's direction, the entry's state, atlas index, the uv sampled)"""
    X, Y, U, V, direction = change_lod(lod, x, y, u, v, lookup_lod)
    ts = P.tree_size
    index = ((side.astype(np.int64) * P.lod_count + lookup_lod.astype(np.int64)) * ts + X.astype(np.int64) % ts) * ts + Y.astype(np.int64) % ts
    atlas_index, atlas_lod = entries[index, 0], entries[index, 1]
    invalid = atlas_lod == INVALID
    X2, Y2, U2, V2, _ = change_lod(lookup_lod, X, Y, U, V, np.where(invalid, lookup_lod, atlas_lod))
    c = T - 2 * b
    scale, offset = F(c) / F(T), F(b) / F(T)
    held = ~invalid & (atlas_index < len(stack))
    value = NM.tap(stack, np.where(held, atlas_index, 0), U2 * scale + offset, V2 * scale + offset)
    value = np.where(held, value, F(0.0)).astype(F)
    state = np.where(invalid, NO_ENTRY, np.where(atlas_lod < lookup_lod, ANCESTOR, OWN)).astype(np.int8)
    return mix(P.min_height, P.max_height, value), direction, state, atlas_index, (U2, V2)


def _vertices(view, P, entries, stack, T, b, tiles, flags, dm=0, db=0, logs=None):
    """steps 1 - 6 for every grid vertex of every tile, the morph's log2 moved dm doubles and the blend's db -> (fields, trace); logs: a
    dict that keeps the two f64 log2 arrays ("m", "b") from one call to the next of the same scene"""
    logs = {} if logs is None else logs
    g = P.grid_size
    G = F(g)
    row = g + 1
    n, V = len(tiles), row * row
    t = np.repeat(np.asarray(tiles, np.uint32).reshape(-1, 4), V, axis=0)
    side, lod, x, y = (t[:, k] for k in range(4))
    cy, cx = np.divmod(np.tile(np.arange(V), n), row)
    tuv = np.stack([cx.astype(F) / G, cy.astype(F) / G], axis=1).astype(F)
    # 2
    world0, n0 = CM.surface(view, t, tuv)
    wp = np.array(list(view.world_position), F)
    delta = ((world0 + F(view.approximate_height) * n0).astype(F) - wp).astype(F)
    with np.errstate(all="ignore"):
        d = CM.length3(delta)
        # 3
        target = np.zeros(n * V, F)
        ratio = np.zeros(n * V, F)
        uv, world, nrm = tuv, world0, n0
        if not flags & NO_MORPH:
            even = ((tuv * G).astype(F).astype(np.uint32) & np.uint32(0xFFFFFFFE)).astype(F) / G
            if "m" not in logs:
                logs["m"] = log2_f64(((F(2.0) * P.morph_distance) / d).astype(F))
            target = step_doubles(logs["m"], dm).astype(F)
            lf = lod.astype(F)
            a = (lf + P.morph_range).astype(F)
            ratio = np.where(lod == 0, F(0.0), sat(((target - a) / (lf - a)).astype(F))).astype(F)
            uv = np.stack([mix(tuv[:, k], even[:, k].astype(F), ratio) for k in range(2)], axis=1)
            world, nrm = CM.surface(view, t, uv)
        # 4
        if "b" not in logs:
            logs["b"] = log2_f64((P.blend_distance / d).astype(F))
        l2 = step_doubles(logs["b"], db).astype(F)
        cap = F(P.lod_count) - F(0.00001)
        tb = np.where(l2 < cap, l2, cap).astype(F)
        bl = np.where(tb > 0, np.trunc(np.where(tb > 0, tb, 0)), 0).astype(np.uint32)
        ratio_b = np.zeros(n * V, F)
        if not flags & NO_BLEND:
            bf = bl.astype(F)
            a = (bf + P.blend_range).astype(F)
            ratio_b = np.where(bl == 0, F(0.0), sat(((tb - a) / (bf - a)).astype(F))).astype(F)
        # 5, 6
        second = ratio_b > 0
        h0, dir0, state0, index0, uv0 = lookup(P, entries, stack, T, b, side, lod, x, y, uv[:, 0], uv[:, 1], bl)
        h1, dir1, state1, index1, uv1 = lookup(P, entries, stack, T, b, side, lod, x, y, uv[:, 0], uv[:, 1], np.where(second, bl - 1, bl).astype(np.uint32))
        height = np.where(second, mix(h0, h1, ratio_b), h0).astype(F)
        position = (world + height[:, None] * nrm).astype(F)
    out = np.zeros(n * V, VERTEX_DTYPE)
    out["position"], out["height"], out["normal"] = position, height, nrm
    out["tile_index"] = np.repeat(np.arange(n, dtype=np.uint32), V)
    out["coordinate_uv"], out["view_distance"], out["blend_ratio"] = uv, d, ratio_b
    trace = dict(side=side, lod=lod, cx=cx, cy=cy, second=second, morph_ratio=ratio, dir0=dir0, dir1=dir1, state0=state0, state1=state1, blend_lod=bl,
                 morph=np.where(ratio == 0, MORPH_ZERO, np.where(ratio == 1, MORPH_ONE, MORPH_BETWEEN)).astype(np.int8),
                 h0=h0, h1=h1, index0=index0, index1=index1, uv0=np.stack(uv0, axis=1), uv1=np.stack(uv1, axis=1), world=world)
    return out, trace


def same_bits(a, b):
    """per vertex: every field of a equals b's bit for bit"""
    return (a.view(np.uint32).reshape(len(a), -1) == b.view(np.uint32).reshape(len(b), -1)).all(axis=1)


def geometry(view, P, entries, layers, T, b, tiles, flags=0, logs=None):
    """TERRAIN GEOMETRY of `tiles` ((n, 4) [side, lod, x, y]) against a tree's entries ((nodes, 2) u32) and the layers {atlas_index: (T, T)
    uint16} -> (vertices (n, slots) VERTEX_DTYPE in the layout `flags` names, trace {name: (n, slots)}, admissible (n, slots) bool).
    logs: a dict that receives the two f64 log2 arrays per grid vertex ("m" morph, "b" blend); one that holds them already is used as it
    is (the tests of the admissibility flag plant boundary values there)"""
    tiles = np.asarray(tiles, np.uint32).reshape(-1, 4)
    stack = NM.stack_layers(layers, T)
    entries = np.asarray(entries, np.uint32).reshape(-1, 2)
    logs = {} if logs is None else logs
    base, trace = _vertices(view, P, entries, stack, T, b, tiles, flags, logs=logs)
    admissible = np.ones(len(base), bool)
    moves = lambda k, step: (step_doubles(logs[k], step).astype(F).view(np.uint32) != logs[k].astype(F).view(np.uint32)).any()
    for dm in ((0,) if flags & NO_MORPH else (-2, 0, 2)):
        for db in (-2, 0, 2):
            # (a move that leaves both f32 values as they were everywhere leaves every vertex as it was)
            if (dm and moves("m", dm)) or (db and moves("b", db)):
                admissible &= same_bits(base, _vertices(view, P, entries, stack, T, b, tiles, flags, dm, db, logs)[0])
    V = (P.grid_size + 1) ** 2
    take = slot_vertices(P.grid_size, bool(flags & GRID))
    shape = lambda a: a.reshape((len(tiles), V) + a.shape[1:])[:, take]
    return shape(base), {k: shape(v) for k, v in trace.items()}, shape(admissible)

"""The definition of the HIGH PRECISION terrain geometry (include/bevy_terrain_amd.h, HIGH PRECISION) written once more on the CPU: the
Taylor coefficients of bt_model_approximation_from_config in binary64 (Python floats: IEEE doubles, math.sqrt correctly rounded, one
rounding per written operation), REL and the hp vertex in numpy binary32 on top of _geometry_model (its mix, sat, log2, change_lod and
lookup; POINT's pair from _cull_model.surface).  TEST INFRASTRUCTURE ONLY.

Written from the header, not from the library.  The view coordinate and its projection onto the six sides come from the second model of
the tile tree (_second_models.TileTreeModel, whose ellipsoid takes the oracle's projection), the f64 surface function of the accuracy and
finite-difference tests is its world_position.

geometry() is _geometry_model.geometry with the approximation: same layouts, same admissibility rule (a vertex is inadmissible when a log2
moved two doubles either way would change one of its bits).  Its trace is _geometry_model's extended by `hp` (the vertex took the series)
and `dir_origin` (the way coordinate_change_lod went from the tile's LOD to origin_lod: GM.UP / NONE / DOWN)."""
import math
import struct
import types

import numpy as np

import _cull_model as CM
import _geometry_model as GM
import _normal_model as NM
import _oracle as O
import _second_models as S

F = np.float32
VIEW_RELATIVE = 8
C_SQR = 0.87 * 0.87
NAMES = ("c", "c_s", "c_t", "c_ss", "c_st", "c_tt")
# SIDE_MATRICES (terrain_model.rs:14-21), column major
SIDE_MATRICES = ((-1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, -1.0, 0.0), (0.0, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0, -1.0, 0.0), (0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0),
                 (1.0, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0, 1.0), (0.0, 0.0, -1.0, 0.0, -1.0, 0.0, 1.0, 0.0, 0.0), (0.0, -1.0, 0.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0))


def tree_model(model):
    """a bt.TerrainModel (sphere or ellipsoid) as the second model of the tile tree: its view coordinate, projection and f64 surface"""
    kind = {"spherical": "sphere", "ellipsoidal": "ellipsoid"}[model.kind]
    tm = S.TileTreeModel(kind, model.translation, model.scale_vec, model.min_height, model.max_height, 1, 1, 1.0)
    tm.project = O.project_point_ellipsoid
    return tm


def cube(x):
    return x * x * x


def pow5(x):
    return (x * x) * (x * x) * x


def side_series(side, s, t, scale, position):
    """the six f64 vectors of a side's series at (s, t), before the casts: p - nothing, p_s, p_t, p_ss, p_st, p_tt (unhalved)"""
    s, t = float(s), float(t)
    u_denom = math.sqrt(1.0 - 4.0 * C_SQR * s * (s - 1.0))
    u = (2.0 * s - 1.0) / u_denom
    u_ds = 2.0 * (C_SQR + 1.0) / cube(u_denom)
    u_dss = 12.0 * C_SQR * (C_SQR + 1.0) * (2.0 * s - 1.0) / pow5(u_denom)

    v_denom = math.sqrt(1.0 - 4.0 * C_SQR * t * (t - 1.0))
    v = (2.0 * t - 1.0) / v_denom
    v_dt = 2.0 * (C_SQR + 1.0) / cube(v_denom)
    v_dtt = 12.0 * C_SQR * (C_SQR + 1.0) * (2.0 * t - 1.0) / pow5(v_denom)

    l = math.sqrt(1.0 + u * u + v * v)
    l_ds = u * u_ds / l
    l_dt = v * v_dt / l
    l_dss = (u * u_dss * l * l + (v * v + 1.0) * u_ds * u_ds) / cube(l)
    l_dst = -(u * v * u_ds * v_dt) / cube(l)
    l_dtt = (v * v_dtt * l * l + (u * u + 1.0) * v_dt * v_dt) / cube(l)

    a = 1.0
    a_ds = -l_ds
    a_dt = -l_dt
    a_dss = 2.0 * l_ds * l_ds - l * l_dss
    a_dst = 2.0 * l_ds * l_dt - l * l_dst
    a_dtt = 2.0 * l_dt * l_dt - l * l_dtt

    b = u
    b_ds = -u * l_ds + l * u_ds
    b_dt = -u * l_dt
    b_dss = 2.0 * u * l_ds * l_ds - l * (2.0 * u_ds * l_ds + u * l_dss) + u_dss * l * l
    b_dst = 2.0 * u * l_ds * l_dt - l * (u_ds * l_dt + u * l_dst)
    b_dtt = 2.0 * u * l_dt * l_dt - l * u * l_dtt

    c = v
    c_ds = -v * l_ds
    c_dt = -v * l_dt + l * v_dt
    c_dss = 2.0 * v * l_ds * l_ds - l * v * l_dss
    c_dst = 2.0 * v * l_ds * l_dt - l * (v_dt * l_ds + v * l_dst)
    c_dtt = 2.0 * v * l_dt * l_dt - l * (2.0 * v_dt * l_dt + v * l_dtt) + v_dtt * l * l

    k = SIDE_MATRICES[side]
    sm = lambda x, y, z: [(k[i] * x + k[3 + i] * y) + k[6 + i] * z for i in range(3)]
    vector = lambda w, d: [float(scale[i]) * (w[i] / d) for i in range(3)]
    p = [q + float(position[i]) for i, q in enumerate(vector(sm(a, b, c), l))]
    return [p, vector(sm(a_ds, b_ds, c_ds), l * l), vector(sm(a_dt, b_dt, c_dt), l * l), vector(sm(a_dss, b_dss, c_dss), cube(l)),
            vector(sm(a_dst, b_dst, c_dst), cube(l)), vector(sm(a_dtt, b_dtt, c_dtt), cube(l))]


def coefficients64(model, position):
    """-> (view side, [(s, t) per side], (6 sides, 6 vectors, 3) float64: c relative to the view, c_ss and c_tt halved, before `as f32`)"""
    tm = tree_model(model)
    side0, uv0 = tm.view_coordinate(np.asarray(position, np.float64))
    out = np.zeros((6, 6, 3), np.float64)
    st = []
    for side in range(6):
        s, t = (float(v) for v in tm.project_to_side(side0, np.asarray(uv0, np.float64), side))
        st.append((s, t))
        p, p_s, p_t, p_ss, p_st, p_tt = side_series(side, s, t, model.scale_vec, model.translation)
        out[side] = [[p[i] - float(position[i]) for i in range(3)], p_s, p_t, [q / 2.0 for q in p_ss], p_st, [q / 2.0 for q in p_tt]]
    return side0, st, out


def approximation(model, view_config, position):
    """bt_model_approximation_from_config -> a namespace: sides (6, 6, 3) float32 in NAMES order, precision_threshold_distance, origin_lod"""
    _, _, c64 = coefficients64(model, position)
    return types.SimpleNamespace(sides=c64.astype(F), origin_lod=int(view_config.origin_lod),
                                 precision_threshold_distance=F(float(view_config.precision_threshold_distance) * NM.model_scale(GM._kind(model))))


def approximation_bytes(A):
    """the 448 bytes of a bt_model_approximation"""
    return A.sides.tobytes() + struct.pack("<fIII", float(A.precision_threshold_distance), A.origin_lod, 0, 0)


def rel(view, A, side, lod, x, y, u, v):
    """REL of arrays of coordinates -> ((n, 3) float32, the direction coordinate_change_lod took to origin_lod)"""
    X, Y, U, V, direction = GM.change_lod(lod, x, y, u, v, np.full_like(lod, A.origin_lod))
    view_xy = np.array([[view.sides[k].view_xy[0], view.sides[k].view_xy[1]] for k in range(6)], np.int64)
    view_uv = np.array([[view.sides[k].view_uv[0], view.sides[k].view_uv[1]] for k in range(6)], F)
    count = F(float(1 << A.origin_lod))
    st = []
    for axis, (XY, UV) in enumerate(((X, U), (Y, V))):
        whole = (XY.astype(np.int64) - view_xy[side, axis] + (1 << 31)) % (1 << 32) - (1 << 31)  # i32, wrapping
        st.append((((whole.astype(F) + UV).astype(F) - view_uv[side, axis]).astype(F) / count).astype(F))
    s, t = st[0][:, None], st[1][:, None]
    k = A.sides[side]  # (n, 6, 3)
    c, c_s, c_t, c_ss, c_st, c_tt = (k[:, i].astype(F) for i in range(6))
    r = ((((c + c_s * s) + c_t * t) + (c_ss * s) * s) + (c_st * s) * t) + (c_tt * t) * t
    assert r.dtype == F
    return r, direction


def _vertices(view, A, P, entries, stack, T, b, tiles, flags, dm=0, db=0, logs=None):
    """_geometry_model._vertices with steps 2h and 3h and BT_GEOMETRY_VIEW_RELATIVE"""
    logs = {} if logs is None else logs
    g = P.grid_size
    G = F(g)
    row = g + 1
    n, V = len(tiles), row * row
    t = np.repeat(np.asarray(tiles, np.uint32).reshape(-1, 4), V, axis=0)
    side, lod, x, y = (t[:, k] for k in range(4))
    cy, cx = np.divmod(np.tile(np.arange(V), n), row)
    tuv = np.stack([cx.astype(F) / G, cy.astype(F) / G], axis=1).astype(F)
    ah = F(view.approximate_height)
    # 2
    world0, n0 = CM.surface(view, t, tuv)
    wp = np.array(list(view.world_position), F)
    with np.errstate(all="ignore"):
        d0 = CM.length3(((world0 + ah * n0).astype(F) - wp).astype(F))
        # 2h
        hp = d0 < A.precision_threshold_distance
        rel0, dir_origin = rel(view, A, side, lod, x, y, tuv[:, 0], tuv[:, 1])
        d = np.where(hp, CM.length3((rel0 + (ah * n0).astype(F)).astype(F)), d0).astype(F)
        # 3
        target = np.zeros(n * V, F)
        ratio = np.zeros(n * V, F)
        uv, world, nrm = tuv, world0, n0
        if not flags & GM.NO_MORPH:
            even = ((tuv * G).astype(F).astype(np.uint32) & np.uint32(0xFFFFFFFE)).astype(F) / G
            if "m" not in logs:
                logs["m"] = GM.log2_f64(((F(2.0) * P.morph_distance) / d).astype(F))
            target = GM.step_doubles(logs["m"], dm).astype(F)
            lf = lod.astype(F)
            a = (lf + P.morph_range).astype(F)
            ratio = np.where(lod == 0, F(0.0), GM.sat(((target - a) / (lf - a)).astype(F))).astype(F)
            uv = np.stack([GM.mix(tuv[:, k], even[:, k].astype(F), ratio) for k in range(2)], axis=1)
            world, nrm = CM.surface(view, t, uv)
        # 3h
        relm, _ = rel(view, A, side, lod, x, y, uv[:, 0], uv[:, 1])
        world = np.where(hp[:, None], (wp + relm).astype(F), world).astype(F)
        nrm = np.where(hp[:, None], n0, nrm).astype(F)
        # 4
        if "b" not in logs:
            logs["b"] = GM.log2_f64((P.blend_distance / d).astype(F))
        l2 = GM.step_doubles(logs["b"], db).astype(F)
        cap = F(P.lod_count) - F(0.00001)
        tb = np.where(l2 < cap, l2, cap).astype(F)
        bl = np.where(tb > 0, np.trunc(np.where(tb > 0, tb, 0)), 0).astype(np.uint32)
        ratio_b = np.zeros(n * V, F)
        if not flags & GM.NO_BLEND:
            bf = bl.astype(F)
            a = (bf + P.blend_range).astype(F)
            ratio_b = np.where(bl == 0, F(0.0), GM.sat(((tb - a) / (bf - a)).astype(F))).astype(F)
        # 5, 6
        second = ratio_b > 0
        h0, dir0, state0, index0, uv0 = GM.lookup(P, entries, stack, T, b, side, lod, x, y, uv[:, 0], uv[:, 1], bl)
        h1, dir1, state1, index1, uv1 = GM.lookup(P, entries, stack, T, b, side, lod, x, y, uv[:, 0], uv[:, 1], np.where(second, bl - 1, bl).astype(np.uint32))
        height = np.where(second, GM.mix(h0, h1, ratio_b), h0).astype(F)
        base = world
        if flags & VIEW_RELATIVE:
            base = np.where(hp[:, None], relm, (world - wp).astype(F)).astype(F)
        position = (base + height[:, None] * nrm).astype(F)
    out = np.zeros(n * V, GM.VERTEX_DTYPE)
    out["position"], out["height"], out["normal"] = position, height, nrm
    out["tile_index"] = np.repeat(np.arange(n, dtype=np.uint32), V)
    out["coordinate_uv"], out["view_distance"], out["blend_ratio"] = uv, d, ratio_b
    trace = dict(side=side, lod=lod, cx=cx, cy=cy, second=second, morph_ratio=ratio, dir0=dir0, dir1=dir1, state0=state0, state1=state1, blend_lod=bl,
                 morph=np.where(ratio == 0, GM.MORPH_ZERO, np.where(ratio == 1, GM.MORPH_ONE, GM.MORPH_BETWEEN)).astype(np.int8),
                 hp=hp, dir_origin=dir_origin)
    return out, trace


def geometry(view, A, P, entries, layers, T, b, tiles, flags=0):
    """HIGH PRECISION TERRAIN GEOMETRY of `tiles` -> (vertices (n, slots), trace {name: (n, slots)}, admissible (n, slots)), as
    _geometry_model.geometry; flags may carry VIEW_RELATIVE"""
    tiles = np.asarray(tiles, np.uint32).reshape(-1, 4)
    stack = NM.stack_layers(layers, T)
    entries = np.asarray(entries, np.uint32).reshape(-1, 2)
    logs = {}
    base, trace = _vertices(view, A, P, entries, stack, T, b, tiles, flags, logs=logs)
    admissible = np.ones(len(base), bool)
    moves = lambda k, step: (GM.step_doubles(logs[k], step).astype(F).view(np.uint32) != logs[k].astype(F).view(np.uint32)).any()
    for dm in ((0,) if flags & GM.NO_MORPH else (-2, 0, 2)):
        for db in (-2, 0, 2):
            if (dm and moves("m", dm)) or (db and moves("b", db)):
                admissible &= GM.same_bits(base, _vertices(view, A, P, entries, stack, T, b, tiles, flags, dm, db, logs)[0])
    V = (P.grid_size + 1) ** 2
    take = GM.slot_vertices(P.grid_size, bool(flags & GM.GRID))
    shape = lambda a: a.reshape((len(tiles), V) + a.shape[1:])[:, take]
    return shape(base), {k: shape(v) for k, v in trace.items()}, shape(admissible)


def truth(model, tiles, uv):
    """the f64 surface (Coordinate::world_position at height 0) at uv ((n, slots, 2), any float type, taken exactly) of each tile ->
    (n, slots, 3) float64 world positions"""
    tm = tree_model(model)
    tiles = np.asarray(tiles, np.uint32).reshape(-1, 4)
    out = np.zeros(uv.shape[:2] + (3,), np.float64)
    for k, (side, lod, x, y) in enumerate(tiles.tolist()):
        st = (np.array([x, y], np.float64) + uv[k].astype(np.float64)) / float(1 << lod)
        out[k] = tm.world_position(side, st, 0.0)
    return out

"""numpy model of bt_atlas_scatter_instances: the SCATTER section of include/bevy_terrain_amd.h, steps 1 - 9, on {coord: tile} dictionaries.

TEST INFRASTRUCTURE ONLY.  State is _edit_model's: heights {(side, lod, x, y): T x T uint16} and, for a mask, {coord: T x T x 4 uint8} of one
atlas.  The taps and s are _normal_model's (the model the normal bake is held to), band() is _splat_model's, the position is the oracle's
orc_coordinate_world_position; the local position behind the mesh normal is coordinate.rs:115-133 written once more in numpy f64 and held
to the oracle's position by tests/test_scatter_model.py.  All binary32 arithmetic is numpy float32, one IEEE rounding per written
operation, in the header's order; the hash is numpy uint32.  A rule is anything with the fields of bevy_terrain_amd.ScatterRule (height,
steep(), height_fade, slope_fade, density, scale, channel()); model: an _oracle model.  Nothing of the package under test is imported."""
import numpy as np

import _normal_model as NM
import _oracle as O
from _splat_model import band

F = np.float32
U = np.uint32
NO_MASK = 0xFFFFFFFF
MAX_RULES = 8
DTYPE = np.dtype([("position", "<f8", 3), ("normal", "<f4", 3), ("scale", "<f4"), ("yaw", "<f4"), ("rule", "<u4"), ("cell", "<u4", 2)])
assert DTYPE.itemsize == 56
C_SQR = 0.87 * 0.87  # math/mod.rs:13


# ---- step 1 ------------------------------------------------------------------------------------------------------------------------------

def mix(x):
    x = np.atleast_1d(np.asarray(x, dtype=np.uint32)).copy()
    with np.errstate(over="ignore"):
        x ^= x >> U(16)
        x *= U(0x7FEB352D)
        x ^= x >> U(15)
        x *= U(0x846CA68B)
        x ^= x >> U(16)
    return x


def key(seed, side, lod, gx, gy):
    return mix(mix(mix(U(seed) ^ U(side << 8 | lod)) ^ np.asarray(gx, dtype=np.uint32)) ^ np.asarray(gy, dtype=np.uint32))


def draw(k, n):
    with np.errstate(over="ignore"):
        return mix(np.asarray(k, dtype=np.uint32) + U((n * 0x9E3779B9) & 0xFFFFFFFF))


def unit(r):
    return (np.asarray(r, dtype=np.uint32) >> U(8)).astype(np.float32) * F(2.0 ** -24)


# ---- steps 2 - 6 for one tile ------------------------------------------------------------------------------------------------------------

def rule_fields(rule):
    lo, hi = rule.steep()
    return dict(height=(F(rule.height[0]), F(rule.height[1]), F(rule.height_fade)), steep=(F(lo), F(hi), F(rule.slope_fade)), density=F(rule.density),
                scale=(F(rule.scale[0]), F(rule.scale[1])), channel=int(rule.channel()))


def cells(coord, c, seed, jitter):
    """steps 1 and 2 for every cell of a tile, j major: dict(i, j, gx, gy, key, uv)"""
    side, lod, X, Y = coord
    j, i = [a.ravel() for a in np.meshgrid(np.arange(c), np.arange(c), indexing="ij")]
    gx, gy = (X * c + i).astype(np.uint32), (Y * c + j).astype(np.uint32)
    k = key(seed, side, lod, gx, gy)
    ax = F(0.5) + (unit(draw(k, 1)) - F(0.5)) * F(jitter)
    ay = F(0.5) + (unit(draw(k, 2)) - F(0.5)) * F(jitter)
    uv = [(i.astype(np.float32) + ax) / F(c), (j.astype(np.float32) + ay) / F(c)]
    return dict(i=i, j=j, gx=gx, gy=gy, key=k, uv=uv)


def centre_tap(h_tile, b, uv):
    """the tap (u_x, u_y) of TILE NORMAL -> (its bilinear value, whether one of its four texels is 0, its first texel (ix, iy) before the clamp)"""
    T = h_tile.shape[0]
    c = T - 2 * b
    scale, offset = F(c) / F(T), F(b) / F(T)
    ux, uy = uv[0] * scale + offset, uv[1] * scale + offset
    value = NM.tap(h_tile[None, :, :], np.zeros(len(ux), np.int64), ux, uy)
    ix, iy = np.trunc(ux * F(T) - F(0.5)).astype(np.int64), np.trunc(uy * F(T) - F(0.5)).astype(np.int64)
    zero = np.zeros(len(ux), bool)
    for x in (0, 1):
        for y in (0, 1):
            zero |= h_tile[np.clip(iy + y, 0, T - 1), np.clip(ix + x, 0, T - 1)] == 0
    return value, zero, (ix, iy)


def tap_extent(T, b, uv):
    """the texels the four taps and the centre tap of TILE NORMAL touch, before the clamp: (lo_x, hi_x, lo_y, hi_y), inclusive"""
    c = T - 2 * b
    scale, offset, o = F(c) / F(T), F(b) / F(T), F(0.5) / F(c)
    out = []
    for a in (0, 1):
        u = uv[a] * scale + offset
        out += [np.trunc((u - o) * F(T) - F(0.5)).astype(np.int64), np.trunc((u + o) * F(T) - F(0.5)).astype(np.int64) + 1]
    return out


def decide(model, h_tile, b, coord, rules, seed, jitter, mask_tile=None, reached=None):
    """steps 1 - 6 for every cell of one tile -> dict(cells..., no_data, rule (-1: none), h, s).  reached (a dict, optional) counts
    "centre_hole": cells whose own texel is 0; "pair_hole": data texels whose centre tap meets a 0; "empty": data cells that place nothing;
    "starved": data cells where a rule with p > 0 stands behind a sum that has reached 1; "mask_0" / "mask_255": data cells whose masked
    rule reads that byte; "clamped": data cells one of whose tap texels is clamped at the layer's edge; "rule_k": cells rule k placed"""
    T = h_tile.shape[0]
    c = T - 2 * b
    lod = coord[1]
    cl = cells(coord, c, seed, jitter)
    raw = h_tile[b + cl["j"], b + cl["i"]]
    v, zero, (ix, iy) = centre_tap(h_tile, b, cl["uv"])
    no_data = (raw == 0) | zero
    lo, hi = F(model.min_height), F(model.max_height)
    h = lo + (hi - lo) * v
    s = NM.tile_normal(model, h_tile[None, :, :], b, np.zeros(c * c, np.int64), np.full(c * c, lod), cl["uv"])
    steep = F(1.0) - s[2].astype(np.float32)
    u = unit(draw(cl["key"], 0))
    A = np.zeros(c * c, np.float32)
    rule = np.full(c * c, -1, np.int64)
    starved = np.zeros(c * c, bool)
    mask_bytes = {0: np.zeros(c * c, bool), 255: np.zeros(c * c, bool)}
    for k, r in enumerate(rules):
        f = rule_fields(r)
        p = (f["density"] * band(h, *f["height"])) * band(steep, *f["steep"])
        if f["channel"] == NO_MASK:
            m = F(1.0)
        else:
            byte = mask_tile[b + cl["j"], b + cl["i"], f["channel"]]
            m = byte.astype(np.float32) / F(255.0)
            for value in mask_bytes:
                mask_bytes[value] |= byte == value
        p = (p * m).astype(np.float32)
        starved |= (p > 0) & (A >= 1)
        A = (A + p).astype(np.float32)
        rule = np.where((rule < 0) & (u < A), k, rule)
    rule = np.where(no_data, -1, rule)
    if reached is not None:
        data = ~no_data
        lo_x, hi_x, lo_y, hi_y = tap_extent(T, b, cl["uv"])
        clamped = (lo_x < 0) | (lo_y < 0) | (hi_x > T - 1) | (hi_y > T - 1)
        for name, where in (("centre_hole", raw == 0), ("pair_hole", (raw != 0) & zero), ("empty", data & (rule < 0)), ("starved", data & starved),
                            ("mask_0", data & mask_bytes[0]), ("mask_255", data & mask_bytes[255]), ("clamped", data & clamped), ("data", data)):
            reached[name] = reached.get(name, 0) + int(where.sum())
        for k in range(len(rules)):
            reached[f"rule_{k}"] = reached.get(f"rule_{k}", 0) + int((rule == k).sum())
    return dict(cl, no_data=no_data, rule=rule, h=h.astype(np.float32), s=s, raw=raw)


# ---- step 7 ------------------------------------------------------------------------------------------------------------------------------

def _normalize3(a):
    r = 1.0 / np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
    return [a[0] * r, a[1] * r, a[2] * r]


def local_position(model, side, uv):
    """coordinate.rs:115-133 in f64 for arrays uv = (x, y): the local position of a coordinate, unit on a spherical model"""
    x, y = np.asarray(uv[0], np.float64), np.asarray(uv[1], np.float64)
    if int(model.kind) == 0:
        return [x - 0.5, np.zeros_like(x), y - 0.5]
    wx, wy = (x - 0.5) / 0.5, (y - 0.5) / 0.5
    qx, qy = wx / np.sqrt(1.0 + C_SQR - C_SQR * wx * wx), wy / np.sqrt(1.0 + C_SQR - C_SQR * wy * wy)
    one = np.ones_like(qx)
    local = {0: [-one, -qy, qx], 1: [qx, -qy, one], 2: [qx, one, qy], 3: [one, -qx, qy], 4: [qy, -qx, -one], 5: [qy, -one, qx]}[side]
    return _normalize3(local)


def model_axes(model):
    kind, a, b = int(model.kind), float(model.a), float(model.b)
    return [a, b, a] if kind == 2 else [a, a, a]


def mesh_normal(model, local):
    """VN of WORLD NORMAL step 2 from a local position: 3 arrays of f32"""
    if int(model.kind) == 0:
        n = len(local[0])
        return [np.zeros(n, np.float32), np.ones(n, np.float32), np.zeros(n, np.float32)]
    scale = model_axes(model)
    return [v.astype(np.float32) for v in _normalize3([local[k] / scale[k] for k in range(3)])]


def world_normal(model, side, s, vn):
    """norm3f(W(s)) of WORLD NORMAL steps 3 and 4 with the tile's side as the face"""
    if int(model.kind) == 0:
        return NM.norm3f([s[0], s[2], s[1]])
    N = NM.norm3f(vn)
    face_up = [np.full(len(s[0]), NM.FACE_UP[side, k], np.float32) for k in range(3)]
    tan = NM.cross(face_up, N)
    bit = NM.cross(N, tan)
    return NM.norm3f([(tan[k] * s[0] + bit[k] * s[1]) + N[k] * s[2] for k in range(3)])


def scatter_tile(model, h_tile, b, coord, rules, seed=0, jitter=1.0, mask_tile=None, reached=None):
    """one listed tile -> (its instances, DTYPE, in the definition's order; its no-data cells)"""
    side, lod, X, Y = coord
    d = decide(model, h_tile, b, coord, rules, seed, jitter, mask_tile, reached)
    at = np.flatnonzero(d["rule"] >= 0)  # (j major, then i: the cells' own order)
    out = np.zeros(len(at), DTYPE)
    rule = d["rule"][at]
    fields = [rule_fields(r) for r in rules]
    lo = np.array([f["scale"][0] for f in fields], np.float32)[rule]
    hi = np.array([f["scale"][1] for f in fields], np.float32)[rule]
    k = d["key"][at]
    out["rule"] = rule
    out["cell"][:, 0], out["cell"][:, 1] = d["gx"][at], d["gy"][at]
    out["scale"] = lo + (hi - lo) * unit(draw(k, 3))
    out["yaw"] = F(6.2831855) * unit(draw(k, 4))
    tiles_per_side = float(1 << lod)
    cu = [(float(X) + d["uv"][0][at].astype(np.float64)) / tiles_per_side, (float(Y) + d["uv"][1][at].astype(np.float64)) / tiles_per_side]
    for n in range(len(at)):
        out["position"][n] = O.coordinate_world_position(model, side, (cu[0][n], cu[1][n]), float(d["h"][at][n]))
    s = [d["s"][k3][at].astype(np.float32) for k3 in range(3)]
    normal = world_normal(model, side, s, mesh_normal(model, local_position(model, side, cu)))
    for k3 in range(3):
        out["normal"][:, k3] = normal[k3]
    return out, int(d["no_data"].sum())


def scatter(model, h_tiles, b, coords, rules, seed=0, jitter=1.0, mask_tiles=None, cache=None, reached=None):
    """the whole call on listed coords -> (instances, first (len + 1) uint64, stats as the binding's dict without launches and written).
    cache: a dict that keeps the tiles' results between calls with the same other arguments (a list may name a tile often)"""
    cache = {} if cache is None else cache
    parts, first, no_data = [], [0], 0
    for coord in coords:
        coord = tuple(int(v) for v in coord)
        if coord not in cache:
            cache[coord] = scatter_tile(model, h_tiles[coord], b, coord, rules, seed, jitter, None if mask_tiles is None else mask_tiles[coord], reached)
        inst, holes = cache[coord]
        parts.append(inst)
        no_data += holes
        first.append(first[-1] + len(inst))
    instances = np.concatenate(parts) if parts else np.zeros(0, DTYPE)
    c = next(iter(h_tiles.values())).shape[0] - 2 * b if h_tiles else 0
    per_rule = [int((instances["rule"] == k).sum()) for k in range(MAX_RULES)]
    stats = dict(total=len(instances), cells=len(parts) * c * c, cells_no_data=no_data, per_rule=per_rule)
    return instances, np.array(first, np.uint64), stats

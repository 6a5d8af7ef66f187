"""The definition of the surface normals (include/bevy_terrain_amd.h: TILE NORMAL, WORLD NORMAL, NORMAL MAP) written once more on the CPU in
numpy, binary32 where the header says binary32, every operation in the header's order.  What the definition takes over from
bt_tile_tree_sample_attachment comes from the oracle (tests/_oracle.py): (lod, ratio) from TileTree.compute_blend, the entries from
TileTree.read(), the side and uv of a surface position from O.coordinate_from_world_position, the ellipsoid's projection from
O.project_point_ellipsoid.  Nothing of the package under test is imported."""
import numpy as np

import _oracle as O

F = np.float32
INVALID = 0xFFFFFFFF


def f32(x):
    return np.asarray(x, dtype=np.float32)


def dot3f(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def norm3f(v):
    with np.errstate(all="ignore"):
        r = F(1.0) / np.sqrt(dot3f(v, v))
        return [v[0] * r, v[1] * r, v[2] * r]


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def enc(v):
    v = f32(v)
    return np.floor(F(0.5) + F(255.0) * np.clip(F(0.5) + F(0.5) * v, F(0.0), F(1.0))).astype(np.uint8)


def model_scale(model):
    kind, a, b = int(model.kind), float(model.a), float(model.b)
    return a / 2.0 if kind == 0 else (a if kind == 1 else (a + b) / 2.0)


def side_length(model):
    scale = F(model_scale(model))
    return scale if int(model.kind) == 0 else (F(3.14159265359) / F(4.0)) * scale


def stack_layers(layers, texture_size):
    """{atlas_index: (T, T) uint16} -> (max index + 1, T, T) uint16, zeros where the dict has no layer"""
    out = np.zeros(((max(layers) + 1) if layers else 1, texture_size, texture_size), np.uint16)
    for i, texels in layers.items():
        out[i] = texels
    return out


def tap(stack, layer, p, q, seen=None):
    """one tap at texture uv (p, q) of layers `layer` (arrays of one length): steps 1 - 8 of the definition.  seen: a list that receives
    which elements took the tap's edge paths (see edge_counts); the values do not depend on it"""
    T = stack.shape[1]
    p, q, layer = f32(p), f32(q), np.asarray(layer, dtype=np.int64)
    tx, ty = p * F(T) - F(0.5), q * F(T) - F(0.5)
    rx, ry = np.fmod(tx, F(1.0)), np.fmod(ty, F(1.0))
    ix, iy = np.trunc(tx).astype(np.int64), np.trunc(ty).astype(np.int64)
    if seen is not None:
        seen.append(dict(negative=(tx < 0) | (ty < 0), high=(ix + 1 > T - 1) | (iy + 1 > T - 1), minus_one=(ix == -1) | (iy == -1)))

    def texel(x, y):  # the exact unorm16 -> f32: the correctly rounded quotient
        raw = stack[layer, np.clip(iy + y, 0, T - 1), np.clip(ix + x, 0, T - 1)]
        return raw.astype(np.float32) / F(65535.0)

    v00, v01, v10, v11 = texel(0, 0), texel(0, 1), texel(1, 0), texel(1, 1)
    a = v00 + (v01 - v00) * ry
    b = v10 + (v11 - v10) * ry
    return a + (b - a) * rx


def taps(stack, border_size, layer, uv, o=None, seen=None):
    """the four taps (left, up, right, down) of centre uv (2 arrays); o: the offset in texture uv (default: the definition's 0.5 / c)"""
    T = stack.shape[1]
    c = T - 2 * border_size
    scale, offset = F(c) / F(T), F(border_size) / F(T)
    o = F(0.5) / F(c) if o is None else F(o)
    ux, uy = f32(uv[0]) * scale + offset, f32(uv[1]) * scale + offset
    return tap(stack, layer, ux - o, uy, seen), tap(stack, layer, ux, uy - o, seen), tap(stack, layer, ux + o, uy, seen), tap(stack, layer, ux, uy + o, seen)


def tile_normal(model, stack, border_size, layer, lod, uv, edges=None):
    """TILE NORMAL s for arrays of (layer, lod, uv); a layer >= len(stack) (nothing loaded) gives (0, 0, 1).  edges: a dict whose
    "negative" / "high" / "minus_one" arrays are or-ed with the elements that hold a layer and one of whose four taps has a negative
    coordinate t / a pair first + 1 beyond T - 1 / a first texel of -1 after the truncation"""
    T = stack.shape[1]
    c = T - 2 * border_size
    layer, lod = np.asarray(layer, dtype=np.int64), np.asarray(lod, dtype=np.int64)
    held = layer < len(stack)
    safe_layer, safe_lod = np.where(held, layer, 0), np.where(held, lod, 0)
    lo, hi = F(model.min_height), F(model.max_height)
    seen = None if edges is None else []
    left, up, right, down = [lo + (hi - lo) * v for v in taps(stack, border_size, safe_layer, uv, seen=seen)]
    if edges is not None:
        for name in ("negative", "high", "minus_one"):
            edges[name] = edges[name] | (held & np.logical_or.reduce([t[name] for t in seen]))
    dist = side_length(model) / (F(c) * np.ldexp(F(1.0), safe_lod).astype(np.float32))
    s = norm3f([left - right, down - up, dist + np.zeros_like(left)])
    return [np.where(held, s[0], F(0.0)), np.where(held, s[1], F(0.0)), np.where(held, s[2], F(1.0))]


def tile_normal_map(model, texels, border_size, lod):
    """NORMAL MAP of one tile ((T, T) uint16) -> (c, c, 4) uint8"""
    T = texels.shape[0]
    c = T - 2 * border_size
    stack = texels[None, :, :]
    j, i = np.meshgrid(np.arange(c), np.arange(c), indexing="ij")
    uv = [(i.ravel().astype(np.float32) + F(0.5)) / F(c), (j.ravel().astype(np.float32) + F(0.5)) / F(c)]
    s = tile_normal(model, stack, border_size, np.zeros(c * c, np.int64), np.full(c * c, lod), uv)
    out = np.stack([enc(s[0]), enc(s[1]), enc(s[2]), np.full(c * c, 255, np.uint8)], axis=1).reshape(c, c, 4)
    out[texels[border_size:border_size + c, border_size:border_size + c] == 0] = (128, 128, 255, 0)
    return out


# ---- WORLD NORMAL ------------------------------------------------------------------------------------------------------------------------

def _dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _normalize3(a):
    r = 1.0 / np.sqrt(_dot3(a, a))
    return [a[0] * r, a[1] * r, a[2] * r]


def surface_and_mesh_normal(model, pts, approximate_height):
    """steps 1 and 2 (f64): surface positions (n, 3) and VN (3 arrays of f32) of world points (n, 3)"""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    p = [pts[:, 0].copy(), pts[:, 1].copy(), pts[:, 2].copy()]
    pos = [float(model.position[i]) for i in range(3)]
    kind, a, b = int(model.kind), float(model.a), float(model.b)
    scale = [a, b, a] if kind == 2 else [a, a, a]
    height = float(np.float32(approximate_height))
    with np.errstate(all="ignore"):
        if kind == 0:
            q = [(p[i] - pos[i]) / scale[i] for i in range(3)]
            local = [1.0 * q[0], 0.0 * q[1], 1.0 * q[2]]
            up = [np.zeros_like(p[0]), np.ones_like(p[0]), np.zeros_like(p[0])]
            vn = [np.zeros(len(pts), np.float32), np.ones(len(pts), np.float32), np.zeros(len(pts), np.float32)]
        else:
            if kind == 1:
                local = _normalize3([(p[i] - pos[i]) / scale[i] for i in range(3)])
            else:
                e = np.array([p[i] - pos[i] for i in range(3)]).T
                s = np.array([O.project_point_ellipsoid((a, a, b), tuple(row)) for row in e]).reshape(-1, 3)
                local = _normalize3([(s[:, i] - pos[i]) / scale[i] for i in range(3)])
            up = local
            vn = [v.astype(np.float32) for v in _normalize3([local[i] / scale[i] for i in range(3)])]
        n = _normalize3([scale[i] * up[i] for i in range(3)])
        surface = np.stack([(scale[i] * local[i] + pos[i]) + height * n[i] for i in range(3)], axis=1)
    return surface, vn


def lookup_tile(entries, lod_count, tree_size, side, uv, tree_lod):
    """TileTree::lookup_tile from the coordinate on -> (atlas_index, atlas_lod, (uv_x, uv_y) f32)"""
    tile_count = float(1 << tree_lod)
    t = [min(uv[0] * tile_count, tile_count - 0.000001), min(uv[1] * tile_count, tile_count - 0.000001)]
    ix, iy = int(t[0]), int(t[1])
    index, lod = entries[((side * lod_count + tree_lod) * tree_size + ix % tree_size) * tree_size + iy % tree_size]
    if lod == INVALID:
        return INVALID, INVALID, (F(0.0), F(0.0))
    div = float(1 << (tree_lod - int(lod)))
    q = [t[0] / div, t[1] / div]
    return int(index), int(lod), (F(q[0] - np.trunc(q[0])), F(q[1] - np.trunc(q[1])))


FACE_UP = np.array([(0, 1, 0), (0, 1, 0), (0, 0, -1), (0, 0, -1), (-1, 0, 0), (-1, 0, 0)], np.float32)


def world_normals(model, otree, approximate_height, texture_size, border_size, layers, pts):
    """WORLD NORMAL of world points (n, 3) against an oracle TileTree in its current state (its approximate height is passed: the oracle
    does not hand it back) and the layers {atlas_index: texels} -> ((n, 3) f32 normals, (n,) f32 up_dot, details)"""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    n = len(pts)
    finite = np.isfinite(pts).all(axis=1)
    safe = np.where(finite[:, None], pts, np.array([float(model.position[i]) for i in range(3)]) + [0.3, 1.0, 0.2])
    surface, vn = surface_and_mesh_normal(model, safe, approximate_height)
    stack = stack_layers(layers, texture_size)
    entries = otree.read()[0]
    lods, ts = otree.lod_count, int(otree.view_config.tree_size)
    spherical = int(model.kind) != 0
    side = np.zeros(n, np.int64)
    ratio = np.zeros(n, np.float32)
    look = [dict(layer=np.zeros(n, np.int64), lod=np.zeros(n, np.int64), u=np.zeros(n, np.float32), v=np.zeros(n, np.float32)) for _ in range(2)]
    for r in range(n):
        s, uv = O.coordinate_from_world_position(model, tuple(surface[r]))
        lod, ratio[r] = otree.compute_blend(tuple(surface[r]))
        side[r] = s
        for k in range(2 if ratio[r] > 0 else 1):
            look[k]["layer"][r], look[k]["lod"][r], (look[k]["u"][r], look[k]["v"][r]) = lookup_tile(entries, lods, ts, s, uv, lod - k)
    N = norm3f(vn)
    if spherical:
        face_up = [FACE_UP[side, k] for k in range(3)]
        tan = cross(face_up, N)
        bit = cross(N, tan)

    def through_tbn(s):
        if not spherical:
            return [s[0], s[2], s[1]]
        return [(tan[k] * s[0] + bit[k] * s[1]) + N[k] * s[2] for k in range(3)]

    first = {name: np.zeros(n, bool) for name in ("negative", "high", "minus_one")}  # per position: the edge paths its taps took
    second = {name: np.zeros(n, bool) for name in first}
    with np.errstate(all="ignore"):
        n1 = norm3f(through_tbn(tile_normal(model, stack, border_size, look[0]["layer"], look[0]["lod"], (look[0]["u"], look[0]["v"]), edges=first)))
        n2 = norm3f(through_tbn(tile_normal(model, stack, border_size, look[1]["layer"], look[1]["lod"], (look[1]["u"], look[1]["v"]), edges=second)))
        blended = [np.where(ratio > 0, n1[k] + (n2[k] - n1[k]) * ratio, n1[k]) for k in range(3)]
        unit = norm3f(blended)
        keep = dot3f(blended, blended) > 0
        out = [np.where(keep, unit[k], N[k]) for k in range(3)]
        up_dot = dot3f(out, N)
    normals = np.stack(out, axis=1).astype(np.float32)
    normals[~finite] = 0.0
    up_dot = np.where(finite, up_dot, F(0.0)).astype(np.float32)
    edges = {"tap_" + name: finite & (first[name] | (second[name] & (ratio > 0))) for name in first}  # the second lookup counts where it is blended in
    return normals, up_dot, dict(ratio=ratio, side=side, layer=look[0]["layer"], lod=look[0]["lod"], N=np.stack(N, axis=1), **edges)

"""numpy model of bt_atlas_splat_from_height: the SPLAT section of include/bevy_terrain_amd.h, steps 1 - 7, on {coord: tile} dictionaries.

TEST INFRASTRUCTURE ONLY.  State is _edit_model's: heights {(side, lod, x, y): T x T uint16} and targets {coord: T x T x 4 uint8} of one
atlas.  Step 3's s is _normal_model.tile_normal (the model the normal bake is held to); propagation is _edit_model.propagate and is the
caller's.  All arithmetic is numpy float32, one IEEE rounding per written operation, in the header's order.  A rule is anything with the
fields of bevy_terrain_amd.SplatRule (height, steep(), height_fade, slope_fade, weight, colour); model: an _oracle model (min_height,
max_height and what _normal_model.side_length reads).  Nothing of the package under test is imported."""
import numpy as np

import _normal_model as NM
from _edit_model import _centre
from _render_model import enc8

F = np.float32
WEIGHTS, COLOUR = "weights", "colour"


def clamp01(t):
    """t > 0 ? (t > 1 ? 1 : t) : 0 on an f32 array: a NaN gives 0"""
    with np.errstate(invalid="ignore"):
        return np.where(t > F(0), np.where(t > F(1), F(1), t), F(0)).astype(np.float32)


def sm(t):
    return (t * t) * (F(3.0) - F(2.0) * t)


def band(x, lo, hi, fade):
    """band(x; lo, hi, fade) of step 4 on an f32 array x"""
    x, lo, hi, fade = np.asarray(x, dtype=np.float32), F(lo), F(hi), F(fade)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if fade > 0:
            r = clamp01((x - (lo - fade)) / fade)
            q = clamp01(((hi + fade) - x) / fade)
        else:
            r = np.where(x >= lo, F(1), F(0)).astype(np.float32)
            q = np.where(x <= hi, F(1), F(0)).astype(np.float32)
    return sm(r) * sm(q)


def rule_fields(rule):
    """(height_lo, height_hi, height_fade, steep_lo, steep_hi, steep_fade, weight, colour[3]) as the C struct carries them (binary32)"""
    lo, hi = rule.steep()
    return (F(rule.height[0]), F(rule.height[1]), F(rule.height_fade), F(lo), F(hi), F(rule.slope_fade), F(rule.weight), [F(v) for v in rule.colour])


def tile_s(model, h_tile, b, lod):
    """step 3's s for every centre texel (i, j) of one height tile -> [s.x, s.y, s.z], (c * c,) f32 each, j major"""
    T = h_tile.shape[0]
    c = T - 2 * b
    j, i = np.meshgrid(np.arange(c), np.arange(c), indexing="ij")
    uv = [(i.ravel().astype(np.float32) + F(0.5)) / F(c), (j.ravel().astype(np.float32) + F(0.5)) / F(c)]
    return NM.tile_normal(model, h_tile[None, :, :], b, np.zeros(c * c, np.int64), np.full(c * c, lod), uv)


def height_and_steep(model, h_tile, b, lod):
    """steps 2 and 3 for every centre texel of one height tile -> (h, steep), (c, c) f32 each"""
    c = h_tile.shape[0] - 2 * b
    s = tile_s(model, h_tile, b, lod)
    v = _centre(h_tile, b).astype(np.float32) / F(65535.0)
    lo, hi = F(model.min_height), F(model.max_height)
    h = lo + (hi - lo) * v
    steep = F(1.0) - s[2].astype(np.float32).reshape(c, c)
    return h.astype(np.float32), steep.astype(np.float32)


def splat_texels(raw, h, steep, mode, rules, fallback, reached=None):
    """steps 1 and 4 - 7 for arrays of texels: raw heights, h and steep of one shape -> (..., 4) uint8.  reached (a dict, optional) counts
    "holes": texels with raw == 0, "fallback": data texels no rule reaches, "zero_rule": data texels step 7 brought back, "mixed": data
    texels at least two rules reach, "partial": data texels a rule reaches with a weight strictly between 0 and its `weight`"""
    assert mode in (WEIGHTS, COLOUR) and 1 <= len(rules) <= (4 if mode == WEIGHTS else 8)
    w = []
    total = np.zeros(raw.shape, np.float32)
    for rule in rules:
        hlo, hhi, hfade, slo, shi, sfade, weight, _ = rule_fields(rule)
        wk = (weight * band(h, hlo, hhi, hfade)) * band(steep, slo, shi, sfade)
        total = total + wk
        w.append(wk.astype(np.float32))
    out = np.zeros(raw.shape + (4,), np.uint8)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if mode == WEIGHTS:
            for k, wk in enumerate(w):
                out[..., k] = enc8(wk / total)
        else:
            for ch in range(3):
                acc = np.zeros(raw.shape, np.float32)
                for rule, wk in zip(rules, w):
                    acc = acc + wk * rule_fields(rule)[7][ch]
                out[..., ch] = enc8(acc / total)
            out[..., 3] = 255
    reaches = total > 0
    out[~reaches] = np.array(fallback, np.uint8)
    data = raw != 0
    emptied = data & (out[..., :3] == 0).all(axis=-1)
    out[..., 0] = np.where(emptied, 1, out[..., 0])
    out[~data] = 0
    if reached is not None:
        hit = np.sum([wk > 0 for wk in w], axis=0)
        partial = np.logical_or.reduce([(wk > 0) & (wk < rule_fields(rule)[6]) for rule, wk in zip(rules, w)])
        for name, mask in (("holes", ~data), ("fallback", data & ~reaches), ("zero_rule", emptied), ("mixed", data & (hit >= 2)), ("partial", data & partial),
                           ("data", data)):
            reached[name] = reached.get(name, 0) + int(mask.sum())
    return out


def apply_splat(h_tiles, g_tiles, model, lod, side, rect, mode, rules, fallback, b, reached=None):
    """the call's first step on a copy of g_tiles: the centre texels of the existing tiles of (side, lod) inside rect = (x0, y0, w, h)
    (mosaic texels) derived from the same texels of h_tiles; nothing is propagated"""
    x0, y0, w, h = rect
    out = {k: v.copy() for k, v in g_tiles.items()}
    for coord, g in out.items():
        if coord[0] != side or coord[1] != lod:
            continue
        centre = _centre(g, b)
        c = centre.shape[0]
        ox, oy = coord[2] * c, coord[3] * c
        xa, xb, ya, yb = max(x0, ox), min(x0 + w, ox + c), max(y0, oy), min(y0 + h, oy + c)
        if xa >= xb or ya >= yb:
            continue
        height, steep = height_and_steep(model, h_tiles[coord], b, lod)
        part = (slice(ya - oy, yb - oy), slice(xa - ox, xb - ox))
        centre[part] = splat_texels(_centre(h_tiles[coord], b)[part], height[part], steep[part], mode, rules, fallback, reached)
    return out


def rect_tiles(lod, side, rect, c):
    """the tile coordinates of `lod` a non-empty rectangle meets"""
    x0, y0, w, h = rect
    return {(side, lod, x, y) for y in range(y0 // c, (y0 + h - 1) // c + 1) for x in range(x0 // c, (x0 + w - 1) // c + 1)}

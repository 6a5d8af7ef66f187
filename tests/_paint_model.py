"""numpy model of bt_atlas_paint and bt_atlas_read_region, beside tests/_edit_model.py (whose propagate() restores F for Rgba8 as well).

TEST INFRASTRUCTURE ONLY.  State is _edit_model's: {(side, lod, x, y): T x T x 4 uint8 array} (R16 tiles for read_region too).  All paint
arithmetic is numpy float32, one IEEE rounding per written operation: the PAINT section of include/bevy_terrain_amd.h line by line.
A stamp is anything with the fields of bevy_terrain_amd.PaintStamp (center, radius, color, opacity, mode, falloff, side, channel_mask()).
"""
import numpy as np

from _edit_model import F32, _centre


def paint_texels(t, gx, gy, stamp, reached=None):
    """one stamp on Rgba8 texels t (..., 4) at mosaic positions (gx, gy) (integer arrays of t's shape without the channel axis).
    reached (a dict, optional) counts "under_disc": texels that pass d2 < r2, "holes_under_disc": those of them without data,
    "zero_rule": data texels the stamp took to rgb == 0 and the last line of the definition brought back"""
    data = (t[..., :3] != 0).any(axis=-1)
    dx = gx.astype(F32) - F32(stamp.center[0])
    dy = gy.astype(F32) - F32(stamp.center[1])
    d2 = (dx * dx) + (dy * dy)
    with np.errstate(over="ignore"):
        r2 = F32(stamp.radius) * F32(stamp.radius)
    disc = d2 < r2
    inside = disc & data
    if stamp.falloff == "hard":
        w = np.ones(d2.shape, F32)
    else:
        with np.errstate(invalid="ignore", divide="ignore"):
            q = d2 / r2
        s = F32(1) - q
        w = s * s
    a = F32(stamp.opacity) * w
    mask = stamp.channel_mask()
    out = t.copy()
    for k in range(4):
        if not (mask >> k) & 1:
            continue
        c = t[..., k].astype(F32) / F32(255)
        colour = F32(stamp.color[k])
        with np.errstate(over="ignore", invalid="ignore"):
            cn = c + (colour - c) * a if stamp.mode == "blend" else c + colour * a
            new = np.floor(F32(0.5) + F32(255) * np.clip(cn, F32(0), F32(1)))
        out[..., k] = np.where(inside, new, t[..., k]).astype(np.uint8)
    emptied = inside & (out[..., :3] == 0).all(axis=-1)
    for k in range(3):
        if (mask >> k) & 1:
            out[..., k] = np.where(emptied, 1, out[..., k])
    if reached is not None:
        for name, hit in (("under_disc", disc), ("holes_under_disc", disc & ~data), ("zero_rule", emptied)):
            reached[name] = reached.get(name, 0) + int(hit.sum())
    return out


def apply_paint(tiles, lod, stamps, b, reached=None):
    """the stamps, in list order, on the centre texels of the existing tiles of `lod` (a copy; nothing is propagated)"""
    out = {k: v.copy() for k, v in tiles.items()}
    for coord, tile in out.items():
        if coord[1] != lod:
            continue
        centre = _centre(tile, b)
        c = centre.shape[0]
        gy, gx = np.mgrid[0:c, 0:c]
        gx, gy = gx + coord[2] * c, gy + coord[3] * c
        for s in stamps:
            if s.side == coord[0]:
                centre[...] = paint_texels(centre, gx, gy, s, reached)
    return out


def read_region(tiles, lod, side, x0, y0, w, h, b):
    """(the w x h rectangle of centre texels at mosaic (x0, y0) of `lod` on `side`, zeros over absent tiles; the number of absent tiles the
    rectangle meets).  R16 ((h, w) uint16) and Rgba8 ((h, w, 4) uint8) alike."""
    some = next(iter(tiles.values()))
    c = some.shape[0] - 2 * b
    out = np.zeros((h, w) + some.shape[2:], some.dtype)
    missing = 0
    if w == 0 or h == 0:
        return out, 0
    for ty in range(y0 // c, (y0 + h - 1) // c + 1):
        for tx in range(x0 // c, (x0 + w - 1) // c + 1):
            tile = tiles.get((side, lod, tx, ty))
            if tile is None:
                missing += 1
                continue
            ox, oy = tx * c, ty * c
            xa, xb, ya, yb = max(x0, ox), min(x0 + w, ox + c), max(y0, oy), min(y0 + h, oy + c)
            out[ya - y0:yb - y0, xa - x0:xb - x0] = _centre(tile, b)[ya - oy:yb - oy, xa - ox:xb - ox]
    return out, missing

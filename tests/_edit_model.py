"""numpy model of in-place editing (bt_atlas_edit_height / bt_atlas_write_region), tile based.

TEST INFRASTRUCTURE ONLY.  State is {(side, lod, x, y): T x T uint16 array (R16) or T x T x 4 uint8 array (Rgba8)} plus the border size and
the spherical flag.  The definition is the invariant F of include/bevy_terrain_amd.h:
  1. a tile none of whose four children exists is primary: its centre texels are data;
  2. any other tile's centre is downsample (downsample.wgsl:12-40) of its children's centres, an absent child reading as 0;
  3. every tile's apron is stitch (stitch.wgsl:53-118) of its neighbours' centres, a missing neighbour clamping into the own centre;
  4. mips come from _oracle.generate_mipmaps (not restated here).
propagate() recomputes 2 and 3 from the primary centres; test_edit_model.py pins it against the committed goldens (the reference's own
WGSL, executed), so it is a second statement of the oracle's downsample + stitch, not a copy of the kernels.  Topology comes from
_oracle.children / _oracle.neighbours.  All brush arithmetic is numpy float32: one IEEE rounding per written operation.
"""
import numpy as np

import _oracle as O

F32 = np.float32
INVALID = (O.INVALID,) * 4

# stitch.wgsl:12-51: per output axis 0 = +x, 1 = +y, 2 = T-1-x, 3 = T-1-y of the input; index (6 + other - own) % 6; (x code, y code)
_EVEN = [(0, 1), (0, 1), (3, 0), (3, 2), (1, 2), (0, 1)]
_ODD = [(0, 1), (0, 1), (1, 2), (1, 0), (3, 0), (0, 1)]


def project_to_side(x, y, T, own, other):
    cx, cy = (_EVEN if own % 2 == 0 else _ODD)[(6 + other - own) % 6]
    v = (x, y, T - 1 - x, T - 1 - y)
    return v[cx], v[cy]


def _centre(tile, b):
    T = tile.shape[0]
    return tile[b:T - b, b:T - b]


def downsample_block(child_centre):
    """one child's c x c centre -> the (c/2) x (c/2) quadrant of its parent; taps in the order (dx, dy) = (0,0), (0,1), (1,0), (1,1)"""
    C = child_centre
    taps = [C[0::2, 0::2], C[1::2, 0::2], C[0::2, 1::2], C[1::2, 1::2]]  # arrays are [y, x]
    if C.ndim == 2:
        value = np.zeros(taps[0].shape, F32)
        count = np.zeros(taps[0].shape, F32)
        for t in taps:
            has = t != 0
            value = np.where(has, value + t.astype(F32) / F32(65535), value)
            count = np.where(has, count + F32(1), count)
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = value / count
        out = np.floor(F32(0.5) + F32(65535) * np.clip(mean, F32(0), F32(1)))
        return np.where(count == 0, 0, out).astype(np.uint16)
    value = np.zeros(taps[0].shape, F32)
    count = np.zeros(taps[0].shape[:2], F32)
    for t in taps:
        has = (t[..., :3] != 0).any(axis=-1)  # rgb != 0, alpha ignored
        value = np.where(has[..., None], value + t.astype(F32) / F32(255), value)
        count = np.where(has, count + F32(1), count)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = value / count[..., None]
    out = np.floor(F32(0.5) + F32(255) * np.clip(mean, F32(0), F32(1)))
    return np.where((count == 0)[..., None], 0, out).astype(np.uint8)


def stitch_tile(tiles, coord, b, spherical):
    """the apron of tiles[coord] from the CENTRES of its neighbours (stitch_source of the library, restated per pixel)"""
    tile = tiles[coord]
    T = tile.shape[0]
    c, o = T - 2 * b, T - b
    nb = O.neighbours(coord, spherical)  # N, E, S, W, NW, NE, SE, SW == regions 0 top, 1 right, 2 bottom, 3 left, 4 TL, 5 TR, 6 BR, 7 BL
    out = tile.copy()
    for py in range(T):
        ry = -1 if py < b else (1 if py >= o else 0)
        for px in range(T):
            rx = -1 if px < b else (1 if px >= o else 0)
            if rx == 0 and ry == 0:
                continue
            region = {(0, -1): 0, (1, 0): 1, (0, 1): 2, (-1, 0): 3, (-1, -1): 4, (1, -1): 5, (1, 1): 6, (-1, 1): 7}[(rx, ry)]
            n = nb[region]
            if n == INVALID or n not in tiles:  # repeat_data: clamp into the own centre
                out[py, px] = tile[min(max(py, b), o - 1), min(max(px, b), o - 1)]
                continue
            sx, sy = project_to_side(px - rx * c, py - ry * c, T, coord[0], n[0])
            out[py, px] = tiles[n][sy, sx] if 0 <= sx < T and 0 <= sy < T else 0
    return out


def propagate(tiles, b, spherical, only=None):
    """F items 2 and 3 applied to a copy of `tiles`: derived centres bottom up, then every apron (only: just the aprons of these tiles).
    A tile whose four children are all absent keeps its centre."""
    out = {k: v.copy() for k, v in tiles.items()}
    for lod in sorted({k[1] for k in out}, reverse=True):
        for coord in [k for k in out if k[1] == lod]:
            kids = O.children(coord)
            if not any(k in out for k in kids):
                continue
            T = out[coord].shape[0]
            c = T - 2 * b
            assert c % 2 == 0, "the model (like the library) needs an even centre size"
            h = c // 2
            centre = _centre(out[coord], b)
            for i, k in enumerate(kids):
                qx, qy = (i & 1) * h, (i >> 1) * h
                if k in out:
                    centre[qy:qy + h, qx:qx + h] = downsample_block(_centre(out[k], b))
                else:
                    centre[qy:qy + h, qx:qx + h] = 0
    if b > 0:
        stitched = {coord: stitch_tile(out, coord, b, spherical) for coord in (out if only is None else only)}
        out.update(stitched)
    return out


def stamp_texels(t, gx, gy, stamp):
    """one stamp on raw R16 texels t at mosaic positions (gx, gy) (integer arrays of t's shape): the header's BRUSH section line by line"""
    dx = gx.astype(F32) - F32(stamp.center[0])
    dy = gy.astype(F32) - F32(stamp.center[1])
    d2 = (dx * dx) + (dy * dy)
    with np.errstate(over="ignore"):
        r2 = F32(stamp.radius) * F32(stamp.radius)
    inside = (d2 < r2) & (t != 0)
    if stamp.falloff == "hard":
        w = np.ones(t.shape, F32)
    else:
        q = d2 / r2
        s = F32(1) - q
        w = s * s
    h = t.astype(F32) / F32(65535)
    with np.errstate(over="ignore", invalid="ignore"):
        if stamp.mode == "flatten":
            hn = h + (F32(stamp.amount) - h) * w
        else:
            hn = h + F32(stamp.amount) * w
    new = np.maximum(1, np.floor(F32(0.5) + F32(65535) * np.clip(hn, F32(0), F32(1))))
    return np.where(inside, new, t).astype(np.uint16)


def apply_stamps(tiles, lod, stamps, b):
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
                centre[...] = stamp_texels(centre, gx, gy, s)
    return out


def stamp_tiles(stamps, lod, c, sides=None):
    """the tile coordinates of `lod` that meet a stamp's box [floor(center - radius), ceil(center + radius)], clipped to the face"""
    n = (1 << lod) * c
    met = set()
    for s in stamps:
        lo = [max(0, int(np.floor(float(s.center[k]) - float(s.radius)))) for k in range(2)]
        hi = [min(n - 1, int(np.ceil(float(s.center[k]) + float(s.radius)))) for k in range(2)]
        if lo[0] > hi[0] or lo[1] > hi[1]:
            continue
        for y in range(lo[1] // c, hi[1] // c + 1):
            for x in range(lo[0] // c, hi[0] // c + 1):
                met.add((s.side, lod, x, y))
    return met


def write_region(tiles, lod, side, x0, y0, texels, b):
    """texels ((h, w) or (h, w, 4)) verbatim over the centre texels at mosaic (x0, y0) of `lod` on `side`; absent tiles are skipped"""
    out = {k: v.copy() for k, v in tiles.items()}
    h, w = texels.shape[:2]
    for coord, tile in out.items():
        if coord[0] != side or coord[1] != lod:
            continue
        centre = _centre(tile, b)
        c = centre.shape[0]
        ox, oy = coord[2] * c, coord[3] * c
        xa, xb, ya, yb = max(x0, ox), min(x0 + w, ox + c), max(y0, oy), min(y0 + h, oy + c)
        if xa < xb and ya < yb:
            centre[ya - oy:yb - oy, xa - ox:xb - ox] = texels[ya - y0:yb - y0, xa - x0:xb - x0]
    return out


def region_tiles(lod, side, x0, y0, w, h, c):
    return {(side, lod, x, y) for y in range(y0 // c, (y0 + h - 1) // c + 1) for x in range(x0 // c, (x0 + w - 1) // c + 1)}


def allowed_changed(tiles, edited, spherical):
    """{edited tiles that exist, their existing ancestors (the chain ends at a missing parent), the existing neighbours of all those}"""
    written = set()
    for coord in edited:
        if coord not in tiles:
            continue
        written.add(coord)
        while coord[1] > 0:
            coord = (coord[0], coord[1] - 1, coord[2] >> 1, coord[3] >> 1)
            if coord not in tiles:
                break
            written.add(coord)
    out = set(written)
    for coord in written:
        out |= {n for n in O.neighbours(coord, spherical) if n in tiles}
    return out

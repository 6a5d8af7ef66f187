"""numpy model of bt_atlas_smooth_height (the SMOOTHING section of include/bevy_terrain_amd.h), on the tiles dictionary of _edit_model.

TEST INFRASTRUCTURE ONLY.  Steps 1 - 3 of the definition: the box sums come from the tile's own layer array, apron included, as it stood
before the call; sum and n are integers, m is ONE binary32 division of two exact operands, the stamps run in list order on a running
value.  Nothing is propagated here: _edit_model.propagate restores F afterwards, _edit_model.stamp_tiles / allowed_changed give the tiles a
call may reach (the stamp's box is the brush's)."""
from collections import namedtuple

import numpy as np

import _edit_model as EM
from _edit_model import allowed_changed, propagate, stamp_tiles  # noqa: F401  (re-exported: the tests take them from here)

F32 = np.float32
Stamp = namedtuple("Stamp", "center radius strength falloff side", defaults=(1.0, "smooth", 0))


def box_mean(layer, b, k):
    """(m, n) over the c x c centre of a T x T layer: m float32 (0 where n == 0), n the number of data texels in the (2k + 1)^2 box"""
    assert 1 <= k <= b
    T = layer.shape[0]
    c = T - 2 * b
    total = np.zeros((c, c), np.int64)
    n = np.zeros((c, c), np.int64)
    for dy in range(-k, k + 1):
        for dx in range(-k, k + 1):
            win = layer[b + dy:b + dy + c, b + dx:b + dx + c]
            total += win
            n += win != 0
    assert total.max() < 1 << 24
    with np.errstate(invalid="ignore", divide="ignore"):
        m = total.astype(F32) / (F32(65535) * n.astype(F32))
    return np.where(n == 0, F32(0), m).astype(F32), n


def smooth_texels(t, m, gx, gy, stamp):
    """one stamp on the running raw values t (uint16 array) with the box means m of the state before the call"""
    dx = gx.astype(F32) - F32(stamp.center[0])
    dy = gy.astype(F32) - F32(stamp.center[1])
    d2 = (dx * dx) + (dy * dy)
    with np.errstate(over="ignore"):
        r2 = F32(stamp.radius) * F32(stamp.radius)
    inside = (d2 < r2) & (t != 0)
    if stamp.falloff == "hard":
        w = np.ones(t.shape, F32)
    else:
        with np.errstate(over="ignore", invalid="ignore"):
            q = d2 / r2
            s = F32(1) - q
            w = s * s
    with np.errstate(over="ignore", invalid="ignore"):
        a = F32(stamp.strength) * w
        h = t.astype(F32) / F32(65535)
        hn = h + (m - h) * a
        new = np.maximum(1, np.floor(F32(0.5) + F32(65535) * np.clip(hn, F32(0), F32(1))))
    return np.where(inside, new, t).astype(np.uint16)


def apply_smooth(tiles, lod, stamps, b, k):
    """the stamps on the centre texels of the existing tiles of `lod` (a copy; nothing is propagated).  Every m is taken from `tiles`."""
    out = {key: v.copy() for key, v in tiles.items()}
    for coord, tile in out.items():
        if coord[1] != lod:
            continue
        m, _ = box_mean(tiles[coord], b, k)
        centre = EM._centre(tile, b)
        c = centre.shape[0]
        gy, gx = np.mgrid[0:c, 0:c]
        gx, gy = gx + coord[2] * c, gy + coord[3] * c
        for s in stamps:
            if s.side == coord[0]:
                centre[...] = smooth_texels(centre, m, gx, gy, s)
    return out


def apply_smooth_in_place(tiles, lod, stamps, b, k):
    """what the definition is NOT: texels taken in row-major order, each box read from the array being written (Gauss-Seidel).  Only for
    showing that the snapshot property is observable."""
    out = {key: v.copy() for key, v in tiles.items()}
    for coord, tile in out.items():
        if coord[1] != lod:
            continue
        c = tile.shape[0] - 2 * b
        for j in range(c):
            for i in range(c):
                py, px = b + j, b + i
                if tile[py, px] == 0:
                    continue
                box = tile[py - k:py + k + 1, px - k:px + k + 1]
                m = F32(int(box.sum(dtype=np.int64))) / (F32(65535) * F32(int((box != 0).sum())))
                one = np.array([[tile[py, px]]], np.uint16)
                gx, gy = np.array([[coord[2] * c + i]]), np.array([[coord[3] * c + j]])
                for s in stamps:
                    if s.side == coord[0]:
                        one = smooth_texels(one, m, gx, gy, s)
                tile[py, px] = one[0, 0]
    return out

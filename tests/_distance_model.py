"""The DISTANCE section of include/bevy_terrain_amd.h by brute force in numpy: every cell against every seed, the argmin over the seeds in
ascending index.  TEST INFRASTRUCTURE ONLY (pinned by tests/test_distance_model.py).

Texels: (h, w) uint16 for R16, (h, w, 4) uint8 for Rgba8.  Everything is integer arithmetic; the bake byte is computed in Python integers."""
import math

import numpy as np

NONE = 0xFFFFFFFF
FROM_TEXELS, INVERT, BAKE_NEAR = 1, 2, 1
SCHEDULE = ("launches", "edit", "changed")  # the entries of the stats that are not functions of the window


def seed_plane(texels, channel=0, lo=None, hi=None, host=None, invert=False):
    """seed(c) of the header, (h, w) bool; lo / hi None: no BT_DISTANCE_FROM_TEXELS"""
    v = texels.astype(np.int64) if texels.ndim == 2 else texels[:, :, channel].astype(np.int64)
    s = np.zeros(v.shape, bool)
    if lo is not None:
        s |= (lo <= v) & (v <= hi)
    if host is not None:
        s |= np.asarray(host) != 0
    return s ^ bool(invert)


def field(seed):
    """(dist2, nearest, stats) of a (h, w) bool seed plane, by all pairs"""
    h, w = seed.shape
    ys, xs = np.nonzero(seed)  # row-major: ascending index
    stats = dict(cells=h * w, seeds=len(ys), max_dist2=0, sum_dist2=0)
    if not len(ys):
        return np.full((h, w), NONE, np.uint32), np.full((h, w), NONE, np.uint32), stats
    cy, cx = np.mgrid[0:h, 0:w]
    dist2, nearest = np.empty((h, w), np.uint32), np.empty((h, w), np.uint32)
    index = ys.astype(np.int64) * w + xs
    for y in range(h):  # a row of cells at a time: (w, seeds) pairs
        d = (cx[y][:, None] - xs[None, :]).astype(np.int64) ** 2 + (y - ys[None, :]).astype(np.int64) ** 2
        k = np.argmin(d, axis=1)  # the first of the minima: the smallest index
        dist2[y], nearest[y] = d[np.arange(w), k], index[k]
    stats["max_dist2"], stats["sum_dist2"] = int(dist2.max()), int(dist2.astype(np.uint64).sum())
    return dist2, nearest, stats


def bake_byte(dist2, reach, near=False):
    """b(c) of the header for one cell, in Python integers"""
    b = 255 if dist2 == NONE else min(255, math.isqrt((int(dist2) * 65025) // (reach * reach)))
    return 255 - b if near else b


def bake_plane(dist2, reach, near=False):
    values = {int(d): bake_byte(int(d), reach, near) for d in np.unique(dist2)}
    return np.vectorize(values.get, otypes=[np.uint8])(dist2)


def bake(texels, dist2, channel, reach, near=False):
    """the Rgba8 texels (h, w, 4) with byte `channel` replaced"""
    out = texels.copy()
    out[:, :, channel] = bake_plane(dist2, reach, near)
    return out


def separable(seed):
    """(dist2, nearest) by the separable reading of the header: r per column, then the lexicographic minimum over the columns; in Python
    integers, for small windows"""
    h, w = seed.shape
    r = [[None] * w for _ in range(h)]
    for x in range(w):
        rows = [y for y in range(h) if seed[y, x]]
        for y in range(h):
            if rows:
                r[y][x] = min(rows, key=lambda s: (abs(s - y), s))  # the upper one on a tie
    dist2, nearest = np.full((h, w), NONE, np.uint32), np.full((h, w), NONE, np.uint32)
    for y in range(h):
        for x in range(w):
            best = min((((x - i) ** 2 + (y - r[y][i]) ** 2, r[y][i], i) for i in range(w) if r[y][i] is not None), default=None)
            if best is not None:
                dist2[y, x], nearest[y, x] = best[0], best[1] * w + best[2]
    return dist2, nearest

"""The REGIONS section of include/bevy_terrain_amd.h in numpy and Python integers, by another algorithm than the device's union-find: a
breadth-first fill started from each member without a label yet, in row-major order, so the start cell is the smallest cell of its region
and hence its label.  Then the table, the stats and the baked rectangle.  TEST INFRASTRUCTURE ONLY (pinned by tests/test_regions_model.py).

Texels: (h, w) uint16 for R16, (h, w, 4) uint8 for Rgba8."""
from collections import deque

import numpy as np

NONE = 0xFFFFFFFF
FROM_TEXELS, INVERT, EIGHT = 1, 2, 4
SCHEDULE = ("launches", "edit", "changed")  # the entries of the stats that are not functions of the window
REGION_DTYPE = np.dtype([("label", "<u4"), ("area", "<u4"), ("x_min", "<u2"), ("y_min", "<u2"), ("x_max", "<u2"), ("y_max", "<u2"), ("v_min", "<u2"),
                         ("v_max", "<u2"), ("edges", "<u4"), ("v_sum", "<u8")])
# the header's stated layout of bt_region: the size, then the offset of every field
REGION_SIZE, REGION_OFFSETS = 32, dict(label=0, area=4, x_min=8, y_min=10, x_max=12, y_max=14, v_min=16, v_max=18, edges=20, v_sum=24)
RULE_SIZE, BAKE_SIZE, STATS_SIZE = 20, 24, 80

FOUR = ((-1, 0), (0, -1), (0, 1), (1, 0))                 # (dy, dx)
DIAGONALS = ((-1, -1), (-1, 1), (1, -1), (1, 1))


def values(texels, channel=0):
    """v(c) of the header, (h, w) int64"""
    return texels.astype(np.int64) if texels.ndim == 2 else texels[:, :, channel].astype(np.int64)


def member_plane(texels, channel=0, lo=None, hi=None, host=None, invert=False):
    """member(c) of the header, (h, w) bool; lo / hi None: no BT_REGIONS_FROM_TEXELS"""
    v = values(texels, channel)
    m = np.zeros(v.shape, bool)
    if lo is not None:
        m |= (lo <= v) & (v <= hi)
    if host is not None:
        m |= np.asarray(host) != 0
    return m ^ bool(invert)


def labels(member, v, max_step=65535, eight=False):
    """label(c), (h, w) uint32: a fill from every member that has none yet, in row-major order"""
    h, w = member.shape
    m, val = member.tolist(), v.tolist()
    out = [[NONE] * w for _ in range(h)]
    around = FOUR + DIAGONALS if eight else FOUR
    for sy in range(h):
        for sx in range(w):
            if not m[sy][sx] or out[sy][sx] != NONE:
                continue
            start = sy * w + sx
            out[sy][sx] = start
            queue = deque([(sy, sx)])
            while queue:
                y, x = queue.popleft()
                for dy, dx in around:
                    ny, nx = y + dy, x + dx
                    if 0 <= ny < h and 0 <= nx < w and m[ny][nx] and out[ny][nx] == NONE and abs(val[y][x] - val[ny][nx]) <= max_step:
                        out[ny][nx] = start
                        queue.append((ny, nx))
    return np.array(out, dtype=np.uint32).reshape(h, w)


def ids(label):
    """id(c): the rank of label(c) among the labels"""
    present = np.unique(label[label != NONE])
    out = np.full(label.shape, NONE, np.uint32)
    out[label != NONE] = np.searchsorted(present, label[label != NONE]).astype(np.uint32)
    return out


def table(label, v):
    """every region's bt_region, in id order, in Python integers"""
    h, w = label.shape
    lab, val = label.tolist(), v.tolist()
    records = {}
    for y in range(h):
        for x in range(w):
            L = lab[y][x]
            if L == NONE:
                continue
            r = records.setdefault(L, dict(label=L, area=0, x_min=x, y_min=y, x_max=x, y_max=y, v_min=val[y][x], v_max=val[y][x], edges=0, v_sum=0))
            r["area"] += 1
            r["x_min"], r["x_max"], r["y_min"], r["y_max"] = min(r["x_min"], x), max(r["x_max"], x), min(r["y_min"], y), max(r["y_max"], y)
            r["v_min"], r["v_max"], r["v_sum"] = min(r["v_min"], val[y][x]), max(r["v_max"], val[y][x]), r["v_sum"] + val[y][x]
            for dy, dx in FOUR:
                ny, nx = y + dy, x + dx
                r["edges"] += not (0 <= ny < h and 0 <= nx < w) or lab[ny][nx] != L
    out = np.zeros(len(records), REGION_DTYPE)
    for k, L in enumerate(sorted(records)):
        out[k] = tuple(records[L][name] for name in REGION_DTYPE.names)
    return out


def stats(member, regions, region_cap=None, baked=0):
    """bt_regions_stats but tiles_missing and the schedule's entries"""
    largest = int(regions["area"].max()) if len(regions) else 0
    return dict(cells=member.size, members=int(member.sum()), regions=len(regions), regions_written=len(regions) if region_cap is None else min(len(regions), region_cap),
                largest_area=largest, largest_label=int(regions["label"][regions["area"] == largest].min()) if len(regions) else NONE, baked=baked)


def area_plane(label, regions):
    """the area of each cell's region; 0 where the cell is no member"""
    out = np.zeros(label.shape, np.int64)
    for r in regions:
        out[label == r["label"]] = r["area"]
    return out


def bake(texels, label, regions, channel, min_area, max_area, value):
    """(the Rgba8 texels (h, w, 4) with byte `channel` replaced where the bake writes, the number of cells written)"""
    area = area_plane(label, regions)
    where = (label != NONE) & (min_area <= area) & (area <= max_area)
    out = texels.copy()
    out[:, :, channel][where] = value
    return out, int(where.sum())


def solve(texels, channel=0, lo=None, hi=None, host=None, invert=False, max_step=65535, eight=False):
    """(member, label, id, regions, stats) of a window"""
    member, v = member_plane(texels, channel, lo, hi, host, invert), values(texels, channel)
    label = labels(member, v, max_step, eight)
    regions = table(label, v)
    return member, label, ids(label), regions, stats(member, regions)

"""The model of the SHAPES section of include/bevy_terrain_amd.h (bt_atlas_rasterize_shapes, bt_shapes_check) in numpy int64 and Python
integers.  TEST INFRASTRUCTURE ONLY; pinned by tests/test_shapes_model.py against a second restatement and answers worked by hand.

A shape is a dict: a polygon {"contours": [[(x, y), ...], ...], "nonzero": bool, "op": OP, "value": v} or a stroke {"points": [(x, y),
...], "r": half_width, "closed": bool, "op": OP, "value": v}; coordinates are integers in 1/256 cell relative to the window's origin.
Every product of two differences stays below 2^51 and is formed in int64; the one comparison that needs more, (d x e)^2 <= r^2 L, is made
in Python integers."""
import numpy as np

POLYGON, STROKE = 0, 1
NONZERO, CLOSED, MORE = 1, 2, 4
SET, MAX, MIN, ADD, SUB = 0, 1, 2, 3, 4
NONE, NO_ENTRY = 0xFFFF, 0xFFFFFFFF
MAX_SHAPES, MAX_ENTRIES, MAX_VERTICES, MAX_COORD, MAX_HALF_WIDTH, MAX_SIDE, MAX_CELLS = 4096, 65536, 1 << 20, 1 << 23, 1 << 20, 8192, 1 << 22
EMPTY = (1, 1, 0, 0)
SCHEDULE = ("launches",)  # the fields of bt_shapes_stats that are not a function of the input


def polygon(contours, nonzero=False, op=SET, value=1):
    if contours and not isinstance(contours[0][0], (tuple, list)):
        contours = [contours]
    return dict(contours=[[(int(x), int(y)) for x, y in c] for c in contours], nonzero=nonzero, op=op, value=value)


def stroke(points, r, closed=False, op=SET, value=1):
    return dict(points=[(int(x), int(y)) for x, y in points], r=int(r), closed=closed, op=op, value=value)


def pack(shapes):
    """the list as the call takes it: vertices (N, 2) int32 and entries (E, 8) uint32 in the field order of bt_shape"""
    vertices, entries = [], []
    for s in shapes:
        if "contours" in s:
            for i, c in enumerate(s["contours"]):
                flags = (NONZERO if s["nonzero"] else 0) | (MORE if i + 1 < len(s["contours"]) else 0)
                entries.append((POLYGON, flags, len(vertices), len(c), 0, s["op"], s["value"], 0))
                vertices += c
        else:
            entries.append((STROKE, CLOSED if s["closed"] else 0, len(vertices), len(s["points"]), s["r"], s["op"], s["value"], 0))
            vertices += s["points"]
    return np.array(vertices, dtype=np.int32).reshape(-1, 2), np.array(entries, dtype=np.uint32).reshape(-1, 8)


def unpack(vertices, entries):
    """the shapes of a VALID packed list"""
    shapes, run = [], []
    for kind, flags, first, n, r, op, value, _ in entries.tolist():
        pts = [tuple(v) for v in vertices[first:first + n].tolist()]
        if kind == STROKE:
            shapes.append(stroke(pts, r, bool(flags & CLOSED), op, value))
            continue
        run.append(pts)
        if not flags & MORE:
            shapes.append(polygon(run, bool(flags & NONZERO), op, value))
            run = []
    return shapes


def validate(vertices, entries, width, height):
    """(None, NO_ENTRY, shapes) for a valid list, otherwise (the rule broken, the entry it names or NO_ENTRY, 0), in the order of the header"""
    if width > MAX_SIDE or height > MAX_SIDE:
        return "side", NO_ENTRY, 0
    if width * height > MAX_CELLS:
        return "cells", NO_ENTRY, 0
    if len(entries) > MAX_ENTRIES:
        return "entries", NO_ENTRY, 0
    if len(vertices) > MAX_VERTICES:
        return "vertices", NO_ENTRY, 0
    shapes = 0
    rows = entries.tolist()
    for i, (kind, flags, first, n, r, op, value, pad) in enumerate(rows):
        if kind not in (POLYGON, STROKE):
            return "kind", i, 0
        if flags & ~((NONZERO | MORE) if kind == POLYGON else CLOSED):
            return "flags", i, 0
        if op > SUB:
            return "op", i, 0
        if value > 65535:
            return "value", i, 0
        if pad:
            return "pad", i, 0
        if kind == POLYGON and r:
            return "half_width on a polygon", i, 0
        if r > MAX_HALF_WIDTH:
            return "half_width", i, 0
        if n < (3 if kind == POLYGON else 1):
            return "vertex_count", i, 0
        if first + n > len(vertices):
            return "range", i, 0
        if np.abs(vertices[first:first + n].astype(np.int64)).max() > MAX_COORD:
            return "coordinate", i, 0
        if i and rows[i - 1][1] & MORE:
            p = rows[i - 1]
            if kind != p[0] or op != p[5] or value != p[6] or (flags ^ p[1]) & NONZERO:
                return "run", i, 0
        else:
            shapes += 1
            if shapes > MAX_SHAPES:
                return "shapes", i, 0
        if i + 1 == len(rows) and flags & MORE:
            return "more on the last", i, 0
    return None, NO_ENTRY, shapes


def points_of(shape):
    return [p for c in shape["contours"] for p in c] if "contours" in shape else shape["points"]


def box(shape, width, height):
    """(x_lo, y_lo, x_hi, y_hi) in cells, or EMPTY.  // on Python integers is the mathematical floor; ceil(v / 256) = -((-v) // 256)"""
    pts, r = points_of(shape), shape.get("r", 0)
    out = []
    for axis, n in ((0, width), (1, height)):
        lo, hi = min(p[axis] for p in pts) - r, max(p[axis] for p in pts) + r
        out.append((max(0, -((-lo) // 256)), min(n - 1, hi // 256)))
    (x_lo, x_hi), (y_lo, y_hi) = out
    return EMPTY if x_lo > x_hi or y_lo > y_hi else (x_lo, y_lo, x_hi, y_hi)


def union(boxes):
    boxes = [b for b in boxes if b != EMPTY]
    if not boxes:
        return EMPTY
    return (min(b[0] for b in boxes), min(b[1] for b in boxes), max(b[2] for b in boxes), max(b[3] for b in boxes))


def sample_points(width, height):
    ys, xs = np.mgrid[0:height, 0:width]
    return xs.astype(np.int64) * 256, ys.astype(np.int64) * 256


def winding(contours, width, height):
    """the winding number of every sample point, by the rule: int64 throughout"""
    px, py = sample_points(width, height)
    w = np.zeros((height, width), np.int64)
    for c in contours:
        for (ax, ay), (bx, by) in zip(c, c[1:] + c[:1]):
            cross = (bx - ax) * (py - ay) - (by - ay) * (px - ax)
            w += ((ay <= py) & (py < by) & (cross > 0)).astype(np.int64)
            w -= ((by <= py) & (py < ay) & (cross < 0)).astype(np.int64)
    return w


def segments(points, closed):
    n = len(points)
    if n == 1:
        return [(points[0], points[0])]
    out = list(zip(points, points[1:]))
    if closed:
        out.append((points[-1], points[0]))
    return out


def stroke_cover(points, r, closed, width, height, wrap64=False):
    """wrap64: the mutant that forms the two sides of the 128-bit comparison in wrapping 64-bit arithmetic"""
    px, py = sample_points(width, height)
    covered = np.zeros((height, width), bool)
    r2 = r * r
    for (ax, ay), (bx, by) in segments(points, closed):
        dx, dy = bx - ax, by - ay
        ex, ey = px - ax, py - ay
        L = dx * dx + dy * dy
        t = ex * dx + ey * dy
        near_a = (ex * ex + ey * ey) <= r2
        near_b = ((px - bx) ** 2 + (py - by) ** 2) <= r2
        cross = (dx * ey - dy * ex).astype(object)  # Python integers from here
        if wrap64:
            inside = np.array([((c * c) & (2 ** 64 - 1)) <= ((r2 * L) & (2 ** 64 - 1)) for c in cross.ravel()], bool).reshape(cross.shape)
        else:
            inside = np.array([c * c <= r2 * L for c in cross.ravel()], bool).reshape(cross.shape)
        covered |= np.where((L == 0) | (t <= 0), near_a, np.where(t >= L, near_b, inside))
    return covered


def cover(shape, width, height):
    """the cells a shape covers, (height, width) bool; evaluated inside its box only where that is cheaper (test_shapes_model.py checks
    that nothing outside the box is covered on the whole window)"""
    if "contours" in shape:
        w = winding(shape["contours"], width, height)
        return w != 0 if shape["nonzero"] else (w & 1) != 0
    b = box(shape, width, height)
    out = np.zeros((height, width), bool)
    if b == EMPTY:
        return out
    x_lo, y_lo, x_hi, y_hi = b
    moved = [(x - 256 * x_lo, y - 256 * y_lo) for x, y in shape["points"]]
    out[y_lo:y_hi + 1, x_lo:x_hi + 1] = stroke_cover(moved, shape["r"], shape["closed"], x_hi - x_lo + 1, y_hi - y_lo + 1)
    return out


def apply_op(v, op, value):
    v = v.astype(np.int64)
    return {SET: np.full_like(v, value), MAX: np.maximum(v, value), MIN: np.minimum(v, value), ADD: v + value, SUB: v - value}[op]


def raster(texels, shapes, channel=0):
    """texels: the window, (h, w) uint16 or (h, w, 4) uint8.  Returns (count uint8, last uint16, the folded texels, stats): the stats of
    bt_shapes_stats that are a function of the list and the texels (tiles_missing is the atlas's, the caller adds it)"""
    height, width = texels.shape[:2]
    wide = texels.ndim == 3
    count = np.zeros((height, width), np.int64)
    last = np.full((height, width), NONE, np.uint16)
    value = (texels[:, :, channel] if wide else texels).astype(np.int64)
    data = value != 0
    boxes = [box(s, width, height) for s in shapes]
    for k, (s, b) in enumerate(zip(shapes, boxes)):
        if b == EMPTY:
            continue
        c = cover(s, width, height)
        count += c
        last[c] = k
        new = apply_op(value, s["op"], s["value"])
        new = np.clip(new, 0, 255) if wide else np.where(data, np.clip(new, 1, 65535), 0)
        value = np.where(c, new, value)
    out = texels.copy()
    if wide:
        out[:, :, channel] = value.astype(np.uint8)
    else:
        out[:] = value.astype(np.uint16)
    changed = (out != texels).any(axis=2) if wide else out != texels
    u = union(boxes)
    stats = dict(cells=width * height, shapes=len(shapes), shapes_culled=sum(b == EMPTY for b in boxes), covered=int((count > 0).sum()), written=int(changed.sum()),
                 box=u)
    return np.minimum(count, 255).astype(np.uint8), last, out, stats

"""The definition of bt_atlas_skyline (the SKYLINE section of include/bevy_terrain_amd.h) by brute force in numpy: for every cell the
maximum of (z_b - z_a) / t over all the cells ahead on its digital line, found by cross-multiplication, the nearest on a tie; lit, mask,
count, the bake byte and the stats.  And, apart from it, the header's hull reading restated one line at a time in plain Python, which
tests/test_skyline_model.py holds against the brute force.

TEST INFRASTRUCTURE ONLY."""
import numpy as np

SCHEDULE = ("launches", "edit", "changed")  # the entries of the stats that are not a function of the input planes
MAX_DIRECTIONS, STACK_BUDGET = 64, 256 << 20


def direction(d):
    """(dx, dy[, sun_num[, sun_den]]) -> (dx, dy, sun_num, sun_den): a sun on the horizontal by default"""
    d = tuple(int(v) for v in d)
    return (d + (0, 1)[len(d) - 2:])[:4]


def axes(dx, dy):
    """(x_major, n, s, m) of the header"""
    x_major = abs(dx) >= abs(dy)
    major, minor = (dx, dy) if x_major else (dy, dx)
    s = 1 if major > 0 else -1
    return x_major, abs(major), s, minor * s


def offsets(length, n, m):
    """off(u) for u = 0 .. length - 1: floor((2 u m + n) / (2 n)), the true floor (numpy's // on integers)"""
    u = np.arange(length, dtype=np.int64)
    return (2 * u * m + n) // (2 * n)


def line_index(h, w, dx, dy):
    """the line j of every cell (h, w) int64, and whether the direction is x-major"""
    x_major, n, s, m = axes(dx, dy)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.int64)
    return (ys - offsets(w, n, m)[None, :], True) if x_major else (xs - offsets(h, n, m)[:, None], False)


def line_counts(h, w, dx, dy):
    """(lines, longest) of one direction: the distinct j and the cells of the fullest one"""
    if not h or not w:
        return 0, 0
    j, _ = line_index(h, w, dx, dy)
    _, sizes = np.unique(j, return_counts=True)
    return len(sizes), int(sizes.max())


def horizon(z, dx, dy):
    """(steps uint16, rise int32) of one direction by the definition: every cell against every cell ahead, t = 1, 2, ... in turn, so that
    of two equal rationals the nearer one stays (the replacement test is strict)"""
    h, w = z.shape
    x_major, n, s, m = axes(dx, dy)
    zz = z.astype(np.int64) if x_major else z.astype(np.int64).T  # (minor, major)
    minor_len, major_len = zz.shape
    off = offsets(major_len, n, m)
    us = np.arange(major_len, dtype=np.int64)[None, :].repeat(minor_len, 0)
    vs = np.arange(minor_len, dtype=np.int64)[:, None].repeat(major_len, 1)
    best_t = np.zeros(zz.shape, np.int64)
    best_r = np.zeros(zz.shape, np.int64)
    for t in range(1, major_len):
        ub = us + s * t
        ok = (ub >= 0) & (ub < major_len)
        ubc = np.clip(ub, 0, major_len - 1)
        vb = vs - off[us] + off[ubc]  # the same j = v - off(u)
        ok &= (vb >= 0) & (vb < minor_len)
        if not ok.any():
            break
        r = zz[np.clip(vb, 0, minor_len - 1), ubc] - zz
        better = ok & ((best_t == 0) | (r * best_t > best_r * t))
        best_t[better], best_r[better] = t, r[better]
    if not x_major:
        best_t, best_r = best_t.T, best_r.T
    return np.ascontiguousarray(best_t).astype(np.uint16), np.ascontiguousarray(best_r).astype(np.int32)


def lit_plane(steps, rise, sun_num, sun_den):
    return rise.astype(np.int64) * sun_den <= steps.astype(np.int64) * sun_num


def skyline(z, directions):
    """(steps (N, h, w) uint16, rise (N, h, w) int32, mask (h, w) uint64, count (h, w) uint8, stats) of the definition; stats without
    tiles_missing, which the window's source knows"""
    directions = [direction(d) for d in directions]
    h, w = z.shape
    n = len(directions)
    steps, rise = np.zeros((n, h, w), np.uint16), np.zeros((n, h, w), np.int32)
    mask = np.zeros((h, w), np.uint64)
    lines = longest = 0
    for k, (dx, dy, num, den) in enumerate(directions):
        steps[k], rise[k] = horizon(z, dx, dy)
        mask |= lit_plane(steps[k], rise[k], num, den).astype(np.uint64) << np.uint64(k)
        a, b = line_counts(h, w, dx, dy)
        lines, longest = lines + a, max(longest, b)
    count = np.zeros((h, w), np.uint8)
    for k in range(n):
        count += ((mask >> np.uint64(k)) & np.uint64(1)).astype(np.uint8)
    stats = dict(cells=h * w, voids=int((z == 0).sum()), directions=n, lines=lines, longest_line=longest, max_steps=int(steps.max()) if steps.size else 0,
                 lit=int(count.sum(dtype=np.int64)), sum_steps=int(steps.sum(dtype=np.int64)))
    return steps, rise, mask, count, stats


def launches(h, w, n, bake=False):
    """the header's formula: the gather, the transpose, a walk and a finish per batch of B directions, a bake's gather"""
    batch = min(n, max(1, STACK_BUDGET // (4 * w * h)))
    return 2 + 2 * -(-n // batch) + (1 if bake else 0)


def bake_plane(count, n, shade=False):
    b = (255 * count.astype(np.int64) // n).astype(np.uint8)
    return (255 - b).astype(np.uint8) if shade else b


def bake(before, count, n, channel, shade=False):
    """the Rgba8 texels (h, w, 4) of the destination after the bake: one byte replaced"""
    after = before.copy()
    after[:, :, channel] = bake_plane(count, n, shade)
    return after


# ---------------------------------------------------------------------------------------------- the hull reading, restated

def lines_of(h, w, dx, dy):
    """every line of the direction as a list of (x, y) in walking order: against the direction, from the far end to the near one"""
    j, x_major = line_index(h, w, dx, dy)
    _, _, s, _ = axes(dx, dy)
    out = {}
    for y in range(h):
        for x in range(w):
            out.setdefault(int(j[y, x]), []).append((x, y))
    key = (lambda c: -s * c[0]) if x_major else (lambda c: -s * c[1])
    return [sorted(cells, key=key) for _, cells in sorted(out.items())], x_major


def hull(z, dx, dy, strict=True):
    """(steps, rise, deepest) by the hull stack; strict False: the pop test with >=, which answers the FARTHEST cell on a tie"""
    h, w = z.shape
    steps, rise = np.zeros((h, w), np.uint16), np.zeros((h, w), np.int32)
    deepest = 0
    lines, x_major = lines_of(h, w, dx, dy)
    for cells in lines:
        stack = []  # (position along the major axis, z), the nearest on top
        for x, y in cells:
            u, za = (x if x_major else y), int(z[y, x])
            while len(stack) >= 2:
                (uq, zq), (up, zp) = stack[-2], stack[-1]
                tp, tq = abs(up - u), abs(uq - u)
                lhs, rhs = (zq - za) * tp, (zp - za) * tq
                if not (lhs > rhs if strict else lhs >= rhs):
                    break
                stack.pop()
            if stack:
                steps[y, x], rise[y, x] = abs(stack[-1][0] - u), stack[-1][1] - za
            stack.append((u, za))
            deepest = max(deepest, len(stack))
    return steps, rise, deepest


def pops(z, dx, dy):
    """per cell, how many entries its arrival popped (h, w) int64"""
    h, w = z.shape
    out = np.zeros((h, w), np.int64)
    lines, x_major = lines_of(h, w, dx, dy)
    for cells in lines:
        stack = []
        for x, y in cells:
            u, za = (x if x_major else y), int(z[y, x])
            while len(stack) >= 2 and (stack[-2][1] - za) * abs(stack[-1][0] - u) > (stack[-1][1] - za) * abs(stack[-2][0] - u):
                stack.pop()
                out[y, x] += 1
            stack.append((u, za))
    return out

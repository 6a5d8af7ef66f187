"""Model of bt_atlas_viewshed: the VIEWSHED section of include/bevy_terrain_amd.h, stated on its own.

TEST INFRASTRUCTURE ONLY.  Imports neither the product nor the oracle.  Vectorised numpy in int64: for one observer it loops over j with
whole-window arrays (every target whose line has a j-th interior point at once), takes q by numpy's floor division (the true floor) and
the ceiling of S_j / j directly at every j, where the device keeps the largest rational and divides once: the ceiling is monotone, so the
maximum is the same number.  A window is raw (h, w) uint16 (0 = no data; texels of tiles the atlas does not hold arrive as 0, as
bt_atlas_read_region delivers them).  test_viewshed_model.py pins it against a restatement in fractions and answers worked by hand."""
import numpy as np

NONE = 0xFFFFFFFF
MAX_OBSERVERS, MAX_SIDE, MAX_CELLS = 64, 32768, 1 << 22
STATS = ("cells", "voids", "tiles_missing", "observers_used", "observers_skipped", "covered", "visible", "max_clearance", "samples")
SCHEDULE = ("launches",)  # the field of bt_viewshed_stats that is no function of the input


def observer(o):
    """(x, y, eye_height, radius) with the defaults of TileAtlas.viewshed"""
    o = tuple(int(v) for v in o)
    return (o + (0, 0))[:4]


def geometry(h, w, ox, oy):
    """dx, dy, n, x_major, m, the step of the major axis: (h, w) int64 / bool arrays for the observer at (ox, oy)"""
    ty, tx = np.mgrid[0:h, 0:w].astype(np.int64)
    dx, dy = tx - ox, ty - oy
    n = np.maximum(np.abs(dx), np.abs(dy))
    x_major = np.abs(dx) >= np.abs(dy)
    return dx, dy, n, x_major, np.where(x_major, dy, dx), np.where(x_major, np.sign(dx), np.sign(dy))


def line_terms(raw, ox, oy, eye_height, j):
    """the cells whose line from (ox, oy) has a j-th interior point (a bool plane) and, for those cells in row-major order, n, S_j"""
    z = np.asarray(raw).astype(np.int64)
    h, w = z.shape
    _, _, n, x_major, m, step = geometry(h, w, ox, oy)
    sel = n > j
    nn, mm, xm, st = n[sel], m[sel], x_major[sel], step[sel]
    q = (mm * j) // nn  # floor, towards minus infinity
    r = mm * j - q * nn
    ax, ay = np.where(xm, ox + st * j, ox + q), np.where(xm, oy + q, oy + st * j)
    bx, by = np.where(xm, ax, ax + 1), np.where(xm, ay + 1, ay)
    za = z[ay, ax]
    zb = np.where(r > 0, z[np.minimum(by, h - 1), np.minimum(bx, w - 1)], 0)  # not read when r == 0
    G = za * (nn - r) + zb * r
    E = int(z[oy, ox]) + eye_height
    return sel, nn, G - E * nn


def observer_clearance(raw, ox, oy, eye_height):
    """C_o of every cell as (h, w) int64 (void targets included: the caller drops them), and n"""
    z = np.asarray(raw).astype(np.int64)
    h, w = z.shape
    n = geometry(h, w, ox, oy)[2]
    E = int(z[oy, ox]) + eye_height
    M = np.full((h, w), -(1 << 62), np.int64)
    for j in range(1, int(n.max())):
        sel, _, S = line_terms(raw, ox, oy, eye_height, j)
        M[sel] = np.maximum(M[sel], -((-S) // j))  # the ceiling, towards plus infinity
    return np.where(n <= 1, 0, np.maximum(0, E + M - z)), n


def line_maxima(raw, ox, oy, eye_height):
    """(S_b, j_b): the largest S_j / j of every line as the pair the device keeps (the first j on a tie), by cross-multiplication;
    j_b = 0 where n <= 1"""
    h, w = np.asarray(raw).shape
    n = geometry(h, w, ox, oy)[2]
    Sb, jb = np.zeros((h, w), np.int64), np.zeros((h, w), np.int64)
    for j in range(1, int(n.max())):
        sel, _, S = line_terms(raw, ox, oy, eye_height, j)
        better = (jb[sel] == 0) | (S * jb[sel] > Sb[sel] * j)
        Sb[sel], jb[sel] = np.where(better, S, Sb[sel]), np.where(better, j, jb[sel])
    return Sb, jb


def grazings(raw, ox, oy, eye_height, target_height):
    """the number of (active target, j) pairs whose sight line to the target's top touches the ground exactly: (Z - E) j == S_j"""
    z = np.asarray(raw).astype(np.int64)
    n = geometry(*z.shape, ox, oy)[2]
    E, total = int(z[oy, ox]) + eye_height, 0
    for j in range(1, int(n.max())):
        sel, _, S = line_terms(raw, ox, oy, eye_height, j)
        total += int((((z[sel] + target_height - E) * j == S) & (z[sel] != 0)).sum())
    return total


def covers(h, w, ox, oy, radius):
    dx, dy = geometry(h, w, ox, oy)[:2]
    if radius == 0 or radius * radius >= h * h + w * w:  # the second: every cell, and radius^2 may not fit int64
        return np.ones((h, w), bool)
    return dx * dx + dy * dy <= radius * radius


def viewshed(raw, observers, target_height=0):
    """-> (clearance (h, w) uint32, count (h, w) uint8, mask (h, w) uint64, stats without tiles_missing and launches)"""
    raw = np.asarray(raw)
    h, w = raw.shape
    active = raw != 0
    best = np.full((h, w), NONE, np.int64)
    count = np.zeros((h, w), np.int64)
    mask = np.zeros((h, w), np.uint64)
    used = skipped = samples = 0
    for o, (ox, oy, eye_height, radius) in enumerate(observer(v) for v in observers):
        if not active[oy, ox]:
            skipped += 1
            continue
        used += 1
        C, n = observer_clearance(raw, ox, oy, eye_height)
        cov = covers(h, w, ox, oy, radius) & active
        best = np.where(cov, np.minimum(best, C), best)
        seen = cov & (C <= target_height)
        count += seen
        mask |= np.where(seen, np.uint64(1 << o), np.uint64(0))
        samples += int(np.maximum(n - 1, 0)[cov].sum())
    covered = best != NONE
    stats = dict(cells=h * w, voids=int((~active).sum()), observers_used=used, observers_skipped=skipped, covered=int(covered.sum()), visible=int((count > 0).sum()),
                 max_clearance=int(best[covered].max()) if covered.any() else 0, samples=samples)
    return best.astype(np.uint32), count.astype(np.uint8), mask, stats

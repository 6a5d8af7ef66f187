"""Second model of the culled tiling prepass and of the height-bounds table (include/bevy_terrain_amd.h, "frustum and height-bounds
culling"): the definition restated in numpy float32, whole arrays of tiles at a time, on top of _refine_model (the divide test) and
_bounds_model (a layer's min / max).  TEST INFRASTRUCTURE ONLY.

numpy's float32 +, -, *, /, sqrt are IEEE and unfused, one rounding per written operation, like the kernels' (-ffp-contract=off).  With
dtype=float64 the same code gives the points the conservativeness test samples."""
import numpy as np

import _bounds_model as B
import _refine_model as R

F = np.float32
WHOLE_RANGE = (0, 65535)


class CullView:
    """bt_cull_view"""

    def __init__(self, planes, margin=0.0, min_height=0.0, max_height=0.0):
        self.planes = np.asarray(planes, dtype=F).reshape(-1, 4)
        self.margin, self.min_height, self.max_height = F(margin), F(min_height), F(max_height)


class Table:
    """bt_height_bounds: data (entries, 2) uint16; level l at sides * (4^l - 1) / 3, entry ((side * n + y) * n + x), n = 1 << l"""

    def __init__(self, sides, levels, data=None):
        self.sides, self.levels = sides, levels
        self.entries = sides * (4 ** levels - 1) // 3
        self.data = np.tile(np.array(WHOLE_RANGE, np.uint16), (self.entries, 1)) if data is None else np.asarray(data, np.uint16).reshape(self.entries, 2)

    def offset(self, level):
        return self.sides * (4 ** level - 1) // 3

    def index(self, side, lod, x, y):
        n = 1 << lod
        return self.offset(lod) + (side * n + y) * n + x


def planes_from_matrix(m):
    """culling_bind_group.rs:25-38 on m[row, column] (float32): left, right, bottom, top, w - z"""
    m = np.asarray(m, dtype=F).reshape(4, 4)
    planes = np.zeros((5, 4), F)
    for i in range(5):
        row = m[i // 2]
        planes[i] = m[3] + row if (i & 1) == 0 and i != 4 else m[3] - row
    return planes


def surface(view, tiles, uv, dtype=F):
    """the world position and the world normal at uv ((n, 2) or (2,)) of each tile: functions.wgsl:73-96, 117-121 — the arithmetic of
    _refine_model.should_be_divided between the tile coordinate and `world + approximate_height * normal`, with uv given"""
    D = dtype
    n = len(tiles)
    side, lod, x, y = (tiles[:, k] for k in range(4))
    uv = np.broadcast_to(np.asarray(uv, dtype=D), (n, 2))
    tc = np.ldexp(D(1.0), lod.astype(np.int32)).astype(D)
    u = ((x.astype(D) + uv[:, 0]) / tc).astype(D)
    w = ((y.astype(D) + uv[:, 1]) / tc).astype(D)
    if view.spherical:
        c = D(F(0.87) * F(0.87))
        u = (u - D(0.5)) / D(0.5)
        w = (w - D(0.5)) / D(0.5)
        u = u / np.sqrt(D(1.0) + c - c * u * u)
        w = w / np.sqrt(D(1.0) + c - c * w * w)
        one = np.ones(n, D)
        faces = {0: (-one, -w, u), 1: (u, -w, one), 2: (u, one, w), 3: (one, -u, w), 4: (w, -u, -one), 5: (w, -one, u)}
        l = np.zeros((n, 3), D)
        for s, (a, b, cc) in faces.items():
            m = side == s
            l[m, 0], l[m, 1], l[m, 2] = a[m], b[m], cc[m]
        ln = np.sqrt(l[:, 0] * l[:, 0] + l[:, 1] * l[:, 1] + l[:, 2] * l[:, 2])
        l = (l / ln[:, None]).astype(D)
        normal0 = l
    else:
        l = np.stack([u - D(0.5), np.zeros(n, D), w - D(0.5)], axis=1).astype(D)
        normal0 = np.tile(np.array([0, 1, 0], D), (n, 1))
    m = np.array(list(view.world_from_local), F).astype(D)
    world = np.stack([(m[r] * l[:, 0] + m[3 + r] * l[:, 1] + m[6 + r] * l[:, 2]) + m[9 + r] for r in range(3)], axis=1).astype(D)
    t = np.array(list(view.local_from_world_transpose), F).astype(D)
    nrm = np.stack([t[r] * normal0[:, 0] + t[3 + r] * normal0[:, 1] + t[6 + r] * normal0[:, 2] for r in range(3)], axis=1).astype(D)
    nl = np.sqrt(nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1] + nrm[:, 2] * nrm[:, 2])
    nrm = (nrm / nl[:, None]).astype(D)
    return world, nrm


def point(view, tiles, uv, h, dtype=F):
    """point(tile, uv, h) = world + h * normal; h a scalar or one value per tile"""
    world, nrm = surface(view, tiles, uv, dtype)
    h = np.broadcast_to(np.asarray(h, dtype=dtype), (len(tiles),))
    return (world + h[:, None] * nrm).astype(dtype)


def raw_range(tiles, table):
    """(vmin, vmax) uint16 arrays: the table entry of the tile, or of its ancestor at the table's last level; (0, 65535) without a table"""
    n = len(tiles)
    if table is None:
        return np.full(n, WHOLE_RANGE[0], np.uint16), np.full(n, WHOLE_RANGE[1], np.uint16)
    side, lod, x, y = (tiles[:, k].astype(np.int64) for k in range(4))
    lb = np.minimum(lod, table.levels - 1)
    sh = lod - lb
    cells = np.int64(1) << lb
    index = table.sides * ((np.int64(4) ** lb - 1) // 3) + (side * cells + (y >> sh)) * cells + (x >> sh)
    return table.data[index, 0], table.data[index, 1]


def heights(cull, v):
    """h = min_height + (max_height - min_height) * (float(v) / 65535.0f)"""
    return (cull.min_height + (cull.max_height - cull.min_height) * (v.astype(F) / F(65535.0))).astype(F)


def length3(v):
    return np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]).astype(F)


def corners_and_slack(view, tiles, cull, table=None):
    """-> (the eight corners (8, n, 3), slack (n,))"""
    vmin, vmax = raw_range(tiles, table)
    h_lo, h_hi = heights(cull, vmin), heights(cull, vmax)
    P = np.stack([point(view, tiles, uv, h) for h in (h_lo, h_hi) for uv in ((0, 0), (1, 0), (0, 1), (1, 1))])
    if view.spherical:
        centre = point(view, tiles, (0.5, 0.5), h_hi)
        mean = (((P[4] + P[5]) + (P[6] + P[7])) * F(0.25)).astype(F)
        bulge = length3((centre - mean).astype(F))
    else:
        bulge = np.zeros(len(tiles), F)
    return P, (bulge + cull.margin).astype(F)


def culled(view, tiles, cull, table=None):
    """the mask of tiles whose volume lies outside one of the planes"""
    out = np.zeros(len(tiles), bool)
    if len(tiles) == 0 or len(cull.planes) == 0:
        return out
    P, slack = corners_and_slack(view, tiles, cull, table)
    with np.errstate(invalid="ignore"):
        for a, b, c, d in cull.planes:
            length = np.sqrt((a * a + b * b) + c * c)
            limit = -(slack * length)
            s = (((a * P[:, :, 0] + b * P[:, :, 1]) + c * P[:, :, 2]) + d).astype(F)
            out |= np.all(s < limit[None, :], axis=0)  # a comparison with a NaN is false
    return out


def refine_culled(view, cull, table=None, passes=None):
    """the culled prepass, breadth first in id order -> (final tiles (n, 4) uint32 in append order, tiles culled, tiles visited);
    `passes` (a list) receives one (tiles visited, tiles dividing) pair per pass that runs"""
    roots = 6 if view.spherical else 1
    current = np.array([[s, 0, 0, 0] for s in range(roots)], np.uint32)
    final, n_culled, n_visited = [], 0, 0
    for p in range(view.refinement_count + 1):
        if len(current) == 0:
            break
        out = culled(view, current, cull, table)
        kept = current[~out]
        divide = R.should_be_divided(view, kept)[0] if len(kept) else np.zeros(0, bool)
        n_visited += len(current)
        n_culled += int(out.sum())
        if passes is not None:
            passes.append((len(current), int(divide.sum())))
        final.append(kept[~divide])
        parents = kept[divide]
        if p == view.refinement_count:
            break
        i = np.tile(np.arange(4, dtype=np.uint32), len(parents))
        rep = np.repeat(parents, 4, axis=0)
        current = np.stack([rep[:, 0], rep[:, 1] + 1, (rep[:, 2] << 1) + (i & 1), (rep[:, 3] << 1) + ((i >> 1) & 1)], axis=1).astype(np.uint32).reshape(-1, 4)
    final = np.concatenate(final) if final else np.zeros((0, 4), np.uint32)
    return final, n_culled, n_visited


def overflows(passes, final_count, capacity):
    """the reference's buffers: a pass needs its parents and the children they append, the final list its tiles"""
    return final_count > capacity or any(visited + 4 * dividing > capacity for visited, dividing in passes)


def build_table(sides, levels, held, own=None):
    """bt_height_bounds_build: held = {(side, lod, x, y): the tile's (T, T) uint16 layer}.  own = min / max of the whole layer
    (_bounds_model.tile_bounds at grid 1); a tile that is not held takes own of its parent, a root the whole range; then every entry is
    united with its children's.  own: {coord: (min, max)} of the held tiles, computed by the caller (for tens of thousands of tiles,
    where one tile_bounds call each takes seconds); held is not looked at then."""
    table = Table(sides, levels)
    if own is not None:
        own = {c: (int(mn), int(mx)) for c, (mn, mx) in own.items() if c[1] < levels}
    else:
        own = {}
        for (side, lod, x, y), layer in held.items():
            if lod < levels:
                mn, mx = B.tile_bounds(np.asarray(layer)[None], 1)[0][0, 0, 0]
                own[(side, lod, x, y)] = (int(mn), int(mx))
    for lod in range(levels):
        for side in range(sides):
            for y in range(1 << lod):
                for x in range(1 << lod):
                    if (side, lod, x, y) not in own:
                        own[(side, lod, x, y)] = own[(side, lod - 1, x >> 1, y >> 1)] if lod else WHOLE_RANGE
    for lod in reversed(range(levels)):
        for side in range(sides):
            for y in range(1 << lod):
                for x in range(1 << lod):
                    mn, mx = own[(side, lod, x, y)]
                    if lod + 1 < levels:
                        for k in range(4):
                            c = table.data[table.index(side, lod + 1, 2 * x + (k & 1), 2 * y + (k >> 1))]
                            mn, mx = min(mn, int(c[0])), max(mx, int(c[1]))
                    table.data[table.index(side, lod, x, y)] = (mn, mx)
    return table


# ---- cameras for the tests (float64 host glue, like the reference's view extraction) --------------------------------------

def clip_from_world(eye, direction, fov_y, aspect, near=0.1, up=(0.0, 1.0, 0.0)):
    """Mat4::perspective_infinite_reverse_rh(fov_y, aspect, near) * Mat4::look_to_rh(eye, direction, up) as m[row, column], float64"""
    eye, f = np.asarray(eye, np.float64), np.asarray(direction, np.float64)
    f = f / np.linalg.norm(f)
    up = np.asarray(up, np.float64)
    if abs(np.dot(f, up)) > 0.999:
        up = np.array([1.0, 0.0, 0.0])
    s = np.cross(f, up)
    s /= np.linalg.norm(s)
    u = np.cross(s, f)
    view = np.eye(4)
    view[0, :3], view[1, :3], view[2, :3] = s, u, -f
    view[:3, 3] = [-np.dot(s, eye), -np.dot(u, eye), np.dot(f, eye)]
    g = 1.0 / np.tan(0.5 * fov_y)
    proj = np.array([[g / aspect, 0, 0, 0], [0, g, 0, 0], [0, 0, 0, near], [0, 0, -1, 0]], np.float64)
    return proj @ view


def random_camera(rng, kind):
    """(eye, clip_from_world) of one of the two models of the tests: planar 1000 / 0..250 and sphere 6371000 / -12000..9000; field of
    view 30..100 degrees, the eye from just above the surface to orbit, looking anywhere from straight down to above the horizon"""
    fov, aspect = np.radians(rng.uniform(30.0, 100.0)), float(rng.choice([1.0, 4.0 / 3.0, 16.0 / 9.0]))
    if kind == "planar":
        eye = np.array([rng.uniform(-600.0, 600.0), 250.0 + 10.0 ** rng.uniform(0.0, 3.5), rng.uniform(-600.0, 600.0)])
        down = np.array([0.0, -1.0, 0.0])
    else:
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        eye = d * (6371000.0 + 9000.0 + 10.0 ** rng.uniform(1.0, 7.2))
        down = -d
    side = rng.normal(size=3)
    side -= down * np.dot(side, down)
    side /= np.linalg.norm(side)
    pitch = np.radians(rng.uniform(-90.0, 15.0))  # -90: straight down, 0: level
    direction = np.cos(pitch) * side - np.sin(pitch) * down
    return eye, clip_from_world(eye, direction, fov, aspect, up=-down)

"""Model of the horizon test of the culled tiling prepass (include/bevy_terrain_amd.h, "horizon culling"): the definition restated in
numpy float32, whole arrays of tiles at a time, beside _cull_model (the frustum test, the height ranges, the cameras).  TEST
INFRASTRUCTURE ONLY.

numpy's float32 +, -, *, /, sqrt are IEEE and unfused, one rounding per written operation, like the kernels' (-ffp-contract=off).  With
dtype=float64 scaled_point gives the points the conservativeness test samples."""
import numpy as np

import _cull_model as M
import _refine_model as R

F = np.float32
GUARD = F(2.0 ** -20)  # BT_HORIZON_GUARD


class HorizonView:
    """bt_horizon_view"""

    def __init__(self, eye, vh, occluder_radius, margin=0.0):
        self.eye = np.asarray(eye, dtype=F).reshape(3)
        self.vh, self.occluder_radius, self.margin = F(vh), F(occluder_radius), F(margin)

    @classmethod
    def from_c(cls, c):
        return cls([c.eye[0], c.eye[1], c.eye[2]], c.vh, c.occluder_radius, c.margin)


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def local_surface(view, tiles, uv, dtype=F):
    """(l, world, normal) at uv of each tile of a spherical view: l is the unit local position of tile_surface (the cube-sphere warp and
    normalisation, before world_from_local); world and normal are _cull_model.surface's, computed from it with the same operations"""
    assert view.spherical
    D = dtype
    n = len(tiles)
    side, lod, x, y = (tiles[:, k] for k in range(4))
    uv = np.broadcast_to(np.asarray(uv, dtype=D), (n, 2))
    tc = np.ldexp(D(1.0), lod.astype(np.int32)).astype(D)
    u = ((x.astype(D) + uv[:, 0]) / tc).astype(D)
    w = ((y.astype(D) + uv[:, 1]) / tc).astype(D)
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
    m = np.array(list(view.world_from_local), F).astype(D)
    world = np.stack([(m[r] * l[:, 0] + m[3 + r] * l[:, 1] + m[6 + r] * l[:, 2]) + m[9 + r] for r in range(3)], axis=1).astype(D)
    t = np.array(list(view.local_from_world_transpose), F).astype(D)
    nrm = np.stack([t[r] * l[:, 0] + t[3 + r] * l[:, 1] + t[6 + r] * l[:, 2] for r in range(3)], axis=1).astype(D)
    nl = np.sqrt(nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1] + nrm[:, 2] * nrm[:, 2])
    nrm = (nrm / nl[:, None]).astype(D)
    return l, world, nrm


def scaled_point(view, tiles, uv, h, dtype=F):
    """q(tile, uv, h) = l + h * g, g = local_from_world * normal; h a scalar or one value per tile"""
    D = dtype
    l, _, nrm = local_surface(view, tiles, uv, D)
    t = np.array(list(view.local_from_world_transpose), F).astype(D)
    g = np.stack([(t[3 * r] * nrm[:, 0] + t[3 * r + 1] * nrm[:, 1]) + t[3 * r + 2] * nrm[:, 2] for r in range(3)], axis=1).astype(D)
    h = np.broadcast_to(np.asarray(h, dtype=D), (len(tiles),))
    return (l + h[:, None] * g).astype(D)


def points_and_margin(view, tiles, cull, horizon, table=None):
    """-> (the eight scaled points (8, n, 3), m (n,))"""
    vmin, vmax = M.raw_range(tiles, table)
    h_lo, h_hi = M.heights(cull, vmin), M.heights(cull, vmax)
    Q = np.stack([scaled_point(view, tiles, uv, h) for h in (h_lo, h_hi) for uv in ((0, 0), (1, 0), (0, 1), (1, 1))])
    centre = scaled_point(view, tiles, (0.5, 0.5), h_hi)
    mean = (((Q[4] + Q[5]) + (Q[6] + Q[7])) * F(0.25)).astype(F)
    d = (centre - mean).astype(F)
    bulge = np.sqrt(dot3(d, d)).astype(F)
    return Q, ((bulge + horizon.margin) + GUARD).astype(F)


def culled(view, tiles, cull, horizon, table=None):
    """the mask of tiles all eight points of which, widened by m, lie behind the occluder's horizon"""
    out = np.zeros(len(tiles), bool)
    if len(tiles) == 0 or horizon is None or not horizon.vh > 0:  # (NaN: false)
        return out
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        Q, m = points_and_margin(view, tiles, cull, horizon, table)
        eye = horizon.eye
        E = np.sqrt(dot3(eye, eye)).astype(F)
        sv = np.sqrt(horizon.vh).astype(F)
        lim = (m * E).astype(F)
        hidden = np.ones(len(tiles), bool)
        for k in range(8):
            vt = (Q[k] - eye).astype(F)
            ap = -dot3(vt, eye[None, :])
            along = (ap / E).astype(F)
            s = (dot3(vt, vt) - along * along).astype(F)
            perp = np.sqrt(np.where(s > 0, s, F(0))).astype(F)  # max(s, 0): s when s > 0, else 0
            hidden &= ((ap - horizon.vh) > lim) & (((along * horizon.occluder_radius) - (perp * sv)) > lim)  # a comparison with a NaN is false
    return hidden


def culled_either(view, tiles, cull, horizon, table=None):
    out = M.culled(view, tiles, cull, table)
    if horizon is not None:
        out = out | culled(view, tiles, cull, horizon, table)
    return out


def refine_culled_horizon(view, cull, horizon, table=None, passes=None):
    """the culled prepass with either test culling, breadth first in id order -> (final tiles (n, 4) uint32 in append order, tiles culled,
    tiles visited); `passes` (a list) receives one (tiles visited, tiles dividing) pair per pass that runs"""
    roots = 6 if view.spherical else 1
    current = np.array([[s, 0, 0, 0] for s in range(roots)], np.uint32)
    final, n_culled, n_visited = [], 0, 0
    for p in range(view.refinement_count + 1):
        if len(current) == 0:
            break
        out = culled_either(view, current, cull, horizon, table)
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


# ---- float64 host glue for the tests ------------------------------------------------------------------------------------------

def round_toward_zero(x):
    f = F(x)
    return np.nextafter(f, F(0)) if abs(float(f)) > abs(float(x)) else f


def round_up(x):
    f = F(x)
    return np.nextafter(f, F(np.inf)) if float(f) < float(x) else f


def horizon_view(model, eye_world, margin_world=0.0):
    """bt_cull_horizon restated in float64 (model: a spherical or ellipsoidal TerrainModel; its scale is (a, a, a) or (a, b, a))"""
    axes = np.asarray(model.scale_vec, np.float64)
    eye = ((np.asarray(eye_world, np.float64) - np.asarray(model.translation, np.float64)) / axes).astype(F)
    radius = round_toward_zero(1.0 + min(float(F(model.min_height)), 0.0) / axes.min())
    e = eye.astype(np.float64)
    vh = F(((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) - float(radius) * float(radius))
    return HorizonView(eye, vh, radius, round_up(float(margin_world) / axes.min()))

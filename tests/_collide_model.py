"""The definitions SPHERE CONTACT and SPHERE SWEEP (include/bevy_terrain_amd.h, "terrain collision") written once more on the CPU: one
sphere at a time, f64 numpy, every operation in the header's order; the 64 lanes of a round are one numpy vector.  The altitude is
_raycast_model.altitude, the height h comes from a callable (world positions (n, 3) -> f32 heights: the oracle's sample_attachment through
_raycast_model.sampler, or an analytic ground).  Nothing of the package under test is imported."""
import numpy as np

import _oracle as O
import _raycast_model as RM

NONE, TOUCHING, BELOW, INVALID, FAR = 0, 1, 2, 3, 4
MISS, HIT, INSIDE, RAY_INVALID = RM.MISS, RM.HIT, RM.INSIDE, RM.INVALID
CONTACT_DTYPE = np.dtype([("status", np.uint32), ("candidate", np.uint32), ("distance", np.float64), ("depth", np.float64), ("point", np.float64, 3),
                          ("normal", np.float64, 3), ("height", np.float32)])
SWEEP_DTYPE = np.dtype([("status", np.uint32), ("step", np.uint32), ("t", np.float64), ("t_above", np.float64), ("contact", CONTACT_DTYPE)])
F = np.float32
LANE = np.arange(64)
SX = (2.0 * (LANE & 7).astype(np.float64) - 7.0) / 7.0
SY = (2.0 * (LANE >> 3).astype(np.float64) - 7.0) / 7.0


def ceiling(model):
    """double(lerp(min_height, max_height, 1.0f))"""
    return float(F(model.min_height) + (F(model.max_height) - F(model.min_height)) * F(1.0))


def _dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _normalize3(a):
    r = 1.0 / np.sqrt(_dot3(a, a))
    return [a[0] * r, a[1] * r, a[2] * r]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def frame(model, pts):
    """(world0, n) of world points (k, 3), each a list of three (k,) arrays: world0 = transform_point(m, local), local =
    position_world_to_local(m, p), and n = normalize3(transform_vector(m, spherical ? local : (0, 1, 0))), so that
    position_local_to_world(m, local, h) = world0 + h * n"""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    p = [pts[:, 0].copy(), pts[:, 1].copy(), pts[:, 2].copy()]
    pos = [float(model.position[i]) for i in range(3)]
    kind = int(model.kind)
    a, b = float(model.a), float(model.b)
    scale = [a, b, a] if kind == 2 else [a, a, a]
    with np.errstate(all="ignore"):
        if kind == 0:
            q = [(p[i] - pos[i]) / scale[i] for i in range(3)]
            local = [1.0 * q[0], 0.0 * q[1], 1.0 * q[2]]
            up = [np.zeros_like(p[0]), np.ones_like(p[0]), np.zeros_like(p[0])]
        elif kind == 1:
            local = _normalize3([(p[i] - pos[i]) / scale[i] for i in range(3)])
            up = local
        else:
            e = np.array([p[i] - pos[i] for i in range(3)]).T
            s = np.array([O.project_point_ellipsoid((a, a, b), tuple(row)) for row in e]).reshape(-1, 3)
            local = _normalize3([(s[:, i] - pos[i]) / scale[i] for i in range(3)])
            up = local
        n = _normalize3([scale[i] * up[i] for i in range(3)])
        world0 = [scale[i] * local[i] + pos[i] for i in range(3)]
    return world0, n


def ground_points(model, sample, pts):
    """G(q) and h_q of world points (k, 3) -> ((k, 3) float64, (k,) float32)"""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    world0, n = frame(model, pts)
    h = np.asarray(sample(pts), dtype=np.float32)
    hd = h.astype(np.float64)
    with np.errstate(all="ignore"):
        return np.column_stack([world0[i] + hd * n[i] for i in range(3)]), h


def stencil(c, e1, e2, ox, oy, w):
    """the 64 sample positions of a round, and their (x, y)"""
    with np.errstate(all="ignore"):
        x, y = ox + w * SX, oy + w * SY
        return np.column_stack([c[i] + (x * e1[i] + y * e2[i]) for i in range(3)]), x, y


def tangent_basis(model, n):
    if int(model.kind) == 0:
        return [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]
    k, least = 0, abs(n[0])
    if abs(n[1]) < least:
        k, least = 1, abs(n[1])
    if abs(n[2]) < least:
        k = 2
    u = [np.float64(1.0 if i == k else 0.0) for i in range(3)]
    with np.errstate(all="ignore"):
        e1 = _normalize3(_cross(u, n))
        return e1, _cross(n, e1)


def contact_one(model, sample, c, r, refine_rounds, skip_above=True, trace=None):
    """SPHERE CONTACT.  skip_above: border_size >= 1 (the caller's attachment) — max_height >= min_height is checked here.  trace: a list
    that receives (x, y) of every winner that became best"""
    out = np.zeros((), CONTACT_DTYPE)
    c = np.asarray(c, dtype=np.float64).reshape(3)
    r = np.float64(r)
    if not (np.isfinite(c).all() and np.isfinite(r)) or r < 0.0:
        out["status"] = INVALID
        return out
    with np.errstate(all="ignore"):
        a = np.float64(RM.altitude(model, c[None, :])[0])
        if skip_above and float(model.max_height) >= float(model.min_height) and a - r > ceiling(model):
            out["status"] = FAR
            return out
        _, n = frame(model, c[None, :])
        n = [np.float64(v[0]) for v in n]
        g, h = ground_points(model, sample, c[None, :])
        g0, h0 = g[0], h[0]
        f = a - np.float64(h0)
        if f <= 0.0:
            out["status"], out["distance"], out["depth"], out["point"], out["normal"], out["height"] = BELOW, f, r - f, g0, n, h0
            return out
        e1, e2 = tangent_basis(model, n)
        d = g0 - c
        best, candidate, point, height = _dot3(d, d), 0, g0, h0
        ox, oy, w = np.float64(0.0), np.float64(0.0), r
        for k in range(refine_rounds + 1):
            q, x, y = stencil(c, e1, e2, ox, oy, w)
            g, h = ground_points(model, sample, q)
            d = g - c[None, :]
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            key = np.where(np.isnan(d2), np.inf, d2)
            l = int(np.argmin(key))  # the first of the smallest: ties to the lowest lane
            if key[l] < best:
                best, candidate, point, height, ox, oy = key[l], 64 * k + l + 1, g[l], h[l], x[l], y[l]
                if trace is not None:
                    trace.append((x[l], y[l]))
            w = w * (2.0 / 7.0)
        distance = np.sqrt(best)
        out["status"] = TOUCHING if distance < r else NONE
        out["candidate"], out["distance"], out["depth"], out["point"], out["height"] = candidate, distance, r - distance, point, height
        out["normal"] = (c - point) * (1.0 / distance) if distance > 0.0 else n
    return out


def contacts(model, sample, centers, radii, refine_rounds, skip_above=True):
    centers = np.asarray(centers, dtype=np.float64).reshape(-1, 3)
    radii = np.broadcast_to(np.asarray(radii, np.float64), len(centers))
    return np.array([contact_one(model, sample, centers[i], radii[i], refine_rounds, skip_above) for i in range(len(centers))], dtype=CONTACT_DTYPE)


def sweep_one(model, sample, origin, direction, radius, t_min, t_max, steps, bisections, refine_rounds, skip_above=True):
    """SPHERE SWEEP"""
    out = np.zeros((), SWEEP_DTYPE)
    origin, direction = np.asarray(origin, dtype=np.float64).reshape(3), np.asarray(direction, dtype=np.float64).reshape(3)
    radius, t_min, t_max = np.float64(radius), np.float64(t_min), np.float64(t_max)
    if not (np.isfinite(origin).all() and np.isfinite(direction).all() and np.isfinite(t_min) and np.isfinite(t_max) and t_max >= t_min
            and (direction != 0.0).any() and np.isfinite(radius) and radius >= 0.0):
        out["status"] = RAY_INVALID
        return out

    def contact(t):
        with np.errstate(all="ignore"):
            return contact_one(model, sample, origin + t * direction, radius, refine_rounds, skip_above)

    def blocked(t):
        return int(contact(t)["status"]) in (TOUCHING, BELOW)

    with np.errstate(all="ignore"):
        dt = (t_max - t_min) / np.float64(steps)
        step = next((i for i in range(steps + 1) if blocked(t_min + np.float64(i) * dt)), None)
        if step is None:
            out["status"] = MISS
            return out
        if step == 0:
            out["status"] = INSIDE
            lo = hi = t_min
        else:
            out["status"] = HIT
            lo, hi = t_min + np.float64(step - 1) * dt, t_min + np.float64(step) * dt
            for _ in range(bisections):
                mid = lo + (hi - lo) * 0.5
                if blocked(mid):
                    hi = mid
                else:
                    lo = mid
    out["step"], out["t"], out["t_above"], out["contact"] = step, hi, lo, contact(hi)
    return out


def sweeps(model, sample, origins, directions, radii, t_min, t_max, steps, bisections, refine_rounds, skip_above=True):
    origins = np.asarray(origins, dtype=np.float64).reshape(-1, 3)
    directions = np.asarray(directions, dtype=np.float64).reshape(-1, 3)
    n = len(origins)
    radii, t_min, t_max = (np.broadcast_to(np.asarray(v, np.float64), n) for v in (radii, t_min, t_max))
    return np.array([sweep_one(model, sample, origins[i], directions[i], radii[i], t_min[i], t_max[i], steps, bisections, refine_rounds, skip_above)
                     for i in range(n)], dtype=SWEEP_DTYPE)

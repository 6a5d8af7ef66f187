"""The definition of bt_tile_tree_raycast (include/bevy_terrain_amd.h) written once more on the CPU: one ray at a time, f64 numpy, every
operation in the header's order.  The height h comes from a callable the caller builds on the oracle's TileTree.sample_attachment
(tests/_oracle.py: the tree's entries and the layer contents are given to it); the altitude is computed here (planar and sphere in numpy,
the ellipsoid's projection through O.project_point_ellipsoid).  Nothing of the package under test is imported."""
import numpy as np

import _oracle as O

MISS, HIT, INSIDE, INVALID = 0, 1, 2, 3
HIT_DTYPE = np.dtype([("status", np.uint32), ("step", np.uint32), ("t", np.float64), ("t_above", np.float64), ("position", np.float64, 3),
                      ("height", np.float32)])


def sampler(otree, texture_size, border_size, layers):
    """h(p) of an oracle TileTree in its current state: positions (n, 3) -> f32 heights"""
    return lambda pts: otree.sample_attachment(O.FORMAT_R16, texture_size, border_size, layers, pts)[1]


def _dot3(a, b):  # bt_model.hpp dot3: (x*x' + y*y') + z*z'
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _normalize3(a):  # v * (1.0 / length)
    r = 1.0 / np.sqrt(_dot3(a, a))
    return [a[0] * r, a[1] * r, a[2] * r]


def altitude(model, pts):
    """altitude of world points (n, 3) above the height-0 surface of an O.Model, measured along position_local_to_world's direction"""
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
        ground0 = [(scale[i] * local[i] + pos[i]) + 0.0 * n[i] for i in range(3)]
        return _dot3([p[i] - ground0[i] for i in range(3)], n)


def f_values(model, sample, pts):
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return altitude(model, pts) - np.asarray(sample(pts), dtype=np.float32).astype(np.float64)


def _points(origin, direction, t):
    t = np.asarray(t, dtype=np.float64).reshape(-1, 1)
    with np.errstate(all="ignore"):
        return origin[None, :] + t * direction[None, :]


def raycast_one(model, sample, origin, direction, t_min, t_max, steps, refine_rounds):
    out = np.zeros((), HIT_DTYPE)
    origin, direction = np.asarray(origin, dtype=np.float64), np.asarray(direction, dtype=np.float64)
    t_min, t_max = np.float64(t_min), np.float64(t_max)
    if not (np.isfinite(origin).all() and np.isfinite(direction).all() and np.isfinite(t_min) and np.isfinite(t_max) and t_max >= t_min
            and (direction != 0.0).any()):
        out["status"] = INVALID
        return out
    dt = (t_max - t_min) / np.float64(steps)
    t = t_min + np.arange(steps + 1, dtype=np.float64) * dt
    below = f_values(model, sample, _points(origin, direction, t)) <= 0.0  # NaN compares false
    if not below.any():
        out["status"] = MISS
        return out
    i = int(np.argmax(below))
    if i == 0:
        out["status"] = INSIDE
        lo = hi = t_min
    else:
        out["status"] = HIT
        lo, hi = t[i - 1], t[i]
        for _ in range(refine_rounds):
            u = lo + (hi - lo) * (np.arange(65, dtype=np.float64) / 64.0)  # u[k], k = 1 .. 63 used
            below = f_values(model, sample, _points(origin, direction, u[1:64])) <= 0.0
            k = int(np.argmax(below)) + 1 if below.any() else 64
            lo, hi = (lo if k == 1 else u[k - 1]), (hi if k == 64 else u[k])
    p = _points(origin, direction, [hi])[0]
    out["step"], out["t"], out["t_above"], out["position"] = i, hi, lo, p
    out["height"] = np.asarray(sample(p[None, :]), dtype=np.float32)[0]
    return out


def raycast(model, sample, origins, directions, t_min, t_max, steps, refine_rounds):
    origins = np.asarray(origins, dtype=np.float64).reshape(-1, 3)
    directions = np.asarray(directions, dtype=np.float64).reshape(-1, 3)
    t_min, t_max = np.broadcast_to(np.asarray(t_min, np.float64), len(origins)), np.broadcast_to(np.asarray(t_max, np.float64), len(origins))
    return np.array([raycast_one(model, sample, origins[r], directions[r], t_min[r], t_max[r], steps, refine_rounds) for r in range(len(origins))],
                    dtype=HIT_DTYPE)

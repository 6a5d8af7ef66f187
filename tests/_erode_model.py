"""The numpy model of bt_atlas_erode_height: the EROSION section of include/bevy_terrain_amd.h line by line, vectorised over the window.

TEST INFRASTRUCTURE ONLY.  Every plane is float32 and every constant an np.float32, so each written operation rounds once to binary32, as the
header demands; numpy's / and sqrt are correctly rounded and x86 keeps subnormals.  tests/test_erode_model.py holds it to a scalar
restatement written from the text, to a hand-computed step and to the fixed points; tests/test_gpu_erode.py holds the device to it."""
import numpy as np

F32 = np.float32
OFFSETS = [(1, 0), (0, 1), (-1, 0), (0, -1)]  # neighbour k = 0..3 as (dx, dy)
TINY = F32(np.finfo(np.float32).tiny)  # the smallest normal number

DEFAULTS = dict(min_height=0.0, max_height=200.0, cell_size=1.0, dt=0.05, rain=0.5, evaporation=0.3, gravity=9.81, capacity=0.05, erode=0.3, deposit=0.3,
                min_tilt=0.05, min_depth=0.01, steps=1)


def params(**kw):
    """a parameter record: DEFAULTS (the issue's prototype) with the given fields replaced"""
    unknown = set(kw) - set(DEFAULTS)
    assert not unknown, unknown
    return dict(DEFAULTS, **kw)


def constants(p):
    """the host constants of the header, each formed once in binary32"""
    f = {k: F32(v) for k, v in p.items() if k != "steps"}
    c = dict(f)
    c["range"] = f["max_height"] - f["min_height"]
    c["rain_dt"] = f["dt"] * f["rain"]
    c["cf"] = (f["dt"] * f["gravity"]) * f["cell_size"]
    c["l2"] = f["cell_size"] * f["cell_size"]
    c["two_l"] = F32(2) * f["cell_size"]
    with np.errstate(over="ignore"):
        e = f["evaporation"] * f["dt"]
    c["keep"] = F32(1) - (e if e < F32(1) else F32(1))
    return c


def neighbour(plane, k, fill):
    """the plane of every cell's neighbour k; `fill` where the neighbour is outside the window"""
    dx, dy = OFFSETS[k]
    out = np.full_like(plane, fill)
    h, w = plane.shape
    ys, yd = (slice(1, h), slice(0, h - 1)) if dy == 1 else (slice(0, h - 1), slice(1, h)) if dy == -1 else (slice(0, h), slice(0, h))
    xs, xd = (slice(1, w), slice(0, w - 1)) if dx == 1 else (slice(0, w - 1), slice(1, w)) if dx == -1 else (slice(0, w), slice(0, w))
    out[yd, xd] = plane[ys, xs]
    return out


def pos(x):
    return np.where(x > 0, x, F32(0)).astype(F32)


def heights(raw, c):
    return (c["min_height"] + c["range"] * (raw.astype(F32) / F32(65535))).astype(F32)


def count(reached, name, mask):
    if reached is not None:
        reached[name] = reached.get(name, 0) + int(np.count_nonzero(mask))


def step(state, act, c, reached=None):
    """one step on state = (b, d, s, [f0, f1, f2, f3]); returns the next state.  Walls hold zeros in d, s and f and keep b"""
    b, d, s, f = state
    act_n = [neighbour(act, k, False) for k in range(4)]
    with np.errstate(all="ignore"):
        # A
        d1 = np.where(act, d + c["rain_dt"], F32(0)).astype(F32)
        H = b + d1
        fn = []
        for k in range(4):
            t = f[k] + c["cf"] * (H - neighbour(H, k, F32(0)))
            fn.append(np.where(act & act_n[k] & (t > 0), t, F32(0)).astype(F32))
        out = ((fn[0] + fn[1]) + fn[2]) + fn[3]
        leaves, vol = out * c["dt"], d1 * c["l2"]
        limited = act & (leaves > vol)
        K = vol / leaves
        fn = [np.where(limited, fk * K, fk).astype(F32) for fk in fn]
        out = ((fn[0] + fn[1]) + fn[2]) + fn[3]
        # B
        fin = [neighbour(fn[(k + 2) & 3], k, F32(0)) for k in range(4)]
        inflow = ((fin[0] + fin[1]) + fin[2]) + fin[3]
        dn = d1 + (c["dt"] * (inflow - out)) / c["l2"]
        d2 = pos(dn)
        dm0 = F32(0.5) * (d1 + d2)
        deep = dm0 > c["min_depth"]
        dm = np.where(deep, dm0, c["min_depth"]).astype(F32)
        wx = F32(0.5) * ((fin[2] - fn[2]) + (fn[0] - fin[0]))
        wy = F32(0.5) * ((fin[3] - fn[3]) + (fn[1] - fin[1]))
        vx, vy = wx / (c["cell_size"] * dm), wy / (c["cell_size"] * dm)
        speed = np.sqrt(vx * vx + vy * vy)
        bn = [np.where(act_n[k], neighbour(b, k, F32(0)), b).astype(F32) for k in range(4)]
        gx, gy = (bn[0] - bn[2]) / c["two_l"], (bn[1] - bn[3]) / c["two_l"]
        g2 = gx * gx + gy * gy
        sin0 = np.sqrt(g2 / (F32(1) + g2))
        steep = sin0 > c["min_tilt"]
        sin_a = np.where(steep, sin0, c["min_tilt"]).astype(F32)
        C = (c["capacity"] * sin_a) * speed
        takes = C > s
        x_e, x_d = c["erode"] * (C - s), c["deposit"] * (s - C)
        b1 = np.where(takes, b - x_e, b + x_d).astype(F32)
        s1 = np.where(takes, s + x_e, s - x_d).astype(F32)
        # C
        m = [np.where(act & (vol > 0), s1 * ((fn[k] * c["dt"]) / vol), F32(0)).astype(F32) for k in range(4)]
        mo = ((m[0] + m[1]) + m[2]) + m[3]
        mn = [neighbour(m[(k + 2) & 3], k, F32(0)) for k in range(4)]
        mi = ((mn[0] + mn[1]) + mn[2]) + mn[3]
        s2 = pos((s1 - mo) + mi)
        d3 = d2 * c["keep"]
    zero = F32(0)
    nxt = (np.where(act, b1, b).astype(F32), np.where(act, d3, zero).astype(F32), np.where(act, s2, zero).astype(F32), fn)
    if reached is not None:
        count(reached, "k_limited", limited)
        count(reached, "erodes", act & takes)
        count(reached, "deposits", act & ~takes)
        count(reached, "deposits_something", act & ~takes & (x_d > 0))
        count(reached, "at_min_tilt", act & ~steep)
        count(reached, "above_min_tilt", act & steep)
        count(reached, "at_min_depth", act & ~deep)
        count(reached, "above_min_depth", act & deep)
        count(reached, "d2_clamped", act & (dn < 0))
        sub = np.zeros(act.shape, dtype=bool)
        for plane in (nxt[1], nxt[2], *fn):
            sub |= (plane != 0) & (np.abs(plane) < TINY)
        count(reached, "subnormal", act & sub)
        count(reached, "wall_neighbours", act & ~(act_n[0] & act_n[1] & act_n[2] & act_n[3]))
    return nxt


def finish(raw, bT, weight, c, reached=None):
    """the blend and the quantisation: the window's new texels"""
    act = raw != 0
    b0 = heights(raw, c)
    w = np.ones(raw.shape, F32) if weight is None else (weight.astype(F32) / F32(255))
    with np.errstate(all="ignore"):
        h = b0 + (bT - b0) * w
        q = (h - c["min_height"]) / c["range"]
        q01 = np.where(q < 0, F32(0), np.where(q > 1, F32(1), q)).astype(F32)
        new = np.floor(F32(0.5) + F32(65535) * q01)
        new = np.where(new > 1, new, F32(1))
    same = bT.view(np.uint32) == b0.view(np.uint32)
    keep = ~act | (w == 0) | same | ~np.isfinite(h)
    count(reached, "kept_wall", ~act)
    count(reached, "kept_weight_0", act & (w == 0))
    count(reached, "kept_same_bits", act & same)
    count(reached, "kept_not_finite", act & ~np.isfinite(h))
    count(reached, "written", ~keep)
    count(reached, "clamped_to_1", ~keep & (new == 1))
    return np.where(keep, raw, np.where(keep, 0, new).astype(np.uint16)).astype(np.uint16)


def erode(raw, p, weight=None, water=None, sediment=None, reached=None):
    """bt_atlas_erode_height on a window of raw texels (zeros: no data or a missing tile): (new texels, water, sediment, bT)"""
    raw = np.ascontiguousarray(raw, dtype=np.uint16)
    c = constants(p)
    act = raw != 0
    zero = np.zeros(raw.shape, F32)
    b = np.where(act, heights(raw, c), F32(0)).astype(F32)
    d = zero.copy() if water is None else np.where(act, np.asarray(water, F32), F32(0)).astype(F32)
    s = zero.copy() if sediment is None else np.where(act, np.asarray(sediment, F32), F32(0)).astype(F32)
    state = (b, d, s, [zero.copy() for _ in range(4)])
    for _ in range(int(p["steps"])):
        state = step(state, act, c, reached)
    texels = finish(raw, state[0], weight, c, reached)
    return texels, state[1], state[2], state[0]

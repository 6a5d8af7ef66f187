"""tests/_erode_model.py, the numpy model of bt_atlas_erode_height, held to the definition without a GPU: a scalar restatement written cell by
cell from the header's EROSION section (bit for bit on the small cases), a step computed by hand, the fixed points, the walls, the four
keep-the-texel rules, the weight blend, and, for every case tests/test_gpu_erode.py runs on the device, that the case reaches what it is
named for."""
import math

import numpy as np
import pytest

import _erode_cases as EC
import _erode_model as M

F = np.float32


def bits(plane):
    return np.ascontiguousarray(plane, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------- the scalar restatement

def scalar_erode(raw, p, weight=None, water=None, sediment=None):
    """the header's EROSION section cell by cell with np.float32 scalars: (texels, water, sediment)"""
    h, w = raw.shape
    f32 = lambda v: F(v)  # noqa: E731
    lo, hi, l, dt = f32(p["min_height"]), f32(p["max_height"]), f32(p["cell_size"]), f32(p["dt"])
    rng = hi - lo
    rain_dt = dt * f32(p["rain"])
    cf = (dt * f32(p["gravity"])) * l
    l2 = l * l
    two_l = F(2) * l
    with np.errstate(all="ignore"):
        e = f32(p["evaporation"]) * dt
    keep = F(1) - (e if e < F(1) else F(1))
    Kc, Ks, Kd, tilt, depth = (f32(p[k]) for k in ("capacity", "erode", "deposit", "min_tilt", "min_depth"))
    step_of = [(1, 0), (0, 1), (-1, 0), (0, -1)]

    def active(x, y):
        return 0 <= x < w and 0 <= y < h and raw[y, x] != 0

    def pos(v):
        return v if v > 0 else F(0)

    cells = [(x, y) for y in range(h) for x in range(w) if active(x, y)]
    b = {(x, y): lo + rng * (F(raw[y, x]) / F(65535)) for x, y in cells}
    b0 = dict(b)
    d = {(x, y): F(water[y, x]) if water is not None else F(0) for x, y in cells}
    s = {(x, y): F(sediment[y, x]) if sediment is not None else F(0) for x, y in cells}
    f = {c: [F(0)] * 4 for c in cells}
    with np.errstate(all="ignore"):
        for _ in range(p["steps"]):
            d1, fn, out = {}, {}, {}
            for c in cells:
                d1[c] = d[c] + rain_dt
            for c in cells:
                H = b[c] + d1[c]
                new = []
                for k, (dx, dy) in enumerate(step_of):
                    n = (c[0] + dx, c[1] + dy)
                    new.append(pos(f[c][k] + cf * (H - (b[n] + d1[n]))) if active(*n) else F(0))
                o = ((new[0] + new[1]) + new[2]) + new[3]
                if o * dt > d1[c] * l2:
                    K = (d1[c] * l2) / (o * dt)
                    new = [v * K for v in new]
                    o = ((new[0] + new[1]) + new[2]) + new[3]
                fn[c], out[c] = new, o
            b1, s1, d2 = {}, {}, {}
            for c in cells:
                nb = [(c[0] + dx, c[1] + dy) for dx, dy in step_of]
                fin = [fn[n][(k + 2) & 3] if active(*n) else F(0) for k, n in enumerate(nb)]
                total_in = ((fin[0] + fin[1]) + fin[2]) + fin[3]
                d2[c] = pos(d1[c] + (dt * (total_in - out[c])) / l2)
                dm = F(0.5) * (d1[c] + d2[c])
                dm = dm if dm > depth else depth
                wx = F(0.5) * ((fin[2] - fn[c][2]) + (fn[c][0] - fin[0]))
                wy = F(0.5) * ((fin[3] - fn[c][3]) + (fn[c][1] - fin[1]))
                vx, vy = wx / (l * dm), wy / (l * dm)
                speed = np.sqrt(vx * vx + vy * vy)
                bn = [b[n] if active(*n) else b[c] for n in nb]
                gx, gy = (bn[0] - bn[2]) / two_l, (bn[1] - bn[3]) / two_l
                g2 = gx * gx + gy * gy
                sin_a = np.sqrt(g2 / (F(1) + g2))
                sin_a = sin_a if sin_a > tilt else tilt
                C = (Kc * sin_a) * speed
                if C > s[c]:
                    x = Ks * (C - s[c])
                    b1[c], s1[c] = b[c] - x, s[c] + x
                else:
                    x = Kd * (s[c] - C)
                    b1[c], s1[c] = b[c] + x, s[c] - x
            m = {}
            for c in cells:
                vol = d1[c] * l2
                m[c] = [s1[c] * ((fn[c][k] * dt) / vol) if vol > 0 else F(0) for k in range(4)]
            for c in cells:
                nb = [(c[0] + dx, c[1] + dy) for dx, dy in step_of]
                mo = ((m[c][0] + m[c][1]) + m[c][2]) + m[c][3]
                got = [m[n][(k + 2) & 3] if active(*n) else F(0) for k, n in enumerate(nb)]
                mi = ((got[0] + got[1]) + got[2]) + got[3]
                s[c] = pos((s1[c] - mo) + mi)
                d[c] = d2[c] * keep
                b[c] = b1[c]
            f = fn
        texels = raw.copy()
        for c in cells:
            x, y = c
            wt = F(1) if weight is None else F(weight[y, x]) / F(255)
            hgt = b0[c] + (b[c] - b0[c]) * wt
            if wt == 0 or bits(b[c]) == bits(b0[c]) or not math.isfinite(float(hgt)):
                continue
            q = (hgt - lo) / rng
            q = F(0) if q < 0 else F(1) if q > 1 else q
            texels[y, x] = max(1, int(np.floor(F(0.5) + F(65535) * q)))
    d_out, s_out = np.zeros((h, w), np.float32), np.zeros((h, w), np.float32)
    for (x, y) in cells:
        d_out[y, x], s_out[y, x] = d[(x, y)], s[(x, y)]
    return texels, d_out, s_out


SMALL = ["one_cell", "one_column", "one_row", "mosaic_edge", "cube_side_3", "subnormal", "overflow"]


@pytest.mark.parametrize("name", SMALL)
def test_scalar_restatement_agrees_bit_for_bit(name):
    raw, _, new, d, s, _, _ = EC.expected(name)
    weight, water, sediment = EC.inputs(name)
    t2, d2, s2 = scalar_erode(raw, EC.CASES[name]["params"], weight, water, sediment)
    assert np.array_equal(t2, new) and np.array_equal(bits(d2), bits(d)) and np.array_equal(bits(s2), bits(s))


def test_scalar_restatement_on_a_window_with_everything():
    """holes, a weight plane, water and sediment going in, several steps: a cut of the largest case small enough for the scalar loops"""
    raw = EC.terrain(14, 17, 21, holes=[(5, 6, 2, 2), (0, 16, 3, 1)])
    weight, water, sediment = EC.round_weight(14, 17), EC.start_plane(14, 17, 5, 0.4), EC.start_plane(14, 17, 6, 0.05)
    p = M.params(steps=12)
    reached = {}
    new, d, s, _ = M.erode(raw, p, weight, water, sediment, reached)
    t2, d2, s2 = scalar_erode(raw, p, weight, water, sediment)
    assert np.array_equal(t2, new) and np.array_equal(bits(d2), bits(d)) and np.array_equal(bits(s2), bits(s))
    assert all(reached[k] >= 1 for k in ("k_limited", "erodes", "deposits_something", "kept_wall", "kept_weight_0", "written")), reached


# ---------------------------------------------------------------------------------------------- a step by hand

def test_one_step_by_hand_on_two_cells():
    """2 x 1 cells, heights 0 .. 65535, l = 1, dt = 0.5, rain 2 (rain_dt = 1), g = 2 (cf = 1), no evaporation, Kc = 0: every number below is
    exact in binary32.  Left raw 40000 -> b = 40000, right raw 20000 -> b = 20000; d1 = 1 on both; H = 40001 and 20001.
    A.  left: f'[0] = 0 + 1 * (40001 - 20001) = 20000; out * dt = 10000 > d1 * l2 = 1: K = 1 / 10000, f'[0] = 20000 * K.  right: f'[2] = pos(-20000) = 0.
    B.  left: d2 = pos(1 + (0.5 * (0 - out)) / 1); right: d2 = 1 + 0.5 * in."""
    raw = np.array([[40000, 20000]], dtype=np.uint16)
    p = M.params(min_height=0.0, max_height=65535.0, cell_size=1.0, dt=0.5, rain=2.0, evaporation=0.0, gravity=2.0, capacity=0.0, steps=1)
    c = M.constants(p)
    assert (c["rain_dt"], c["cf"], c["l2"], c["two_l"], c["keep"]) == (1.0, 1.0, 1.0, 2.0, 1.0)
    act = raw != 0
    z = np.zeros((1, 2), np.float32)
    b = M.heights(raw, c)
    assert b.tolist() == [[40000.0, 20000.0]]
    b1, d3, s2, f = M.step((b, z.copy(), z.copy(), [z.copy() for _ in range(4)]), act, c)
    K = F(1) / F(10000)
    flux = F(20000) * K
    assert f[0][0, 0] == flux and f[0][0, 1] == 0 and all((f[k] == 0).all() for k in (1, 2, 3))
    left = F(1) + (F(0.5) * (F(0) - flux)) / F(1)
    right = F(1) + (F(0.5) * (flux - F(0))) / F(1)
    assert d3[0, 0] == (left if left > 0 else F(0)) and d3[0, 1] == right
    assert abs(float(d3[0, 0])) < 1e-6 and abs(float(d3[0, 1]) - 2.0) < 1e-6  # all of the left cell's water went to the right one
    assert np.array_equal(b1, b) and (s2 == 0).all()  # capacity 0 and no sediment: C = 0 = s, the deposit branch moves nothing


# ---------------------------------------------------------------------------------------------- the fixed points and the walls

@pytest.mark.parametrize("name", EC.FIXED_POINTS)
def test_fixed_points(name):
    raw, _, new, d, s, bT, reached = EC.expected(name)
    c = M.constants(EC.CASES[name]["params"])
    assert np.array_equal(new, raw)
    assert np.array_equal(bits(bT), bits(np.where(raw != 0, M.heights(raw, c), F(0)))), "a height moved"
    assert (s == 0).all() and reached["written"] == 0
    if name == "flat":
        assert (d[raw != 0] > 0).all() and len(set(bits(d[raw != 0]).tolist())) == 1, "rain falls evenly and goes nowhere"
    if name == "no_water":
        assert (d == 0).all()
    if name == "capacity_0":
        assert reached["k_limited"] >= 1 and len(set(bits(d[raw != 0]).tolist())) > 100, "the water did not move"


def test_walls_take_and_give_nothing():
    """a hole and the window's edge: after any number of steps the walls hold zeros, and the water on the active cells is the rain that
    fell on them less what evaporated (none here), up to rounding: nothing left through a wall"""
    raw = EC.terrain(20, 23, 31, holes=[(7, 9, 4, 5), (0, 0, 2, 2), (19, 22, 1, 1)])
    p = M.params(steps=25, evaporation=0.0, capacity=0.0)
    new, d, s, bT = M.erode(raw, p, None, np.zeros(raw.shape, np.float32), np.zeros(raw.shape, np.float32))
    walls = raw == 0
    assert (d[walls] == 0).all() and (s[walls] == 0).all() and (bT[walls] == 0).all() and np.array_equal(new[walls], raw[walls])
    fell = 25 * 0.05 * 0.5 * np.count_nonzero(~walls)
    assert abs(float(d.astype(np.float64).sum()) - fell) < 1e-4 * fell
    # the state planes going in are forced to 0 on walls
    wet = np.full(raw.shape, 0.5, np.float32)
    _, d_in, s_in, _ = M.erode(raw, M.params(steps=1, rain=0.0, evaporation=0.0), None, wet, wet)
    assert (d_in[walls] == 0).all() and (s_in[walls] == 0).all()


def test_inactive_cells_never_change_and_holes_are_not_filled():
    for name in ("missing_tile_hole_at_block_corner", "several_blocks_t16", "cube_side_3"):
        raw, _, new, d, s, _, reached = EC.expected(name)
        assert np.array_equal(new == 0, raw == 0) and reached["kept_wall"] == np.count_nonzero(raw == 0) > 0


# ---------------------------------------------------------------------------------------------- the finish: keep rules and the blend

def test_the_four_keep_rules_and_the_blend():
    p = M.params()
    c = M.constants(p)
    raw = np.array([[0, 30000, 30000, 30000, 30000, 30000, 30000, 30000]], dtype=np.uint16)
    b0 = M.heights(raw, c)
    bT = b0.copy()
    bT[0, 0] = 50.0                    # a wall: kept whatever its plane holds
    bT[0, 1] += F(10)                  # weight 0: kept
    # [0, 2]: bT == b0 bit for bit: kept although the weight is 255
    bT[0, 3] = np.inf                  # h is not finite: kept
    bT[0, 4] = np.nan
    bT[0, 5] += F(10)                  # weight 255: all of the change
    bT[0, 6] += F(10)                  # weight 128: 128 / 255 of it
    bT[0, 7] = F(-1e6)                 # far below min_height: clamps to q = 0 and the texel becomes 1, never 0
    weight = np.array([[255, 0, 255, 255, 255, 255, 128, 255]], dtype=np.uint8)
    reached = {}
    new = M.finish(raw, bT, weight, c, reached)
    assert new[0, :5].tolist() == [0, 30000, 30000, 30000, 30000]
    assert (reached["kept_wall"], reached["kept_weight_0"], reached["kept_same_bits"], reached["kept_not_finite"]) == (1, 1, 1, 2)

    def quantise(h):
        return max(1, int(np.floor(F(0.5) + F(65535) * ((h - F(0)) / F(200)))))

    assert new[0, 5] == quantise(b0[0, 5] + (bT[0, 5] - b0[0, 5]) * F(1)) == 30000 + round(10 / 200 * 65535)
    assert new[0, 6] == quantise(b0[0, 6] + (bT[0, 6] - b0[0, 6]) * (F(128) / F(255)))
    assert 30000 < new[0, 6] < new[0, 5]
    assert new[0, 7] == 1 and reached["clamped_to_1"] == 1
    # without a weight plane w is 1
    assert M.finish(raw, bT, None, c)[0, 1] == new[0, 5]


def test_a_dt_that_overflows_leaves_the_texels():
    raw, _, new, d, s, bT, reached = EC.expected("overflow")
    assert reached["kept_not_finite"] >= 1 and not np.isfinite(bT[raw != 0]).all()
    changed = new != raw
    assert np.isfinite(bT[changed]).all()


# ---------------------------------------------------------------------------------------------- the GPU cases reach what they are named for

@pytest.mark.parametrize("name", list(EC.CASES))
def test_cases_reach_their_branches(name):
    case = EC.CASES[name]
    raw, missing, new, d, s, bT, reached = EC.expected(name)
    for want in case["reach"]:
        assert reached.get(want, 0) >= 1, (name, want, reached)
    kind, lod, c = EC.geometry(case)
    x0, y0, w, h = case["rect"]
    assert x0 + w <= c << lod and y0 + h <= c << lod
    if name == "missing_tile_hole_at_block_corner":
        B = EC.BLOCK
        assert missing == 1 and (raw[B - 1:B + 1, B - 1:B + 1] == 0).all() and raw[B + 1, B + 1] != 0 and raw[B - 2, B - 2] != 0
        assert {(x0 + dx) // c for dx in (0, w - 1)} == {0, 1} and {(y0 + dy) // c for dy in (0, h - 1)} == {0, 1}
    if name == "mosaic_edge":
        assert x0 + w == c << lod
    if name == "two_blocks_plus_1":
        assert (w, h) == (2 * EC.BLOCK + 1, 2 * EC.BLOCK + 1)
        weight = EC.inputs(name)[0]
        assert ((weight[:, :-1] == 0) & (weight[:, 1:] == 255)).any(), "no weights 0 and 255 next to each other"
    if name == "subnormal":
        assert case["params"]["rain"] == 1e-30 and reached["subnormal"] >= 1


def test_the_cases_together_reach_every_branch():
    union = set()
    for name in EC.CASES:
        union |= {k for k, v in EC.expected(name)[6].items() if v >= 1}
    assert {"k_limited", "erodes", "deposits", "deposits_something", "at_min_tilt", "above_min_tilt", "at_min_depth", "above_min_depth", "d2_clamped", "subnormal",
            "kept_wall", "kept_weight_0", "kept_same_bits", "kept_not_finite", "written", "wall_neighbours"} <= union
    assert {EC.CASES[n]["params"]["steps"] for n in EC.WINDOWS} >= {1, 2, 37}


def test_two_calls_of_five_differ_from_one_of_ten_only_by_the_flux_restart():
    """the model of the resumed call: the state of five steps goes back in; the heights go through the texels (quantised) and the fluxes
    restart at 0, so ten steps in one call give something else"""
    raw, _, new5, d5, s5, _, _ = EC.expected("five_steps_state_out")
    case = EC.CASES["five_steps_state_out"]
    weight, water, sediment = EC.inputs("five_steps_state_out")
    again, d10, s10, _ = M.erode(new5, case["params"], weight, d5, s5)
    once, d_once, s_once, _ = M.erode(raw, dict(case["params"], steps=10), weight, water, sediment)
    assert not np.array_equal(bits(d10), bits(d_once)) and np.isfinite(d10).all() and np.isfinite(d_once).all()
    assert np.abs(again.astype(np.int64) - once.astype(np.int64)).max() < 2000, "the two ways are the same simulation up to the restart"

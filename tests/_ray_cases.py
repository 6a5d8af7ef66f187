"""The cases of tests/test_gpu_ray_shapes.py and tests/test_ray_cases.py: scenes for the three kernels that march rays (raycast_kernel,
render_kernel<false|true>, occlusion_kernel) whose results are closed forms, and terrains on which the ceiling skip of ray_eval
(bt_raycast_device.hpp) takes each of its three forms.  Nothing here runs the package's kernels: test_ray_cases.py asserts without a device
that every case reaches what it is named for, test_gpu_ray_shapes.py compares the device with these expectations.

A. EXACT PLANAR SCENES.  The terrain is the planar entry of MODELS with every texel 65535: the ground is the plane at hi = max_height.
Scene(delta, m, j) is a ray straight down from altitude hi + (m - j / 64) * delta with t_min = 0, t_max = steps * delta, delta a power
of two, so dt == delta and sample i has altitude hi + (m - j / 64 - i) * delta, all exact in binary64.  The first sample at or under the
ground is i = m (for 0 <= j < 64); the refinement's first round finds k = 64 - j (64, nothing, when j == 0) and lands t exactly on the
ground when j > 0, after which every round finds nothing (k == 64) and only t_above moves.  Hence expected_hit.

For cameras whose pixel offsets are not multiples of delta (a width of 17) the same march is run in exact rational arithmetic on the
binary64 pixel origins (exact_march); it returns how close any compared sample came to the ground, which test_ray_cases.py bounds from
below so that no rounding of the kernel's binary64 points can change a comparison.

B. THE CEILING SKIP.  skip_above = border_size >= 1 && max_height >= min_height.  B0: border 0 (off: the bilinear sample extrapolates
half a texel past a tile's first row and column, so the ground can stand above lerp(min, max, 1.0f)); B1: border 1 (on, the smallest
border: plateaus of value exactly 1.0 beside tile edges, met at the ceiling itself); B2: max_height < min_height (off)."""
import math
import types
from fractions import Fraction

import numpy as np

import _oracle as O
import _raycast_model as RM
import _render_model as R
from test_tile_tree_host import MODELS

F = np.float32
OMODEL = MODELS["planar"][1]
POS = np.array([float(OMODEL.position[i]) for i in range(3)])
HI = float(OMODEL.max_height)
GROUND_Y = float(POS[1]) + HI  # the world y of the ground plane (245.0: a small integer, so every scene below is exact)
DOWN, UP = np.array([0.0, -1.0, 0.0]), np.array([0.0, 1.0, 0.0])

# ---- A1: the rays of raycast_kernel ---------------------------------------------------------------------------------------------------------

MARCHES = [(1, 4), (63, 0), (64, 1), (65, 2), (128, 2), (200, 4)]
JS = (0, 1, 31, 63)
DELTAS = (2.0 ** -20, 2.0 ** -4, 1.0, 4.0)


def m_values(steps):
    return sorted({0, 1, 62, 63, 64, 65, 127, 128, steps - 1, steps, steps + 1})


def constant_sampler(pts):
    """h(p) of the all-65535 terrain"""
    return np.full(len(np.asarray(pts).reshape(-1, 3)), F(HI), np.float32)


def expected_hit(origin, delta, m, j, steps, rounds):
    """the closed form of Scene(delta, m, j) marched at (steps, rounds), as a record of _raycast_model.HIT_DTYPE"""
    out = np.zeros((), RM.HIT_DTYPE)
    origin = np.asarray(origin, dtype=np.float64)
    if m - j / 64.0 <= 0.0:
        out["status"], out["position"], out["height"] = RM.INSIDE, origin, F(HI)  # step 0, t = t_above = t_min = 0
        return out
    if m > steps:
        return out  # MISS: every field 0
    if rounds == 0:
        t, t_above = m * delta, (m - 1) * delta
    elif j == 0:
        t, t_above = m * delta, (m - 64.0 ** -rounds) * delta
    else:
        k = 64 - j
        t = (m - 1 + k / 64.0) * delta
        t_above = (m - 1 + (k - 1) / 64.0) * delta if rounds == 1 else t - 64.0 ** -rounds * delta
    out["status"], out["step"], out["t"], out["t_above"], out["height"] = RM.HIT, m, t, t_above, F(HI)
    out["position"] = origin + t * DOWN
    return out


def refine_ks(j, rounds):
    """the k of each refinement round of a HIT of Scene(., ., j)"""
    return [64 - j if (r == 0 and j > 0) else 64 for r in range(rounds)]


def _spot(index):
    """a place over the terrain for ray `index`: whole numbers within 450 of the centre"""
    return POS[0] + float((index * 37) % 901 - 450), POS[2] + float((index * 101) % 901 - 450)


def a1_batch(steps, rounds):
    """every Scene(delta, m, j) of the march, then six rays with t_min == t_max (dt == 0: every sample is the one point p(t_min)), under,
    on and above the ground.  -> namespace of origins, directions, t_min, t_max, expected (HIT_DTYPE), m, j, delta (nan / -1 for the
    last six)"""
    rows = []
    for delta in DELTAS:
        for m in m_values(steps):
            for j in JS:
                x, z = _spot(len(rows))
                origin = np.array([x, GROUND_Y + (m - j / 64.0) * delta, z])
                rows.append((origin, 0.0, steps * delta, expected_hit(origin, delta, m, j, steps, rounds), m, j, delta))
    for delta in (2.0 ** -20, 1.0):
        for off in (-1.0, 0.0, 1.0):  # p(t_min) at altitude hi + off * delta
            x, z = _spot(len(rows))
            origin, tau = np.array([x, GROUND_Y + (3.0 + off) * delta, z]), 3.0 * delta
            exp = np.zeros((), RM.HIT_DTYPE)
            if off <= 0.0:
                exp["status"], exp["t"], exp["t_above"], exp["position"], exp["height"] = RM.INSIDE, tau, tau, origin + tau * DOWN, F(HI)
            rows.append((origin, tau, tau, exp, -1, -1, float("nan")))
    b = types.SimpleNamespace(steps=steps, rounds=rounds)
    b.origins = np.array([r[0] for r in rows])
    b.directions = np.tile(DOWN, (len(rows), 1))
    b.t_min, b.t_max = np.array([r[1] for r in rows]), np.array([r[2] for r in rows])
    b.expected = np.array([r[3] for r in rows], dtype=RM.HIT_DTYPE)
    b.m, b.j, b.delta = np.array([r[4] for r in rows]), np.array([r[5] for r in rows]), np.array([r[6] for r in rows])
    return b


# ---- the same march in exact arithmetic, for any altitude ------------------------------------------------------------------------------------

def exact_march(a, steps, rounds):
    """a ray straight down from altitude hi + a * delta (a: a Fraction), t_max = steps * delta -> (status, step, t_above / delta,
    t / delta, [k of each round], margin): the march of the definition in rational arithmetic.  margin is the smallest |u - a| over the
    samples u (in units of delta) next to each decision, 0 when a sample lies exactly on the ground (then f == 0 exactly: every scene
    whose offsets are multiples of delta / 64)"""
    a = Fraction(a)
    if a <= 0:
        return RM.INSIDE, 0, Fraction(0), Fraction(0), [], -a
    m = math.ceil(a)
    if m > steps:
        return RM.MISS, 0, Fraction(0), Fraction(0), [], a - steps
    lo, hi, ks = Fraction(m - 1), Fraction(m), []
    margin = min(a - lo, hi - a)
    for _ in range(rounds):
        width = hi - lo
        k = next((k for k in range(1, 64) if lo + width * Fraction(k, 64) >= a), 64)
        lo, hi = lo + width * Fraction(k - 1, 64), (hi if k == 64 else lo + width * Fraction(k, 64))
        ks.append(k)
        margin = min(margin, a - lo, hi - a)
    return RM.HIT, m, lo, hi, ks, margin


# ---- A2: cameras of render_kernel ------------------------------------------------------------------------------------------------------------

SUN = tuple(float(v) for v in R._unit((0.3, 0.8, 0.5)))
BACKGROUND = (10, 20, 30, 255)
# (width, height, steps, rounds, delta, base): the camera's origin is base * delta above the ground
A2_CAMERAS = [
    (8, 8, 200, 0, 0.25, Fraction(151)),              # m = 88 .. 214, even, within the block: HIT up to m == steps and, beyond, MISS
    (8, 8, 200, 0, 0.25, Fraction(41)),               # m = -22 .. 104: INSIDE (one pixel exactly on the ground) and HIT
    (8, 8, 128, 2, 0.25, Fraction(101) - Fraction(31, 64)),   # j = 31: k = 33, then 64; m = 38 .. 164: HIT up to m == steps, and MISS
    (8, 8, 128, 2, 0.25, Fraction(41) - Fraction(31, 64)),    # INSIDE and HIT
    (17, 9, 200, 0, 1.0, Fraction(150) + Fraction(3, 8)),
    (17, 9, 128, 2, 1.0, Fraction(60) + Fraction(3, 8) + Fraction(1, 448)),
]


def ortho_camera(width, height, steps, delta, base, sun=SUN, lighting=True, right_x=64.0, up_z=-48.0):
    """an orthographic camera straight down whose right and up vectors have vertical components 8 delta and 64 delta: at 8 x 8 pixel
    (x, y) starts ((2 x - 7) + 8 (7 - 2 y)) * delta above the camera's origin, 64 different odd multiples spanning 126 steps"""
    origin = (POS[0] + 20.0, GROUND_Y + float(base) * delta, POS[2] - 30.0)
    return R.camera(origin, DOWN, (right_x, 8.0 * delta, 0.0), (0.0, 64.0 * delta, up_z), width, height, 0.0, steps * delta, orthographic=True,
                    lighting=lighting, sun=sun, ambient=0.25, background=BACKGROUND)


def pixel_offsets(c, delta):
    """a of every pixel, row-major: (the binary64 y of the pixel's origin by the header's formula - the ground's y) / delta, exactly"""
    return [(Fraction(float(y)) - Fraction(GROUND_Y)) / Fraction(delta) for y in R.rays(c)[0][:, 1]]


def expected_planes(c, steps, rounds, delta):
    """t, status and the stats of the camera's picture from exact_march -> namespace(t, status, stats, step, ks, margin)"""
    marches = [exact_march(a, steps, rounds) for a in pixel_offsets(c, delta)]
    out = types.SimpleNamespace()
    out.status = np.array([m[0] for m in marches], np.uint8).reshape(c.height, c.width)
    out.step = np.array([m[1] for m in marches]).reshape(c.height, c.width)
    out.t = np.array([float(m[3]) * delta for m in marches]).reshape(c.height, c.width)  # (a dyadic rational of few bits: exact)
    out.ks = [m[4] for m in marches]
    out.margin = min(m[5] for m in marches)
    out.stats = dict(launches=R.launches(c.width, c.height, steps, rounds)[0], hit_pixels=int((out.status == RM.HIT).sum()),
                     inside_pixels=int((out.status == RM.INSIDE).sum()), miss_pixels=int((out.status == RM.MISS).sum()))
    return out


# ---- A3: points of occlusion_kernel, and the shadow plane of the A2 pictures -----------------------------------------------------------------

A3_COUNT, A3_STEPS, A3_DELTA, A3_LIFT = 70, 65, 0.25, 2.0  # (the lift in units of delta)


def a3_points():
    """70 points q_g at altitude hi + m_g * delta - lift, m_g = g - 2 (-2 .. 67): lifted, the shadow ray of point g starts m_g * delta above
    the ground.  Two directions, down and up, distance = steps * delta.  Ray g of the launch is point g % 70 of direction g / 70: rays 64 ..
    69 are in the second wave with the first 58 rays of the up direction.  -> points, directions, m, expected (70, 2)"""
    g = np.arange(A3_COUNT)
    m = g - 2
    points = np.column_stack([POS[0] + 3.0 * g - 100.0, GROUND_Y + (m - A3_LIFT) * A3_DELTA, POS[2] - 2.0 * g + 60.0])
    down = np.where(m <= 0, RM.INSIDE, np.where(m <= A3_STEPS, RM.HIT, RM.MISS))
    up = np.where(m <= 0, RM.INSIDE, RM.MISS)
    return points, np.array([DOWN, UP]), m, np.stack([down, up], axis=1).astype(np.uint8)


SHADOW_LIFT, SHADOW_STEPS, SHADOW_DS = 2.0, 4, 2.0  # in units of delta: distance = SHADOW_STEPS * SHADOW_DS * delta


def expected_shadow(exp, offsets, sun_up):
    """the SHADOW PLANE of a picture marched without refinement from whole offsets: a HIT pixel's point lies on the ground, an INSIDE
    pixel's at its origin, a offsets under it; lifted by SHADOW_LIFT its shadow ray starts e above the ground: INSIDE for e <= 0, else
    lit under a sun straight up, and under a sun straight down HIT at step ceil(e / SHADOW_DS) if that is within SHADOW_STEPS"""
    out = np.full(exp.status.shape, 255, np.uint8)
    for i, a in enumerate(offsets):
        y, x = divmod(i, exp.status.shape[1])
        if exp.status[y, x] == RM.MISS:
            continue
        e = (Fraction(0) if exp.status[y, x] == RM.HIT else a) + Fraction(SHADOW_LIFT)
        if e <= 0:
            out[y, x] = RM.INSIDE
        elif sun_up:
            out[y, x] = RM.MISS
        else:
            out[y, x] = RM.HIT if math.ceil(e / Fraction(SHADOW_DS)) <= SHADOW_STEPS else RM.MISS
    return out


# ---- A4: the render's short launch -----------------------------------------------------------------------------------------------------------

A4 = types.SimpleNamespace(width=488, height=8, steps=4096, rounds=4, delta=2.0 ** -4, base=Fraction(4090) - Fraction(31, 64))


def a4_camera():
    """488 x 8 at (4096, 4): 61 blocks of 64 * (4097 + 252) worst-case samples, 60 to a launch: less than one row of blocks.  Only the up
    vector has a vertical component (8 delta: row y starts (7 - 2 y) * delta above the origin), the width not being a power of two.  The
    origin is 4090 - 31 / 64 steps above the ground: m = 4083 .. 4097, so the last row but for its refinement is above the ground all
    the way, row 0 misses (m = 4097 > steps), and all but the last few samples of every ray are above the ceiling."""
    origin = (POS[0], GROUND_Y + float(A4.base) * A4.delta, POS[2])
    return R.camera(origin, DOWN, (400.0, 0.0, 0.0), (0.0, 8.0 * A4.delta, -40.0), A4.width, A4.height, 0.0, A4.steps * A4.delta, orthographic=True,
                    lighting=False, background=BACKGROUND)


# ---- B: terrains for the three forms of the ceiling skip -------------------------------------------------------------------------------------

def b0_tile(tile):
    """border 0: the tile's relief at half height, its edge rows and columns saturated.  Within half a texel of a tile's first row or
    column the bilinear sample extrapolates (t = uv * T - 0.5 < 0 keeps texels 0 and 1 with a negative weight): value up to 1.27"""
    out = (tile // 2 + 8000).astype(np.uint16)
    out[[0, -1], :] = 65535
    out[:, [0, -1]] = 65535
    return out


def b1_tile(tile):
    """border 1: 65535 on the border, on the centre's edge and beside it: a plateau of value exactly 1.0 one and a half texels wide"""
    out = (tile // 2 + 8000).astype(np.uint16)
    out[[0, 1, 2, -3, -2, -1], :] = 65535
    out[:, [0, 1, 2, -3, -2, -1]] = 65535
    return out


def ceiling(omodel):
    """lerp(min_height, max_height, 1.0f) in binary32, widened"""
    return float(F(omodel.min_height) + (F(omodel.max_height) - F(omodel.min_height)) * F(1.0))


def b0_rays(omodel, n=96, seed=41):
    """grazing rays over the planar terrain at altitudes between hi and hi + 0.2 span, level to within 0.02, 400 long: they cross the edges
    of tiles of every LOD, where the border-0 ground stands above the ceiling"""
    rng = np.random.default_rng(seed)
    pos = np.array([float(omodel.position[i]) for i in range(3)])
    hi, span = float(omodel.max_height), float(omodel.max_height) - float(omodel.min_height)
    origins = pos + np.column_stack([rng.uniform(-300, 300, n), hi + rng.uniform(0.0, 0.2, n) * span, rng.uniform(-300, 300, n)])
    angle = rng.uniform(0.0, 2.0 * np.pi, n)
    directions = np.column_stack([np.cos(angle), rng.uniform(0.0, 0.02, n), np.sin(angle)])  # level or rising: every sample above the ceiling
    return origins, directions, np.zeros(n), np.full(n, 400.0)


def hits_above_ceiling(omodel, hits):
    """of the model's hits: (HIT at a position whose altitude is above the ceiling, MISS)"""
    hit = hits["status"] == RM.HIT
    above = RM.altitude(omodel, hits["position"][hit]) > ceiling(omodel)
    return int(above.sum()), int((hits["status"] == RM.MISS).sum())


def up_vectors(omodel, view, n, rng):
    """n ground points of the height-0 surface near the view and their up vectors (test_gpu_raycast.py's ceiling test places them so)"""
    pos = np.array([float(omodel.position[i]) for i in range(3)])
    if int(omodel.kind) == 0:
        up = np.tile(UP, (n, 1))
        return pos + np.column_stack([rng.uniform(-450, 450, n), np.zeros(n), rng.uniform(-450, 450, n)]), up
    radial = np.asarray(view, dtype=np.float64) - pos
    up = radial / np.linalg.norm(radial) + rng.normal(size=(n, 3)) * 0.2
    up /= np.linalg.norm(up, axis=1, keepdims=True)
    return pos + up * float(omodel.a), up


B1_DELTA = 2.0 ** -8


def b1_rays(omodel, view, sample, seed=43, candidates=600, each=24):
    """rays straight down in 128 steps of delta from 64 delta above the ceiling, so sample 64 is at the ceiling to within the rounding of
    the altitude: `each` of them over the plateaus beside tile edges (where the model's h is exactly f32(hi)) and `each` elsewhere"""
    rng = np.random.default_rng(seed)
    ground, up = up_vectors(omodel, view, candidates, rng)
    hi = float(omodel.max_height)
    flat = sample(ground + up * hi) == F(hi)
    pick = np.concatenate([np.flatnonzero(flat)[:each], np.flatnonzero(~flat)[:each]])
    assert flat.sum() >= each and (~flat).sum() >= each, (flat.sum(), len(flat))
    origins = ground[pick] + up[pick] * (hi + 64.0 * B1_DELTA)
    return origins, -up[pick], np.zeros(len(pick)), np.full(len(pick), 128.0 * B1_DELTA)


def met_at_the_ceiling(omodel, hits):
    """how many of the model's hits have h == f32(hi) at a position whose altitude is in (ceiling - delta, ceiling]"""
    hit = hits["status"] == RM.HIT
    alt = RM.altitude(omodel, hits["position"][hit])
    c = ceiling(omodel)
    return int(((alt > c - B1_DELTA) & (alt <= c) & (hits["height"][hit] == F(omodel.max_height))).sum())


def inverted_models():
    """the planar MODELS entry with its height range inverted: (TerrainModel, oracle model)"""
    import bevy_terrain_amd as bt
    return (bt.TerrainModel.planar((10.0, -5.0, 3.0), 1000.0, 250.0, 0.0), O.make_model("planar", (10.0, -5.0, 3.0), 1000.0, 0.0, 250.0, 0.0))


def geometric_range(omodel):
    """what make_rays reads of a model, with min_height / max_height the lowest and highest ground: the rays of families A to D are
    placed by where the ground is, whichever way the model's range runs"""
    lo, hi = sorted((float(omodel.min_height), float(omodel.max_height)))
    return types.SimpleNamespace(kind=omodel.kind, position=omodel.position, a=omodel.a, b=omodel.b, min_height=lo, max_height=hi)

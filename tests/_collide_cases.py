"""The inputs of tests/test_gpu_collide.py and the conditions they must satisfy, without the package: spheres made from the model's ray hit
positions moved along the up direction by multiples of their radius, sweeps of such spheres, and the counts the batches must reach.
tests/test_collide_model.py asserts the conditions on a terrain built without a device, test_gpu_collide.py on the device's terrain
before the device is asked.

Below those, the cases of tests/test_gpu_collide_shapes.py and tests/test_collide_cases.py (sections A to D there): scenes for
collide_kernel and sweep_kernel whose results are closed forms, a terrain on which two lanes of a round tie below the foot, and inputs
that meet each of the three forms of the ceiling skip.  Nothing here runs the package's kernels: test_collide_cases.py asserts without a
device that every case reaches what it is named for, test_gpu_collide_shapes.py compares the device with these expectations."""
import types
from fractions import Fraction

import numpy as np

import _collide_model as CM
import _oracle as O
import _ray_cases as RC
import _raycast_model as RM
from _ray_cases import up_vectors

# the centre is placed k radii above the ray's hit position (which lies at or just under the ground): under it, inside, grazing, clear,
# and so far clear that even the gentle slopes of the globes (a texel is tens of kilometres) move the nearest point off the foot
MULTIPLES = (-1.5, -0.25, 0.0, 0.5, 0.9, 0.99, 1.01, 1.5, 3.0, 0.7, 12.0, 25.0)
RADII = (0.5, 2.0, 8.0, 32.0)
FAR_COUNT, SPHERES = 8, 270  # 270 spheres: 68 workgroups of four waves, the last one half full


def _ranges(omodel):
    lo, hi = float(omodel.min_height), float(omodel.max_height)
    return lo, hi, hi - lo


def _drop(omodel):
    """how far a ray straight down from up_vectors' points lifted by hi + 0.05 span must go to pass the lowest ground (those points lie on
    the sphere of radius a, up to a - b above the ellipsoid)"""
    lo, hi, span = _ranges(omodel)
    return 1.2 * span + (float(omodel.a) - float(omodel.b) if int(omodel.kind) == 2 else 0.0)


def make_spheres(omodel, sample, view, n=SPHERES, seed=31):
    """-> (centers (n, 3), radii (n,)): n - FAR_COUNT - 1 spheres around the ground (three of radius 0), FAR_COUNT above the ceiling by more than their
    radius, and one whose centre has a NaN"""
    rng = np.random.default_rng(seed)
    lo, hi, span = _ranges(omodel)
    m = n - FAR_COUNT - 1
    ground, up = up_vectors(omodel, view, n, rng)
    hits = RM.raycast(omodel, sample, ground[:m] + up[:m] * (hi + 0.05 * span), -up[:m], 0.0, _drop(omodel), 64, 2)
    assert (hits["status"] == RM.HIT).all()
    radii = np.array([RADII[i % len(RADII)] for i in range(n)]) * (1.0 if int(omodel.kind) == 0 else 40.0)  # (a texel of the globes is kilometres wide)
    k = np.array([MULTIPLES[(i // len(RADII)) % len(MULTIPLES)] for i in range(m)])
    centers = np.empty((n, 3))
    centers[:m] = hits["position"] + up[:m] * (k * radii[:m])[:, None]
    for i in (5, 17, 29):  # radius 0: every stencil point is the centre, the foot stays whatever R
        radii[i] = 0.0
        centers[i] = hits["position"][i] + up[i] * (3.0 * RADII[i % len(RADII)] * (1.0 if int(omodel.kind) == 0 else 40.0))
    centers[m:n - 1] = ground[m:n - 1] + up[m:n - 1] * (hi + radii[m:n - 1] * rng.uniform(1.5, 4.0, FAR_COUNT))[:, None]
    centers[n - 1] = centers[0]
    centers[n - 1, 1] = np.nan
    order = rng.permutation(n)  # the kinds mixed through the batch, so that every prefix holds several
    return centers[order], radii[order]


def contact_figures(contacts):
    status = contacts["status"]
    searched = (status == CM.TOUCHING) | (status == CM.NONE)
    candidate = contacts["candidate"][searched]
    return dict(touching=int((status == CM.TOUCHING).sum()), none=int((status == CM.NONE).sum()), below=int((status == CM.BELOW).sum()),
                far=int((status == CM.FAR).sum()), invalid=int((status == CM.INVALID).sum()), foot=int((candidate == 0).sum()),
                round0=int(((candidate >= 1) & (candidate <= 64)).sum()), later=int((candidate > 64).sum()))


def assert_contact_mix(figures, refine_rounds):
    """conditions on the INPUT, from the model's contacts"""
    assert figures["touching"] >= 20 and figures["none"] >= 20 and figures["below"] >= 20, figures
    assert figures["far"] >= 5 and figures["invalid"] >= 1, figures
    # winners: the foot at every R (the spheres of radius 0 at least); with one round only round 0 can win, with more a later round
    # improves on it wherever the ground is not flat
    assert figures["foot"] >= 3, figures
    assert figures["round0" if refine_rounds == 0 else "later"] >= 3, figures


SWEEPS = 36


def make_sweeps(omodel, sample, view, n=SWEEPS, seed=47):
    """-> namespace(origins, directions, radii, t_min, t_max): spheres coming down on the ground steeply and obliquely (HIT), starting in
    touch with it or under it (INSIDE), moving level above the relief (MISS), and four that cannot be marched (INVALID)"""
    rng = np.random.default_rng(seed)
    lo, hi, span = _ranges(omodel)
    scale = 1.0 if int(omodel.kind) == 0 else 40.0
    ground, up = up_vectors(omodel, view, n, rng)
    side = np.cross(up, rng.normal(size=(n, 3)))
    side /= np.linalg.norm(side, axis=1, keepdims=True)
    hits = RM.raycast(omodel, sample, ground + up * (hi + 0.05 * span), -up, 0.0, _drop(omodel), 64, 2)
    assert (hits["status"] == RM.HIT).all()
    surface = hits["position"]
    s = types.SimpleNamespace()
    s.radii = np.array([RADII[i % len(RADII)] for i in range(n)]) * scale
    s.origins, s.directions = np.empty((n, 3)), np.empty((n, 3))
    s.t_min, s.t_max = np.zeros(n), np.empty(n)
    for i in range(n):
        family = i % 4
        if family in (0, 1):  # down from 0.3 .. 0.8 span above the surface point, family 1 with a sideways drift; not normalised
            height = rng.uniform(0.3, 0.8) * span
            s.origins[i] = surface[i] + up[i] * height
            s.directions[i] = (-up[i] + side[i] * (rng.uniform(0.2, 0.8) if family == 1 else 0.0)) * height
            s.t_max[i] = rng.uniform(1.1, 1.5)
        elif family == 2:  # starts within its radius of the ground, or under it
            s.origins[i] = surface[i] + up[i] * (s.radii[i] * rng.choice([-0.5, 0.3, 0.8]))
            s.directions[i] = side[i] + up[i] * rng.uniform(-0.2, 0.2)
            s.t_max[i] = 10.0 * scale
        else:  # level flight above the highest ground
            s.origins[i] = ground[i] + up[i] * (hi + s.radii[i] * rng.uniform(1.2, 2.0))
            s.directions[i] = side[i]
            s.t_max[i] = 20.0 * scale
    s.t_min[::5] = 0.05 * s.t_max[::5]
    s.radii[n - 1] = -1.0
    s.directions[n - 2] = 0.0
    s.origins[n - 3, 2] = np.inf
    s.t_max[n - 4] = np.nan
    return s


def assert_sweep_mix(hits, steps):
    status = hits["status"]
    counts = np.bincount(status, minlength=4)
    assert counts[CM.RAY_INVALID] == 4 and counts[CM.INSIDE] >= 4 and counts[CM.MISS] >= 4, counts
    if steps > 1:
        assert counts[CM.HIT] >= 8, counts
    else:
        assert counts[CM.HIT] >= 1, counts


# ==== the cases of test_gpu_collide_shapes.py ==================================================================================================

F = np.float32

# ---- terrain P: the exact plane -----------------------------------------------------------------------------------------------------------------
# planar, centred on (0, -8, 0), side 1024, heights 0 .. 256, every texel 65535: the ground is y = 248, the altitude of a point y + 8,
# h = 256.0f whatever the LOD and the blend ratio (1 + (1 - 1) * ratio), and the ceiling lerp(0, 256, 1.0f) = 256 is the ground itself.
# Every number of sections A and B is a small binary fraction: each operation of the definition is exact, "equal" means the same bits.
P_POSITION, P_SIDE, P_MIN, P_MAX = (0.0, -8.0, 0.0), 1024.0, 0.0, 256.0
P_GROUND_Y, P_H = 248.0, 256.0
P_OMODEL = O.make_model("planar", P_POSITION, P_SIDE, 0.0, P_MIN, P_MAX)


def plane_models():
    """(TerrainModel, oracle model) of terrain P, as test_gpu_raycast.Streamed takes them"""
    import bevy_terrain_amd as bt
    return bt.TerrainModel.planar(P_POSITION, P_SIDE, P_MIN, P_MAX), P_OMODEL


def plane_sampler(pts):
    """h(p) of terrain P"""
    return np.full(len(np.asarray(pts).reshape(-1, 3)), F(P_H), np.float32)


def _exact(q):
    """a rational as the binary64 it must be"""
    v = float(q)
    assert Fraction(v) == q, q
    return v


def _spot(index):
    """a place over terrain P for case `index`: whole numbers within 400 of the origin"""
    return float((index * 37) % 801 - 400), float((index * 101) % 801 - 400)


def plane_contact(x, alt, z, r):
    """SPHERE CONTACT on terrain P of the centre (x, 248 + alt, z) and the radius r >= 0, in closed form: the ground is flat, so the foot is
    the nearest point whatever R (a lane's d2 = x^2 + alt^2 + y^2 is never below alt^2, and at r == 0 equals it: strictly, the foot stays);
    the ceiling is the ground, so a - r > ceiling is alt > r"""
    out = np.zeros((), CM.CONTACT_DTYPE)
    alt, r = np.float64(alt), np.float64(r)
    if alt > r:
        out["status"] = CM.FAR
        return out
    out["distance"], out["depth"], out["point"], out["height"] = alt, r - alt, (x, P_GROUND_Y, z), F(P_H)
    if alt <= 0.0:
        out["status"], out["normal"] = CM.BELOW, (0.0, 1.0, 0.0)
    else:  # (c - point) * (1.0 / distance): the product is not always 1
        out["status"], out["normal"] = (CM.TOUCHING if alt < r else CM.NONE), (0.0, alt * (1.0 / alt), 0.0)
    return out


# ---- A: contacts on P ---------------------------------------------------------------------------------------------------------------------------

A_RADII = (0.0, 2.0 ** -30, 0.5, 1.5, 7.0, 200.0)
A_ROUNDS = (0, 2, 6)
A_INVALID = [((np.nan, 100.0, 0.0), 1.0), ((0.0, np.inf, 0.0), 1.0), ((0.0, 100.0, -np.inf), 1.0), ((0.0, 100.0, 0.0), np.nan), ((0.0, 100.0, 0.0), np.inf),
             ((0.0, 100.0, 0.0), -2.0 ** -60)]  # test_collide_model.test_flat_ground_statuses_at_their_edges'
PICKS = (1, 3, 4, 5)  # the counts below, at and above the four waves of a workgroup
# beside the grid, whose every alt * (1.0 / alt) happens to be 1: altitudes for which the normal's y is 1 - 2^-53 (49 * (1.0 / 49) < 1)
A_EXTRA = [(7.0, 49.0 / 64.0), (1.5, 49.0 / 64.0), (200.0, 49.0), (0.5, 49.0 / 64.0)]


def a_altitudes(r):
    """under the ground, on it, just above it, just inside the radius, at it (NONE with depth 0, not FAR), just beyond it (FAR), far"""
    e = 2.0 ** -40
    return sorted({-300.0, -0.5, 0.0, e, r, r + e, 2.0 * r, 300.0} | ({r - e} if r - e > 0.0 else set()))


def a_batch():
    """-> namespace(centers, radii, expected (CONTACT_DTYPE), searched): every (r, alt) of the grid and the six INVALID inputs, ordered so
    that every workgroup of four waves holds waves that leave early (INVALID, FAR, BELOW) and waves that search"""
    rows = []
    for r, alt in [(r, alt) for r in A_RADII for alt in a_altitudes(r)] + A_EXTRA:
        x, z = _spot(len(rows))
        assert np.float64(P_GROUND_Y) + alt - P_GROUND_Y == alt  # the centre's y holds alt exactly
        rows.append(((x, P_GROUND_Y + alt, z), r, plane_contact(x, alt, z, r)))
    invalid = np.zeros((), CM.CONTACT_DTYPE)
    invalid["status"] = CM.INVALID
    rows += [(c, r, invalid) for c, r in A_INVALID]
    searching = [row for row in rows if int(row[2]["status"]) in (CM.NONE, CM.TOUCHING)]
    early = [row for row in rows if int(row[2]["status"]) not in (CM.NONE, CM.TOUCHING)]
    assert len(rows) % 4 == 0 and len(searching) >= len(rows) // 4
    groups = [[] for _ in range(len(rows) // 4)]
    for k, row in enumerate(searching):
        groups[k % len(groups)].append(row)
    for g in groups:
        while len(g) < 4:
            g.append(early.pop())
    assert not early
    rows = [g[(k + i) % 4] for i, g in enumerate(groups) for k in range(4)]  # the searching wave at another place in each workgroup
    b = types.SimpleNamespace()
    b.centers, b.radii = np.array([row[0] for row in rows]), np.array([row[1] for row in rows])
    b.expected = np.array([row[2] for row in rows], dtype=CM.CONTACT_DTYPE)
    b.searched = np.isin(b.expected["status"], (CM.NONE, CM.TOUCHING))
    return b


def picks(n, count):
    """`count` indices into a batch of n, spread over it"""
    return (5 + 9 * np.arange(count)) % n


# ---- B: sweeps on P -----------------------------------------------------------------------------------------------------------------------------
# A sweep straight down (direction y == -1) from alt0 = r + e * delta with t_min = tau * delta and t_max = t_min + steps * delta, delta a
# power of two: dt == delta, and in units of delta sample u has altitude r + (e - u).  blocked(u) is distance < r, u > e, for r > 0 (a
# sample exactly at grazing is NONE) and f <= 0, u >= e, for r == 0.

B_MARCHES = [(1, 0), (1, 20), (7, 1), (64, 0), (65, 5), (200, 32)]
B_ROUNDS = (0, 1)
B_RADII = (0.0, 1.5)
B_DELTAS = (0.25, 2.0 ** -10, 1.0)
B_RHOS = (Fraction(0), Fraction(5, 16), 1 - Fraction(1, 2 ** 30))  # test_collide_model.test_vertical_descent_onto_flat_ground's
OBLIQUE = (3.0, -1.0, 2.0)  # not unit, not vertical: the altitude still falls by t, the point moves by (3 t, 2 t)


def exact_sweep(e, tau, steps, bisections, strict, moving=True):
    """the march of SPHERE SWEEP in rational arithmetic, in units of delta: samples u_i = tau + i (tau when not `moving`: t_min == t_max,
    dt == 0), blocked(u) = u > e (strict: r > 0) or u >= e -> (status, step, t_above, t, [every u at which a contact is evaluated])"""
    e, tau = Fraction(e), Fraction(tau)
    blocked = (lambda u: u > e) if strict else (lambda u: u >= e)
    dt = Fraction(1 if moving else 0)
    seen = []
    step = None
    for i in range(steps + 1):
        seen.append(tau + i * dt)
        if blocked(seen[-1]):
            step = i
            break
    if step is None:
        return CM.MISS, 0, Fraction(0), Fraction(0), seen
    if step == 0:
        return CM.INSIDE, 0, tau, tau, seen + [tau]
    lo, hi = tau + (step - 1) * dt, tau + step * dt
    for _ in range(bisections):
        mid = lo + (hi - lo) / 2
        seen.append(mid)
        if blocked(mid):
            hi = mid
        else:
            lo = mid
    return CM.HIT, step, lo, hi, seen + [hi]


def b_cases(steps):
    """(name, e - tau in units of delta as a function of r / delta, moving) of one march: where the edge lies, counted from sample 0"""
    half, mid = Fraction(1, 2), (steps + 1) // 2
    cases = [("step 1", lambda k: half, True), ("step `steps`", lambda k: steps - half, True), ("first at steps + 1", lambda k: steps + half, True),
             ("grazing at sample steps - 1", lambda k: Fraction(steps - 1), True), ("grazing at sample `steps`", lambda k: Fraction(steps), True),
             ("inside, e < 0", lambda k: -half, True), ("on the ground", lambda k: -k, True), ("under the ground", lambda k: -k - 1, True),
             ("dt == 0, blocked", lambda k: -half, False), ("dt == 0, clear", lambda k: half, False)]
    for m in sorted({1, mid, steps}):
        for rho in B_RHOS:
            cases.append((f"edge m {m} rho {float(rho):g}", lambda k, v=m - 1 + rho: v, True))
    return cases


def b_batch(steps, bisections):
    """-> namespace(origins, directions, radii, t_min, t_max, expected (SWEEP_DTYPE), names): every case at both radii, each with another
    delta, tau and place and every third one oblique, then the four INVALID sweeps of make_sweeps"""
    rows = []
    for name, e_of, moving in b_cases(steps):
        for r in B_RADII:
            index = len(rows)
            oblique = index % 3 == 1
            delta = Fraction(0.25 if oblique else B_DELTAS[(index // 2) % len(B_DELTAS)])
            tau = Fraction(3 * (index % 2)) if moving else Fraction(3)
            e = tau + Fraction(e_of(Fraction(r) / delta))  # (the cases count from the first sample)
            status, step, lo, hi, seen = exact_sweep(e, tau, steps, bisections, r > 0.0, moving)
            x, z = _spot(index)
            x, z = np.trunc(x / 2.0), np.trunc(z / 2.0)  # (whole numbers within 200: room for the oblique ones to move)
            d = OBLIQUE if oblique else (0.0, -1.0, 0.0)
            y0 = Fraction(P_GROUND_Y) + Fraction(r) + e * delta
            for u in seen:  # every centre the march visits is exact in binary64
                _exact(y0 - u * delta), _exact(Fraction(x) + Fraction(d[0]) * u * delta), _exact(Fraction(z) + Fraction(d[2]) * u * delta)
            exp = np.zeros((), CM.SWEEP_DTYPE)
            if status != CM.MISS:
                t = _exact(hi * delta)
                exp["status"], exp["step"], exp["t"], exp["t_above"] = status, step, t, _exact(lo * delta)
                exp["contact"] = plane_contact(x + d[0] * t, _exact(Fraction(r) + (e - hi) * delta), z + d[2] * t, r)
            t_min = _exact(tau * delta)
            rows.append(((x, _exact(y0), z), d, r, t_min, _exact(tau * delta + steps * delta) if moving else t_min, exp, f"{name}, r {r:g}"))
    origin = (5.0, P_GROUND_Y + 10.0, -3.0)
    invalid = np.zeros((), CM.SWEEP_DTYPE)
    invalid["status"] = CM.RAY_INVALID
    for change in (dict(r=-1.0), dict(d=(0.0, 0.0, 0.0)), dict(origin=(5.0, P_GROUND_Y + 10.0, np.inf)), dict(t_max=np.nan)):
        kw = dict(origin=origin, d=(0.0, -1.0, 0.0), r=1.5, t_min=0.0, t_max=20.0)
        kw.update(change)
        rows.append((kw["origin"], kw["d"], kw["r"], kw["t_min"], kw["t_max"], invalid, f"invalid {list(change)[0]}"))
    b = types.SimpleNamespace(steps=steps, bisections=bisections, names=[row[6] for row in rows])
    b.origins, b.directions = np.array([row[0] for row in rows]), np.array([row[1] for row in rows])
    b.radii, b.t_min, b.t_max = (np.array([row[k] for row in rows]) for k in (2, 3, 4))
    b.expected = np.array([row[5] for row in rows], dtype=CM.SWEEP_DTYPE)
    return b


# ---- C: a tie that beats the foot -----------------------------------------------------------------------------------------------------------------
# Terrain V is terrain P with every loaded tile replaced by a function of the texel's row alone: constant along x, so bilerp's a + (b - a) *
# rem_x has a == b and a sample does not depend on x, and steep enough along z that the nearest ground is off the foot.  Centres at
# x == 0 (the model's own x: position_world_to_local and back are odd in x) with r = 0.875 (every stencil x of round 0 a whole number of
# eighths): lanes 8 j + 3 and 8 j + 4 (x = -w / 7 and +w / 7) see the same ground at the same distance.

C_RADIUS = 0.875
# (z, how far the centre is above the ground under it, R): the tie is in round R.  Along x == 0 the tree of these scenes holds LOD 0
# beyond about 200 units from the view and LOD 1 nearer, both with blend ratio 0.  Each centre keeps the condition when the tree's
# approximate height (which moves every surface point, and with it the blend) is 10 units higher or lower than the model scene's
C_CENTRES = [(-373.5, 0.5, 1), (-318.25, 1.0, 0), (-126.5, 0.5, 0), (-110.25, 1.0, 0), (3.5, 0.5, 0), (65.25, 1.0, 0), (227.75, 0.5, 1), (283.0, 1.0, 0)]


def v_tile(tile):
    """a V along the rows: about 5.9 units of height per texel, 0.16 (LOD 0) to 1.3 (LOD 3) per unit of z"""
    rows = np.arange(tile.shape[0])
    return np.broadcast_to((20000 + 1500 * np.abs(rows - tile.shape[0] // 2)).astype(np.uint16)[:, None], tile.shape).copy()


def c_spheres(sample):
    """-> centers, rounds: the centres of C_CENTRES over the ground `sample` gives under them, and the R of each"""
    z = np.array([c[0] for c in C_CENTRES])
    feet = np.column_stack([np.zeros(len(z)), np.zeros(len(z)), z])
    y = np.asarray(sample(feet), np.float32).astype(np.float64) + P_POSITION[1] + np.array([c[1] for c in C_CENTRES])
    return np.column_stack([np.zeros(len(z)), y, z]), [c[2] for c in C_CENTRES]


def all_lanes_tie_with_the_foot(sample, c, R):
    """asserts, on the model, that at radius 0 every lane of every round has the foot's d2 bit for bit, and that the foot stays (the
    improvement is strict) -> the model's contact"""
    contact = CM.contact_one(P_OMODEL, sample, c, 0.0, R)
    q, _, _ = CM.stencil(c, [1.0, 0.0, 0.0], [0.0, 0.0, 1.0], np.float64(0.0), np.float64(0.0), np.float64(0.0))
    d = CM.ground_points(P_OMODEL, sample, q)[0] - c[None, :]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert (d2 == d2[0]).all() and np.sqrt(d2[0]) == contact["distance"] > 0.0
    assert contact["status"] == CM.NONE and contact["candidate"] == 0 and contact["depth"] == -contact["distance"]
    return contact


def tie_below_the_foot(sample, otree, approximate_height, c, R):
    """asserts, on the model, that the contact of (c, C_RADIUS, R) is won in round R by lane 8 j + 3 in a bit-equal tie with lane 8 j + 4
    that is the round's minimum and strictly below the foot's d2, and that both lanes blend the same LODs with the same ratio -> the
    model's contact and (lane, lod, ratio)"""
    r = np.float64(C_RADIUS)
    trace = []
    contact = CM.contact_one(P_OMODEL, sample, c, r, R, trace=trace)
    assert len(trace) == 1, trace  # no earlier round improved on the foot: the winning round's window is centred on the foot
    k, lane = divmod(int(contact["candidate"]) - 1, 64)
    assert int(contact["candidate"]) > 0 and k == R and lane % 8 == 3, (contact["candidate"], R)
    q, x, _ = CM.stencil(c, [1.0, 0.0, 0.0], [0.0, 0.0, 1.0], np.float64(0.0), np.float64(0.0), r * (2.0 / 7.0) ** k if k else r)
    g, _ = CM.ground_points(P_OMODEL, sample, q)
    d = g - c[None, :]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    foot = CM.ground_points(P_OMODEL, sample, c[None, :])[0][0] - c
    assert d2[lane].tobytes() == d2[lane + 1].tobytes() and d2[lane] == d2.min() and (np.delete(d2, [lane, lane + 1]) > d2[lane]).all()
    assert d2[lane] < CM._dot3(foot, foot) and x[lane] == -x[lane + 1] < 0.0
    assert contact["point"][0] == x[lane] < 0.0 and trace == [(x[lane], trace[0][1])]
    surface = q[[lane, lane + 1]].copy()
    surface[:, 1] = P_POSITION[1] + approximate_height  # position_local_to_world(local, approximate_height)
    blends = [otree.compute_blend(tuple(p)) for p in surface]
    assert blends[0] == blends[1] and blends[0][1] in (0.0, 1.0), blends
    return contact, (lane,) + blends[0]


# ---- D: inputs for the three forms of the ceiling skip --------------------------------------------------------------------------------------------
# the terrains are section B's of _ray_cases.py; the expectations are the model's, which is told whether the border allows the skip

def _planar_up(n):
    return np.tile(RC.UP, (n, 1))


def b0_spheres(omodel, sample, limit=64):
    """border 0, skip off: around the model's ray hits that lie above the ceiling (b0_rays), by a quarter of their height above it: the
    centre on the hit (BELOW), half a radius above it (TOUCHING) and forty radii above it (NONE: clear of the ridge the ray ran into).
    -> centers, radii"""
    hits = RM.raycast(omodel, sample, *RC.b0_rays(omodel), 256, 2)
    p = hits["position"][hits["status"] == RM.HIT]
    margin = RM.altitude(omodel, p) - RC.ceiling(omodel)
    p, margin = p[margin > 0.0][:limit // 3], margin[margin > 0.0][:limit // 3]
    radii = np.repeat(margin / 4.0, 3)
    centers = np.repeat(p, 3, axis=0) + _planar_up(len(radii)) * (np.tile([0.0, 0.5, 40.0], len(p)) * radii)[:, None]
    return centers, radii


def skipped_wrongly(omodel, centers, radii, off, on):
    """how many spheres above the ceiling by more than their radius are TOUCHING or BELOW with the skip off and FAR with it on"""
    above = RM.altitude(omodel, centers) - radii > RC.ceiling(omodel)
    return int((above & np.isin(off["status"], (CM.TOUCHING, CM.BELOW)) & (on["status"] == CM.FAR)).sum())


def b0_sweeps(omodel, sample, n=16):
    """the same hits approached from forty radii above them, straight down and a little obliquely: steps, bisections, R = 16, 4, 1"""
    centers, radii = b0_spheres(omodel, sample, 3 * n)
    p, r = centers[::3][:n], radii[::3][:n]
    s = types.SimpleNamespace(radii=r, t_min=np.zeros(len(r)), t_max=np.full(len(r), 1.5))
    s.origins = p + _planar_up(len(r)) * (40.0 * r)[:, None]
    s.directions = (-_planar_up(len(r)) + np.array([0.02, 0.0, -0.01]) * (np.arange(len(r)) % 2)[:, None]) * (40.0 * r)[:, None]
    return s


def sweep_hits_above(omodel, sweeps, hits):
    """how many HITs have a contact centre c(t) with a - r > ceiling"""
    hit = hits["status"] == CM.HIT
    c = sweeps.origins[hit] + hits["t"][hit, None] * sweeps.directions[hit]
    return int((RM.altitude(omodel, c) - sweeps.radii[hit] > RC.ceiling(omodel)).sum())


B1_RADII = (0.5, 1.0, 2.0, 4.0)  # a = ceiling + r stays below 256, where one ulp of the centre's y is one ulp of a and of a - r


def b1_spots(omodel, view, sample, each, seed=59, candidates=600):
    """places over the planar border-1 terrain: `each` on the plateaus of value exactly 1.0 beside tile edges, `each` elsewhere"""
    rng = np.random.default_rng(seed)
    ground, up = up_vectors(omodel, view, candidates, rng)
    flat = sample(ground + up * float(omodel.max_height)) == F(omodel.max_height)
    assert flat.sum() >= each and (~flat).sum() >= each, (flat.sum(), len(flat))
    return ground[np.concatenate([np.flatnonzero(flat)[:each], np.flatnonzero(~flat)[:each]])]


def b1_spheres(omodel, view, sample, each=12):
    """pairs of spheres: a - r == ceiling exactly (searched), and the centre one ulp higher (a - r one ulp above the ceiling: FAR).  The
    model is planar with position.y = -5 and ceiling 250: a = y + 5.  -> centers, radii; pair k is rows 2 k and 2 k + 1"""
    assert int(omodel.kind) == 0 and RC.ceiling(omodel) == 250.0 and float(omodel.position[1]) == -5.0
    ground = b1_spots(omodel, view, sample, each)
    radii = np.repeat([B1_RADII[k % len(B1_RADII)] for k in range(len(ground))], 2)
    centers = np.repeat(ground, 2, axis=0)
    y = 245.0 + radii[::2]
    centers[::2, 1], centers[1::2, 1] = y, np.nextafter(y, np.inf)
    a = RM.altitude(omodel, centers)
    assert (a[::2] - radii[::2] == 250.0).all() and (a[1::2] - radii[1::2] == np.nextafter(250.0, np.inf)).all()
    return centers, radii


def b1_pairs(contacts):
    """how many pairs are searched at the ceiling and FAR one ulp above it"""
    return int((np.isin(contacts["status"][::2], (CM.NONE, CM.TOUCHING)) & (contacts["status"][1::2] == CM.FAR)).sum())


def b1_sweeps(omodel, view, sample, each=8):
    """straight down in 8 steps of 2^-8 from a - r = ceiling + 4 steps: samples 0 .. 3 are FAR, sample 4 has a - r == ceiling and is
    searched, on the plateaus it grazes there (NONE) and sample 5 touches: steps, bisections, R = 8, 3, 1"""
    ground = b1_spots(omodel, view, sample, each)
    n = len(ground)
    s = types.SimpleNamespace(radii=np.full(n, 0.5), t_min=np.zeros(n), t_max=np.full(n, 8.0 * RC.B1_DELTA), directions=np.tile(RC.DOWN, (n, 1)))
    s.origins = ground.copy()
    s.origins[:, 1] = 245.5 + 4.0 * RC.B1_DELTA
    return s


def b2_spheres(omodel, sample, view):
    """the inverted range, skip off: make_spheres placed by where the ground is.  64 spheres"""
    return make_spheres(RC.geometric_range(omodel), sample, view, n=64)


def searched_above(omodel, centers, radii, contacts):
    """how many spheres with a - r > ceiling(model) have a status that is not FAR (nor INVALID)"""
    with np.errstate(all="ignore"):
        above = RM.altitude(omodel, centers) - radii > RC.ceiling(omodel)
    return int((above & ~np.isin(contacts["status"], (CM.FAR, CM.INVALID))).sum())

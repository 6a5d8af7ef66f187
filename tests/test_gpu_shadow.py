"""Sun shadows on the device: bt_tile_tree_sun_occlusion and bt_tile_tree_render_shadowed byte-equal to the CPU model of their definition
(tests/_shadow_model.py) and to the existing device calls (bt_tile_tree_raycast on the shadow rays built in numpy, bt_tile_tree_render
for every plane it already makes), both forms across a launch boundary, optional planes, and the refusals.

The terrains are test_gpu_raycast.py's Streamed (T = 32, b = 2, 4 LODs; planar, sphere, ellipsoid), the cameras _render_model.scene_cameras
under the low suns of _shadow_model.scene_shadow.  No tolerance and no excluded ray or pixel anywhere; the note of test_gpu_raycast.py on the
last place of the f64 log2 applies here as it does there.  The model's statuses are computed once per terrain and march and shared."""
import ctypes as C
import types

import numpy as np
import pytest

import _raycast_model as RM
import _render_model as R
import _shadow_model as S
import bevy_terrain_amd as bt
from bevy_terrain_amd import _ffi
from test_gpu_raycast import Streamed
from test_gpu_render import assert_planes_equal, device_camera, painted  # noqa: F401  (painted: a fixture)

pytestmark = pytest.mark.gpu
BT_ERR_INVALID_ARGUMENT, BT_ERR_UNSUPPORTED = -1, -5
PLANES = ("t", "status", "normal", "rgba", "shadow")
COUNTS, POINTS = [1, 63, 64, 65, 257], 257  # a partial wave, a whole wave, the wave's edge, the 256-thread workgroup's edge
NAN_POINT = 5


@pytest.fixture(scope="module")
def device():
    return bt.Device(0)


@pytest.fixture(scope="module")
def terrains(device, tmp_path_factory):
    cache = {}

    def get(kind):
        if kind not in cache:
            s = Streamed(device, tmp_path_factory.mktemp(kind), kind)
            s.T, s.B = R.T, R.B
            s.approximate_height = s.tree.view_state().approximate_height  # the height the kernels read: the last frame's sample
            s.sun, s.lift, s.distance = S.scene_shadow(kind, s.omodel, s.view)
            s.cameras = {name: S.shadow_camera(kind, s.omodel, s.view, name)[0] for name in ("main", "inside", "ortho")}
            s.sun64 = np.array([np.float64(np.float32(v)) for v in s.sun])  # the cameras' sun, widened
            s.points, s.directions = query_input(s)
            s.model_status = {}
            cache[kind] = s
        return cache[kind]

    return get


def query_input(s):
    """257 points: the hit positions of the scene's main camera (the model's, at (96, 2): the march's residual is far under the scene's
    lift), each also raised into the air and sunk under the ground by up to a fifth of the height span along n, shuffled so that every
    prefix holds all three, one of them non-finite; and three directions: the scene's sun, the zero vector (INVALID) and straight down
    at the view (occluded)"""
    hits = R.render(s, s.cameras["main"], 96, 2).hits
    p = hits["position"][hits["status"] == RM.HIT]
    assert len(p) >= 80
    rng = np.random.default_rng(23)
    n = S.up_direction(s.omodel, p)
    span = float(s.omodel.max_height) - float(s.omodel.min_height)
    pool = np.vstack([p, p + n * rng.uniform(0.01, 0.2, (len(p), 1)) * span, p - n * rng.uniform(0.01, 0.2, (len(p), 1)) * span])
    points = pool[rng.permutation(len(pool))[:POINTS]].copy()
    assert len(points) == POINTS
    points[NAN_POINT, 1] = np.nan
    if int(s.omodel.kind) == 0:
        down = np.array([0.0, -1.0, 0.0])
    else:
        down = -R._unit(np.asarray(s.view, dtype=np.float64) - np.array([float(s.omodel.position[i]) for i in range(3)]))
    return points, np.array([s.sun64, [0.0, 0.0, 0.0], down])


def model_status(s, steps):
    """the model's (257, 3) statuses of the scene's points and directions at `steps`, computed once"""
    if steps not in s.model_status:
        status = S.occlusion(s.omodel, s.sample, s.points, s.directions, s.lift, s.distance, steps)[0]
        finite = np.arange(POINTS) != NAN_POINT
        # the input: INVALID exactly where it must be, everything under a sun that points down occluded, and under the real sun a mix
        assert (status[NAN_POINT] == S.INVALID).all() and (status[:, 1] == S.INVALID).all() and np.isin(status[finite, 2], (S.HIT, S.INSIDE)).all()
        assert (status[finite, 0] != S.INVALID).all() and (status[:, 0] == S.MISS).sum() >= 20 and (status[:, 0] == S.INSIDE).sum() >= 20
        assert steps == 1 or (status[:, 0] == S.HIT).sum() >= 10
        s.model_status[steps] = status
    return s.model_status[steps]


def counts_of(status):
    return dict(lit=int((status == S.MISS).sum()), occluded=int(((status == S.HIT) | (status == S.INSIDE)).sum()), invalid=int((status == S.INVALID).sum()))


# ---- 1. the query ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("steps", S.SHADOW_STEPS)
@pytest.mark.parametrize("kind", ["planar", "sphere", "ellipsoid"])
def test_the_query_equals_the_model_and_the_existing_call(terrains, kind, steps):
    """every count x direction_count on one terrain and march: the statuses are the model's, the stats its counts, and the same
    statuses come from bt_tile_tree_raycast (refine 0) on the shadow rays built in numpy with the model's n(q)"""
    s = terrains(kind)
    exp = model_status(s, steps)
    for count in (COUNTS if kind != "ellipsoid" else [65]):
        for k in (1, 3):
            got, stats = s.tree.sun_occlusion(0, s.points[:count], s.directions[:k], s.lift, s.distance, steps)
            assert got.shape == (count, k) and got.dtype == np.uint8
            assert np.array_equal(got, exp[:count, :k]), (count, k, np.argwhere(got != exp[:count, :k])[:8])
            assert stats == dict(launches=1, **counts_of(exp[:count, :k])), (count, k)
    origins, directions = S.shadow_rays(s.omodel, s.points, s.directions, s.lift)
    hits = s.tree.raycast(0, origins, directions, 0.0, s.distance, steps=steps, refine_rounds=0)
    got = s.tree.sun_occlusion(0, s.points, s.directions, s.lift, s.distance, steps)[0]
    assert np.array_equal(got.ravel(), hits["status"].astype(np.uint8))


@pytest.mark.parametrize("kind", ["planar", "sphere"])
def test_the_scenes_satisfy_their_input_conditions(terrains, kind):
    """test_shadow_model.py asserts these on a scene built without a device; here on the streamed one itself"""
    S.assert_input_conditions(S.input_conditions(terrains(kind), kind))


def test_the_query_in_two_launches(terrains):
    """4096 steps: 63 waves, 4032 rays, to a launch.  4100 rays of which only the 60 around ray 4032 have a finite position (the others
    are INVALID at no cost on either side): the second launch's first_ray, its 68 rays in a 256-thread workgroup, and the counters
    summed over both launches"""
    s = terrains("planar")
    assert S.occlusion_launches(4100, 4096) == (2, 4032)
    points = np.full((4100, 3), np.nan)
    points[4002:4062] = s.points[6:66]
    got, stats = s.tree.sun_occlusion(0, points, s.sun64, s.lift, s.distance, 4096)
    exp = np.full((4100, 1), S.INVALID, np.uint8)
    exp[4002:4062] = S.occlusion(s.omodel, s.sample, s.points[6:66], s.sun64, s.lift, s.distance, 4096)[0]
    for part in (exp[4002:4032], exp[4032:4062]):  # both sides of the boundary hold lit and occluded rays
        assert (part == S.MISS).any() and np.isin(part, (S.HIT, S.INSIDE)).any()
    assert np.array_equal(got, exp), np.argwhere(got != exp)[:8]
    assert stats == dict(launches=2, **counts_of(exp))
    # point-fastest over two directions: ray 4032 is point 4032 of direction 0, the second direction's rays are all in the second launch
    got2, stats2 = s.tree.sun_occlusion(0, points[:2100], [s.sun64, [0.0, -1.0, 0.0]], s.lift, s.distance, 4096)
    assert stats2["launches"] == 2 and (got2 == S.INVALID).all() and stats2["invalid"] == 4200


# ---- 2. the shadowed render ------------------------------------------------------------------------------------------------------------------

def shadowed(s, c, steps, rounds, shadow_steps, planes=PLANES, distance=None):
    return s.tree.render_shadowed(device_camera(c), s.lift, s.distance if distance is None else distance, shadow_steps, steps=steps, refine_rounds=rounds,
                                  planes=planes)


def assert_shadowed_equal(got, exp):
    assert_planes_equal(got, exp)
    assert got["shadow"].dtype == np.uint8 and np.array_equal(got["shadow"], exp.shadow), np.argwhere(got["shadow"] != exp.shadow)[:8]


@pytest.mark.parametrize("steps,rounds", [(64, 0), (96, 2)])
@pytest.mark.parametrize("width,height", R.SIZES)
@pytest.mark.parametrize("kind", ["planar", "sphere"])
def test_planes_equal_the_model(terrains, kind, width, height, steps, rounds):
    """all five planes and the stats, at shadow marches of 1, 48 and 200 steps"""
    s = terrains(kind)
    c = R.resized(s.cameras["main"], width, height)
    for shadow_steps in S.SHADOW_STEPS:
        exp = S.render_shadowed(s, c, steps, rounds, s.lift, s.distance, shadow_steps)
        assert_shadowed_equal(shadowed(s, c, steps, rounds, shadow_steps), exp)


@pytest.mark.parametrize("kind,name,lighting", [("planar", "inside", False), ("planar", "ortho", True), ("sphere", "ortho", True), ("sphere", "main", False),
                                                ("ellipsoid", "main", True)])
def test_other_cameras_equal_the_model(terrains, kind, name, lighting):
    """pixels INSIDE the ground at t_min (their shadow rays start at p(t_min)), the orthographic camera, no lighting (the colour is then
    the plain one, the shadow plane defined all the same), the ellipsoid; at (96, 2), whose residual the scene's lift exceeds (at
    (64, 0) it does not: most pixels of test_planes_equal_the_model's coarser march shadow themselves, which the model says too)"""
    s = terrains(kind)
    c = R.resized(s.cameras[name], 8, 8) if kind == "ellipsoid" else types.SimpleNamespace(**vars(s.cameras[name]))
    c.lighting = lighting
    exp = S.render_shadowed(s, c, 96, 2, s.lift, s.distance, 48)
    occluded = np.isin(exp.shadow, (S.HIT, S.INSIDE))
    assert occluded.sum() >= 4 and (exp.shadow == S.MISS).sum() >= 4, (occluded.sum(), (exp.shadow == S.MISS).sum())
    assert name != "inside" or (occluded & (exp.status == RM.INSIDE)).any()
    assert_shadowed_equal(shadowed(s, c, 96, 2, 48), exp)


def existing_composition(tree, cam, c, steps, rounds, lift, distance, shadow_steps, got):
    """what the existing entry points say the shadowed picture must be: t, status and normal are bt_tile_tree_render's; the colour is its
    colour where the pixel is lit and its colour with the sun put out where the pixel is occluded; the shadow plane at the pixels that
    met the ground is bt_tile_tree_sun_occlusion at p(t)"""
    plain = tree.render(cam, steps=steps, refine_rounds=rounds)
    dark = types.SimpleNamespace(**vars(c))
    dark.sun = (0.0, 0.0, 0.0)
    unlit = tree.render(device_camera(dark), steps=steps, refine_rounds=rounds, planes=("rgba",))["rgba"]
    for name in ("t", "status", "normal"):
        assert got[name].tobytes() == plain[name].tobytes(), name
    assert got["stats"] == plain["stats"]
    met = np.isin(plain["status"], (_ffi.RAY_HIT, _ffi.RAY_INSIDE))
    assert np.array_equal(got["shadow"] == _ffi.SHADOW_NONE, ~met)
    origins, directions = bt.render_rays(cam)
    p = (origins + plain["t"].reshape(-1, 1) * directions)[met.ravel()]
    sun = np.array([np.float64(np.float32(v)) for v in c.sun])
    status = tree.sun_occlusion(0, p, sun, lift, distance, shadow_steps)[0][:, 0]
    assert np.array_equal(got["shadow"][met], status)
    occluded = np.isin(got["shadow"], (_ffi.RAY_HIT, _ffi.RAY_INSIDE))
    assert got["rgba"].tobytes() == np.where(occluded[..., None], unlit, plain["rgba"]).tobytes()
    return int(occluded.sum()), int((got["shadow"] == _ffi.RAY_MISS).sum()), int((unlit != plain["rgba"]).any(axis=2).sum())


@pytest.mark.parametrize("kind", ["planar", "sphere", "ellipsoid"])
def test_planes_equal_the_existing_calls(terrains, kind):
    """independent of the model's march, 33 x 17 at (256, 2) with 200 shadow steps: five blocks across, three down, partial on both edges;
    perspective and orthographic, with the light and without"""
    s = terrains(kind)
    for name, lighting in (("main", True), ("main", False), ("ortho", True)):
        c = R.resized(s.cameras[name], 33, 17)
        c.lighting = lighting
        got = shadowed(s, c, 256, 2, 200)
        occluded, lit, differ = existing_composition(s.tree, device_camera(c), c, 256, 2, s.lift, s.distance, 200, got)
        assert occluded >= 20 and lit >= 20 and (differ > 0) == lighting, (name, lighting, occluded, lit, differ)


def test_albedo(painted):
    """an Rgba8 albedo attachment and the grey, lit and unlit, perspective and orthographic, against the existing calls"""
    s = painted
    sun, lift, distance = S.scene_shadow("planar", s.omodel, s.view)
    base = R.scene_cameras("planar", s.omodel, s.view)
    seen = []
    for name in ("main", "ortho"):
        for albedo, lighting in ((1, False), (1, True), (None, False), (None, True)):
            c = types.SimpleNamespace(**vars(base[name]))
            c.albedo, c.lighting, c.sun, c.background = albedo, lighting, tuple(float(np.float32(v)) for v in sun), (3, 2, 1, 0)
            cam = device_camera(c)
            got = s.tree.render_shadowed(cam, lift, distance, 48, steps=96, refine_rounds=2)
            seen.append(existing_composition(s.tree, cam, c, 96, 2, lift, distance, 48, got))
    assert sum(v[0] for v in seen) >= 8 and sum(v[1] for v in seen) >= 8, seen  # (this terrain has no model: all that is known of its shadows)


def test_optional_planes_an_invalid_shadow_and_an_invalid_camera(terrains):
    """each plane NULL in turn, and each alone: the others do not change (without the shadow plane the march is skipped where the colour
    cannot show it, which must not show either).  A bad distance is INVALID in the shadow plane and lit in the colour, not an error."""
    s = terrains("sphere")
    c = s.cameras["main"]
    full = shadowed(s, c, 96, 2, 48)
    assert np.isin(full["shadow"], (S.HIT, S.INSIDE)).sum() >= 10
    subsets = [tuple(q for q in PLANES if q != p) for p in PLANES] + [(p,) for p in PLANES]
    for planes in subsets:
        got = shadowed(s, c, 96, 2, 48, planes=planes)
        assert set(got) == set(planes) | {"stats"} and got["stats"] == full["stats"], planes
        for p in planes:
            assert got[p].tobytes() == full[p].tobytes(), (planes, p)
    unlit = types.SimpleNamespace(**vars(c))
    unlit.lighting = False
    assert shadowed(s, unlit, 96, 2, 48, planes=("rgba",))["rgba"].tobytes() == s.tree.render(device_camera(unlit), steps=96, refine_rounds=2)["rgba"].tobytes()
    plain = s.tree.render(device_camera(c), steps=96, refine_rounds=2)
    met = np.isin(plain["status"], (_ffi.RAY_HIT, _ffi.RAY_INSIDE))
    for distance in (-1.0, float("nan"), float("inf")):
        got = shadowed(s, c, 96, 2, 48, distance=distance)  # BT_OK: render_shadowed() raises on anything else
        assert (got["shadow"][met] == _ffi.RAY_INVALID).all() and (got["shadow"][~met] == _ffi.SHADOW_NONE).all()
        assert all(got[p].tobytes() == plain[p].tobytes() for p in ("t", "status", "normal", "rgba"))
    bad = types.SimpleNamespace(**vars(c))
    bad.forward = np.array([c.forward[0], np.nan, c.forward[2]])
    got = shadowed(s, bad, 96, 2, 48)
    assert (got["status"] == _ffi.RAY_INVALID).all() and (got["shadow"] == _ffi.SHADOW_NONE).all() and (got["rgba"] == np.array(c.background, np.uint8)).all()
    assert got["stats"] == dict(launches=1, hit_pixels=0, inside_pixels=0, miss_pixels=0)


def test_the_render_in_two_launches(terrains):
    """8 x 512 at one primary step and 4096 shadow steps: 64 blocks of 64 * 4099 worst-case samples, 63 to a launch.  The camera
    (_shadow_model.boundary_camera) lets only the last rows meet the ground, a few of them above row 504, where the second launch begins.
    A march of one step leaves its hits up to 10 under the ground: the lift is 10.5 here, which leaves some of them lit."""
    s = terrains("planar")
    c = S.boundary_camera(s)
    assert S.shadowed_launches(c.width, c.height, 1, 0, 4096) == (2, 63)
    exp = S.render_shadowed(s, c, 1, 0, 10.5, s.distance, 4096)
    for rows in (slice(0, 504), slice(504, 512)):
        assert 4 <= (exp.status[rows] == RM.HIT).sum() <= 64, (exp.status[rows] == RM.HIT).sum()
    assert np.isin(exp.shadow, (S.HIT, S.INSIDE)).any() and (exp.shadow == S.MISS).any() and exp.stats["launches"] == 2
    got = s.tree.render_shadowed(device_camera(c), 10.5, s.distance, 4096, steps=1, refine_rounds=0)
    assert got["stats"]["launches"] == 2
    assert_shadowed_equal(got, exp)


def test_the_plain_render_is_unchanged_around_a_shadowed_call(terrains):
    """the two entry points share a body and a scratch: bt_tile_tree_render gives the same bytes before and after a shadowed call, of a
    larger image and of the same one"""
    s = terrains("planar")
    cam = device_camera(s.cameras["main"])
    before = s.tree.render(cam, steps=96, refine_rounds=2)
    shadowed(s, R.resized(s.cameras["main"], 33, 17), 96, 2, 48)
    shadowed(s, s.cameras["main"], 96, 2, 48)
    after = s.tree.render(cam, steps=96, refine_rounds=2)
    assert all(before[p].tobytes() == after[p].tobytes() for p in ("t", "status", "normal", "rgba")) and before["stats"] == after["stats"]
    assert_planes_equal(after, R.render(s, s.cameras["main"], 96, 2))


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------------------

def test_the_query_refuses_before_any_device_work(device, terrains, painted):
    L = _ffi.lib()
    s = terrains("planar")
    n, k = 6, 2
    points = np.ascontiguousarray(s.points[6:6 + n])
    directions = np.ascontiguousarray(s.directions[[0, 2]])
    out = np.full(n * k + 8, 0xAB, np.uint8)  # (8 bytes of canary behind the statuses)
    stats = _ffi.OcclusionStatsC(9, 9, 9, 9)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None
    tree, atlas = s.tree._h, s.atlas._h

    def call(tree=tree, atlas=atlas, ai=0, points=points, count=n, directions=directions, dcount=k, lift=s.lift, distance=s.distance, steps=48, out=out):
        return L.bt_tile_tree_sun_occlusion(tree, atlas, ai, dp(points), count, dp(directions), dcount, lift, distance, steps,
                                            out.ctypes.data_as(C.POINTER(C.c_uint8)) if out is not None else None, C.byref(stats))

    other = bt.Device(0)
    foreign = bt.TileAtlas.new(s.atlas.config, other)
    invalid = {
        "NULL tree": dict(tree=None), "NULL atlas": dict(atlas=None), "an atlas of another context": dict(atlas=foreign._h), "attachment 1": dict(ai=1),
        "NULL points": dict(points=None), "NULL directions": dict(directions=None), "NULL out_status": dict(out=None),
        "lift NaN": dict(lift=float("nan")), "lift inf": dict(lift=float("inf")), "lift -inf": dict(lift=float("-inf")),
        "steps 0": dict(steps=0), "steps 4097": dict(steps=4097), "too many rays": dict(count=1 << 24, dcount=2), "too many rays (one more)": dict(count=(1 << 24) + 1, dcount=1),
        "too many rays (32-bit product)": dict(count=1 << 31, dcount=2),
    }
    for what, kw in invalid.items():
        assert call(**kw) == BT_ERR_INVALID_ARGUMENT, what
        assert L.bt_last_error(), what
    assert call(tree=painted.tree._h, atlas=painted.atlas._h, ai=1) == BT_ERR_UNSUPPORTED  # an Rgba8 attachment
    assert (out == 0xAB).all() and (stats.launches, stats.lit, stats.occluded, stats.invalid) == (9, 9, 9, 9)
    # no rays: BT_OK, nothing touched but the stats, which are zeroed (NULL arrays are then fine)
    for kw in (dict(count=0), dict(dcount=0), dict(count=0, points=None, out=None), dict(dcount=0, directions=None)):
        stats.launches = stats.lit = stats.occluded = stats.invalid = 9
        assert call(**kw) == _ffi.BT_OK and (stats.launches, stats.lit, stats.occluded, stats.invalid) == (0, 0, 0, 0), kw
    assert (out == 0xAB).all()
    # a bad distance or direction is no error: INVALID statuses; the limits themselves are accepted; the canary stays
    exp = S.occlusion(s.omodel, s.sample, points, directions, s.lift, s.distance, 4096)[0]
    assert call(steps=4096) == _ffi.BT_OK and np.array_equal(out[:n * k].reshape(n, k), exp) and (out[n * k:] == 0xAB).all()
    assert dict(lit=stats.lit, occluded=stats.occluded, invalid=stats.invalid) == counts_of(exp) and stats.launches == 1 and stats.occluded >= n
    for distance in (-1.0, float("nan"), float("inf"), float("-inf")):
        assert call(distance=distance) == _ffi.BT_OK and (out[:n * k] == _ffi.RAY_INVALID).all() and stats.invalid == n * k, distance
    assert call(directions=np.array([[0.0, 0.0, 0.0], [np.inf, 0.0, 1.0]])) == _ffi.BT_OK and (out[:n * k] == _ffi.RAY_INVALID).all() and (out[n * k:] == 0xAB).all()
    assert L.bt_tile_tree_sun_occlusion(tree, atlas, 0, dp(points), n, dp(directions), k, s.lift, s.distance, 48, out.ctypes.data_as(C.POINTER(C.c_uint8)), None) == _ffi.BT_OK
    # the scratch stays in the context until bt_ctx_trim, and the call works again after it
    before = s.tree.sun_occlusion(0, s.points, s.directions, s.lift, s.distance, 48)
    assert device.trim() > 0
    again = s.tree.sun_occlusion(0, s.points, s.directions, s.lift, s.distance, 48)
    assert np.array_equal(before[0], again[0]) and before[1] == again[1]


def test_the_shadowed_render_refuses_before_any_device_work(device, terrains, painted):
    L = _ffi.lib()
    s = terrains("planar")
    good = device_camera(s.cameras["main"]).c()
    n = good.width * good.height
    t, status, shadow = np.full(n + 8, 7.5), np.full(n + 8, 0xAB, np.uint8), np.full(n + 8, 0xAB, np.uint8)
    normal, rgba = np.full(3 * n + 8, 7.5, np.float32), np.full(4 * n + 8, 0xAB, np.uint8)
    planes = (t.ctypes.data_as(C.POINTER(C.c_double)), status.ctypes.data_as(C.POINTER(C.c_uint8)), normal.ctypes.data_as(C.POINTER(C.c_float)),
              rgba.ctypes.data_as(C.POINTER(C.c_uint8)), shadow.ctypes.data_as(C.POINTER(C.c_uint8)))
    stats = _ffi.RenderStatsC(9, 9, 9, 9)
    tree, atlas = s.tree._h, s.atlas._h
    march = _ffi.SunShadowC(s.lift, s.distance, 48, 0)

    def call(tree=tree, atlas=atlas, ai=0, cam=good, steps=64, rounds=1, shadow=march, planes=planes):
        return L.bt_tile_tree_render_shadowed(tree, atlas, ai, C.byref(cam) if cam is not None else None, steps, rounds,
                                              C.byref(shadow) if shadow is not None else None, *planes, C.byref(stats))

    def changed(**fields):
        cam = _ffi.RenderCameraC.from_buffer_copy(good)
        for name, value in fields.items():
            if name == "sun":
                for i in range(3):
                    cam.sun[i] = value[i]
            else:
                setattr(cam, name, value)
        return cam

    other = bt.Device(0)
    foreign = bt.TileAtlas.new(s.atlas.config, other)
    invalid = {
        # the shadowed form's own
        "NULL shadow": dict(shadow=None), "shadow steps 0": dict(shadow=_ffi.SunShadowC(s.lift, s.distance, 0, 0)),
        "shadow steps 4097": dict(shadow=_ffi.SunShadowC(s.lift, s.distance, 4097, 0)), "lift NaN": dict(shadow=_ffi.SunShadowC(float("nan"), s.distance, 48, 0)),
        "lift inf": dict(shadow=_ffi.SunShadowC(float("inf"), s.distance, 48, 0)), "all five planes NULL": dict(planes=(None,) * 5),
        # bt_tile_tree_render's
        "NULL tree": dict(tree=None), "NULL atlas": dict(atlas=None), "NULL camera": dict(cam=None),
        "width 0": dict(cam=changed(width=0)), "height 0": dict(cam=changed(height=0)), "too many pixels": dict(cam=changed(width=4097, height=4096)),
        "steps 0": dict(steps=0), "steps 4097": dict(steps=4097), "refine_rounds 5": dict(rounds=5), "height attachment 1": dict(ai=1),
        "albedo attachment 1": dict(cam=changed(albedo_attachment=1)), "ambient NaN": dict(cam=changed(ambient=float("nan"))),
        "ambient inf": dict(cam=changed(ambient=float("inf"))), "sun NaN": dict(cam=changed(sun=(0.0, float("nan"), 0.0))),
        "sun inf": dict(cam=changed(sun=(float("-inf"), 0.0, 0.0))), "unknown flag": dict(cam=changed(flags=4)), "unknown flags": dict(cam=changed(flags=0x80000001)),
        "an atlas of another context": dict(atlas=foreign._h),
    }
    for what, kw in invalid.items():
        assert call(**kw) == BT_ERR_INVALID_ARGUMENT, what
        assert L.bt_last_error(), what
    ptree, patlas = painted.tree._h, painted.atlas._h
    assert call(tree=ptree, atlas=patlas, ai=1) == BT_ERR_UNSUPPORTED
    assert call(tree=ptree, atlas=patlas, ai=0, cam=changed(albedo_attachment=0)) == BT_ERR_UNSUPPORTED
    assert call(tree=ptree, atlas=patlas, ai=0, cam=changed(albedo_attachment=2)) == BT_ERR_INVALID_ARGUMENT
    # nothing was touched by any of the above
    assert (t == 7.5).all() and (status == 0xAB).all() and (normal == 7.5).all() and (rgba == 0xAB).all() and (shadow == 0xAB).all()
    assert (stats.launches, stats.hit_pixels, stats.inside_pixels, stats.miss_pixels) == (9, 9, 9, 9)
    # the shadow plane alone is a picture; the limits themselves are accepted (one pixel, stats == NULL); the canaries stay
    assert call(planes=(None, None, None, None, planes[4])) == _ffi.BT_OK and (shadow[:n] != 0xAB).all() and (shadow[n:] == 0xAB).all() and (status == 0xAB).all()
    one = changed(width=1, height=1)
    limit = _ffi.SunShadowC(s.lift, s.distance, 4096, 0)
    assert L.bt_tile_tree_render_shadowed(tree, atlas, 0, C.byref(one), 4096, 4, C.byref(limit), *planes, None) == _ffi.BT_OK
    assert t[0] != 7.5 and (t[1:] == 7.5).all() and (status[1:] == 0xAB).all() and status[0] in (0, 1, 2) and (rgba[4:] == 0xAB).all() and (normal[3:] == 7.5).all()
    assert call() == _ffi.BT_OK and (t[n:] == 7.5).all() and (status[n:] == 0xAB).all() and (normal[3 * n:] == 7.5).all() and (rgba[4 * n:] == 0xAB).all()
    assert (shadow[n:] == 0xAB).all()
    # the scratch stays in the context until bt_ctx_trim, and the call works again after it
    before = shadowed(s, s.cameras["main"], 64, 1, 48)
    assert device.trim() > 0
    again = shadowed(s, s.cameras["main"], 64, 1, 48)
    assert all(before[p].tobytes() == again[p].tobytes() for p in PLANES) and before["stats"] == again["stats"]

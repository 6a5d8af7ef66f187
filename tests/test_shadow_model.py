"""Sun shadows without a GPU: the CPU model of SUN OCCLUSION and of bt_tile_tree_render_shadowed (tests/_shadow_model.py) against closed
forms, so that model and kernel cannot share a misreading; the entry points' export, layouts and NULL-handle refusals; the two launch
rules at the sizes test_gpu_shadow.py uses; and the conditions the scenes of test_gpu_shadow.py must satisfy for its comparisons to mean
something, asserted on scenes built without a device.

Closed forms.  Over a flat terrain a lifted point sees every sun above the horizon; a point at or under the ground is INSIDE at lift 0.
Behind a step of height H (a plateau whose edge runs along z) the low ground is in shadow up to H / tan(e) from the edge for a sun of
elevation e over the plateau: the shadow ray of a point x behind the edge, lifted by L, passes the edge at height L + x tan(e) over the
low ground, under the plateau's top when x < (H - L) / tan(e).  The sampled step is not sharp (bilinear texels, two blended LODs): the
test measures where it starts and ends along its line (x_a, x_b) and asserts only outside the band that leaves undecided."""
import ctypes as C
import math
import types

import numpy as np
import pytest

import _oracle as O
import _raycast_model as RM
import _render_model as R
import _shadow_model as S
from test_render_model import constant_scene, cpu_scene
from test_tile_tree_host import MODELS

F = np.float32


def test_the_entry_points_are_exported_and_refuse_null_handles():
    from bevy_terrain_amd import _ffi
    for name in ("bt_tile_tree_sun_occlusion", "bt_tile_tree_render_shadowed"):
        assert name in _ffi.header_symbols() and name in _ffi.PROTOTYPES
    assert C.sizeof(_ffi.OcclusionStatsC) == 16 and C.sizeof(_ffi.SunShadowC) == 24
    assert _ffi.SunShadowC.distance.offset == 8 and _ffi.SunShadowC.steps.offset == 16
    assert (_ffi.OCCLUSION_MAX_RAYS, _ffi.SHADOW_NONE) == (1 << 24, 255) == (S.SAMPLES_PER_LAUNCH, S.NONE)
    L = _ffi.lib()
    q, s, out = (C.c_double * 3)(1.0, 2.0, 3.0), (C.c_double * 3)(0.0, 1.0, 0.0), (C.c_uint8 * 1)(7)
    stats = _ffi.OcclusionStatsC(9, 9, 9, 9)
    assert L.bt_tile_tree_sun_occlusion(None, None, 0, q, 1, s, 1, 1.0, 10.0, 8, out, C.byref(stats)) == -1  # BT_ERR_INVALID_ARGUMENT
    assert b"NULL" in L.bt_last_error() and out[0] == 7 and stats.launches == 9
    cam, shadow = _ffi.RenderCameraC(), _ffi.SunShadowC(1.0, 10.0, 8, 0)
    cam.width = cam.height = 1
    assert L.bt_tile_tree_render_shadowed(None, None, 0, C.byref(cam), 64, 1, C.byref(shadow), None, None, None, None, out, None) == -1
    assert b"NULL" in L.bt_last_error() and out[0] == 7


# ---- closed forms ----------------------------------------------------------------------------------------------------------------------------

def ground_points(s, n, seed):
    rng = np.random.default_rng(seed)
    y = float(s.omodel.position[1]) + s.h
    return np.column_stack([rng.uniform(-400.0, 400.0, n) + 10.0, np.full(n, y), rng.uniform(-400.0, 400.0, n) + 3.0])


def test_a_flat_terrain_is_lit_by_every_sun_above_the_horizon():
    s = constant_scene("planar")
    sample = RM.sampler(s.otree, s.T, s.B, s.layers)
    q = ground_points(s, 12, 1)
    rng = np.random.default_rng(2)
    suns = rng.normal(size=(9, 3)) * [[3.0, 1.0, 3.0]]
    suns[:, 1] = np.abs(suns[:, 1]) + 0.01  # elevations from under a degree up; lengths from 0.01 to several
    status, stats = S.occlusion(s.omodel, sample, q, suns, 0.5, 300.0, 64)
    assert (status == S.MISS).all() and stats == dict(lit=12 * 9, occluded=0, invalid=0)
    # the ground shadows itself without a lift: f(q) = 0 at the first sample, whatever the sun
    status, stats = S.occlusion(s.omodel, sample, q, suns, 0.0, 300.0, 64)
    assert (status == S.INSIDE).all() and stats["occluded"] == 12 * 9
    # a lift is along +n: a negative one puts the origin under the ground
    assert (S.occlusion(s.omodel, sample, q, suns[:2], -0.5, 300.0, 64)[0] == S.INSIDE).all()
    # a sun under the horizon: the lifted ray comes down on the ground (lift 0.5, |s_y| * distance >= 3)
    down = suns * [[1.0, -1.0, 1.0]]
    assert (S.occlusion(s.omodel, sample, q, down, 0.5, 300.0, 64)[0] == S.HIT).all()
    # INVALID: a zero or non-finite direction, a negative or non-finite distance, a non-finite point; a distance of 0 is a march of
    # equal samples at the origin
    bad = np.array([[0.0, 0.0, 0.0], [0.0, np.nan, 1.0], [np.inf, 1.0, 0.0]])
    assert (S.occlusion(s.omodel, sample, q, bad, 0.5, 300.0, 64)[0] == S.INVALID).all()
    for distance in (-1.0, np.nan, np.inf):
        assert (S.occlusion(s.omodel, sample, q[:3], suns[:2], 0.5, distance, 64)[0] == S.INVALID).all()
    assert (S.occlusion(s.omodel, sample, q[:3], suns[:2], 0.5, 0.0, 64)[0] == S.MISS).all()
    q[1, 2], q[4, 0] = np.nan, -np.inf
    status = S.occlusion(s.omodel, sample, q, suns[:2], 0.5, 300.0, 64)[0]
    assert (status[[1, 4]] == S.INVALID).all() and (np.delete(status, [1, 4], axis=0) == S.MISS).all()


@pytest.mark.parametrize("kind", ["sphere", "ellipsoid"])
def test_the_lift_is_along_the_altitude_direction(kind):
    """on a globe with nothing loaded the ground is the min_height surface: n is a unit vector, lifting a point by L along it raises its
    altitude by L (on the ellipsoid n leans up to 0.0034 rad, the flattening, off the line altitude is measured along at the lifted
    point: L (1 - cos) = 0.0015 at L = 250; 0.01 covers it and the arithmetic), a sun along +n is never occluded, one along -n always"""
    s = constant_scene(kind, load=False)
    sample = RM.sampler(s.otree, s.T, s.B, s.layers)
    rng = np.random.default_rng(3)
    u = R._unit(np.asarray(s.view))[None, :] + rng.normal(size=(6, 3)) * 0.2
    q0 = np.array([float(s.omodel.position[i]) for i in range(3)]) + u / np.linalg.norm(u, axis=1, keepdims=True) * 6.36e6
    q = q0 - RM.altitude(s.omodel, q0)[:, None] * S.up_direction(s.omodel, q0)  # on the height-0 surface, to rounding
    q = q + s.h * S.up_direction(s.omodel, q)  # on the ground
    n = S.up_direction(s.omodel, q)
    assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() < 1e-15
    lifted = S.shadow_origins(s.omodel, q, 250.0)
    assert np.abs(RM.altitude(s.omodel, lifted) - RM.altitude(s.omodel, q) - 250.0).max() < 0.01
    assert np.abs(RM.altitude(s.omodel, q) - s.h).max() < 1.0  # (q is on the ground to within the same lean over 12 km)
    for k in range(len(q)):
        assert S.occlusion(s.omodel, sample, q[k], n[k], 250.0, 5.0e4, 32)[0][0, 0] == S.MISS
        assert S.occlusion(s.omodel, sample, q[k], -n[k], 250.0, 5.0e4, 32)[0][0, 0] == S.HIT
        assert S.occlusion(s.omodel, sample, q[k], n[k], -250.0, 5.0e4, 32)[0][0, 0] == S.INSIDE


RIDGE_T, RIDGE_B, RIDGE_LODS, LOW, HIGH = 32, 2, 4, 13107, 52428  # unorm 0.2 and 0.8: 50 and 200 over the planar model's 0 .. 250


@pytest.fixture(scope="module")
def ridge():
    """the planar model under a raster that is HIGH in its first 100 columns and LOW elsewhere, preprocessed by the oracle and streamed
    into its tree: a plateau over x < about -100, 150 higher than the ground beyond, its edge along z"""
    om = MODELS["planar"][1]
    W = 2 ** (RIDGE_LODS - 1) * (RIDGE_T - 2 * RIDGE_B) + 13
    raster = np.full((W, W), LOW, np.uint16)
    raster[:, :100] = HIGH
    atlas = O.OracleAtlas(RIDGE_LODS, 400, False, [(RIDGE_T, RIDGE_B, 1, O.FORMAT_R16)])
    atlas.clear_attachment(0)
    atlas.preprocess_tile(0, raster, (0, RIDGE_LODS))
    atlas.run(4)
    tiles = {coord: atlas.tile(0, i) for coord, i in atlas.tiles()}
    s = types.SimpleNamespace(omodel=om, T=RIDGE_T, B=RIDGE_B, layers={}, approximate_height=0.0, view=(10.0, 300.0, 3.0))
    s.otree = O.TileTree(om, RIDGE_LODS, O.make_view_config(tree_size=4, load_distance=1.2, blend_distance=1.0))
    stream = O.Stream(256, 1, existing=list(tiles))
    for _ in range(4):
        s.otree.update(s.view)
        for coord, index in stream.finish_loads(stream.pending_loads()):
            s.layers[index] = tiles[coord]
        s.otree.apply_requests(stream)
        s.otree.adjust_to_tile_atlas(stream)
    s.sample = RM.sampler(s.otree, s.T, s.B, s.layers)
    s.z = 3.0
    # the step as sampled along the line the test's rays run over: flat at `high` up to x_a, flat at `low` from x_b on
    xs = np.arange(-480.0, 480.0, 0.25)
    h = s.sample(np.column_stack([xs, np.zeros_like(xs), np.full_like(xs, s.z)]))
    s.low, s.high = float(h.min()), float(h.max())
    s.x_a, s.x_b = float(xs[h < s.high][0]) - 0.25, float(xs[h > s.low][-1]) + 0.25
    assert (s.low, s.high) == (50.0, 200.0) and -140.0 < s.x_a < s.x_b < -20.0 and (h[xs <= s.x_a] == s.high).all() and (h[xs >= s.x_b] == s.low).all()
    return s


@pytest.mark.parametrize("elevation_degrees", [25.0, 38.0])
def test_a_ridge_shadows_the_ground_behind_it_up_to_h_over_tan_e(ridge, elevation_degrees):
    s = ridge
    e = math.radians(elevation_degrees)
    H, lift, steps = s.high - s.low, 1.0, 400
    reach = (H - lift) / math.tan(e)  # how far behind a sharp edge the shadow would end
    assert 150.0 < reach < 420.0
    sun = np.array([-math.cos(e), math.sin(e), 0.0])  # over the plateau, unit: `distance` is in world units
    distance = 800.0
    step_x = distance / steps * math.cos(e)
    # in shadow: from a few texels behind the step's foot to where the ray still passes x_a more than two march steps under the top
    inside = np.arange(s.x_b + 5.0, s.x_a + reach - 3.0 * step_x, 5.0)
    # in the sun: from where the ray clears the top already over the step's foot, to the terrain's far side; and on the plateau itself
    outside = np.arange(s.x_b + reach + 1.0, 480.0, 7.0)
    assert len(inside) >= 20 and len(outside) >= 20 and outside[0] - inside[-1] < (s.x_b - s.x_a) + 3.0 * step_x + 8.0 + 7.0
    on = lambda xs, h: np.column_stack([xs, np.full(len(xs), float(s.omodel.position[1]) + h), np.full(len(xs), s.z)])
    assert (S.occlusion(s.omodel, s.sample, on(inside, s.low), sun, lift, distance, steps)[0] == S.HIT).all()
    assert (S.occlusion(s.omodel, s.sample, on(outside, s.low), sun, lift, distance, steps)[0] == S.MISS).all()
    plateau = np.arange(-470.0, s.x_a - 5.0, 25.0)
    assert len(plateau) >= 10 and (S.occlusion(s.omodel, s.sample, on(plateau, s.high), sun, lift, distance, steps)[0] == S.MISS).all()
    # the mirrored sun, over the low ground: nothing rises in front of the same points
    mirrored = sun * [-1.0, 1.0, 1.0]
    assert (S.occlusion(s.omodel, s.sample, on(inside, s.low), mirrored, lift, distance, steps)[0] == S.MISS).all()
    # ... and a reach that ends before the step does not see it: distance is the ray's t_max
    far = inside[inside > s.x_b + 60.0]
    assert len(far) >= 10 and (S.occlusion(s.omodel, s.sample, on(far, s.low), sun, lift, 40.0, steps)[0] == S.MISS).all()


def test_hit_points_are_inside_without_a_lift(ridge):
    """a point a ray query reported lies at or under the ground: INSIDE at lift 0 for any sun, and for a sun that nothing stands in
    front of, lit once the lift exceeds the march's residual"""
    s = ridge
    rng = np.random.default_rng(5)
    n = 24
    origins = np.column_stack([rng.uniform(0.0, 400.0, n), np.full(n, 500.0), rng.uniform(-300.0, 300.0, n)])
    directions = np.column_stack([rng.uniform(-0.1, 0.1, n), np.full(n, -1.0), rng.uniform(-0.1, 0.1, n)])  # (the hits stay on the flat low ground)
    hits = RM.raycast(s.omodel, s.sample, origins, directions, 0.0, 600.0, 64, 1)
    assert (hits["status"] == RM.HIT).all()
    sun = np.array([0.6, 0.8, 0.0])  # away from the plateau
    assert (S.occlusion(s.omodel, s.sample, hits["position"], sun, 0.0, 500.0, 64)[0] == S.INSIDE).all()
    residual = 600.0 / 64 / 64  # the bracket of one refinement round, along a ray that is at most |d| = 1.01 long per unit t
    assert (S.occlusion(s.omodel, s.sample, hits["position"], sun, 1.01 * residual + 0.01, 500.0, 64)[0] == S.MISS).all()


# ---- the shadowed picture ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scenes():
    cache = {}

    def get(kind):
        if kind not in cache:
            cache[kind] = cpu_scene(kind, MODELS[kind][1])
        return cache[kind]

    return get


@pytest.mark.parametrize("lighting", [True, False])
def test_the_shadowed_picture_is_the_plain_one_with_the_sun_put_out_where_occluded(scenes, lighting):
    """the rule of the colour plane against its consequence: l * 1 = l and l * 0 = 0, so the shadowed colour is the plain render's where
    the pixel is lit and the plain render's with sun = (0, 0, 0) where it is occluded; the other planes are the plain render's"""
    scene = scenes("planar")
    c, lift, distance = S.shadow_camera("planar", scene.omodel, scene.view)
    c.lighting = lighting
    got = S.render_shadowed(scene, c, 64, 0, lift, distance, 48)
    plain = R.render(scene, c, 64, 0)
    dark = types.SimpleNamespace(**vars(c))
    dark.sun = (0.0, 0.0, 0.0)
    unlit = R.render(scene, dark, 64, 0)
    occluded = (got.shadow == S.HIT) | (got.shadow == S.INSIDE)
    assert np.array_equal(got.status, plain.status) and got.t.tobytes() == plain.t.tobytes() and got.normal.tobytes() == plain.normal.tobytes()
    assert np.array_equal(got.shadow == S.NONE, ~plain.met.reshape(c.height, c.width)) and got.stats == plain.stats
    assert occluded.sum() >= 10 and (got.shadow == S.MISS).sum() >= 10
    assert np.array_equal(got.rgba, np.where(occluded[..., None], unlit.rgba, plain.rgba))
    assert (got.rgba != plain.rgba).any() == lighting


@pytest.mark.parametrize("kind", ["planar", "sphere", "ellipsoid"])
def test_the_gpu_scenes_satisfy_their_input_conditions(scenes, kind):
    """the main camera of test_gpu_shadow.py under the scene's sun, on the same terrain built without a device"""
    figures = S.input_conditions(scenes(kind), kind)
    print(figures)
    S.assert_input_conditions(figures)


def test_the_launch_rules_reach_one_and_two_launches(scenes):
    # the query: 63 waves of 4097 worst-case samples per lane fit 2^24, so 4100 rays at 4096 steps are two launches, cut at ray 4032
    assert S.occlusion_launches(4100, 4096) == (2, 4032) and S.occlusion_launches(4032, 4096) == (1, 4032)
    assert S.occlusion_launches(257 * 3, 200) == (1, 64 * 1304) and S.occlusion_launches(1, 1) == (1, 1 << 23)
    assert S.occlusion_launches(1 << 24, 1) == (2, 1 << 23) and S.occlusion_launches(1 << 24, 4096)[0] == 4162
    # the render: 8 x 512 at one primary step and 4096 shadow steps is 64 blocks of 64 * 4099 samples, 63 to a launch
    assert S.shadowed_launches(8, 512, 1, 0, 4096) == (2, 63)
    assert S.shadowed_launches(17, 9, 96, 2, 200) == (1, 6) and S.shadowed_launches(1, 1, 64, 0, 1) == (1, 1)
    # the shadow's samples count: 31 blocks of 64 * 8194 samples fit, cut to three bands of 8; the plain render's rule fits seven bands
    assert S.shadowed_launches(64, 64, 4096, 0, 4096) == (3, 24) and R.launches(64, 64, 4096, 0) == (2, 56)
    # the camera of the two-launch render: a few pixels meet the ground on either side of row 504, none above row 480
    scene = scenes("planar")
    c = S.boundary_camera(scene)
    origins, directions = R.rays(c)
    status = RM.raycast(scene.omodel, RM.sampler(scene.otree, scene.T, scene.B, scene.layers), origins, directions, 0.0, 1.0, 1, 0)["status"].reshape(512, 8)
    assert not (status[:480] != RM.MISS).any() and 4 <= (status[:504] == RM.HIT).sum() <= 40 and 8 <= (status[504:] == RM.HIT).sum() <= 64

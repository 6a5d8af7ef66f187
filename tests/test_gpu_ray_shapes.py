"""The three kernels that march rays (raycast_kernel, render_kernel<false|true>, occlusion_kernel) on the device, branch by branch, on the
cases of tests/_ray_cases.py (test_ray_cases.py shows without a device that each case reaches what it is named for):

A. exact planar scenes whose results are closed forms: hit steps at chosen lanes and rounds, chosen k in every refinement round, ray
   counts 1, 3 and 5, t_min == t_max; pictures whose 64 lanes of a block each leave the march at another, known step; 70 shadow rays
   across a wave and a direction boundary; a picture whose launches hold less than one row of 8 x 8 blocks.
B. the three forms of the ceiling skip (skip_above in bt_raycast_device.hpp): border 0 and an inverted height range, where it is off,
   and border 1, the smallest border at which it is on.  These compare with the CPU models, which never skip.

No tolerance anywhere and no excluded ray or pixel."""
import numpy as np
import pytest

import _cases as K
import _ray_cases as RC
import _raycast_model as RM
import _render_model as R
import _shadow_model as S
import bevy_terrain_amd as bt
from bevy_terrain_amd import _ffi
from test_gpu_raycast import Streamed, assert_hits_equal, assert_mix, make_rays
from test_gpu_render import assert_planes_equal, device_camera
from test_gpu_shadow import assert_shadowed_equal, counts_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device():
    return bt.Device(0)


def as_scene(s, texture_size=R.T, border_size=R.B):
    """a Streamed terrain as the render and shadow models want it"""
    s.T, s.B = texture_size, border_size
    s.approximate_height = s.tree.view_state().approximate_height  # the height the kernels read: the last frame's sample
    return s


def overwrite(s, make):
    """every loaded tile replaced, on the device and in the oracle's copy, by make(tile): the preprocess's downsampling would smear a
    pattern put into the source raster, and the tree of these scenes blends two LODs nearly everywhere"""
    for index in s.layers:
        s.layers[index] = make(s.layers[index])
        s.atlas.upload_tile(0, index, s.layers[index])
    assert np.array_equal(s.atlas.download_tile(0, max(s.layers)), s.layers[max(s.layers)])
    return s


@pytest.fixture(scope="module")
def plane(device, tmp_path_factory):
    """the terrain of test_ground_at_max_height_is_met_at_the_ceiling: every texel 65535, the ground is the plane at max_height"""
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(K, "smooth_raster", lambda h, w, seed, device=None: np.full((h, w), 65535, np.uint16))
        s = as_scene(Streamed(device, tmp_path_factory.mktemp("plane"), "planar"))
    assert all((layer == 65535).all() for layer in s.layers.values())
    return s


# ---- A1: raycast_kernel ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("steps,rounds", RC.MARCHES)
def test_raycast_equals_the_closed_forms(plane, steps, rounds):
    """the whole grid of the march in one batch, every byte; then the same rays at counts 1, 3 and 5 (waves of the only workgroup leave at
    index >= count, the second workgroup of 5 is partial)"""
    b = RC.a1_batch(steps, rounds)
    got = plane.tree.raycast(0, b.origins, b.directions, b.t_min, b.t_max, steps=steps, refine_rounds=rounds)
    assert_hits_equal(got, b.expected)
    for count in (1, 3, 5):
        sel = (21 + 37 * np.arange(count)) % len(got)
        few = plane.tree.raycast(0, b.origins[sel], b.directions[sel], b.t_min[sel], b.t_max[sel], steps=steps, refine_rounds=rounds)
        assert len(few) == count and few.tobytes() == got[sel].tobytes(), count
        assert_hits_equal(few, b.expected[sel])


# ---- A2: render_kernel, both instances -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", RC.A2_CAMERAS, ids=lambda c: f"{c[0]}x{c[1]}-{c[2]}-{c[3]}-{float(c[5]):g}")
def test_pictures_equal_the_closed_forms(plane, case):
    """t, status and the counters are the closed form; normal and colour the model's; bt_tile_tree_render_shadowed gives the same four
    planes, and its shadow plane is the model's"""
    width, height, steps, rounds, delta, base = case
    c = RC.ortho_camera(width, height, steps, delta, base)
    exp = RC.expected_planes(c, steps, rounds, delta)
    got = plane.tree.render(device_camera(c), steps=steps, refine_rounds=rounds)
    assert np.array_equal(got["status"], exp.status), np.argwhere(got["status"] != exp.status)[:8]
    assert got["t"].tobytes() == exp.t.tobytes(), np.argwhere(got["t"] != exp.t)[:8]
    assert got["stats"] == exp.stats
    assert_planes_equal(got, R.render(plane, c, steps, rounds))
    lift, distance = RC.SHADOW_LIFT * delta, RC.SHADOW_STEPS * RC.SHADOW_DS * delta
    shadowed = plane.tree.render_shadowed(device_camera(c), lift, distance, RC.SHADOW_STEPS, steps=steps, refine_rounds=rounds)
    assert np.array_equal(shadowed["status"], exp.status) and shadowed["t"].tobytes() == exp.t.tobytes() and shadowed["stats"] == exp.stats
    assert_shadowed_equal(shadowed, S.render_shadowed(plane, c, steps, rounds, lift, distance, RC.SHADOW_STEPS))


# ---- A3: occlusion_kernel and the shadowed render ----------------------------------------------------------------------------------------------

def test_occlusion_equals_the_closed_form(plane):
    """70 points x (down, up): ray g crosses a wave boundary at 64 and a direction boundary at 70, every lane leaves at its own step"""
    points, directions, m, exp = RC.a3_points()
    lift, distance = RC.A3_LIFT * RC.A3_DELTA, RC.A3_STEPS * RC.A3_DELTA
    got, stats = plane.tree.sun_occlusion(0, points, directions, lift, distance, RC.A3_STEPS)
    assert got.shape == (70, 2) and np.array_equal(got, exp), np.argwhere(got != exp)[:8]
    assert stats == dict(launches=1, **counts_of(exp))
    for k in (0, 1):  # each direction alone
        got, stats = plane.tree.sun_occlusion(0, points, directions[k], lift, distance, RC.A3_STEPS)
        assert np.array_equal(got[:, 0], exp[:, k]) and stats == dict(launches=1, **counts_of(exp[:, k])), k


@pytest.mark.parametrize("sun_up", [False, True])
@pytest.mark.parametrize("base", [151, 41])
def test_the_shadow_plane_equals_the_closed_form(plane, base, sun_up):
    """the 8 x 8 pictures at (200, 0) under a sun straight down or straight up: BT_SHADOW_NONE where the pixel missed, INSIDE where the
    lifted point is still under the ground, else HIT (down, at step 1) or lit (up)"""
    delta = 0.25
    c = RC.ortho_camera(8, 8, 200, delta, base, sun=(0.0, 1.0 if sun_up else -1.0, 0.0))
    exp = RC.expected_planes(c, 200, 0, delta)
    lift, distance = RC.SHADOW_LIFT * delta, RC.SHADOW_STEPS * RC.SHADOW_DS * delta
    got = plane.tree.render_shadowed(device_camera(c), lift, distance, RC.SHADOW_STEPS, steps=200, refine_rounds=0)
    assert np.array_equal(got["shadow"], RC.expected_shadow(exp, RC.pixel_offsets(c, delta), sun_up))
    assert np.array_equal(got["shadow"] == _ffi.SHADOW_NONE, exp.status == RM.MISS)
    assert np.array_equal(got["status"], exp.status) and got["t"].tobytes() == exp.t.tobytes() and got["stats"] == exp.stats
    assert_shadowed_equal(got, S.render_shadowed(plane, c, 200, 0, lift, distance, RC.SHADOW_STEPS))


# ---- A4: the render's short launch ---------------------------------------------------------------------------------------------------------------

def test_a_launch_shorter_than_a_row_of_blocks(plane):
    """488 x 8 at (4096, 4): 60 of the 61 blocks in the first launch, one in the second.  The camera is so high that all but the last few
    samples of every ray are above the ceiling and fetch nothing, so the launch is cheap."""
    a = RC.A4
    count, per_launch = R.launches(a.width, a.height, a.steps, a.rounds)
    assert count == 2 and per_launch < (a.width + 7) // 8
    c = RC.a4_camera()
    exp = RC.expected_planes(c, a.steps, a.rounds, a.delta)
    got = plane.tree.render(device_camera(c), steps=a.steps, refine_rounds=a.rounds)
    assert got["stats"]["launches"] == 2 and got["stats"] == exp.stats
    assert np.array_equal(got["status"], exp.status), np.argwhere(got["status"] != exp.status)[:8]
    assert got["t"].tobytes() == exp.t.tobytes(), np.argwhere(got["t"] != exp.t)[:8]
    hit = exp.status == RM.HIT
    normal = np.zeros((a.height, a.width, 3), np.float32)
    normal[hit] = (0.0, 1.0, 0.0)
    rgba = np.tile(np.array(RC.BACKGROUND, np.uint8), (a.height, a.width, 1))
    rgba[hit] = (128, 128, 128, 255)  # enc8(0.5 * 1.0), unlit
    assert got["normal"].tobytes() == normal.tobytes() and got["rgba"].tobytes() == rgba.tobytes()


# ---- B0: border 0, the skip is off ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def border0(device, tmp_path_factory):
    s = Streamed(device, tmp_path_factory.mktemp("border0"), "planar", texture_size=32, border_size=0)
    return as_scene(overwrite(s, RC.b0_tile), 32, 0)


@pytest.mark.parametrize("steps,rounds", [(256, 2), (65, 4)])
def test_border_0_rays_hit_above_the_ceiling(border0, steps, rounds):
    """every sample of these rays is above lerp(min, max, 1.0f): a kernel that skipped there whatever the border would report 96 misses"""
    s = border0
    origins, directions, t_min, t_max = RC.b0_rays(s.omodel)
    exp = RM.raycast(s.omodel, s.sample, origins, directions, t_min, t_max, steps, rounds)
    above, miss = RC.hits_above_ceiling(s.omodel, exp)
    assert above >= 8 and miss >= 8, (above, miss)
    got = s.tree.raycast(0, origins, directions, t_min, t_max, steps=steps, refine_rounds=rounds)
    assert_hits_equal(got, exp)
    # the border-0 sample itself, which the sampling tests do not cover: the device's equals the oracle's at the hit positions
    p = exp["position"][exp["status"] == RM.HIT]
    heights = s.tree.sample_attachment(0, p)[1]
    assert heights.tobytes() == np.asarray(s.sample(p), np.float32).tobytes() and (heights > np.float32(s.omodel.max_height)).sum() >= 8


def test_border_0_picture(border0):
    s = border0
    c = R.resized(R.scene_cameras("planar", s.omodel, s.view)["main"], 17, 9)
    exp = R.render(s, c, 96, 2)
    assert exp.stats["hit_pixels"] >= 30 and exp.stats["miss_pixels"] >= 10, exp.stats
    assert_planes_equal(s.tree.render(device_camera(c), steps=96, refine_rounds=2), exp)


B0_SUNS = np.array([R._unit((0.9, 0.05, 0.3)), [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])


def test_border_0_shadow_rays(border0):
    """shadow rays from the points the grazing rays met, towards a low sun, level along x and straight up: they start and stay above the
    ceiling, and more than a few are occluded"""
    s = border0
    origins, directions, t_min, t_max = RC.b0_rays(s.omodel)
    hits = RM.raycast(s.omodel, s.sample, origins, directions, t_min, t_max, 256, 2)
    points = hits["position"][hits["status"] == RM.HIT]
    status, counts = S.occlusion(s.omodel, s.sample, points, B0_SUNS, 1.0, 300.0, 200)
    assert len(points) >= 8 and counts["occluded"] >= 8 and counts["lit"] >= 8, counts
    assert (RM.altitude(s.omodel, S.shadow_origins(s.omodel, points, 1.0)) > RC.ceiling(s.omodel)).sum() >= 8
    got, stats = s.tree.sun_occlusion(0, points, B0_SUNS, 1.0, 300.0, 200)
    assert np.array_equal(got, status), np.argwhere(got != status)[:8]
    assert stats == dict(launches=1, **counts)


def test_border_0_shadowed_picture(border0):
    s = border0
    c = R.resized(R.scene_cameras("planar", s.omodel, s.view)["main"], 17, 9)
    c.sun = tuple(float(np.float32(v)) for v in B0_SUNS[0])
    exp = S.render_shadowed(s, c, 96, 2, 1.0, 300.0, 48)
    assert np.isin(exp.shadow, (S.HIT, S.INSIDE)).sum() >= 8 and (exp.shadow == S.MISS).sum() >= 8
    assert_shadowed_equal(s.tree.render_shadowed(device_camera(c), 1.0, 300.0, 48, steps=96, refine_rounds=2), exp)


# ---- B1: border 1, the smallest at which the skip is on ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["planar", "sphere"])
def test_border_1_ground_is_met_at_the_ceiling(device, tmp_path, kind):
    """plateaus of value exactly 1.0 beside every tile edge (the first sample coordinate of a tile is b - 0.5 = 0.5): rays straight down
    whose sample 64 lies at the ceiling.  Those samples must be fetched, and they hit."""
    s = as_scene(overwrite(Streamed(device, tmp_path, kind, texture_size=32, border_size=1), RC.b1_tile), 32, 1)
    origins, directions, t_min, t_max = RC.b1_rays(s.omodel, s.view, s.sample)
    exp = RM.raycast(s.omodel, s.sample, origins, directions, t_min, t_max, 128, 2)
    assert RC.met_at_the_ceiling(s.omodel, exp) >= 8 and (exp["status"] == RM.MISS).sum() >= 8
    got = s.tree.raycast(0, origins, directions, t_min, t_max, steps=128, refine_rounds=2)
    assert_hits_equal(got, exp)
    if kind == "planar":  # every ray has the one direction: the same rays as shadow rays without a lift, one lane each
        status, stats = s.tree.sun_occlusion(0, origins, directions[0], 0.0, 128.0 * RC.B1_DELTA, 128)
        assert np.array_equal(status[:, 0], exp["status"].astype(np.uint8)) and stats["occluded"] == int((exp["status"] == RM.HIT).sum())
    c = R.resized(R.scene_cameras(kind, s.omodel, s.view)["main"], 17, 9)
    assert_planes_equal(s.tree.render(device_camera(c), steps=96, refine_rounds=2), R.render(s, c, 96, 2))


# ---- B2: an inverted height range, the skip is off -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def inverted(device, tmp_path_factory):
    """max_height < min_height: lerp(min, max, 1.0f) is the LOWEST ground, a skip above it would drop nearly every hit"""
    s = as_scene(Streamed(device, tmp_path_factory.mktemp("inverted"), "planar", model=RC.inverted_models()))
    assert float(s.omodel.max_height) < float(s.omodel.min_height)
    return s


def test_inverted_range_rays(inverted):
    s = inverted
    origins, directions, t_min, t_max = make_rays(RC.geometric_range(s.omodel), s.view, 200, seed=356)
    exp = RM.raycast(s.omodel, s.sample, origins, directions, t_min, t_max, 256, 2)
    assert_mix(exp, 256)
    hit = exp["status"] == RM.HIT
    assert (RM.altitude(s.omodel, exp["position"][hit]) > RC.ceiling(s.omodel)).sum() * 2 >= hit.sum()
    assert_hits_equal(s.tree.raycast(0, origins, directions, t_min, t_max, steps=256, refine_rounds=2), exp)


def test_inverted_range_picture_and_shadow_rays(inverted):
    s = inverted
    c = R.resized(R.scene_cameras("planar", RC.geometric_range(s.omodel), s.view)["main"], 17, 9)
    exp = R.render(s, c, 96, 2)
    assert exp.stats["hit_pixels"] >= 30, exp.stats
    got = s.tree.render(device_camera(c), steps=96, refine_rounds=2)
    points = exp.hits["position"][exp.met][:70]
    suns = np.array([R._unit((np.cos(2.8), 0.2, np.sin(2.8))), [0.0, -1.0, 0.0]])
    status, counts = S.occlusion(s.omodel, s.sample, points, suns, 5.0, 600.0, 48)
    assert counts["occluded"] >= 8 and counts["lit"] >= 8, counts
    occlusion, stats = s.tree.sun_occlusion(0, points, suns, 5.0, 600.0, 48)
    assert_planes_equal(got, exp)
    assert np.array_equal(occlusion, status) and stats == dict(launches=1, **counts)

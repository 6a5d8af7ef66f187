"""bt_tile_tree_render without a GPU: the CPU model of its definition (tests/_render_model.py: pixel rays, _raycast_model's march,
_normal_model's WORLD NORMAL, the oracle's sample_attachment, f32 shading) against closed forms, so that model and kernel cannot share a
misreading; bt.render_rays against the model's rays; the entry point's export and NULL-handle refusal; and the conditions the scenes of
test_gpu_render.py must satisfy for its comparisons to mean something, asserted on scenes built without a device.

Closed forms.  On a terrain with nothing loaded every sample is 0: the ground is the min_height surface, the tile normal (0, 0, 1), the
grey 0.  On a terrain whose tiles all hold one value the ground is a plane / sphere at that height, the world normal the mesh normal, the
grey half the value.  The slack on t is test_raycast_model.py's (64 ulp of four times the coordinates' magnitude, derived there)."""
import ctypes as C
import math
import types

import numpy as np
import pytest

import _cases as K
import _oracle as O
import _raycast_model as RM
import _render_model as R
from test_gpu_tile_tree import camera_path
from test_raycast_model import ulp_slack
from test_tile_tree_host import MODELS

F = np.float32
T, B, LODS, VALUE = 16, 2, 3, 40000


def constant_scene(kind, load=True, value=VALUE):
    """test_raycast_model.constant_terrain as a scene of the render model: an oracle tree two frames into streaming a terrain whose every
    tile holds `value` (load=False: nothing is ever loaded)"""
    om = MODELS[kind][1]
    sides = 1 if kind == "planar" else 6
    existing = [(s, l, x, y) for s in range(sides) for l in range(LODS) for x in range(2 ** l) for y in range(2 ** l)]
    stream = O.Stream(len(existing) + 8, 1, existing=existing if load else [])
    s = types.SimpleNamespace(omodel=om, T=T, B=B, layers={}, approximate_height=0.0)
    s.otree = O.TileTree(om, LODS, O.make_view_config(tree_size=4, load_distance=1.2, blend_distance=1.0))
    s.view = (10.0, 300.0, 3.0) if kind == "planar" else (0.4 * 6.4e6, 0.8 * 6.4e6, 0.45 * 6.4e6)
    for _ in range(2):
        s.otree.update(s.view)
        for _, index in stream.finish_loads(stream.pending_loads()):
            s.layers[index] = np.full((T, T), value, np.uint16)
        s.otree.apply_requests(stream)
        s.otree.adjust_to_tile_atlas(stream)
    s.unorm = F(value if load else 0) / F(65535.0)
    s.h = float(F(om.min_height) + (F(om.max_height) - F(om.min_height)) * s.unorm)
    return s


def test_the_entry_point_is_exported_and_refuses_null_handles():
    from bevy_terrain_amd import _ffi
    assert "bt_tile_tree_render" in _ffi.header_symbols() and "bt_tile_tree_render" in _ffi.PROTOTYPES
    assert C.sizeof(_ffi.RenderCameraC) == 152 and C.sizeof(_ffi.RenderStatsC) == 16
    assert _ffi.RenderCameraC.t_min.offset == 96 and _ffi.RenderCameraC.width.offset == 112 and _ffi.RenderCameraC.sun.offset == 128
    assert _ffi.RenderCameraC.background.offset == 144
    L = _ffi.lib()
    cam = _ffi.RenderCameraC()
    cam.width = cam.height = 1
    t = (C.c_double * 1)(7.0)
    assert L.bt_tile_tree_render(None, None, 0, C.byref(cam), 64, 1, t, None, None, None, None) == -1  # BT_ERR_INVALID_ARGUMENT
    assert b"NULL" in L.bt_last_error() and t[0] == 7.0


@pytest.mark.parametrize("orthographic", [False, True])
@pytest.mark.parametrize("width,height", [(1, 1), (9, 7), (64, 3)])
def test_render_rays_equal_the_model(width, height, orthographic):
    import bevy_terrain_amd as bt
    rng = np.random.default_rng(width * 10 + height)
    v = rng.normal(size=(4, 3)) * [[1000.0], [1.0], [0.7], [0.4]]
    cm = R.camera(v[0], v[1], v[2], v[3], width, height, 0.0, 1.0, orthographic=orthographic)
    cb = bt.RenderCamera(v[0], v[1], v[2], v[3], width, height, 0.0, 1.0, orthographic=orthographic)
    exp, got = R.rays(cm), bt.render_rays(cb)
    for a, b in zip(got, exp):
        assert a.dtype == np.float64 and a.shape == (width * height, 3) and a.tobytes() == b.tobytes()
    # the constructors: a unit forward, right and up orthogonal to it and to one another, scaled by the half extents
    mk = bt.RenderCamera.orthographic if orthographic else bt.RenderCamera.perspective
    c = mk(v[0], v[1], (0.0, 1.0, 0.0), 0.8, width, height, 0.5, 9.0) if not orthographic else mk(v[0], v[1], (0.0, 1.0, 0.0), 30.0, 20.0, width, height, 0.5, 9.0)
    assert abs(np.linalg.norm(c.forward) - 1.0) < 1e-15 and abs(c.forward @ c.right) < 1e-12 and abs(c.forward @ c.up) < 1e-12 and abs(c.right @ c.up) < 1e-12
    ex, ey = (30.0, 20.0) if orthographic else (math.tan(0.4) * width / height, math.tan(0.4))
    assert np.isclose(np.linalg.norm(c.right), ex, rtol=1e-14) and np.isclose(np.linalg.norm(c.up), ey, rtol=1e-14)
    assert c.orthographic == orthographic and (c.t_min, c.t_max) == (0.5, 9.0) and c.up[1] > 0.0


def test_the_first_and_last_pixel_centres():
    """sx, sy run from -1 + 1 / width to 1 - 1 / width: pixel (0, 0) is the top left"""
    c = R.camera((0, 0, 0), (0, 0, -1), (1, 0, 0), (0, 1, 0), 4, 2, 0.0, 1.0)
    d = R.rays(c)[1].reshape(2, 4, 3)
    assert np.array_equal(d[0, 0], [-0.75, 0.5, -1.0]) and np.array_equal(d[1, 3], [0.75, -0.5, -1.0])


@pytest.mark.parametrize("steps,rounds", [(64, 0), (96, 2)])
def test_top_down_over_the_plane(steps, rounds):
    """an orthographic camera straight down over the planar model: every pixel meets the ground plane at the same depth, with the normal
    (0, 1, 0); nothing loaded, the grey is 0 whatever the light; all tiles at VALUE, it is enc8(g * (ambient + (1 - ambient) * sun.y))"""
    for load in (False, True):
        s = constant_scene("planar", load=load)
        ground = float(s.omodel.position[1]) + s.h
        eye_y = ground + 431.0
        sun, ambient = (0.36, 0.8, 0.48), 0.3
        c = R.look((35.0, eye_y, -20.0), (0.0, -1.0, 0.0), (1.0, 0.0, 0.0), 300.0, 200.0, 9, 7, 0.0, 600.0, orthographic=True, lighting=True, sun=sun,
                   ambient=ambient, background=(1, 2, 3, 4))
        assert np.array_equal(c.forward, [0.0, -1.0, 0.0])
        r = R.render(s, c, steps, rounds)
        assert (r.status == RM.HIT).all() and r.stats == dict(launches=1, hit_pixels=63, inside_pixels=0, miss_pixels=0)
        slack, width = ulp_slack(1000.0), (600.0 / steps) / 64.0 ** rounds
        assert (r.t + slack >= 431.0).all() and (r.t - width - slack <= 431.0).all()
        assert np.array_equal(r.normal, np.broadcast_to(np.array([0.0, 1.0, 0.0], np.float32), (7, 9, 3)))
        g = F(0.5) * s.unorm
        k = F(ambient) + (F(1.0) - F(ambient)) * F(sun[1])
        byte = int(np.floor(F(0.5) + F(255.0) * (g * k)))
        assert (byte == 0) == (not load) and (not load or byte == round(255 * 0.5 * VALUE / 65535 * (0.3 + 0.7 * 0.8)))
        assert np.array_equal(r.rgba, np.broadcast_to(np.array([byte, byte, byte, 255], np.uint8), (7, 9, 4)))
        # without the light: the grey itself
        c.lighting = False
        plain = int(np.floor(F(0.5) + F(255.0) * g))
        assert np.array_equal(R.render(s, c, steps, rounds).rgba[..., 0], np.full((7, 9), plain, np.uint8))


def test_perspective_above_the_sphere_misses_where_the_rays_miss_it():
    """nothing loaded: the ground is the sphere of radius a + min_height.  A ray misses it when its closest approach to the centre stays
    outside, and must be found when its chord is longer than two steps; the camera is chosen so that every pixel is one or the other by
    more than a step, and then MISS pixels are exactly the rays that miss the sphere"""
    s = constant_scene("sphere", load=False)
    centre = np.array([float(s.omodel.position[i]) for i in range(3)])
    radius = float(s.omodel.a) + s.h
    up = R._unit(s.view)
    eye = centre + up * (radius + 2.0e6)
    east = R._unit(np.cross(up, (0.0, 0.0, 1.0)))
    steps, reach = 256, 9.0e6
    c = R.look(eye, R._unit(-up * 0.55 + east * 0.8), up, 0.8, 0.5, 17, 9, 0.0, reach, background=(9, 8, 7, 6))
    origins, directions = R.rays(c)
    step_length = np.linalg.norm(directions, axis=1) * reach / steps
    u = directions / np.linalg.norm(directions, axis=1, keepdims=True)
    along = np.einsum("ij,ij->i", centre - origins, u)
    closest = np.linalg.norm((centre - origins) - along[:, None] * u, axis=1)
    chord = 2.0 * np.sqrt(np.maximum(radius ** 2 - closest ** 2, 0.0))
    misses = closest > radius + step_length
    meets = (chord > 2.0 * step_length) & (along - 0.5 * chord + 2.0 * step_length < np.linalg.norm(directions, axis=1) * reach)
    assert (misses | meets).all() and misses.sum() >= 20 and meets.sum() >= 40  # the input: no pixel grazes within a step
    r = R.render(s, c, steps, 2)
    assert np.array_equal(r.status.ravel() == RM.MISS, misses) and np.array_equal(r.status.ravel() == RM.HIT, meets)
    # ... and a miss has the background, no depth and no normal; a hit the closed-form depth (in units of the unnormalised direction)
    miss = r.status == RM.MISS
    assert (r.rgba[miss] == (9, 8, 7, 6)).all() and not r.t[miss].any() and not r.normal[miss].any()
    exact = ((along - 0.5 * chord) / np.linalg.norm(directions, axis=1))[meets]
    slack, width = ulp_slack(6.4e6), (reach / steps) / 64.0 ** 2
    t = r.t.ravel()[meets]
    assert (t + slack >= exact).all() and (t - width - 8.0 * np.spacing(reach) - slack <= exact).all()
    # the world normal over a constant field is the mesh normal: the unit vector from the centre to the hit point
    p = r.hits["position"][meets]
    assert np.abs(r.normal.reshape(-1, 3)[meets] - p / np.linalg.norm(p, axis=1, keepdims=True)).max() < 4 * 2.0 ** -24


def test_statuses_background_and_invalid_cameras():
    s = constant_scene("planar")
    ground = float(s.omodel.position[1]) + s.h
    c = R.look((0.0, ground - 5.0, 0.0), (0.0, 1.0, 0.0), (1.0, 0.0, 0.0), 10.0, 10.0, 3, 2, 1.5, 50.0, orthographic=True, background=(5, 6, 7, 8))
    r = R.render(s, c, 16, 2)  # an origin under the ground: INSIDE at t_min, shaded like a hit
    assert (r.status == RM.INSIDE).all() and (r.t == 1.5).all() and (r.rgba[..., 3] == 255).all() and r.stats["inside_pixels"] == 6
    c.forward = np.array([0.0, np.nan, 0.0])
    r = R.render(s, c, 16, 2)
    assert (r.status == RM.INVALID).all() and not r.t.any() and not r.normal.any() and (r.rgba == (5, 6, 7, 8)).all()
    assert r.stats == dict(launches=1, hit_pixels=0, inside_pixels=0, miss_pixels=0)


def test_enc8_and_launches():
    v = np.array([-1.0, 0.0, 0.5 / 255.0, 0.4999 / 255.0, 0.5, 1.0, 2.0, np.nan, np.inf, -np.inf], np.float32)
    assert R.enc8(v).tolist() == [0, 0, 1, 0, 128, 255, 255, 0, 255, 0]
    # 64 x 64 at 4096 steps: a band of 8 blocks costs 8 * 64 * 4097 samples, seven bands fit 2^24, the eighth is a launch of its own
    assert R.launches(64, 64, 4096, 0) == (2, 56)
    assert R.launches(17, 9, 96, 2) == (1, 6) and R.launches(1, 1, 1, 0) == (1, 1)
    # an image wider than a launch: runs of blocks within a band
    per_block = 64 * (4096 + 1 + 63 * 4)
    assert R.launches(8 * 100, 8, 4096, 4) == (-(-100 // ((1 << 24) // per_block)), (1 << 24) // per_block)


def cpu_scene(kind, omodel, frames=12, texture_size=R.T, border_size=R.B):
    """test_gpu_raycast.Streamed without a device: the oracle preprocesses the same rasters, its tree streams the tiles along the same camera
    path, and the approximate height of each frame is the oracle's sample_height at the view position"""
    W = 2 ** (R.LODS - 1) * (texture_size - 2 * border_size) + 13
    spherical = kind != "planar"
    atlas = O.OracleAtlas(R.LODS, 6 * 400 if spherical else 400, spherical, [(texture_size, border_size, 1, O.FORMAT_R16)])
    atlas.clear_attachment(0)
    if spherical:
        atlas.preprocess_spherical(0, [K.smooth_raster(W, W, seed=3 + s) for s in range(6)], (0, R.LODS))
    else:
        atlas.preprocess_tile(0, K.smooth_raster(W, W, seed=3), (0, R.LODS))
    atlas.run(4)
    tiles = {coord: atlas.tile(0, i) for coord, i in atlas.tiles()}
    s = types.SimpleNamespace(omodel=omodel, T=texture_size, B=border_size, layers={}, approximate_height=0.0)
    s.otree = O.TileTree(omodel, R.LODS, O.make_view_config(tree_size=4, load_distance=1.2, blend_distance=1.0))
    stream = O.Stream(256 if kind == "planar" else 512, 1, existing=list(tiles))
    for pos in camera_path(kind, frames, seed=5):
        s.otree.update(pos)
        for coord, index in stream.finish_loads(stream.pending_loads()):
            s.layers[index] = tiles[coord]
        s.otree.apply_requests(stream)
        s.otree.adjust_to_tile_atlas(stream)
        s.approximate_height = float(s.otree.sample_attachment(O.FORMAT_R16, texture_size, border_size, s.layers, [pos])[1][0])
        s.otree.set_approximate_height(s.approximate_height)
        s.view = pos
    return s


@pytest.mark.parametrize("kind", ["planar", "sphere"])
def test_the_gpu_scenes_satisfy_their_input_conditions(kind):
    """the cameras of test_gpu_render.py on the same terrain built without a device (the oracle preprocesses the raster and streams it along
    the same camera path): the model alone says that the pictures hold hits, misses, pixels inside the ground, several hit steps within
    a block, several LODs and blended hits"""
    scene = cpu_scene(kind, MODELS[kind][1])
    figures = R.input_conditions(scene, R.scene_cameras(kind, scene.omodel, scene.view))
    print(figures)
    R.assert_input_conditions(figures, kind)
    ortho = R.render(scene, R.scene_cameras(kind, scene.omodel, scene.view)["ortho"], 64, 0)
    assert ortho.stats["hit_pixels"] >= 100 and len(set(ortho.rgba[..., 0].ravel().tolist())) >= 8

"""bt_tile_tree_render on the device: byte equality of all four planes and the stats with the CPU model of its definition
(tests/_render_model.py), equality with the existing device calls on the same rays and hit points (independent of the model's march),
several launches, an albedo attachment, optional planes, the call as a read of the atlas, and the refusals.

The terrains are test_gpu_raycast.py's Streamed (T = 32, b = 2, 4 LODs; planar, sphere, ellipsoid), the cameras _render_model.scene_cameras
at the last position of the camera path.  No tolerance and no excluded pixel anywhere; the note of test_gpu_raycast.py on the last place of
the f64 log2 applies here as it does there."""
import ctypes as C
import types

import numpy as np
import pytest

import _oracle as O
import _render_model as R
import bevy_terrain_amd as bt
from bevy_terrain_amd import _ffi
from test_gpu_raycast import Streamed
from test_tile_tree_host import MODELS

pytestmark = pytest.mark.gpu
BT_ERR_INVALID_ARGUMENT, BT_ERR_UNSUPPORTED = -1, -5
PLANES = ("t", "status", "normal", "rgba")


@pytest.fixture(scope="module")
def device():
    return bt.Device(0)


@pytest.fixture(scope="module")
def terrains(device, tmp_path_factory):
    cache = {}

    def get(kind):
        if kind not in cache:
            s = Streamed(device, tmp_path_factory.mktemp(kind), kind)
            # the scene as the render model wants it
            s.T, s.B = R.T, R.B
            s.approximate_height = s.tree.view_state().approximate_height  # the height the kernels read: the last frame's sample
            s.cameras = R.scene_cameras(kind, s.omodel, s.view)
            cache[kind] = s
        return cache[kind]

    return get


def device_camera(c):
    """the model's camera as the package's: the same vectors, bit for bit"""
    return bt.RenderCamera(c.origin, c.forward, c.right, c.up, c.width, c.height, c.t_min, c.t_max, orthographic=c.orthographic, lighting=c.lighting,
                           albedo_attachment=c.albedo, sun=c.sun, ambient=c.ambient, background=c.background)


def assert_planes_equal(got, exp):
    assert np.array_equal(got["status"], exp.status), np.argwhere(got["status"] != exp.status)[:8]
    for name in ("t", "normal", "rgba"):
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(getattr(exp, name))
        assert a.dtype == b.dtype and a.shape == b.shape, name
        assert a.tobytes() == b.tobytes(), (name, np.argwhere((a != b).reshape(a.shape[0], a.shape[1], -1).any(axis=2))[:8])
    assert got["stats"] == exp.stats


def enc8(v):
    return R.enc8(np.asarray(v, dtype=np.float32))


# ---- 1. equality with the model -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("steps,rounds", R.MARCHES)
@pytest.mark.parametrize("width,height", R.SIZES)
@pytest.mark.parametrize("kind", ["planar", "sphere"])
def test_planes_equal_the_model(terrains, kind, width, height, steps, rounds):
    """1 x 1: one lane; 8 x 8: one full block; 9 x 7: partial blocks on both edges; 17 x 9: three blocks across with a partial last one and
    two block rows.  The lit perspective scene, and the one whose t_min plane cuts the ground (INSIDE pixels)."""
    s = terrains(kind)
    for name in ("main", "inside"):
        c = R.resized(s.cameras[name], width, height)
        exp = R.render(s, c, steps, rounds)
        got = s.tree.render(device_camera(c), steps=steps, refine_rounds=rounds)
        assert_planes_equal(got, exp)


@pytest.mark.parametrize("kind", ["planar", "sphere"])
def test_the_scenes_satisfy_their_input_conditions(terrains, kind):
    """test_render_model.py asserts these on a scene built without a device; here on the streamed one itself, so the comparison above
    cannot pass on pictures without hits, misses, pixels inside the ground, several hit steps in a block, several LODs or blended hits"""
    s = terrains(kind)
    R.assert_input_conditions(R.input_conditions(s, s.cameras), kind)


def test_the_ellipsoid_equals_the_model(terrains):
    s = terrains("ellipsoid")
    c = R.resized(s.cameras["main"], 8, 8)
    exp = R.render(s, c, 64, 0)
    assert exp.stats["hit_pixels"] >= 12 and exp.stats["miss_pixels"] >= 6, exp.stats
    assert_planes_equal(s.tree.render(device_camera(c), steps=64, refine_rounds=0), exp)


@pytest.mark.parametrize("kind", ["planar", "sphere"])
def test_the_orthographic_camera_equals_the_model(terrains, kind):
    s = terrains(kind)
    c = s.cameras["ortho"]
    exp = R.render(s, c, 96, 2)
    assert exp.stats["hit_pixels"] >= 100, exp.stats
    assert_planes_equal(s.tree.render(device_camera(c), steps=96, refine_rounds=2), exp)


# ---- 2. equality with the existing device calls -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["planar", "sphere", "ellipsoid"])
def test_planes_equal_the_existing_calls(terrains, kind):
    """independent of the model's march: t and status are tree.raycast's on bt.render_rays(camera), the normal plane tree.sample_normal's
    at those positions, the grey enc8(0.5 * value) of tree.sample_attachment there.  33 x 17 at (256, 2): five blocks across, three
    down, partial on both edges."""
    s = terrains(kind)
    c = R.resized(s.cameras["main"], 33, 17)
    c.lighting = False
    cam = device_camera(c)
    got = s.tree.render(cam, steps=256, refine_rounds=2)
    origins, directions = bt.render_rays(cam)
    hits = s.tree.raycast(0, origins, directions, c.t_min, c.t_max, steps=256, refine_rounds=2)
    met = (hits["status"] == _ffi.RAY_HIT) | (hits["status"] == _ffi.RAY_INSIDE)
    assert met.sum() * 5 >= len(hits) and (hits["status"] == _ffi.RAY_MISS).sum() * 10 >= len(hits)
    assert np.array_equal(got["status"].ravel(), hits["status"].astype(np.uint8))
    assert got["t"].tobytes() == np.ascontiguousarray(hits["t"]).tobytes()
    # position and height: the render's t gives the position raycast reports, and the grey is made of the height's value
    assert np.array_equal(origins[met] + got["t"].ravel()[met, None] * directions[met], hits["position"][met])
    normals = np.zeros((len(hits), 3), np.float32)
    normals[met] = s.tree.sample_normal(0, hits["position"][met])[0]
    assert got["normal"].tobytes() == normals.tobytes()
    values, heights = s.tree.sample_attachment(0, hits["position"][met])
    assert heights.tobytes() == np.ascontiguousarray(hits["height"][met]).tobytes()
    rgba = np.tile(np.array(c.background, np.uint8), (len(hits), 1))
    grey = enc8(np.float32(0.5) * values[:, 0])
    rgba[met] = np.stack([grey, grey, grey, np.full_like(grey, 255)], axis=1)
    assert got["rgba"].tobytes() == rgba.tobytes() and len(set(grey.tolist())) >= 8
    assert got["stats"] == dict(launches=1, hit_pixels=int((hits["status"] == _ffi.RAY_HIT).sum()), inside_pixels=int((hits["status"] == _ffi.RAY_INSIDE).sum()),
                                miss_pixels=int((hits["status"] == _ffi.RAY_MISS).sum()))
    # with the light: the Lambert term on those normals
    c.lighting = True
    lit = s.tree.render(device_camera(c), steps=256, refine_rounds=2, planes=("rgba",))["rgba"]
    base = np.stack([np.float32(0.5) * values[:, 0]] * 3 + [np.ones(len(values), np.float32)], axis=1)
    rgba[met] = R.shade(c, base, normals[met])
    assert lit.tobytes() == rgba.tobytes()


# ---- 3. several launches ------------------------------------------------------------------------------------------------------------------------

def test_two_launches(terrains):
    """64 x 64 at 4096 steps: a band of 8 x 8 blocks is 8 * 64 * 4097 worst-case samples, seven bands fit BT_RAYCAST_MAX_SAMPLES, so rows
    0 .. 55 are one launch and rows 56 .. 63 the next"""
    s = terrains("planar")
    c = R.resized(s.cameras["ortho"], 64, 64)
    c.lighting = False
    cam = device_camera(c)
    count, per_launch = R.launches(64, 64, 4096, 0)
    assert (count, per_launch) == (2, 56)
    boundary = per_launch // 8 * 8  # the first row of the second launch
    got = s.tree.render(cam, steps=4096, refine_rounds=0)
    assert got["stats"]["launches"] >= 2 and got["stats"]["launches"] == count
    origins, directions = bt.render_rays(cam)
    batch = _ffi.RAYCAST_MAX_SAMPLES // (64 * ((4096 + 1 + 63) // 64))  # raycast's own limit: whole rounds of 64 per ray
    hits = np.concatenate([s.tree.raycast(0, origins[i:i + batch], directions[i:i + batch], c.t_min, c.t_max, steps=4096, refine_rounds=0)
                           for i in range(0, len(origins), batch)])
    assert len(hits) == 4096 and batch < 4096
    status = hits["status"].reshape(64, 64)
    assert (status[boundary - 1] == _ffi.RAY_HIT).any() and (status[boundary] == _ffi.RAY_HIT).any()
    assert (status[:boundary] == _ffi.RAY_HIT).sum() >= 1000 and (status[boundary:] == _ffi.RAY_HIT).sum() >= 100
    assert np.array_equal(got["status"], status.astype(np.uint8))
    assert got["t"].tobytes() == np.ascontiguousarray(hits["t"]).tobytes()
    met = hits["status"] == _ffi.RAY_HIT
    normals = np.zeros((4096, 3), np.float32)
    normals[met] = s.tree.sample_normal(0, hits["position"][met])[0]
    assert got["normal"].tobytes() == normals.tobytes()
    grey = enc8(np.float32(0.5) * s.tree.sample_attachment(0, hits["position"][met])[0][:, 0])
    rgba = np.tile(np.array(c.background, np.uint8), (4096, 1))
    rgba[met] = np.stack([grey, grey, grey, np.full_like(grey, 255)], axis=1)
    assert got["rgba"].tobytes() == rgba.tobytes()
    assert got["stats"]["hit_pixels"] == int(met.sum()) and got["stats"]["hit_pixels"] + got["stats"]["miss_pixels"] + got["stats"]["inside_pixels"] == 4096


# ---- 4. an albedo attachment --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def painted(device):
    """a planar atlas with an R16 height and an Rgba8 attachment (different texture sizes), every tile of a 3-LOD pyramid allocated and
    filled without a job, and a tree adjusted to it"""
    import _cases as K
    model = MODELS["planar"][0]
    lods = 3
    cfg = bt.TerrainConfig(lod_count=lods, atlas_size=32, path="terrains/painted", model=model)
    cfg.add_attachment(bt.AttachmentConfig(name="height", texture_size=16, border_size=2, format=bt.AttachmentFormat.R16))
    cfg.add_attachment(bt.AttachmentConfig(name="albedo", texture_size=20, border_size=1, format=bt.AttachmentFormat.Rgba8))
    atlas = bt.TileAtlas.new(cfg, device)
    rng = np.random.default_rng(17)
    for lod in range(lods):
        for x in range(2 ** lod):
            for y in range(2 ** lod):
                index = atlas.get_or_allocate_tile(bt.TileCoordinate(0, lod, x, y))[1]
                atlas.upload_tile(0, index, K.smooth_raster(16, 16, seed=100 + index))
                atlas.upload_tile(1, index, rng.integers(0, 256, size=(20, 20, 4), dtype=np.uint8))
    tree = bt.TileTree.new(atlas, bt.TerrainViewConfig(tree_size=4, load_distance=1.2, blend_distance=1.0))
    view = (60.0, 320.0, -40.0)
    tree.update(view)
    tree.adjust_to_tile_atlas()
    entries = tree.read()[0]
    assert len(set(entries[entries[:, 1] != O.INVALID, 1].tolist())) >= 2
    return types.SimpleNamespace(atlas=atlas, tree=tree, view=view, omodel=MODELS["planar"][1])


def test_albedo(painted):
    s = painted
    base = R.scene_cameras("planar", s.omodel, s.view)["main"]
    base.background = (3, 2, 1, 0)
    origins, directions = bt.render_rays(device_camera(base))
    hits = s.tree.raycast(0, origins, directions, base.t_min, base.t_max, steps=96, refine_rounds=2)
    met = (hits["status"] == _ffi.RAY_HIT) | (hits["status"] == _ffi.RAY_INSIDE)
    assert met.sum() >= 60 and (~met).sum() >= 15
    normals = s.tree.sample_normal(0, hits["position"][met])[0]
    colours = s.tree.sample_attachment(1, hits["position"][met])[0]
    greys = s.tree.sample_attachment(0, hits["position"][met])[0][:, 0]
    assert len(set(map(tuple, enc8(colours).tolist()))) >= 30  # the picture is not one colour
    for albedo, lighting in ((1, False), (1, True), (None, False), (None, True)):
        c = types.SimpleNamespace(**vars(base))
        c.albedo, c.lighting = albedo, lighting
        got = s.tree.render(device_camera(c), steps=96, refine_rounds=2)
        assert np.array_equal(got["status"].ravel(), hits["status"].astype(np.uint8))
        exp = np.tile(np.array(c.background, np.uint8), (len(hits), 1))
        value = colours if albedo is not None else np.stack([np.float32(0.5) * greys] * 3 + [np.ones(len(greys), np.float32)], axis=1)
        exp[met] = R.shade(c, value, normals)
        assert got["rgba"].tobytes() == exp.tobytes(), (albedo, lighting)
    assert len(set(enc8(colours[:, 3]).tolist())) >= 20  # (the albedo's alpha, which no light touches, varies too)


# ---- 5. optional planes, an invalid camera ------------------------------------------------------------------------------------------------------

def test_optional_planes_and_an_invalid_camera(terrains):
    s = terrains("sphere")
    c = s.cameras["main"]
    cam = device_camera(c)
    full = s.tree.render(cam, steps=64, refine_rounds=1)
    subsets = [(p,) for p in PLANES] + [(p, q) for i, p in enumerate(PLANES) for q in PLANES[i + 1:]]
    assert len(subsets) == 10
    for planes in subsets:
        got = s.tree.render(cam, steps=64, refine_rounds=1, planes=planes)
        assert set(got) == set(planes) | {"stats"} and got["stats"] == full["stats"], planes
        for p in planes:
            assert got[p].tobytes() == full[p].tobytes(), (planes, p)
    bad = types.SimpleNamespace(**vars(c))
    bad.forward = np.array([c.forward[0], np.nan, c.forward[2]])
    got = s.tree.render(device_camera(bad), steps=64, refine_rounds=1)  # BT_OK: render() raises on anything else
    assert (got["status"] == _ffi.RAY_INVALID).all() and not got["t"].any() and not got["normal"].any()
    assert (got["rgba"] == np.array(c.background, np.uint8)).all()
    assert got["stats"] == dict(launches=1, hit_pixels=0, inside_pixels=0, miss_pixels=0)


# ---- 6. a read ------------------------------------------------------------------------------------------------------------------------------------

def test_render_is_a_read(device, terrains):
    """test_gpu_raycast.test_raycast_is_a_read for the render call: a render of an atlas nothing has written leaves Attachment::written
    alone, so the job with no-data texels that follows takes prev_zero as often as it does without the call; and a render of a loaded
    atlas leaves every layer's bytes unchanged"""
    from test_gpu_tile_bounds import holed_job
    counts = []
    for read_first in (False, True):
        atlas, pre = holed_job(device)
        if read_first:
            tree = bt.TileTree.new(atlas, bt.TerrainViewConfig(tree_size=4))
            model = atlas.config.model
            eye = np.array(model.translation, dtype=np.float64) + [0.0, float(model.max_height) + 10.0, 0.0]
            cam = bt.RenderCamera.orthographic(eye, (0.0, -1.0, 0.0), (1.0, 0.0, 0.0), 50.0, 50.0, 4, 4, 0.0, float(model.max_height - model.min_height) + 20.0)
            got = tree.render(cam)
            assert got["stats"]["hit_pixels"] == 16 and (got["rgba"] == (0, 0, 0, 255)).all()
        pre.run(atlas)
        counts.append(pre.stats()["prev_zero_launches"])
    assert counts[0] > 0 and counts[1] == counts[0], counts
    s = terrains("planar")
    used = max(s.layers) + 1
    before = s.atlas.download_tiles(0, 0, used).copy()
    s.tree.render(device_camera(s.cameras["main"]))
    assert np.array_equal(s.atlas.download_tiles(0, 0, used), before)


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_planes_untouched(device, terrains, painted):
    L = _ffi.lib()
    s = terrains("planar")
    good = device_camera(s.cameras["main"]).c()
    n = good.width * good.height
    t, status = np.full(n, 7.5), np.full(n, 0xAB, np.uint8)
    normal, rgba = np.full(3 * n, 7.5, np.float32), np.full(4 * n, 0xAB, np.uint8)
    planes = (t.ctypes.data_as(C.POINTER(C.c_double)), status.ctypes.data_as(C.POINTER(C.c_uint8)), normal.ctypes.data_as(C.POINTER(C.c_float)),
              rgba.ctypes.data_as(C.POINTER(C.c_uint8)))
    stats = _ffi.RenderStatsC(9, 9, 9, 9)
    tree, atlas = s.tree._h, s.atlas._h

    def call(tree=tree, atlas=atlas, ai=0, cam=good, steps=64, rounds=1, planes=planes):
        return L.bt_tile_tree_render(tree, atlas, ai, C.byref(cam) if cam is not None else None, steps, rounds, *planes, C.byref(stats))

    def changed(**fields):
        cam = _ffi.RenderCameraC.from_buffer_copy(good)
        for name, value in fields.items():
            if name in ("sun",):
                for i in range(3):
                    cam.sun[i] = value[i]
            else:
                setattr(cam, name, value)
        return cam

    other = bt.Device(0)  # a second context on the same GPU
    foreign = bt.TileAtlas.new(s.atlas.config, other)
    invalid = {
        "NULL tree": dict(tree=None), "NULL atlas": dict(atlas=None), "NULL camera": dict(cam=None), "all planes NULL": dict(planes=(None, None, None, None)),
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
    # the formats: a height attachment that is Rgba8, an albedo attachment that is R16
    ptree, patlas = painted.tree._h, painted.atlas._h
    assert call(tree=ptree, atlas=patlas, ai=1) == BT_ERR_UNSUPPORTED
    assert call(tree=ptree, atlas=patlas, ai=0, cam=changed(albedo_attachment=0)) == BT_ERR_UNSUPPORTED
    assert call(tree=ptree, atlas=patlas, ai=0, cam=changed(albedo_attachment=2)) == BT_ERR_INVALID_ARGUMENT
    # nothing was touched by any of the above
    assert (t == 7.5).all() and (status == 0xAB).all() and (normal == 7.5).all() and (rgba == 0xAB).all()
    assert (stats.launches, stats.hit_pixels, stats.inside_pixels, stats.miss_pixels) == (9, 9, 9, 9)
    # the limits themselves are accepted: 4096 steps, 4 refinement rounds (one pixel), stats == NULL; and the planes are then written
    one = changed(width=1, height=1)
    assert L.bt_tile_tree_render(tree, atlas, 0, C.byref(one), 4096, 4, *planes, None) == _ffi.BT_OK
    assert t[0] != 7.5 and (t[1:] == 7.5).all() and (status[1:] == 0xAB).all() and status[0] in (0, 1, 2)
    # the scratch stays in the context until bt_ctx_trim, and the call works again after it
    before = s.tree.render(device_camera(s.cameras["main"]), steps=64, refine_rounds=1)
    assert device.trim() > 0
    again = s.tree.render(device_camera(s.cameras["main"]), steps=64, refine_rounds=1)
    assert all(before[p].tobytes() == again[p].tobytes() for p in PLANES) and before["stats"] == again["stats"]

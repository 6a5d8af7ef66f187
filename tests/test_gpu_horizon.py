"""Horizon culling in the tiling prepass: the three kernels' forms, with a horizon view set, against the numpy model of the definition
(tests/_horizon_model.py), bit-exact — the plain form's list in order, the unordered form's set, the indirect arguments, the visit and
cull counts — on spheres and ellipsoids, from just above the ground to orbit."""
import ctypes as C
import math

import numpy as np
import pytest

import _cull_model as M
import _horizon_model as H
import _refine_model as R
import bevy_terrain_amd as bt
from bevy_terrain_amd import _ffi
from test_gpu_culling import device_table, random_table, set_culling, three_forms, travel_cameras
from test_gpu_refine import form_positions, sorted_rows
from test_horizon_model import eye_above, make_model

pytestmark = pytest.mark.gpu

NO_PLANES = np.zeros((0, 4), np.float32)


@pytest.fixture(scope="module")
def device():
    return bt.Device(0)


def set_state(prepass, model, pos, cull, hb, margin=0.0):
    """culling and the horizon view of a frame on the prepass; -> the model's HorizonView of what bt_cull_horizon gave"""
    set_culling(prepass, cull, hb)
    hc = bt.cull_horizon(model, tuple(pos), margin)
    prepass.set_horizon(hc)
    return H.HorizonView.from_c(hc)


def check_forms(prepass, view, cull, horizon, table, note):
    """all three forms of a prepass with culling and a horizon view set against the model; -> (final tiles, tiles culled)"""
    exp, exp_culled, exp_visited = H.refine_culled_horizon(view, cull, horizon, table)
    exp_indirect = (view.vertices_per_tile * len(exp), 1, 0, 0)
    prepass.run(view, plain=True)
    plain, indirect = prepass.read()
    assert np.array_equal(plain, exp), note
    assert tuple(indirect) == exp_indirect and prepass.cull_stats() == (exp_visited, exp_culled), note
    plain = plain.copy()
    prepass.run(view)
    ours, indirect = prepass.read()
    assert np.array_equal(ours, plain) and tuple(indirect) == exp_indirect and prepass.cull_stats() == (exp_visited, exp_culled), note
    prepass.run(view, unordered=True)
    ours, indirect = prepass.read()
    assert len(ours) == len(exp) and np.array_equal(sorted_rows(ours), sorted_rows(exp)), note
    assert tuple(indirect) == exp_indirect and prepass.cull_stats() == (exp_visited, exp_culled), note
    return len(exp), exp_culled


def ascent(model, n=6):
    """(eye, clip_from_world) from 2 m above max_height to orbit over a point off every cube face's centre, looking down, level and above
    the horizon at each height"""
    d = np.array([0.35, 0.85, -0.4])
    d /= np.linalg.norm(d)
    side = np.cross(d, [0.0, 0.0, 1.0])
    side /= np.linalg.norm(side)
    out = []
    for k in range(n):
        eye = eye_above(model, d, model.max_height + 2.0 * 10.0 ** (k * 6.9 / (n - 1)))
        for pitch in (-70.0, 0.0, 12.0):
            direction = math.cos(math.radians(pitch)) * side + math.sin(math.radians(pitch)) * d
            out.append((eye, M.clip_from_world(eye, direction, math.radians(60.0), 16.0 / 9.0, near=0.1, up=d)))
    return out


@pytest.mark.parametrize("planes", [5, 0])
@pytest.mark.parametrize("with_table", [False, True])
@pytest.mark.parametrize("kind", ["sphere", "ellipsoid"])
def test_camera_path(device, kind, with_table, planes):
    model = make_model(kind, position=(0.0, 0.0, 0.0) if kind == "sphere" else (3.0e7, -2.0e6, 5.0e5))
    cfg = bt.TerrainViewConfig(geometry_tile_count=300000)
    prepass = bt.TilingPrepass(device, cfg.geometry_tile_count)
    table = random_table(np.random.default_rng(2), 6, 4) if with_table else None
    hb = device_table(device, table)
    kept = culled = unculled = 0
    for eye, clip in ascent(model):
        v = bt.make_view_state(model, cfg, tuple(eye))
        cull = M.CullView(bt.cull_planes(clip) if planes else NO_PLANES, 0.0, model.min_height, model.max_height)
        horizon = set_state(prepass, model, eye, cull, hb)
        n, c = check_forms(prepass, v, cull, horizon, table, (kind, tuple(eye)))
        frustum_only = len(M.refine_culled(v, cull, table)[0])
        assert n < frustum_only or planes  # alone, the horizon test always drops the far side
        kept, culled, unculled = kept + n, culled + c, unculled + frustum_only
    assert culled > 500 and 18 * 4 < kept < unculled


@pytest.mark.parametrize("seed", range(8))
def test_random_views(device, seed):
    """random models (off the origin, small and large), view configs, eyes, cameras, plane counts, tables and margins"""
    rng = np.random.default_rng(52_000 + seed)
    major = float(rng.choice([50.0, 6378137.0]))
    centre = tuple(float(x) for x in rng.uniform(-500.0, 500.0, 3) * major / 50.0)
    lo, hi = float(rng.choice([-0.002, 0.0, 0.0005])) * major, 0.0015 * major
    model = bt.TerrainModel.sphere(centre, major, lo, hi) if seed % 2 else bt.TerrainModel.ellipsoid(centre, major, major * float(rng.choice([0.5, 0.9966])), lo, hi)
    cfg = bt.TerrainViewConfig(geometry_tile_count=150000, refinement_count=int(rng.choice([4, 12, 30])), grid_size=int(rng.choice([4, 16, 32])),
                               subdivision_tolerance=float(rng.choice([0.05, 0.1, 0.5])), morph_distance=float(rng.choice([2.0, 8.0, 16.0])),
                               origin_lod=int(rng.integers(0, 14)))
    prepass = bt.TilingPrepass(device, cfg.geometry_tile_count)
    table = random_table(rng, 6, int(rng.integers(1, 6))) if seed % 3 else None
    hb = device_table(device, table)
    culled = 0
    for frame in range(8):
        d = rng.normal(size=3)
        eye = eye_above(model, d / np.linalg.norm(d), hi + major * 10.0 ** rng.uniform(-6.0, 0.5))
        v = bt.make_view_state(model, cfg, tuple(eye), approximate_height=float(rng.uniform(lo, hi)))
        clip = M.clip_from_world(eye, rng.normal(size=3), math.radians(rng.uniform(30.0, 100.0)), float(rng.choice([1.0, 16.0 / 9.0])), near=10.0 ** rng.uniform(-3, 1))
        cull = M.CullView(bt.cull_planes(clip)[: int(rng.integers(0, 6))], float(rng.choice([0.0, 0.0, 0.1 * (hi - lo)])), lo, hi)
        horizon = set_state(prepass, model, eye, cull, hb, margin=float(rng.choice([0.0, 0.0, 0.01 * major])))
        culled += check_forms(prepass, v, cull, horizon, table, (seed, frame, tuple(eye)))[1]
    assert culled > 0


@pytest.mark.parametrize("kind", ["sphere", "ellipsoid"])
def test_result_does_not_depend_on_the_window(device, kind):
    """the walk over the tiles no window covers applies the horizon test in place: radius 1 and 5 push most of the tree through it"""
    model, positions = form_positions(kind)
    cfg = bt.TerrainViewConfig(geometry_tile_count=400000)
    prepass = bt.TilingPrepass(device, cfg.geometry_tile_count)
    table = random_table(np.random.default_rng(3), 6, 3)
    hb = device_table(device, table)
    rng = np.random.default_rng(4)
    total = 0
    for i, pos in enumerate(positions[::3]):
        v = bt.make_view_state(model, cfg, pos)
        clip = M.clip_from_world(pos, rng.normal(size=3), math.radians(70.0), 16.0 / 9.0, near=0.1)
        cull = M.CullView(bt.cull_planes(clip) if i % 2 else NO_PLANES, 0.0, model.min_height, model.max_height)
        horizon = set_state(prepass, model, pos, cull, hb)
        exp, exp_culled, exp_visited = H.refine_culled_horizon(v, cull, horizon, table)
        for radius in (1, 5, 0):
            prepass.set_window(radius)
            prepass.run(v, unordered=True)
            ours, indirect = prepass.read()
            assert len(ours) == len(exp) and np.array_equal(sorted_rows(ours), sorted_rows(exp)), (kind, pos, radius)
            assert tuple(indirect) == (v.vertices_per_tile * len(exp), 1, 0, 0) and prepass.cull_stats() == (exp_visited, exp_culled), (kind, pos, radius)
        total += len(exp)
    assert total > 500


def test_none_restores_the_frustum_only_result(device):
    for kind in ("sphere", "ellipsoid"):
        model, positions = form_positions(kind)
        cfg = bt.TerrainViewConfig(geometry_tile_count=400000)
        fresh, prepass = bt.TilingPrepass(device, cfg.geometry_tile_count), bt.TilingPrepass(device, cfg.geometry_tile_count)
        hb = device_table(device, random_table(np.random.default_rng(5), 6, 2))
        fewer = 0
        for pos in positions[::5]:
            v = bt.make_view_state(model, cfg, pos)
            planes = bt.cull_planes(M.clip_from_world(pos, (0.3, -0.5, 0.8), math.radians(50.0), 1.0))
            for state in (fresh, prepass):
                state.set_culling(planes, min_height=model.min_height, max_height=model.max_height, bounds=hb)
            expected = three_forms(fresh, v)
            prepass.set_horizon(bt.cull_horizon(model, pos))
            on = three_forms(prepass, v)
            prepass.set_horizon(None)
            off = three_forms(prepass, v)
            assert prepass.cull_stats() == fresh.cull_stats()
            for a, b, c in zip(expected, off, on):
                assert np.array_equal(a[0], b[0]) and a[1] == b[1] and len(c[0]) <= len(a[0])
            # the eye inside the occluder (vh <= 0): the view is accepted and culls nothing
            inside = bt.cull_horizon(model, tuple(eye_above(model, (0.0, 1.0, 0.0), model.min_height - 5000.0)))
            assert inside.vh < 0
            prepass.set_horizon(inside)
            for a, b in zip(expected, three_forms(prepass, v)):
                assert np.array_equal(a[0], b[0]) and a[1] == b[1]
            prepass.set_horizon(None)
            fewer += sum(len(a[0]) - len(c[0]) for a, c in zip(expected, on))
        assert fewer > 0


def test_frame_update_runs_the_prepass_with_its_horizon_state(device, tmp_path):
    """two streaming instances of one spherical terrain in lock step, culling and the horizon view set on both prepasses: A makes the
    separate calls, B one bt_frame_update per frame"""
    from test_gpu_tile_tree import MODELS, build_terrain, camera_path

    model, _ = MODELS["sphere"]
    lods, T, b = 3, 32, 2
    root, cfg, _ = build_terrain(device, tmp_path, model, lods, T, b)
    vc = bt.TerrainViewConfig(tree_size=4, load_distance=1.2, blend_distance=1.0, geometry_tile_count=40000)

    def instance():
        scfg = bt.TerrainConfig(lod_count=lods, atlas_size=512, path=cfg.path, model=model)
        scfg.add_attachment(bt.AttachmentConfig(name="height", texture_size=T, border_size=b, format=bt.AttachmentFormat.R16, mip_level_count=3))
        atlas = bt.TileAtlas.new(scfg, device)
        atlas.load_tile_config(root)
        return atlas, bt.TileTree.new(atlas, vc), bt.TilingPrepass(device, vc.geometry_tile_count)

    atlas_a, tree_a, prepass_a = instance()
    atlas_b, tree_b, prepass_b = instance()
    path = camera_path("sphere", 9, seed=5)
    horizon_culled = 0
    for frame, (pos, clip) in enumerate(zip(path, travel_cameras(path, centre=(0.0, 0.0, 0.0)))):
        cull = M.CullView(bt.cull_planes(clip) if frame % 2 else NO_PLANES, 0.0, model.min_height, model.max_height)
        horizon = set_state(prepass_a, model, pos, cull, None)
        set_state(prepass_b, model, pos, cull, None)
        form = [{}, {"unordered": True}, {"plain": True}][frame % 3]
        tree_a.update(pos)
        atlas_a.update(root)
        tree_a.apply_requests()
        tree_a.adjust_to_tile_atlas()
        tree_a.approximate_height()
        v = tree_a.view_state()
        prepass_a.run(v, **form)
        atlas_b.update(root)
        tree_b.frame_update(pos, prepass_b, **form)
        ta, ia = prepass_a.read()
        tb, ib = prepass_b.read()
        assert tuple(ia) == tuple(ib) and prepass_a.cull_stats() == prepass_b.cull_stats(), frame
        assert np.array_equal(sorted_rows(ta), sorted_rows(tb)) and ("unordered" in form or np.array_equal(ta, tb)), frame
        exp, exp_culled, exp_visited = H.refine_culled_horizon(v, cull, horizon)
        assert np.array_equal(sorted_rows(tb), sorted_rows(exp)) and prepass_b.cull_stats() == (exp_visited, exp_culled), frame
        horizon_culled += exp_culled - M.refine_culled(v, cull)[1]
    assert horizon_culled > 0


def test_overflow_verdict_counts_horizon_culled_tiles_as_visited(device):
    model = make_model("sphere")
    pos = tuple(eye_above(model, np.array([0.6, 0.64, 0.48]), 40000.0))
    cull = M.CullView(NO_PLANES, 0.0, model.min_height, model.max_height)
    horizon = H.HorizonView.from_c(bt.cull_horizon(model, pos))
    v_full = bt.make_view_state(model, bt.TerrainViewConfig(geometry_tile_count=100000), pos)
    passes = []
    exp, exp_culled, _ = H.refine_culled_horizon(v_full, cull, horizon, None, passes)
    assert 50 < len(exp) < 20000 and exp_culled > 0
    verdicts = []
    for capacity in range(8, 2 * len(exp) + 64, max(13, len(exp) // 23)):
        prepass = bt.TilingPrepass(device, capacity)
        v = bt.make_view_state(model, bt.TerrainViewConfig(geometry_tile_count=capacity), pos)
        set_state(prepass, model, pos, cull, None)
        expected = M.overflows(passes, len(exp), capacity)
        for form in ({"plain": True}, {}, {"unordered": True}):
            prepass.run(v, **form)
            try:
                tiles, _ = prepass.read()
                assert not expected and len(tiles) == len(exp), (capacity, form)
            except bt.BtError as e:
                assert e.status == -7 and expected, (capacity, form)
        verdicts.append(expected)
        prepass.close()
    assert any(verdicts) and not all(verdicts)


def test_refusals(device):
    L = _ffi.lib()
    model = make_model("sphere")
    cfg = bt.TerrainViewConfig(geometry_tile_count=50000)
    pos = (0.0, 6500000.0, 0.0)
    v = bt.make_view_state(model, cfg, pos)
    prepass = bt.TilingPrepass(device, cfg.geometry_tile_count)
    good = bt.cull_horizon(model, pos, 10.0)

    def status(fn):
        with pytest.raises(bt.BtError) as e:
            fn()
        assert str(e.value).split(": ", 2)[2]  # a message
        return e.value.status

    def altered(**fields):
        h = _ffi.HorizonViewC.from_buffer_copy(good)
        for name, value in fields.items():
            if name == "eye":
                h.eye[1] = value
            else:
                setattr(h, name, value)
        return h

    for bad in (float("nan"), float("inf"), -float("inf")):
        for field in ("eye", "vh", "occluder_radius", "margin"):
            assert status(lambda: prepass.set_horizon(altered(**{field: bad}))) == -1, (field, bad)
    for radius in (0.0, -0.5, 1.0000001):
        assert status(lambda: prepass.set_horizon(altered(occluder_radius=radius))) == -1
    assert status(lambda: prepass.set_horizon(altered(margin=-1.0e-6))) == -1
    prepass.set_horizon(altered(occluder_radius=1.0, margin=0.0, vh=-3.0))  # legal: the edge of the radius, an eye inside the occluder
    assert L.bt_tiling_prepass_set_horizon(None, C.byref(good)) == -1 and L.bt_tiling_prepass_set_horizon(None, None) == -1
    # a refused view leaves the state as it was: still runnable, and the horizon view without culling is refused by every run
    prepass.set_horizon(good)
    for form in ({}, {"plain": True}, {"unordered": True}):
        assert status(lambda: prepass.run(v, **form)) == -1
    prepass.set_culling(NO_PLANES, min_height=model.min_height, max_height=model.max_height)
    expected = H.refine_culled_horizon(v, M.CullView(NO_PLANES, 0.0, model.min_height, model.max_height), H.HorizonView.from_c(good))
    for form in ({}, {"plain": True}):
        prepass.run(v, **form)
        assert np.array_equal(prepass.read()[0], expected[0]) and prepass.cull_stats() == (expected[2], expected[1]) and expected[1] > 0
    prepass.set_culling(None)
    assert status(lambda: prepass.run(v)) == -1
    # a planar view
    planar = bt.TerrainModel.planar((0.0, 0.0, 0.0), 1000.0, 0.0, 250.0)
    pv = bt.make_view_state(planar, cfg, (10.0, 300.0, 20.0))
    flat = bt.TilingPrepass(device, cfg.geometry_tile_count)
    flat.set_culling(NO_PLANES, min_height=0.0, max_height=250.0)
    flat.set_horizon(good)
    for form in ({}, {"plain": True}, {"unordered": True}):
        assert status(lambda: flat.run(pv, **form)) == -1
    flat.set_horizon(None)
    flat.run(pv)
    assert len(flat.read()[0]) == len(R.refine(pv)[0])

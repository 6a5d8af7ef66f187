"""Frustum and height-bounds culling in the tiling prepass: the three kernels' forms against the numpy model of the definition
(tests/_cull_model.py), bit-exact — the plain form's list in order, the unordered form's set, the indirect arguments, the visit and cull
counts — and bt_height_bounds_build against the table rules on atlases filled by real preprocessing jobs."""
import ctypes as C
import math

import numpy as np
import pytest

import _cases as K
import _cull_model as M
import _refine_model as R
import bevy_terrain_amd as bt
from bevy_terrain_amd import _ffi
from test_cull_model import visited_tiles
from test_gpu_refine import form_positions, sorted_rows, spiral

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device():
    return bt.Device(0)


def random_table(rng, sides, levels):
    table = M.Table(sides, levels)
    lo = rng.integers(0, 50000, table.entries)
    table.data[:, 0] = lo
    table.data[:, 1] = lo + rng.integers(0, 15000, table.entries)
    return table


def device_table(device, table):
    if table is None:
        return None
    hb = bt.HeightBounds(device, table.sides, table.levels)
    hb.write(table.data)
    assert np.array_equal(hb.read(), table.data)
    return hb


def set_culling(prepass, cull, hb):
    prepass.set_culling(cull.planes, margin=float(cull.margin), min_height=float(cull.min_height), max_height=float(cull.max_height), bounds=hb)


def check_forms(prepass, view, cull, table, note):
    """all three forms of a prepass with culling set against the model; -> (final tiles, tiles culled)"""
    exp, exp_culled, exp_visited = M.refine_culled(view, cull, table)
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


def travel_cameras(positions, centre=None):
    """a 60 degree x 16:9 camera at every position of a path, looking along the direction of travel"""
    out = []
    for i, pos in enumerate(positions):
        a, b = (positions[i], positions[i + 1]) if i + 1 < len(positions) else (positions[i - 1], positions[i])
        direction = np.asarray(b, np.float64) - np.asarray(a, np.float64)
        up = (0.0, 1.0, 0.0) if centre is None else tuple(np.asarray(pos, np.float64) - np.asarray(centre, np.float64))
        out.append(M.clip_from_world(pos, direction, math.radians(60.0), 16.0 / 9.0, near=0.1, up=up))
    return out


@pytest.mark.parametrize("with_table,margin", [(False, 0.0), (True, 0.0), (True, 12.5)])
def test_planar_camera_path(device, with_table, margin):
    model = bt.TerrainModel.planar((0.0, 0.0, 0.0), 1000.0, 0.0, 250.0)
    cfg = bt.TerrainViewConfig(geometry_tile_count=200000)
    prepass = bt.TilingPrepass(device, cfg.geometry_tile_count)
    table = random_table(np.random.default_rng(1), 1, 5) if with_table else None
    hb = device_table(device, table)
    positions = list(spiral(24, 700.0, 900.0, 130.0))
    kept = total = culled = 0
    for pos, clip in zip(positions, travel_cameras(positions)):
        v = bt.make_view_state(model, cfg, pos)
        cull = M.CullView(bt.cull_planes(clip), margin, 0.0, 250.0)
        set_culling(prepass, cull, hb)
        n, c = check_forms(prepass, v, cull, table, pos)
        kept, culled, total = kept + n, culled + c, total + len(R.refine(v)[0])
    assert culled > 100 and 24 * 4 < kept < total


@pytest.mark.parametrize("with_table,margin", [(False, 0.0), (True, 0.0), (False, 2500.0)])
def test_spherical_camera_path(device, with_table, margin):
    model = bt.TerrainModel.sphere((0.0, 0.0, 0.0), 6371000.0, -12000.0, 9000.0)
    cfg = bt.TerrainViewConfig(geometry_tile_count=300000)
    prepass = bt.TilingPrepass(device, cfg.geometry_tile_count)
    table = random_table(np.random.default_rng(2), 6, 4) if with_table else None
    hb = device_table(device, table)
    positions = []
    for x, h, z in spiral(16, 1.0, 4.0e6, 2.0e3):
        d = np.array([0.3 + x, 0.9, 0.2 + z])
        positions.append(tuple(d / np.linalg.norm(d) * (6371000.0 + h)))
    kept = culled = 0
    for pos, clip in zip(positions, travel_cameras(positions, centre=(0.0, 0.0, 0.0))):
        v = bt.make_view_state(model, cfg, pos)
        cull = M.CullView(bt.cull_planes(clip), margin, -12000.0, 9000.0)
        set_culling(prepass, cull, hb)
        n, c = check_forms(prepass, v, cull, table, pos)
        kept, culled = kept + n, culled + c
    assert culled > 500 and kept > 16 * 4


@pytest.mark.parametrize("seed", range(12))
def test_random_views(device, seed):
    """random models, view configs, camera teleports, cameras, plane counts, tables and margins"""
    from test_gpu_tile_tree import draw_tree_case

    model, _, _, tree_cfg, pts = draw_tree_case(2000 + seed)
    rng = np.random.default_rng(47_000 + seed)
    sides = 6 if model.is_spherical() else 1
    cfg = bt.TerrainViewConfig(geometry_tile_count=150000, refinement_count=int(rng.choice([4, 12, 30])), grid_size=int(rng.choice([4, 16, 32])),
                               subdivision_tolerance=float(rng.choice([0.05, 0.1, 0.5])), morph_distance=float(rng.choice([2.0, 8.0, 16.0])),
                               origin_lod=tree_cfg["origin_lod"])
    prepass = bt.TilingPrepass(device, cfg.geometry_tile_count)
    table = random_table(rng, sides, int(rng.integers(1, 7))) if seed % 3 else None
    hb = device_table(device, table)
    span = float(model.max_height - model.min_height)
    for frame, pos in enumerate(pts[:8]):
        v = bt.make_view_state(model, cfg, pos, approximate_height=float(rng.uniform(0.0, 1.0)))
        direction = rng.normal(size=3)
        clip = M.clip_from_world(pos, direction, math.radians(rng.uniform(30.0, 100.0)), float(rng.choice([1.0, 16.0 / 9.0])), near=10.0 ** rng.uniform(-3, 1))
        planes = bt.cull_planes(clip)[: int(rng.integers(1, 6))]
        cull = M.CullView(planes, float(rng.choice([0.0, 0.0, 0.1 * span])), model.min_height, model.max_height)
        set_culling(prepass, cull, hb)
        check_forms(prepass, v, cull, table, (seed, frame, pos))


@pytest.mark.parametrize("kind", ["planar", "sphere"])
def test_result_does_not_depend_on_the_window(device, kind):
    """the walk over the tiles no window covers culls in place: radius 1 and 5 push most of the tree through it"""
    model, positions = form_positions(kind)
    sides = 6 if kind == "sphere" else 1
    cfg = bt.TerrainViewConfig(geometry_tile_count=400000)
    prepass = bt.TilingPrepass(device, cfg.geometry_tile_count)
    table = random_table(np.random.default_rng(3), sides, 3)
    hb = device_table(device, table)
    rng = np.random.default_rng(4)
    total = 0
    for pos in positions[::3]:
        v = bt.make_view_state(model, cfg, pos)
        clip = M.clip_from_world(pos, rng.normal(size=3), math.radians(70.0), 16.0 / 9.0, near=0.1)
        cull = M.CullView(bt.cull_planes(clip), 0.0, model.min_height, model.max_height)
        set_culling(prepass, cull, hb)
        exp, exp_culled, exp_visited = M.refine_culled(v, cull, table)
        for radius in (1, 5, 0):
            prepass.set_window(radius)
            prepass.run(v, unordered=True)
            ours, indirect = prepass.read()
            assert len(ours) == len(exp) and np.array_equal(sorted_rows(ours), sorted_rows(exp)), (kind, pos, radius)
            assert tuple(indirect) == (v.vertices_per_tile * len(exp), 1, 0, 0) and prepass.cull_stats() == (exp_visited, exp_culled), (kind, pos, radius)
        total += len(exp)
    assert total > 500


def three_forms(prepass, v):
    out = []
    for form in ({}, {"plain": True}, {"unordered": True}):
        prepass.run(v, **form)
        tiles, indirect = prepass.read()
        out.append((sorted_rows(tiles) if form.get("unordered") else tiles.copy(), tuple(indirect)))
    return out


def test_off_means_off(device):
    for kind in ("planar", "sphere"):
        model, positions = form_positions(kind)
        cfg = bt.TerrainViewConfig(geometry_tile_count=400000)
        fresh, prepass = bt.TilingPrepass(device, cfg.geometry_tile_count), bt.TilingPrepass(device, cfg.geometry_tile_count)
        hb = device_table(device, random_table(np.random.default_rng(5), 6 if kind == "sphere" else 1, 2))
        for pos in positions[::5]:
            v = bt.make_view_state(model, cfg, pos)
            clip = M.clip_from_world(pos, (0.3, -0.5, 0.8), math.radians(50.0), 1.0)
            expected = three_forms(fresh, v)
            prepass.set_culling(bt.cull_planes(clip), min_height=model.min_height, max_height=model.max_height, bounds=hb)
            culled = three_forms(prepass, v)
            prepass.set_culling(None)
            off = three_forms(prepass, v)
            assert prepass.cull_stats() == (len(visited_tiles(v)), 0)
            prepass.set_culling(np.zeros((0, 4), np.float32), min_height=model.min_height, max_height=model.max_height, bounds=hb)
            none = three_forms(prepass, v)
            for a, b, c, d in zip(expected, off, none, culled):
                assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[0], c[0]) and a[1] == c[1]
                assert len(d[0]) <= len(a[0])


def test_frame_update_runs_the_prepass_with_its_culling_state(device, tmp_path):
    """two streaming instances of one terrain in lock step, culling set on both prepasses: A makes the separate calls, B one
    bt_frame_update per frame (no new flag: it runs the form its flags pick on the prepass it is given)"""
    from test_gpu_tile_tree import MODELS, build_terrain, camera_path

    model, _ = MODELS["planar"]
    lods, T, b = 4, 32, 2
    root, cfg, _ = build_terrain(device, tmp_path, model, lods, T, b)
    vc = bt.TerrainViewConfig(tree_size=4, load_distance=1.2, blend_distance=1.0, geometry_tile_count=20000)

    def instance():
        scfg = bt.TerrainConfig(lod_count=lods, atlas_size=256, path=cfg.path, model=model)
        scfg.add_attachment(bt.AttachmentConfig(name="height", texture_size=T, border_size=b, format=bt.AttachmentFormat.R16, mip_level_count=3))
        atlas = bt.TileAtlas.new(scfg, device)
        atlas.load_tile_config(root)
        return atlas, bt.TileTree.new(atlas, vc), bt.TilingPrepass(device, vc.geometry_tile_count)

    atlas_a, tree_a, prepass_a = instance()
    atlas_b, tree_b, prepass_b = instance()
    path = camera_path("planar", 12, seed=5)
    culled_total = 0
    for frame, (pos, clip) in enumerate(zip(path, travel_cameras(path))):
        cull = M.CullView(bt.cull_planes(clip), 0.0, model.min_height, model.max_height)
        set_culling(prepass_a, cull, None)
        set_culling(prepass_b, cull, None)
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
        exp, exp_culled, exp_visited = M.refine_culled(v, cull)
        assert np.array_equal(sorted_rows(tb), sorted_rows(exp)) and prepass_b.cull_stats() == (exp_visited, exp_culled), frame
        culled_total += exp_culled
    assert culled_total > 0


def test_overflow_verdict_counts_culled_tiles_as_visited(device):
    model = bt.TerrainModel.planar((0.0, 0.0, 0.0), 1000.0, 0.0, 0.0)
    pos = (40.0, 30.0, -20.0)
    clip = M.clip_from_world(pos, (1.0, -0.4, 0.3), math.radians(60.0), 16.0 / 9.0)
    cull = M.CullView(bt.cull_planes(clip), 0.0, 0.0, 0.0)
    v_full = bt.make_view_state(model, bt.TerrainViewConfig(geometry_tile_count=100000), pos)
    passes = []
    exp, exp_culled, _ = M.refine_culled(v_full, cull, None, passes)
    assert 50 < len(exp) < 20000 and exp_culled > 0
    verdicts = []
    for capacity in range(8, 2 * len(exp) + 64, max(13, len(exp) // 23)):
        prepass = bt.TilingPrepass(device, capacity)
        v = bt.make_view_state(model, bt.TerrainViewConfig(geometry_tile_count=capacity), pos)
        set_culling(prepass, cull, None)
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


def job_atlas(device, kind, T=64, b=2, lods=3, lod_range=None, rect=None, seed=11):
    """an atlas filled by a real preprocessing job"""
    spherical = kind == "cube"
    model = bt.TerrainModel.sphere((0.0, 0.0, 0.0), 6371000.0, -12000.0, 9000.0) if spherical else bt.TerrainModel.planar((0.0, 0.0, 0.0), 1000.0, 0.0, 250.0)
    W = 2 ** (lods - 1) * (T - 2 * b) + 13
    cfg = bt.TerrainConfig(lod_count=lods, atlas_size=(6 if spherical else 1) * 64, path="terrains/bounds", model=model)
    cfg.add_attachment(bt.AttachmentConfig(name="height", texture_size=T, border_size=b, format=bt.AttachmentFormat.R16))
    atlas = bt.TileAtlas.new(cfg, device)
    server = bt.AssetServer()
    pre = bt.Preprocessor.new().clear_attachment(0, atlas)
    lod_range = lod_range or range(0, lods)
    if spherical:
        paths = [f"face{s}" for s in range(6)]
        for s, p in enumerate(paths):
            server.insert(p, K.smooth_raster(W, W, seed=seed + s))
        pre.preprocess_spherical(bt.SphericalDataset(attachment_index=0, paths=paths, lod_range=lod_range), server, atlas)
    else:
        server.insert("src", K.smooth_raster(W, W, seed=seed))
        extent = dict(top_left=rect[0], bottom_right=rect[1]) if rect else {}
        pre.preprocess_tile(bt.PreprocessDataset(attachment_index=0, path="src", lod_range=lod_range, **extent), server, atlas)
    pre.run(atlas)
    return model, atlas


@pytest.mark.parametrize("case", ["planar", "planar_holes", "cube", "cube_partial_lods", "planar_released"])
def test_height_bounds_build(device, case):
    kind = case.split("_")[0]
    model, atlas = job_atlas(device, kind, rect=((0.3, 0.1), (0.8, 0.55)) if case == "planar_holes" else None,
                             lod_range=range(1, 3) if case == "cube_partial_lods" else None)
    sides = 6 if kind == "cube" else 1
    if case == "planar_released":
        for c, _ in atlas.tiles()[::2]:
            atlas.release_tile(c)  # back on the LRU list, still held
    held = {(c.side, c.lod, c.x, c.y): atlas.download_tile(0, i) for c, i in atlas.tiles() if i != _ffi.INVALID_ATLAS_INDEX}
    full = sides * (4 ** 3 - 1) // 3
    assert len(held) == full if case in ("planar", "cube", "planar_released") else 0 < len(held) < full
    last = None
    for levels in (2, 3, 4):
        expected = M.build_table(sides, levels, held)
        hb = bt.HeightBounds(device, sides, levels)
        assert np.array_equal(hb.read(), M.Table(sides, levels).data)  # every entry (0, 65535) after create
        got = hb.build(atlas, 0).read()
        assert np.array_equal(got, expected.data), (case, levels)
        assert np.all(got[:, 0] <= got[:, 1])
        other = bt.HeightBounds(device, sides, levels)
        other.write(got)
        assert np.array_equal(other.read(), got)
        other.close()
        last = (hb, expected)
    hb, table = last
    assert len(np.unique(table.data, axis=0)) > 3  # (the job's heights differ from tile to tile)
    # a culled run with the built table
    cfg = bt.TerrainViewConfig(geometry_tile_count=200000)
    prepass = bt.TilingPrepass(device, cfg.geometry_tile_count)
    rng = np.random.default_rng(9)
    for _ in range(3):
        eye, clip = M.random_camera(rng, "planar" if kind == "planar" else "sphere")
        v = bt.make_view_state(model, cfg, tuple(eye))
        cull = M.CullView(bt.cull_planes(clip), 0.0, model.min_height, model.max_height)
        set_culling(prepass, cull, hb)
        check_forms(prepass, v, cull, table, (case, tuple(eye)))


def test_refusals(device):
    L = _ffi.lib()
    model = bt.TerrainModel.sphere((0.0, 0.0, 0.0), 6371000.0, -12000.0, 9000.0)
    cfg = bt.TerrainViewConfig(geometry_tile_count=50000)
    v = bt.make_view_state(model, cfg, (0.0, 6500000.0, 0.0))
    prepass = bt.TilingPrepass(device, cfg.geometry_tile_count)
    planes = bt.cull_planes(M.clip_from_world((0.0, 6500000.0, 0.0), (1.0, -1.0, 0.0), 1.0, 1.0))

    def status(fn):
        with pytest.raises(bt.BtError) as e:
            fn()
        assert str(e.value).split(": ", 2)[2]  # a message
        return e.value.status

    view = _ffi.CullViewC()
    view.plane_count = 6
    assert L.bt_tiling_prepass_set_culling(prepass._h, C.byref(view), None) == -1
    assert status(lambda: prepass.set_culling(planes, margin=-1.0)) == -1
    assert status(lambda: prepass.set_culling(planes, margin=float("nan"))) == -1
    assert status(lambda: prepass.set_culling(planes, margin=float("inf"))) == -1
    one_side = bt.HeightBounds(device, 1, 3)
    prepass.set_culling(planes, min_height=-12000.0, max_height=9000.0, bounds=one_side)
    for form in ({}, {"plain": True}, {"unordered": True}):
        assert status(lambda: prepass.run(v, **form)) == -1
    assert status(lambda: bt.HeightBounds(device, 1, 0)) == -1 and status(lambda: bt.HeightBounds(device, 6, 12)) == -1
    assert status(lambda: bt.HeightBounds(device, 2, 3)) == -1
    tcfg = bt.TerrainConfig(lod_count=2, atlas_size=8, path="terrains/none", model=bt.TerrainModel.planar((0.0, 0.0, 0.0), 10.0, 0.0, 1.0))
    tcfg.add_attachment(bt.AttachmentConfig(name="albedo", texture_size=16, border_size=2, format=bt.AttachmentFormat.Rgba8))
    atlas = bt.TileAtlas.new(tcfg, device)
    assert status(lambda: one_side.build(atlas, 0)) == -5
    assert status(lambda: one_side.build(atlas, 1)) == -1
    assert status(lambda: one_side.write(np.zeros((3, 2), np.uint16))) == -1
    # NULL handles: statuses, no crash
    out = C.c_void_p()
    assert L.bt_height_bounds_create(None, 1, 1, C.byref(out)) == -1 and L.bt_height_bounds_create(device._h, 1, 1, None) == -1
    assert L.bt_height_bounds_build(None, atlas._h, 0) == -1 and L.bt_height_bounds_build(one_side._h, None, 0) == -1
    assert L.bt_height_bounds_read(None, None, 0) == -1 and L.bt_height_bounds_read(one_side._h, None, 1 << 20) == -1
    assert L.bt_height_bounds_write(None, None, 0) == -1 and L.bt_height_bounds_write(one_side._h, None, 84) == -1
    assert L.bt_tiling_prepass_set_culling(None, None, None) == -1 and L.bt_tiling_prepass_cull_stats(None, None, None) == -1
    assert L.bt_tiling_prepass_cull_stats(prepass._h, None, None) == 0
    L.bt_height_bounds_destroy(None)
    L.bt_cull_planes(None, None)
    # NaN planes cull nothing; beside a real plane they leave its verdict alone
    prepass.set_culling(None)
    expected = three_forms(prepass, v)
    prepass.set_culling(np.full((5, 4), np.nan, np.float32), min_height=-12000.0, max_height=9000.0)
    for a, b in zip(expected, three_forms(prepass, v)):
        assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    assert prepass.cull_stats()[1] == 0
    mixed = np.stack([np.full(4, np.nan, np.float32), planes[0]])
    cull = M.CullView(mixed, 0.0, -12000.0, 9000.0)
    set_culling(prepass, cull, None)
    n, culled = check_forms(prepass, v, cull, None, "mixed")
    assert culled > 0

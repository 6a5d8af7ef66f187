"""The tiling prepass's three forms — plain, assisted (bt_tiling_prepass_run above the estimate's threshold) and unordered — on the cases
of tests/_prepass_cases.py, whose reach (which kernel, which fallback, which source of a pass) test_prepass_cases.py asserts on the CPU:
lists against the oracle in order (the unordered form as a set, its length apart), the indirect arguments, the visit counts against the
numpy model, the exact capacity edges with a byte pattern behind the list, and bt_frame_update's estimate from a height one frame old.
Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import _oracle as O
import _prepass_cases as P
import bevy_terrain_amd as bt
from bevy_terrain_amd import _ffi
from test_refine_model import oracle_view
from test_tile_tree_host import MODELS

pytestmark = pytest.mark.gpu

FORMS = {"plain": dict(plain=True), "default": dict(), "unordered": dict(unordered=True)}
PATTERN = 0xA5  # no tile has a side of 0xA5A5A5A5


@pytest.fixture(scope="module")
def device():
    return bt.Device(0)


def sorted_rows(a):
    return a[np.lexsort(a.T[::-1])]


def assert_list(ours, exp, form, where):
    if form == "unordered":  # the set, each tile once
        assert len(ours) == len(exp), where
        assert np.array_equal(sorted_rows(ours), sorted_rows(exp)), where
    else:
        assert np.array_equal(ours, exp), where


def runs(radii=P.RADII):
    """(form, window radius of the unordered form): the ordered forms once, the unordered form per radius"""
    return [("plain", 0), ("default", 0)] + [("unordered", r) for r in radii]


def read_status(prepass):
    """bt_tiling_prepass_read without a list -> (status, the count prepare_render left)"""
    n = C.c_uint32()
    status = _ffi.lib().bt_tiling_prepass_read(prepass._h, None, 0, C.byref(n), None)
    return status, n.value


@pytest.mark.parametrize("case", P.CASES, ids=repr)
def test_every_form_gives_the_list_the_counts_and_the_arguments(device, case):
    """One prepass per case with the model's smallest capacity (n_min: it fits, exactly).  Each form twice — the second run reuses the
    bits and the counters of the first.  cull_stats() is (the model's visited, 0) whatever the form: counters[2] of the ordered kernels,
    the per-LOD counts of the collector and its walk.  The two cases of _prepass_cases.CULL once more with their plane set, against
    _cull_model's culled list and counts: the walk's in-place cull test, with tiles it culls (asserted on the CPU)."""
    t = P.case_trace(case.name)
    capacity = max(t.n_min, 8)
    v = case.view(capacity)
    exp, exp_indirect, _ = O.refine(oracle_view(v))
    assert np.array_equal(exp, t.final)
    prepass = bt.TilingPrepass(device, capacity)
    for form, radius in runs():
        prepass.set_window(radius)
        for again in range(2):
            prepass.run(v, **FORMS[form])
            ours, indirect = prepass.read()
            assert_list(ours, exp, form, (case, form, radius, again))
            assert list(indirect) == exp_indirect, (case, form, radius, again)
            assert prepass.cull_stats() == (t.visited, 0), (case, form, radius, again)
    if case.name in P.CULL:
        cull = P.CULL[case.name]
        prepass.set_culling(cull["planes"], min_height=cull["min_height"], max_height=cull["max_height"])
        for form, radius in runs():
            c = P.culled_trace(case.name, radius)
            prepass.set_window(radius)
            prepass.run(v, **FORMS[form])
            ours, indirect = prepass.read()
            assert_list(ours, c.final, form, (case, "culled", form, radius))
            assert list(indirect) == [v.vertices_per_tile * len(c.final), 1, 0, 0]
            assert prepass.cull_stats() == (c.visited, c.culled), (case, "culled", form, radius)
    prepass.close()


@pytest.mark.parametrize("name", ["second-sweep", "pass-decides"])
def test_the_capacity_edge_is_exact_and_nothing_is_stored_past_it(device, name):
    """n_min = max(final count, max over the passes of visited + 4 * dividing) fits and n_min - 1 overflows (status -7), in every form
    (the unordered one also at radius 2, where its walk stores finals): second-sweep's final list decides, pass-decides's last pass
    does (256 + 4 * 244 against 12 finals: only the per-LOD test of the unordered verdict sees it).  The capacity comes either from the
    prepass (created with N) or from the view (geometry_tile_count N on buffers of C > N tiles); then final_tiles holds a byte pattern
    before each run and rows [min(count, N), C) hold it afterwards, whether the run fitted or not.  C is more than the view produces
    without a limit: a guard that lets a store through writes inside the allocation."""
    case, t = P.BY_NAME[name], P.case_trace(name)
    exp = t.final
    generous = t.n_min + 64
    assert generous >= len(exp) + 64
    pattern = np.full((generous, 4), PATTERN * 0x01010101, np.uint32)
    for n in (t.n_min, t.n_min - 1):
        fits = n == t.n_min
        for way in ("created", "view"):
            prepass = bt.TilingPrepass(device, n if way == "created" else generous)
            v = case.view(generous if way == "created" else n)
            final_ptr, _ = prepass.buffers()
            for form, radius in runs((0, 2)):
                where = (name, n, way, form, radius)
                prepass.set_window(radius)
                if way == "view":
                    _ffi.check(_ffi.lib().bt_memcpy_h2d(device._h, C.c_void_p(final_ptr), pattern.ctypes.data_as(C.c_void_p), pattern.nbytes))
                prepass.run(v, **FORMS[form])
                status, count = read_status(prepass)
                if fits:
                    assert status == 0 and count == len(exp), where
                    ours, indirect = prepass.read()
                    assert_list(ours, exp, form, where)
                    assert list(indirect) == [v.vertices_per_tile * len(exp), 1, 0, 0], where
                else:
                    assert status == -7, where
                    with pytest.raises(bt.BtError) as e:
                        prepass.read()
                    assert e.value.status == -7, where
                if way == "view":
                    rows = device.download(final_ptr, (generous, 4), np.uint32)
                    kept = min(count, n)
                    assert np.array_equal(rows[kept:], pattern[kept:]), (where, np.flatnonzero((rows != pattern).any(axis=1))[-4:])
                    if form != "unordered":  # what was stored is the head of the list, also when the run overflowed
                        assert np.array_equal(rows[:kept], exp[:kept]), where
            prepass.close()


def test_stale_height_through_frame_update(device, tmp_path):
    """bt_frame_update estimates the LODs that get bits from the host's height, one frame old, while the kernels read the device's.
    Frame 1 is over low ground; frame 2 teleports to 0.25 m above ground about 8 m higher: the stale clearance (about 4 m) gives about 14
    LODs of bits, the real tree (clearance 0.25 m) reaches about LOD 16.  The tiles deeper than the bits take `tile.lod < assist_lods` in
    the assisted kernel and `lod >= lods` in WindowBits::inside with the walk below it.  Two instances in lock step as in
    test_gpu_tile_tree.test_frame_update_equals_the_separate_calls: A makes the separate calls and supplies the view with the fresh
    height for the oracle, B one bt_frame_update per frame, the teleport once per form; a third instance learns the ground first."""
    from test_gpu_tile_tree import build_terrain

    model, _ = MODELS["planar"]
    lods, T, b = 4, 32, 2
    root, cfg, _ = build_terrain(device, tmp_path, model, lods, T, b)
    vc = bt.TerrainViewConfig(tree_size=4, load_distance=1.2, blend_distance=1.0, geometry_tile_count=100000)

    def instance():
        scfg = bt.TerrainConfig(lod_count=lods, atlas_size=256, path=cfg.path, model=model)
        scfg.add_attachment(bt.AttachmentConfig(name="height", texture_size=T, border_size=b, format=bt.AttachmentFormat.R16, mip_level_count=3))
        atlas = bt.TileAtlas.new(scfg, device)
        atlas.load_tile_config(root)
        return atlas, bt.TileTree.new(atlas, vc)

    def separate(atlas, tree, pos):
        """the reference's chain (plugin.rs:46-56) -> the height sampled at pos"""
        tree.update(pos)
        atlas.update(root)
        tree.apply_requests()
        tree.adjust_to_tile_atlas()
        return tree.approximate_height()

    # the warm-up instance: the ground under the low camera, a place nearby (inside the finest tiles already loaded) about 8 m higher,
    # and the height a frame there samples (R16 over 0 .. 250 m resolves 4 mm)
    low = (110.0, 300.0, -47.0)
    atlas_w, tree_w = instance()
    for _ in range(4):
        ground_low = separate(atlas_w, tree_w, low)
    gx, gz = np.meshgrid(np.arange(-100.0, 101.0, 5.0), np.arange(-100.0, 101.0, 5.0))
    pts = np.column_stack([low[0] + gx.ravel(), np.full(gx.size, low[1]), low[2] + gz.ravel()])
    heights = tree_w.sample_attachment(0, pts)[1]
    pick = int(np.argmin(np.abs(heights - (ground_low + 8.0))))
    assert abs(float(heights[pick]) - (ground_low + 8.0)) < 1.0
    ground_high, base = float(heights[pick]), model.translation[1]  # (heights are over the model's plane)
    for _ in range(3):  # the teleport itself and back: the first visit requests the tiles around the new place, the later ones find them loaded
        high = (float(pts[pick, 0]), base + ground_high + 0.25, float(pts[pick, 2]))
        ground_high = separate(atlas_w, tree_w, high)
        print(f"warm-up: camera {high[1]:.3f} over ground {ground_high:.3f} (low ground {ground_low:.3f})")
        separate(atlas_w, tree_w, low)
    high = (float(pts[pick, 0]), base + ground_high + 0.25, float(pts[pick, 2]))

    atlas_a, tree_a = instance()
    atlas_b, tree_b = instance()
    prepass_b = bt.TilingPrepass(device, vc.geometry_tile_count)
    for pos in (low, low, low, high, low, high):  # the same visits as the warm-up instance: every later teleport samples what it sampled
        separate(atlas_a, tree_a, pos)
        atlas_b.update(root)
        tree_b.frame_update(pos)
    for form in FORMS:
        stale_height = separate(atlas_a, tree_a, low)  # frame 1: what the host of B knows in frame 2
        atlas_b.update(root)
        tree_b.frame_update(low)
        fresh_height = separate(atlas_a, tree_a, high)  # frame 2
        fresh = tree_a.view_state()
        assert fresh.approximate_height == fresh_height
        exp, exp_indirect, _ = O.refine(oracle_view(fresh))
        stale_lods = P.estimate_lods(bt.view_state_from_config(model, vc, high, stale_height))
        print(f"{form}: ground {stale_height:.3f} -> {fresh_height:.3f}, camera {high[1]:.3f}, restated stale lods {stale_lods}, "
              f"deepest LOD {int(exp[:, 1].max())}, {len(exp)} tiles")
        assert stale_lods >= 13 and int(exp[:, 1].max()) >= stale_lods  # the assisted kernel, and tiles deeper than its bits
        atlas_b.update(root)
        info = tree_b.frame_update(high, prepass_b, **FORMS[form])
        assert info.approximate_height == stale_height  # what B's host had when it estimated
        ours, indirect = prepass_b.read()
        assert_list(ours, exp, form, form)
        assert list(indirect) == exp_indirect, form
        tree_b.read()  # (a synchronising call of the tree: the host's copy catches up)
        assert tree_b.view_state().approximate_height == fresh_height  # what B's kernels read on the device was A's fresh height

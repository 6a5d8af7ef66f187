"""The smoothing brush on the device (bt_atlas_smooth_height) against the numpy model of its definition (tests/_smooth_model.py, pinned by
test_smooth_model.py), propagated by the model of F (tests/_edit_model.py).

Every comparison is the one of tests/test_gpu_edit.py (its helpers are imported, not copied): ALL layers downloaded after every call, every
existing tile byte-equal to propagate(apply_smooth(before)), every layer outside `changed` byte-equal to before, `changed` inside the
allowed set, the stats identities (stats["launches"] == 2 + downsample levels + stitch + mips); mips, where the attachment has them,
against the oracle's generate_mipmaps.  Every case asserts from its own inputs that it reaches the branch it is named for (the plan's
rectangles restated by test_gpu_edit_shapes.plan_levels, no device).

What each shape is for, in terms of bt_edit.hip's edit_smooth_kernel: a workgroup stages 16 rows + k above and below by 64 dword pairs + a
halo left and right in LDS; a wider rectangle is walked in column chunks, a taller one in row blocks; the new texels go to scratch and a
second launch copies them in, so no lane reads what the call wrote."""
import numpy as np
import pytest

import _cases as K
import _cull_model as M
import _edit_model as EM
import _oracle as O
import _smooth_model as SM
import bevy_terrain_amd as bt
from bevy_terrain_amd import SmoothStamp as S
from test_gpu_edit import ATLAS, R16, RGBA8, Snapshot, ancestors_levels, check_edit, geometry, planar, source_r16
from test_gpu_edit_shapes import CASES, LANES, ROW_BLOCK, branches_reached, device_atlas, plan_levels, stamp_boxes

BT_ERR_UNSUPPORTED = -5


@pytest.fixture(scope="module")
def device():
    return bt.Device(0)


def mip_runs(layers):
    layers = sorted(layers)
    return sum(1 for i, l in enumerate(layers) if i == 0 or layers[i - 1] != l - 1)


def smooth_and_check(atlas, stamps, k, lod=None, held=True, mips_before=None):
    """one bt_atlas_smooth_height call compared as the module docstring says; returns (before, after, changed, stats)"""
    b, c, spherical = geometry(atlas)
    lod = atlas.lod_count - 1 if lod is None else lod
    before = Snapshot(atlas)
    if held:  # the definition's precondition (after a checked call the state equals a propagate() result, so it need not be repeated)
        F = EM.propagate(before.tiles, b, spherical)
        assert all(np.array_equal(F[key], before.tiles[key]) for key in before.tiles), "the state before the call is not F of its primary centres"
    changed, stats = atlas.smooth_height(0, stamps, k, lod)
    coarse = {key: v for key, v in before.tiles.items() if key[1] <= lod}  # tiles finer than `lod` are not touched
    expected = dict(before.tiles)
    expected.update(EM.propagate(SM.apply_smooth(coarse, lod, stamps, b, k), b, spherical))
    edited = SM.stamp_tiles(stamps, lod, c)
    levels = ancestors_levels(before, edited)
    after = check_edit(atlas, before, expected, changed, stats, edited, levels)
    mip_count = atlas.config.attachments[0].mip_level_count
    layers = {before.index[(t.side, t.lod, t.x, t.y)] for t in changed}
    if stats["tiles_edited"]:
        assert stats["launches"] == 2 + levels + (1 if b else 0) + (mip_count - 1) * (mip_runs(layers) if mip_count > 1 else 0)
        assert stats["layers_mipped"] == (len(layers) if mip_count > 1 else 0)
    if mips_before is not None:
        T = atlas.config.attachments[0].texture_size
        for i in range(atlas.atlas_size):
            got = [atlas.download_mip(0, level, i) for level in range(1, mip_count)]
            if i in layers:
                chain = O.generate_mipmaps(R16, after.data[i], mip_count)
                want, base = [], T * T
                for level in range(1, mip_count):
                    n = T >> level
                    want.append(chain[base:base + n * n].reshape(n, n))
                    base += n * n
                assert all(np.array_equal(g, w) for g, w in zip(got, want)), f"mips of changed layer {i}"
                mips_before[i] = got
            else:
                assert all(np.array_equal(g, w) for g, w in zip(got, mips_before[i])), f"mips of untouched layer {i}"
    return before, after, changed, stats


def differing(before, after):
    return [key for key in before.tiles if not np.array_equal(before.tiles[key], after.tiles[key])]


def reaches(atlas, stamps, lod=None):
    """the branch names (test_gpu_edit_shapes.branches_reached) and plan levels of a call on this atlas, from index arithmetic alone"""
    b, c, spherical = geometry(atlas)
    lod = atlas.lod_count - 1 if lod is None else lod
    existing = {(t.side, t.lod, t.x, t.y) for t, _ in atlas.tiles()}
    boxes = stamp_boxes(stamps, lod, c)
    levels = plan_levels(boxes, lod, c, existing)
    return branches_reached(boxes, levels, lod, c, b, R16, existing, spherical, stamps), levels


def random_planar(device, T, b, seed, holes=0.0, lods=3):
    n = (T - 2 * b) << (lods - 1)
    return planar(device, T, b, lods, src=K.random_raster(R16, n, n, seed=seed, holes=holes))


# ---------------------------------------------------------------------------------------------- 1. a four-tile corner, then a second call

@pytest.mark.gpu
@pytest.mark.parametrize("falloff", ["smooth", "hard"])
@pytest.mark.parametrize("k", [1, 2])
def test_four_tile_corner_then_a_second_call(device, k, falloff):
    """T = 16, b = 2 (c = 12), lod_count 3: a stamp where four finest tiles meet (the boxes of the texels at the tile edges read the aprons:
    the neighbours' centres), then a second call onto the smoothed state, which matches only if the first call restored the aprons"""
    atlas = planar(device, 16, 2)
    first, second = [S((12.3, 11.6), 3.5, 0.875, falloff)], [S((11.0, 12.5), 4.0, 1.0, falloff), S((13.5, 10.0), 2.5, 0.5, "hard")]
    assert SM.stamp_tiles(first, 2, 12) == SM.stamp_tiles(second, 2, 12) == {(0, 2, 0, 0), (0, 2, 1, 0), (0, 2, 0, 1), (0, 2, 1, 1)}
    before, after, changed, stats = smooth_and_check(atlas, first, k)
    assert stats["tiles_edited"] == 4 and stats["tiles_downsampled"] == 2 and stats["launches"] == 5
    assert {(0, 2, 0, 0), (0, 2, 1, 0), (0, 2, 0, 1), (0, 2, 1, 1)} <= set(differing(before, after))
    # the aprons the second call reads have changed: without their restoration it would see the old neighbours
    tile = (0, 2, 0, 0)
    assert not np.array_equal(before.tiles[tile][2:14, 14:16], after.tiles[tile][2:14, 14:16]), "the first call changed no apron texel of a box of the second"
    before2, after2, _, _ = smooth_and_check(atlas, second, k, held=False)
    assert len(differing(before2, after2)) >= 4


# ---------------------------------------------------------------------------------------------- 2. the snapshot

@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 2])
def test_every_mean_comes_from_the_state_before_the_call(device, k):
    """T = 72, b = 2 (c = 68: five row blocks), random data, one HARD stamp of strength 1 over a whole tile: every texel lands on its box
    mean, so a read of any row or column the call has written, inside a row block or across two, changes bytes (asserted on the model:
    an in-place pass differs on most texels)"""
    T, b = 72, 2
    c = T - 2 * b
    atlas = random_planar(device, T, b, seed=31, holes=0.01)
    stamps = [S((1.5 * c, 1.5 * c), float(c), 1.0, "hard")]
    names, levels = reaches(atlas, stamps)
    assert levels[0][(0, 2, 1, 1)] == (0, 0, c - 1, c - 1) and "edit_second_row_block" in names and -(-c // ROW_BLOCK) == 5
    gy, gx = np.mgrid[c:2 * c, c:2 * c]
    assert ((gx - 1.5 * c) ** 2 + (gy - 1.5 * c) ** 2 < c * c).all(), "the stamp does not cover the tile"
    before, after, changed, stats = smooth_and_check(atlas, stamps, k)
    tile = {(0, 2, 1, 1): before.tiles[(0, 2, 1, 1)]}
    model, in_place = SM.apply_smooth(tile, 2, stamps, b, k)[(0, 2, 1, 1)], SM.apply_smooth_in_place(tile, 2, stamps, b, k)[(0, 2, 1, 1)]
    assert (model != in_place).sum() > c * c // 2 and np.array_equal(after.tiles[(0, 2, 1, 1)][b:-b, b:-b], model[b:-b, b:-b])
    assert stats["tiles_edited"] == 9


# ---------------------------------------------------------------------------------------------- 3. the second lane trip, column chunks

@pytest.mark.gpu
@pytest.mark.parametrize("b", [2, 3])
def test_rows_beyond_one_lane_trip_are_staged_in_column_chunks(device, b):
    """T = 136 with b = 2 (k = 2, c = 132) and b = 3 (k = 3, c = 130): a centre row is dwords 1 .. 66, more than one trip of the 64 lanes, so
    the window is staged twice per row block, the second chunk with a halo of its own.  First a rectangle inside one tile that starts on
    an odd and ends on an even texel 64 dwords apart (half dwords at both ends, the right one on the later chunk), then a face-wide
    stamp (full rows of every tile; with b = 3 every one starts and ends in half a dword)."""
    T, k = 136, b
    c = T - 2 * b
    n = 4 * c
    atlas = random_planar(device, T, b, seed=32 + b, holes=0.02)
    x0 = 1 if b % 2 == 0 else 2               # b + x0 odd
    x1 = c - 2 if (b + c) % 2 == 0 else c - 1  # b + x1 even, (b + x1) >> 1 == 66
    inside = [S(((c + x0 + c + x1) / 2.0, 1.5 * c), (x1 - x0) / 2.0 - 0.5, 1.0, "hard")]  # its box is exactly [c + x0, c + x1] in x
    names, levels = reaches(atlas, inside)
    r = levels[0][(0, 2, 1, 1)]
    assert (r[0], r[2]) == (x0, x1) and ((b + x1) >> 1) - ((b + x0) >> 1) >= LANES and (b + x0) % 2 == 1 and (b + x1) % 2 == 0
    assert {"edit_second_trip", "edit_second_row_block", "edit_first_dword_half", "edit_last_dword_half_on_second_trip"} <= names
    before, after, changed, stats = smooth_and_check(atlas, inside, k)
    # texels of the later chunk changed, and so did texels whose box reaches across the chunk boundary (pairs 64 / 65 of the row)
    d = before.tiles[(0, 2, 1, 1)] != after.tiles[(0, 2, 1, 1)]
    assert d[b:-b, 130:b + x1 + 1].any() and d[b:-b, 126:132].any() and not d[b:-b, b + x1 + 1:].any() and not d[b:-b, :b + x0].any()
    wide = [S((n / 2.0, n / 2.0), 4.0 * n, 0.75)]
    names, levels = reaches(atlas, wide)
    assert {"edit_second_trip", "edit_second_row_block"} <= names and len(levels[0]) == 16
    assert (b % 2 == 0) or {"edit_first_dword_half", "edit_last_dword_half_on_second_trip"} <= names
    smooth_and_check(atlas, wide, k, held=False)


# ---------------------------------------------------------------------------------------------- 4. holes

@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 2])
def test_holes_stay_and_do_not_count(device, k):
    """a hole mask written into the finest LOD (write_region leaves F intact): a block of holes with ONE data texel in its middle whose
    whole box is holes (n = 1: a fixed point), scattered holes, and a stamp lying entirely over the block.  Zeros stay zero, nothing
    becomes zero, and the means leave the holes out (the comparison with the model)"""
    atlas = planar(device, 16, 2)
    rng = np.random.default_rng(7)
    patch = rng.integers(1, 65536, size=(24, 24), dtype=np.uint16)
    patch[rng.random(patch.shape) < 0.15] = 0
    patch[2:13, 2:13] = 0   # mosaic texels 14 .. 24 in x and y: across the corner of four tiles
    patch[7, 7] = 51234     # mosaic (19, 19): its 5 x 5 box is all holes
    atlas.write_region(0, patch, 12, 12)
    stamps = [S((24.0, 24.0), 13.0, 1.0, "hard"), S((17.0, 17.0), 2.0, 0.5), S((30.0, 30.0), 5.0, 0.75)]
    gy, gx = np.mgrid[0:48, 0:48]
    under = (gx - 17.0) ** 2 + (gy - 17.0) ** 2 < 4.0
    assert under.any() and (patch[gy[under] - 12, gx[under] - 12] == 0).all(), "the second stamp does not lie entirely over holes"
    before, after, changed, stats = smooth_and_check(atlas, stamps, k)
    lone = before.tiles[(0, 2, 1, 1)]
    assert lone[2 + 7, 2 + 7] == 51234 and (lone[2 + 7 - k:2 + 7 + k + 1, 2 + 7 - k:2 + 7 + k + 1] != 0).sum() == 1
    assert after.tiles[(0, 2, 1, 1)][2 + 7, 2 + 7] == 51234
    finest = [key for key in before.tiles if key[1] == 2]
    assert all(np.array_equal(before.tiles[key] == 0, after.tiles[key] == 0) for key in finest), "the hole mask changed"
    assert sum(int((before.tiles[key][2:14, 2:14] == 0).sum()) for key in finest) > 150 and len(differing(before, after)) >= 9


# ---------------------------------------------------------------------------------------------- 5. the cube

@pytest.mark.gpu
def test_cube_face_edges_corner_tile_and_mips(device):
    """T = 16, b = 2, lod_count 3, mip_level_count 3, k = 2, 126 tiles, all compared after every call with their mips: a stamp at a face
    edge on an even side and on an odd side (the boxes read the re-projected neighbour face from the apron), at a cube-corner tile (the
    diagonal apron is clamped), and at LOD 1 (finer tiles keep their bytes)"""
    spec, _ = CASES["d_cube"]
    atlas = device_atlas(device, spec, mips=3)
    atlas.generate_mipmaps(0)
    assert len(atlas.tiles()) == 126
    mips = {i: [atlas.download_mip(0, level, i) for level in (1, 2)] for i in range(atlas.atlas_size)}
    calls = [
        ([S((0.5, 23.0), 3.5, 1.0, side=0)], None, "edge_tile_that_is_no_corner_tile"),
        ([S((47.0, 20.0), 3.0, 0.75, "hard", side=3)], None, "edge_tile_that_is_no_corner_tile"),
        ([S((1.0, 46.0), 3.0, 1.0, "hard", side=2), S((46.5, 1.0), 2.5, 0.5, side=5)], None, "corner_tile"),
        ([S((11.5, 12.5), 4.0, 1.0, side=2), S((23.0, 0.5), 3.0, 0.875, "hard", side=1)], 1, "corner_tile"),
    ]
    for n, (stamps, lod, name) in enumerate(calls):
        names, levels = reaches(atlas, stamps, lod)
        assert name in names, (n, sorted(names))
        before, after, changed, stats = smooth_and_check(atlas, stamps, 2, lod, held=(n == 0), mips_before=mips)
        sides = {s.side for s in stamps}
        assert {t.side for t in changed} - sides, "no tile of a neighbouring face was re-stitched"
        assert {key[0] for key in differing(before, after)} - sides, "no tile of a neighbouring face changed"
        if lod == 1:
            assert all(t.lod <= 1 for t in changed) and stats["tiles_with_children"] == stats["tiles_edited"] > 0
            assert all(np.array_equal(before.tiles[key], after.tiles[key]) for key in before.tiles if key[1] == 2)
    assert len({t.side for t in changed}) >= 3


# ---------------------------------------------------------------------------------------------- 6. missing tiles

@pytest.mark.gpu
def test_missing_neighbour_is_the_clamped_apron(device):
    """a tile whose west and north neighbours are absent and whose data reach its edges: the boxes there read its own centre clamped (F
    item 3)"""
    atlas = planar(device, 16, 2, top_left=(0.25, 0.25), bottom_right=(0.75, 0.75))
    index = {(t.side, t.lod, t.x, t.y) for t, _ in atlas.tiles()}
    assert (0, 2, 1, 1) in index and not {(0, 2, 0, 0), (0, 2, 0, 1), (0, 2, 1, 0)} & index
    held = Snapshot(atlas).tiles[(0, 2, 1, 1)]
    assert held[2:14, 2].all() and held[2, 2:14].all() and np.array_equal(held[2:14, 0], held[2:14, 2]) and np.array_equal(held[0, 2:14], held[2, 2:14])
    before, after, changed, stats = smooth_and_check(atlas, [S((11.0, 13.0), 4.0, 1.0, "hard")], 2)
    assert stats["tiles_missing"] == 3 and stats["tiles_edited"] == 1
    d = before.tiles[(0, 2, 1, 1)] != after.tiles[(0, 2, 1, 1)]
    assert d[2:14, 2].any() and d[2, 2:14].any(), "no texel at the clamped edges changed"
    before, after, changed, stats = smooth_and_check(atlas, [S((3.0, 3.0), 2.0, 1.0)], 1, held=False)  # only absent tiles
    assert stats["tiles_missing"] == 1 and stats["tiles_edited"] == 0 and stats["launches"] == 0 and changed == []


@pytest.mark.gpu
@pytest.mark.parametrize("name,reach", [("c_no_lod0", "chain_ends_at_a_missing_parent"), ("c_box_over_more_tiles", "box_over_more_tiles_than_the_atlas_holds")])
def test_missing_parent_and_a_box_over_more_tiles_than_the_atlas_holds(device, name, reach):
    """the atlases of test_gpu_edit_shapes.py: one without LOD 0 (the chain of ancestors ends at LOD 1), one that holds 16 of the 64 finest
    tiles under a stamp over the whole face"""
    spec, _ = CASES[name]
    atlas = device_atlas(device, spec)
    stamps = [S((23.5, 23.5), 5.0, 1.0, "hard")] if name == "c_no_lod0" else [S((48.0, 48.0), 200.0, 0.75), S((5.0, 5.0), 2.0, 1.0)]
    names, levels = reaches(atlas, stamps)
    assert reach in names
    before, after, changed, stats = smooth_and_check(atlas, stamps, 2)
    assert len(differing(before, after)) >= 4
    if name == "c_no_lod0":
        assert all(t.lod > 0 for t in changed) and stats["tiles_downsampled"] == 4
    else:
        assert stats["tiles_edited"] == 16 and stats["tiles_missing"] == 48


# ---------------------------------------------------------------------------------------------- 7. overlap

def overlapping_256():
    rng = np.random.default_rng(13)
    stamps = []
    for n in range(256):
        cx, cy = (rng.integers(10 * 4, 38 * 4, size=2) / 4.0).tolist()
        stamps.append(S((cx, cy), float(rng.integers(8, 33)) / 4.0, float(rng.integers(1, 9)) / 8.0, "hard" if n % 3 == 0 else "smooth"))
    return stamps


@pytest.mark.gpu
def test_256_overlapping_stamps_in_one_call(device):
    """the documented limit: every stamp moves the running value towards the SAME mean (of the state before the call)"""
    atlas = planar(device, 16, 2)
    stamps = overlapping_256()
    gy, gx = np.mgrid[0:48, 0:48]
    cover = sum(((gx - s.center[0]) ** 2 + (gy - s.center[1]) ** 2 < s.radius ** 2).astype(int) for s in stamps)
    assert len(stamps) == 256 and cover.max() >= 32, "the stamps do not overlap"
    before, after, changed, stats = smooth_and_check(atlas, stamps, 2)
    assert stats["tiles_edited"] == 16


@pytest.mark.gpu
def test_two_calls_of_one_stamp_are_not_one_call_of_two(device):
    """unlike ADD / FLATTEN: the second call's means come from the first call's result.  The model shows the difference; the device
    matches the model both ways"""
    s1, s2 = S((20.0, 21.0), 6.0, 1.0, "hard"), S((24.0, 22.0), 6.0, 0.75, "hard")
    one = random_planar(device, 16, 2, seed=41)
    start = Snapshot(one)
    _, after_one, _, _ = smooth_and_check(one, [s1, s2], 2)
    two = random_planar(device, 16, 2, seed=41)
    assert np.array_equal(Snapshot(two).data, start.data)
    smooth_and_check(two, [s1], 2)
    _, after_two, _, _ = smooth_and_check(two, [s2], 2, held=False)
    model_one = SM.apply_smooth(start.tiles, 2, [s1, s2], 2, 2)
    model_two = SM.apply_smooth(EM.propagate(SM.apply_smooth(start.tiles, 2, [s1], 2, 2), 2, False), 2, [s2], 2, 2)
    finest = [key for key in start.tiles if key[1] == 2]
    assert sum(int((model_one[key] != model_two[key]).sum()) for key in finest) > 20, "the model: both orders of calling agree"
    assert sum(int((after_one.tiles[key] != after_two.tiles[key]).sum()) for key in finest) > 20


# ---------------------------------------------------------------------------------------------- 8. refusals

@pytest.mark.gpu
def test_refusals_leave_the_atlas_alone(device):
    def status(call):
        with pytest.raises(bt.BtError) as e:
            call()
        return e.value.status

    atlas = planar(device, 16, 2)
    before = Snapshot(atlas)
    stamp = [S((12.0, 12.0), 4.0, 1.0)]
    assert status(lambda: atlas.smooth_height(0, stamp, 3)) == BT_ERR_UNSUPPORTED  # k = 3 with b = 2
    assert np.array_equal(Snapshot(atlas).data, before.data)
    changed, stats = atlas.smooth_height(0, [], 2)
    assert changed == [] and not any(stats.values()) and np.array_equal(Snapshot(atlas).data, before.data)
    rgba = planar(device, 16, 2, fmt=RGBA8)
    rgba_before = Snapshot(rgba)
    assert status(lambda: rgba.smooth_height(0, stamp, 1)) == BT_ERR_UNSUPPORTED
    assert np.array_equal(Snapshot(rgba).data, rgba_before.data)
    cfg = bt.TerrainConfig(lod_count=3, atlas_size=4, path="terrains/edit", model=bt.TerrainModel.planar((0, 0, 0), 1000.0, 0.0, 1.0))
    cfg.add_attachment(bt.AttachmentConfig(name="att", texture_size=17, border_size=2, format=bt.AttachmentFormat.R16))  # c = 13
    odd = bt.TileAtlas.new(cfg, device)
    assert status(lambda: odd.smooth_height(0, stamp, 1)) == BT_ERR_UNSUPPORTED
    assert not odd.download_tiles(0, 0, 4).any()


# ---------------------------------------------------------------------------------------------- 9. the culling table

@pytest.mark.gpu
def test_height_bounds_update_follows_a_smooth(device):
    atlas = random_planar(device, 16, 2, seed=43, holes=0.02)
    hb = bt.HeightBounds(device, 1, 3).build(atlas, 0)
    table_before = hb.read().copy()
    before, after, changed, stats = smooth_and_check(atlas, [S((24.0, 24.0), 9.0, 1.0, "hard")], 2)
    hb.update(atlas, changed)
    table = hb.read()
    assert not np.array_equal(table, table_before), "the smooth moved no bound: the comparison would be empty"
    assert np.array_equal(table, M.build_table(1, 3, after.tiles).data)
    assert np.array_equal(table, bt.HeightBounds(device, 1, 3).build(atlas, 0).read())


# ---------------------------------------------------------------------------------------------- 10. the workload's tile size

@pytest.mark.gpu
def test_workload_tile_size_once(device):
    """T = 512, b = 2, lod_count 3, k = 2, one stamp of radius 300 across a tile corner (rectangles of up to 302 texels: three column
    chunks, 19 row blocks): the centres of the edited tiles and of their ancestors against the model, every other layer against before
    (the model's per-pixel stitch at this size is not worth its seconds; the aprons are covered at the small sizes)"""
    T, b, lods, k = 512, 2, 3, 2
    c = T - 2 * b
    atlas = planar(device, T, b, lods, src=K.smooth_raster(1024, 1024, 9, device=device))
    before = Snapshot(atlas)
    stamps = [S((c + 0.25, 2 * c - 0.5), 300.0, 1.0)]
    edited = SM.stamp_tiles(stamps, 2, c)
    assert edited == {(0, 2, 0, 1), (0, 2, 1, 1), (0, 2, 0, 2), (0, 2, 1, 2)}
    changed, stats = atlas.smooth_height(0, stamps, k)
    after = Snapshot(atlas)
    changed = [(t.side, t.lod, t.x, t.y) for t in changed]
    assert stats["tiles_edited"] == 4 and stats["launches"] == 5 and stats["tiles_downsampled"] == 3
    written = edited | {(0, 1, 0, 0), (0, 1, 0, 1), (0, 0, 0, 0)}
    assert written <= set(changed) <= SM.allowed_changed(before.tiles, edited, False)
    smoothed = SM.apply_smooth({key: before.tiles[key] for key in edited}, 2, stamps, b, k)
    primary = dict(before.tiles)
    primary.update(smoothed)
    expected = EM.propagate(primary, b, False, only=[])  # derived centres only: nothing is stitched
    for key in before.index:
        if key in written:
            assert np.array_equal(after.tiles[key][b:-b, b:-b], expected[key][b:-b, b:-b]), key
        elif key not in changed:
            assert np.array_equal(after.tiles[key], before.tiles[key]), key
    assert all(not np.array_equal(after.tiles[key][b:-b, b:-b], before.tiles[key][b:-b, b:-b]) for key in edited)

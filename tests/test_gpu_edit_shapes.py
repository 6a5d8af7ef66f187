"""The shapes of in-place editing that tests/test_gpu_edit.py leaves out: rows longer than one trip of the 64 lanes (with the half dwords
at odd edges on the later trip), rectangles taller than one row block (Rgba8 included), the rarer branches of the host's plan (a box over
more tiles than the atlas holds, ancestor chains that end, a parent rectangle over a quadrant nobody edited), the cube at lod_count 3,
256 stamps in one call, and the wrap of the plan ring.

Every comparison is the one of tests/test_gpu_edit.py (its helpers are imported, not copied): all layers downloaded, every existing tile
byte-equal to the numpy model, every layer outside `changed` byte-equal to before, `changed` inside the allowed set, the stats identities.

Every case proves from its own inputs that it reaches the branch it is named for.  plan_levels() restates the host's rule for the dirty
rectangles (numpy and the model only, no device); branches_reached() names the branches those rectangles reach.  The GPU cases assert the
names listed in CASES, and test_cases_reach_their_branches asserts them again without a GPU, on states the CPU oracle makes from the same
jobs, together with the check that keeps plan_levels() honest: every centre texel the model changes lies inside a rectangle."""
import ctypes
import functools
import math

import numpy as np
import pytest

import _cases as K
import _cull_model as M
import _edit_model as EM
import _oracle as O
import bevy_terrain_amd as bt
from bevy_terrain_amd import EditStamp as S
from bevy_terrain_amd import _ffi
from test_gpu_edit import ATLAS, R16, RGBA8, Snapshot, ancestors_levels, check_edit, cube, cube_faces, edit_and_check, geometry, planar, source_r16

F32 = np.float32
LANES = 64      # bt_edit.hip, for_each_dword: p += 64u
ROW_BLOCK = 16  # bt_edit.hip: kEditRows
RING_BYTES = 1 << 20  # bt_edit.cpp, PlanRing::commit(): `std::max<uint64_t>(1ull << 20, 2u * need)`, the plan ring's initial size
MAX_STAMPS = 256      # BT_EDIT_MAX_STAMPS


@pytest.fixture(scope="module")
def device():
    return bt.Device(0)


# ---------------------------------------------------------------------------------------------- the plan, restated

def stamp_boxes(stamps, lod, c):
    """[(side, x0, y0, x1, y1)], inclusive mosaic texels: [floor(center - radius), ceil(center + radius)] of the binary32 values the
    library receives, computed in binary64 and clipped to the face; a box that misses the face is dropped"""
    n = (1 << lod) * c
    boxes = []
    for s in stamps:
        ctr, r = [float(F32(v)) for v in s.center], float(F32(s.radius))
        lo = [max(0, math.floor(ctr[k] - r)) for k in range(2)]
        hi = [min(n - 1, math.ceil(ctr[k] + r)) for k in range(2)]
        if lo[0] <= hi[0] and lo[1] <= hi[1]:
            boxes.append((s.side, lo[0], lo[1], hi[0], hi[1]))
    return boxes


def _unite(rects, key, r):
    u = rects.get(key)
    rects[key] = r if u is None else (min(u[0], r[0]), min(u[1], r[1]), max(u[2], r[2]), max(u[3], r[3]))


def plan_levels(boxes, lod, c, existing):
    """[{tile: (x0, y0, x1, y1) in centre texels, inclusive}]: [0] the existing tiles of `lod` the boxes meet, [k] their existing ancestors
    of lod - k.  The host's rule: a parent's rectangle is [x0 >> 1, x1 >> 1] plus the quadrant offset, united per parent; a tile whose
    parent does not exist passes nothing up, and the levels end where none is left."""
    cur = {}
    for side, x0, y0, x1, y1 in boxes:
        for ty in range(y0 // c, y1 // c + 1):
            for tx in range(x0 // c, x1 // c + 1):
                if (side, lod, tx, ty) in existing:
                    ox, oy = tx * c, ty * c
                    _unite(cur, (side, lod, tx, ty), (max(x0, ox) - ox, max(y0, oy) - oy, min(x1, ox + c - 1) - ox, min(y1, oy + c - 1) - oy))
    levels = [cur]
    while cur:
        up = {}
        for (side, l, x, y), r in cur.items():
            parent = (side, l - 1, x >> 1, y >> 1)
            if l == 0 or parent not in existing:
                continue
            ox, oy = (x & 1) * (c // 2), (y & 1) * (c // 2)
            _unite(up, parent, (ox + (r[0] >> 1), oy + (r[1] >> 1), ox + (r[2] >> 1), oy + (r[3] >> 1)))
        if up:
            levels.append(up)
        cur = up
    return levels


def branches_reached(boxes, levels, lod, c, b, fmt, existing, spherical, stamps=()):
    """the names of the kernel lines and plan branches these inputs reach.  A row of an item is the dwords (b + x0) >> 1 .. (b + x1) >> 1
    (R16: two texels each; Rgba8: one texel each, b + x0 .. b + x1), lane k of the wave takes dword first + k + 64 * trip."""
    out = set()
    for k, level in enumerate(levels[:2]):  # the brush / region launch and the first downsample launch
        tag = "edit" if k == 0 else "parent"
        for r in level.values():
            px0, px1 = b + r[0], b + r[2]
            first, last = (px0 >> 1, px1 >> 1) if fmt == R16 else (px0, px1)
            if last - first >= LANES:
                out.add(tag + "_second_trip")
            if r[3] - r[1] + 1 > ROW_BLOCK:
                out.add(tag + "_second_row_block")
            if fmt == R16:
                if px0 % 2 == 1:  # texel 2 * first lies left of the rectangle: in1 and not in0
                    out.add(tag + "_first_dword_half")
                if px1 % 2 == 0 and last - first >= LANES:  # texel 2 * last + 1 lies right of it: in0 and not in1, on a later trip
                    out.add(tag + "_last_dword_half_on_second_trip")
    if any((x1 // c - x0 // c + 1) * (y1 // c - y0 // c + 1) > len(existing) for _, x0, y0, x1, y1 in boxes):
        out.add("box_over_more_tiles_than_the_atlas_holds")
    for k, level in enumerate(levels):
        order = sorted(level)  # the host walks a std::map ordered by (side, lod, x, y)
        orphan = [l > 0 and (side, l - 1, x >> 1, y >> 1) not in existing for side, l, x, y in order]
        if any(orphan):
            out.add("chain_ends_at_a_missing_parent")
            if False in orphan[orphan.index(True):]:
                out.add("chain_goes_on_behind_an_ended_one")
        if k == 0:
            continue
        for (side, l, x, y), r in level.items():  # quadrants of a parent's rectangle that no dirty child stands behind
            for i in range(4):
                child = (side, l + 1, 2 * x + (i & 1), 2 * y + (i >> 1))
                qx, qy = (i & 1) * (c // 2), (i >> 1) * (c // 2)
                meets = r[0] < qx + c // 2 and r[2] >= qx and r[1] < qy + c // 2 and r[3] >= qy
                if meets and child not in levels[k - 1]:
                    out.add("rectangle_over_an_untouched_quadrant" if child in existing else "rectangle_over_an_absent_quadrant")
    if spherical:
        m = 1 << lod
        for _, _, x, y in levels[0]:
            on_edge = (x in (0, m - 1)) + (y in (0, m - 1))
            out.add(("interior_tile_beside_a_seam_tile", "edge_tile_that_is_no_corner_tile", "corner_tile")[on_edge])
    if len(stamps) == MAX_STAMPS:
        out.add("256_stamps")
    with np.errstate(over="ignore", under="ignore"):
        r2 = [F32(s.radius) * F32(s.radius) for s in stamps]
    if any(np.isinf(v) for v in r2):
        out.add("radius_squared_overflows")
    if any(v == 0 for v in r2):
        out.add("radius_squared_underflows")
    return out


# ---------------------------------------------------------------------------------------------- the cases

def stamp_over(lo, hi, cy, amount, **kw):
    """a stamp whose box is exactly [lo, hi] in x (centre and radius are multiples of 1/4: exact in binary32)"""
    return S(((lo + hi) / 2.0, float(cy)), (hi - lo) / 2.0 - 0.5, amount, **kw)


def region_texels(fmt, h, w, seed):
    rng = np.random.default_rng(seed)
    texels = rng.integers(1, 65536, size=(h, w), dtype=np.uint16) if fmt == R16 else rng.integers(1, 256, size=(h, w, 4), dtype=np.uint8)
    texels[h // 3:h // 3 + 3, w // 4:w // 2] = 0
    texels[h - 1, 0] = 0
    return texels


def Edit(stamps=None, region=None, lod=None, reach=()):
    """stamps: one bt_atlas_edit_height call; region: (x0, y0, w, h, seed) of one bt_atlas_write_region call; reach: branch names"""
    return dict(stamps=stamps, region=region, lod=lod, reach=set(reach))


@functools.lru_cache(maxsize=None)
def big_r16(n):
    return source_r16(n)


def case_a(b):
    """T = 136: a full row of the centre is dwords 1 .. 66.  With b = 3 every full row starts and ends in half a dword; with b = 2 the
    stamps that start on an odd and end on an even texel of the tile do."""
    T = 136
    c = T - 2 * b
    n = 4 * c
    x0 = 1 if b % 2 == 0 else 2               # b + x0 odd
    x1 = c - 2 if (b + c) % 2 == 0 else c - 1  # b + x1 even, (b + x1) >> 1 == 66
    half = {"_first_dword_half", "_last_dword_half_on_second_trip"}
    full = {"edit_second_trip", "edit_second_row_block", "parent_second_trip", "parent_second_row_block"}
    edits = [
        Edit([S((n / 2.0, n / 2.0), 4.0 * n, 0.05)], reach=full | ({t + h for t in ("edit", "parent") for h in half} if b % 2 else set())),
        # inside tile 1 of the row: texels x0 .. x1
        Edit([stamp_over(c + x0, c + x1, 1.5 * c, -0.1)], reach={"edit_second_trip", "edit_second_row_block"} | {"edit" + h for h in half}),
        # over tiles 0 and 1 so that their parent's rectangle is x0 .. x1
        Edit([stamp_over(2 * x0, 2 * x1, c, 0.1)], reach={"edit_second_trip", "parent_second_trip", "parent_second_row_block"} | {"parent" + h for h in half}),
        Edit([S((2 * c + 0.25, c - 0.5), 9.0, -0.2, falloff="hard")]),
        Edit(region=(c - 1, c - 9, 131, 40, 3), reach={"edit_second_trip", "edit_second_row_block"} | ({"edit" + h for h in half} if b % 2 else set())),
    ]
    return dict(kind="planar", T=T, b=b, lods=3, fmt=R16, src=lambda: big_r16(n)), edits


def case_b(b):
    T = 72
    c = T - 2 * b
    n = 4 * c
    edits = [
        Edit(region=(0, 0, n, n, 4), reach={"edit_second_trip", "edit_second_row_block", "parent_second_trip", "parent_second_row_block"}),
        # odd origin and size; 66 texels and 36 rows of it inside tile (1, 1)
        Edit(region=(c - 3, c - 5, 69, 41, 5), reach={"edit_second_trip", "edit_second_row_block", "parent_second_row_block"}),
    ]
    return dict(kind="planar", T=T, b=b, lods=3, fmt=RGBA8, src=lambda: K.random_raster(RGBA8, n, n, seed=8, holes=0.03)), edits


def small(**kw):
    return dict(dict(kind="planar", T=16, b=2, lods=3, fmt=R16, src=source_r16), **kw)


def rect(x0, y0, x1, y1):
    return dict(top_left=(x0, y0), bottom_right=(x1, y1))


def stamps_256():
    """mixed modes and falloffs, radii of 0.75 .. 3 texels (most texels see a few stamps, some many), one over the hole of the source, one
    whose radius squared is infinite in binary32 (every texel of the face: d2 < inf, q = 0, w = 1) and one whose radius squared is 0"""
    rng = np.random.default_rng(12)
    stamps = []
    for k in range(MAX_STAMPS):
        cx, cy = (rng.integers(0, 48 * 4, size=2) / 4.0).tolist()
        stamps.append(S((cx, cy), float(rng.integers(3, 13)) / 4.0, float(rng.integers(-8, 9)) / 64.0 if k % 3 else float(rng.integers(8, 56)) / 64.0,
                        mode="add" if k % 3 else "flatten", falloff="hard" if k % 4 == 1 else "smooth"))
    stamps[17] = S((24.0, 16.0), 5.0, 0.2)
    stamps[100] = S((20.0, 30.0), 1e30, 0.015625)
    stamps[200] = S((30.0, 20.0), 1e-30, 0.5, falloff="hard")
    return stamps


FILLERS = [S((-100.0 - k, -50.0), 5.0, 0.5, falloff="hard") for k in range(MAX_STAMPS - 1)]  # discs wholly outside the face


def live_stamp(k):
    return S(((7 * k) % 48 + 0.5, (11 * k) % 48 + 0.25), 2.5, 0.03125 if k % 2 else -0.03125, falloff="hard" if k % 5 == 0 else "smooth")


CUBE_EDITS = [
    Edit([S((0.5, 23.0), 3.5, 0.25, side=0)], reach={"edge_tile_that_is_no_corner_tile"}),  # a face edge, away from the corners, even side
    Edit([S((47.0, 20.0), 3.0, -0.2, side=3, falloff="hard")], reach={"edge_tile_that_is_no_corner_tile"}),  # the same on an odd side
    Edit([S((1.0, 46.0), 3.0, 0.2, side=2)], reach={"corner_tile"}),
    Edit([S((18.0, 18.0), 3.0, 0.15, side=5)], reach={"interior_tile_beside_a_seam_tile"}),
    Edit([S((24.0, 0.5), 4.0, 0.15, side=0), S((0.5, 30.0), 4.0, -0.1, side=1, falloff="hard"), S((40.0, 47.0), 3.0, 0.6, side=4, mode="flatten")],
         reach={"edge_tile_that_is_no_corner_tile"}),
    Edit([S((11.5, 12.5), 4.0, 0.25, side=2)], lod=1, reach={"corner_tile"}),
]

CASES = {
    "a_r16_b2": case_a(2),
    "a_r16_b3": case_a(3),
    "b_rgba8_b2": case_b(2),
    "b_rgba8_b1": case_b(1),
    # 64 finest tiles on the face, 16 + 4 + 4 + 1 in the atlas; the third stamp lies over absent tiles only
    "c_box_over_more_tiles": (small(lods=4, extent=rect(0.3, 0.3, 0.7, 0.7)),
                              [Edit([S((48.0, 48.0), 200.0, 0.05), S((40.0, 50.0), 150.0, -0.03, falloff="hard"), S((5.0, 5.0), 2.0, 0.2)],
                                    reach={"box_over_more_tiles_than_the_atlas_holds"})]),
    "c_no_lod0": (small(lod_range=range(1, 3)), [Edit([S((23.5, 23.5), 5.0, 0.2)], reach={"chain_ends_at_a_missing_parent"})]),
    # LOD 2 on the left half only, LODs 1 and 2 on the right half, the left half again (its aprons now see the right half): the tiles of
    # column 1 have no parent, those of column 2 have one, and column 1 comes first in the plan's order
    "c_parent_of_some": (small(lod_range=range(2, 3), extent=rect(0.0, 0.0, 0.5, 1.0),
                               then=[(range(1, 3), rect(0.5, 0.0, 1.0, 1.0)), (range(2, 3), rect(0.0, 0.0, 0.5, 1.0))]),
                         [Edit([S((23.5, 23.5), 5.0, 0.2)], reach={"chain_ends_at_a_missing_parent", "chain_goes_on_behind_an_ended_one"})]),
    "c_gap": (small(lod_range=range(0, 1), then=[(range(2, 3), {})]), [Edit([S((23.5, 23.5), 5.0, 0.2)], reach={"chain_ends_at_a_missing_parent"})]),
    "c_quadrant_untouched": (small(), [Edit([S((5.0, 5.0), 2.0, 0.2), S((17.0, 18.0), 2.0, -0.2, falloff="hard")], reach={"rectangle_over_an_untouched_quadrant"})]),
    # the tiles (0, 0) and (1, 1) of LOD 2 and their ancestors: two jobs, and the first again for its aprons
    "c_quadrant_absent": (small(extent=rect(0.0, 0.0, 0.25, 0.25), then=[(range(0, 3), rect(0.25, 0.25, 0.5, 0.5)), (range(0, 3), rect(0.0, 0.0, 0.25, 0.25))]),
                          [Edit([S((5.0, 5.0), 2.0, 0.2), S((17.0, 18.0), 2.0, -0.2, falloff="hard")], reach={"rectangle_over_an_absent_quadrant"})]),
    "d_cube": (dict(kind="cube", T=16, b=2, lods=3, fmt=R16), CUBE_EDITS),
    "e_256_stamps": (small(), [Edit(stamps_256(), reach={"256_stamps", "radius_squared_overflows", "radius_squared_underflows"})]),
    "f_ring_frame": (small(), [Edit([live_stamp(1)] + FILLERS, reach={"256_stamps"})]),
}


def device_atlas(device, spec, **kw):
    if spec["kind"] == "cube":
        return cube(device, spec["T"], spec["b"], spec["lods"], atlas_size=128, **kw)
    return planar(device, spec["T"], spec["b"], spec["lods"], spec["fmt"], src=spec["src"](), lod_range=spec.get("lod_range"), then=spec.get("then", ()),
                  **spec.get("extent", {}), **kw)


def oracle_tiles(spec):
    """the state the jobs of `spec` leave, made by the CPU oracle: {(side, lod, x, y): tile}"""
    T, b, lods, fmt = spec["T"], spec["b"], spec["lods"], spec["fmt"]
    atlas = O.OracleAtlas(lods, 128, spec["kind"] == "cube", [(T, b, 1, fmt)])
    atlas.clear_attachment(0)
    if spec["kind"] == "cube":
        atlas.preprocess_spherical(0, cube_faces(), (0, lods)).run(4)
    else:
        src = spec["src"]()
        for levels, extent in [(spec.get("lod_range") or range(0, lods), spec.get("extent", {}))] + list(spec.get("then", ())):
            atlas.preprocess_tile(0, src, (levels.start, levels.stop), **extent).run(4)
    return {coord: atlas.tile(0, i) for coord, i in atlas.tiles()}


def edit_reaches(spec, edit, existing):
    """(boxes, levels, names) of one edit of a case on an atlas that holds `existing`"""
    c = spec["T"] - 2 * spec["b"]
    lod = spec["lods"] - 1 if edit["lod"] is None else edit["lod"]
    if edit["stamps"] is not None:
        boxes = stamp_boxes(edit["stamps"], lod, c)
    else:
        x0, y0, w, h, _ = edit["region"]
        boxes = [(0, x0, y0, x0 + w - 1, y0 + h - 1)]
    levels = plan_levels(boxes, lod, c, existing)
    return boxes, levels, branches_reached(boxes, levels, lod, c, spec["b"], spec["fmt"], existing, spec["kind"] == "cube", edit["stamps"] or ())


def model_edit(tiles, spec, edit):
    """the model's centres after the edit (nothing stitched)"""
    lod = spec["lods"] - 1 if edit["lod"] is None else edit["lod"]
    coarse = {k: v for k, v in tiles.items() if k[1] <= lod}
    if edit["stamps"] is not None:
        primary = EM.apply_stamps(coarse, lod, edit["stamps"], spec["b"])
    else:
        x0, y0, w, h, seed = edit["region"]
        primary = EM.write_region(coarse, lod, 0, x0, y0, region_texels(spec["fmt"], h, w, seed), spec["b"])
    out = dict(tiles)
    out.update(EM.propagate(primary, spec["b"], spec["kind"] == "cube", only=[]))
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_cases_reach_their_branches(name):
    """no GPU: the conditions the GPU cases assert, on the oracle's state of the same jobs, and plan_levels() against the model: every
    centre texel the model changes, on every LOD, lies in the rectangle of its tile (the rectangles may cover more: they are boxes)"""
    spec, edits = CASES[name]
    b = spec["b"]
    tiles = start = oracle_tiles(spec)
    held = EM.propagate(tiles, b, spec["kind"] == "cube")
    assert all(np.array_equal(held[k], tiles[k]) for k in tiles), "the jobs do not leave a state that is F of its primary centres"
    for n, edit in enumerate(edits):
        boxes, levels, names = edit_reaches(spec, edit, set(tiles))
        assert edit["reach"] <= names, (name, n, sorted(edit["reach"] - names))
        after = model_edit(tiles, spec, edit)
        rects = {k: r for level in levels for k, r in level.items()}
        differing = 0
        for k in tiles:
            d = np.argwhere(tiles[k][b:-b, b:-b] != after[k][b:-b, b:-b])
            if len(d):
                assert k in rects, (name, n, k)
                x0, y0, x1, y1 = rects[k]
                assert d[:, 0].min() >= y0 and d[:, 0].max() <= y1 and d[:, 1].min() >= x0 and d[:, 1].max() <= x1, (name, n, k, rects[k])
                differing += 1
        assert differing, "the edit changes nothing"
        tiles = after
    if name == "e_256_stamps":
        gy, gx = np.mgrid[12:24, 24:36]
        hole = (start[(0, 2, 2, 1)][b:-b, b:-b] == 0) & ((gx - 24.0) ** 2 + (gy - 16.0) ** 2 < 25.0)
        assert hole.any() and np.array_equal(start[(0, 2, 2, 1)][b:-b, b:-b] == 0, tiles[(0, 2, 2, 1)][b:-b, b:-b] == 0), "no hole under stamp 17"


# ---------------------------------------------------------------------------------------------- running a case on the device

def region_and_check(atlas, x0, y0, texels, lod=None):
    """edit_and_check for bt_atlas_write_region"""
    b, c, spherical = geometry(atlas)
    lod = atlas.lod_count - 1 if lod is None else lod
    before = Snapshot(atlas)
    held = EM.propagate(before.tiles, b, spherical)
    assert all(np.array_equal(held[k], before.tiles[k]) for k in before.tiles), "the state before the edit is not F of its primary centres"
    changed, stats = atlas.write_region(0, texels, x0, y0, lod)
    coarse = {k: v for k, v in before.tiles.items() if k[1] <= lod}
    expected = dict(before.tiles)
    expected.update(EM.propagate(EM.write_region(coarse, lod, 0, x0, y0, texels, b), b, spherical))
    edited = EM.region_tiles(lod, 0, x0, y0, texels.shape[1], texels.shape[0], c)
    levels = ancestors_levels(before, edited)
    after = check_edit(atlas, before, expected, changed, stats, edited, levels)
    assert stats["layers_mipped"] == 0 and stats["launches"] == (1 + levels + (1 if b else 0) if stats["tiles_edited"] else 0)
    return before, after, changed, stats


def run_case(device, name, atlas=None):
    """every edit of CASES[name] in turn on one atlas: the branches asserted from the atlas's own tiles, then the edit compared"""
    spec, edits = CASES[name]
    atlas = atlas or device_atlas(device, spec)
    results = []
    for n, edit in enumerate(edits):
        existing = {(c.side, c.lod, c.x, c.y) for c, _ in atlas.tiles()}
        _, levels, names = edit_reaches(spec, edit, existing)
        assert edit["reach"] <= names, (name, n, sorted(edit["reach"] - names))
        if edit["stamps"] is not None:
            before, after, changed, stats = edit_and_check(atlas, edit["stamps"], edit["lod"])
        else:
            x0, y0, w, h, seed = edit["region"]
            before, after, changed, stats = region_and_check(atlas, x0, y0, region_texels(spec["fmt"], h, w, seed), edit["lod"])
        differing = sum(1 for k in before.tiles if not np.array_equal(before.tiles[k], after.tiles[k]))
        assert differing >= 1, "the edit changed nothing: the comparison would be empty"
        assert stats["tiles_edited"] == len(levels[0]) and stats["tiles_downsampled"] == sum(len(level) for level in levels[1:])
        results.append((before, after, changed, stats, levels))
    return atlas, results


# ---------------------------------------------------------------------------------------------- A. R16: the second lane trip, odd edges

@pytest.mark.gpu
@pytest.mark.parametrize("b", [2, 3])
def test_r16_rows_beyond_one_lane_trip(device, b):
    """T = 136, lod_count 3, a source with holes: a face-wide stamp (full rows, dwords 1 .. 66), a smooth stamp whose rectangle in a tile
    starts on an odd and ends on an even texel 64 dwords apart, one whose PARENT rectangle does, a hard stamp across a four-tile corner,
    and a region 131 texels wide with an odd origin across a tile boundary.  With `if` for the lane loop, or with the half-dword write-back
    wrong on the later trip, the texels (or the apron halves) right of dword first + 63 differ from the model."""
    atlas, results = run_case(device, f"a_r16_b{b}")
    assert (atlas.download_tiles(0, 0, ATLAS)[:, b:-b, b:-b] == 0).any(), "no hole left in the centres"


# ---------------------------------------------------------------------------------------------- B. Rgba8 beyond one block

@pytest.mark.gpu
@pytest.mark.parametrize("b", [2, 1])
def test_rgba8_regions_beyond_one_block(device, b):
    """T = 72: a region over the whole mosaic (68 / 70 texels and rows per tile, and per parent) and an odd rectangle with more than 64
    texels and 32 rows inside one of its four tiles; both hold zero texels"""
    run_case(device, f"b_rgba8_b{b}")


# ---------------------------------------------------------------------------------------------- C. the plan's branches

@pytest.mark.gpu
def test_box_over_more_tiles_than_the_atlas_holds(device):
    spec, edits = CASES["c_box_over_more_tiles"]
    atlas, [(before, after, changed, stats, levels)] = run_case(device, "c_box_over_more_tiles")
    assert 64 > len(atlas.tiles())
    finest = {k for k in before.index if k[1] == 3}
    met = EM.stamp_tiles(edits[0]["stamps"], 3, 12)
    assert len(met) == 64 and len(finest) == 16
    assert stats["tiles_edited"] == len(finest) and stats["tiles_missing"] == len(met - finest) == 48
    assert EM.stamp_tiles(edits[0]["stamps"][2:], 3, 12).isdisjoint(finest), "the small stamp meets an existing tile"


@pytest.mark.gpu
def test_chain_ends_at_a_missing_parent(device):
    """an atlas without LOD 0: the chain of ancestors ends at LOD 1"""
    atlas, [(before, after, changed, stats, levels)] = run_case(device, "c_no_lod0")
    assert {k[1] for k in before.index} == {1, 2}
    assert all(t.lod > 0 for t in changed) and stats["tiles_downsampled"] == len(levels[1]) == 4 and len(levels) == 2


@pytest.mark.gpu
def test_chain_ends_for_some_tiles_and_goes_on_for_others(device):
    """edited tiles without a parent beside edited tiles with one, the parentless first in the plan's order: the others' parents follow"""
    atlas, [(before, after, changed, stats, levels)] = run_case(device, "c_parent_of_some")
    assert {k for k in before.index if k[1] == 1} == {(0, 1, 1, 0), (0, 1, 1, 1)} and len([k for k in before.index if k[1] == 2]) == 16
    assert stats["tiles_edited"] == 4 and stats["tiles_downsampled"] == 2
    assert all(not np.array_equal(before.tiles[k], after.tiles[k]) for k in levels[1])


@pytest.mark.gpu
def test_gap_in_the_chain(device):
    """LOD 0 and LOD 2 but no LOD 1 (two jobs, the second without the clear): the edit writes LOD 2 only; the root has no existing child, so
    it is primary under rule 1 of the model and keeps its bytes"""
    atlas, [(before, after, changed, stats, levels)] = run_case(device, "c_gap")
    assert {k[1] for k in before.index} == {0, 2} and (0, 0, 0, 0) in before.index
    assert stats["tiles_downsampled"] == 0 and all(t.lod == 2 for t in changed) and stats["launches"] == 2
    assert np.array_equal(after.tiles[(0, 0, 0, 0)], before.tiles[(0, 0, 0, 0)])


@pytest.mark.gpu
@pytest.mark.parametrize("others", ["untouched", "absent"])
def test_parent_rectangle_over_a_quadrant_nobody_edited(device, others):
    """two small stamps in diagonal children of one parent: the parent's united rectangle covers texels of the other two quadrants, whose
    children exist and are untouched (the kernel recomputes the same values) or do not exist (it writes the zeros that are there)"""
    atlas, [(before, after, changed, stats, levels)] = run_case(device, f"c_quadrant_{others}")
    assert set(levels[0]) == {(0, 2, 0, 0), (0, 2, 1, 1)} and set(levels[1]) == {(0, 1, 0, 0)}
    assert ((0, 2, 1, 0) in before.index) == ((0, 2, 0, 1) in before.index) == (others == "untouched")


# ---------------------------------------------------------------------------------------------- D. the cube at lod_count 3

@pytest.mark.gpu
def test_cube_lod_count_3(device):
    """T = 16, b = 2, 126 tiles, all compared after every edit: edge tiles that are no corner tiles on an even and on an odd side, a corner
    tile, an interior tile beside seam tiles, three sides in one call, and an edit at LOD 1 that leaves the finer tiles alone"""
    atlas, results = run_case(device, "d_cube")
    assert len(atlas.tiles()) == 126
    for (before, after, changed, stats, levels), edit in zip(results[:2], CUBE_EDITS):
        assert {t.side for t in changed} - {edit["stamps"][0].side}, "no tile of a neighbouring face was re-stitched"
    assert {t.side for t in results[2][2]} >= {2} and len({t.side for t in results[2][2]}) >= 3, "a face corner touches three faces"
    assert {k[0] for k in results[4][4][0]} == {0, 1, 4}
    before, after, changed, stats, levels = results[5]
    assert all(t.lod <= 1 for t in changed) and stats["tiles_with_children"] == stats["tiles_edited"] > 0
    assert all(np.array_equal(before.tiles[k], after.tiles[k]) for k in before.tiles if k[1] == 2)


@pytest.mark.gpu
def test_cube_mips_of_changed_layers_follow(device):
    spec, _ = CASES["d_cube"]
    atlas = device_atlas(device, spec, mips=3)
    atlas.generate_mipmaps(0)
    layers_all = range(atlas.atlas_size)
    mips_before = {i: [atlas.download_mip(0, k, i) for k in (1, 2)] for i in layers_all}
    before, after, changed, stats = edit_and_check(atlas, CUBE_EDITS[2]["stamps"])
    layers = {before.index[(t.side, t.lod, t.x, t.y)] for t in changed}
    assert stats["layers_mipped"] == len(layers) > 0 and len({t.side for t in changed}) >= 3
    for i in layers_all:
        got = [atlas.download_mip(0, k, i) for k in (1, 2)]
        if i in layers:
            chain = O.generate_mipmaps(R16, after.data[i], 3)
            want = [chain[256:320].reshape(8, 8), chain[320:336].reshape(4, 4)]
            assert all(np.array_equal(g, w) for g, w in zip(got, want)), f"mips of changed layer {i}"
        else:
            assert all(np.array_equal(g, w) for g, w in zip(got, mips_before[i])), f"mips of untouched layer {i}"


# ---------------------------------------------------------------------------------------------- E. 256 stamps

@pytest.mark.gpu
def test_256_stamps_in_one_call_and_one_by_one(device):
    """the documented limit in one call, compared with the model; then the same stamps as 256 calls of one stamp, back to back, on a second
    atlas: the brush quantises after every stamp, so both are the same function of the finest centres (asserted on the model first)"""
    spec, [edit] = CASES["e_256_stamps"]
    stamps = edit["stamps"]
    atlas, [(before, after, changed, stats, levels)] = run_case(device, "e_256_stamps")
    assert stats["tiles_edited"] == 16
    one, each = EM.apply_stamps(before.tiles, 2, stamps, 2), before.tiles
    for s in stamps:
        each = EM.apply_stamps(each, 2, [s], 2)
    assert all(np.array_equal(one[k], each[k]) for k in one), "the model: one call and 256 calls differ"
    nothing = EM.apply_stamps(before.tiles, 2, [stamps[200]], 2)
    assert all(np.array_equal(nothing[k], before.tiles[k]) for k in nothing) and EM.stamp_tiles([stamps[200]], 2, 12) <= set(before.index)
    hole = before.tiles[(0, 2, 2, 1)][2:14, 2:14] == 0
    assert hole.any() and np.array_equal(hole, after.tiles[(0, 2, 2, 1)][2:14, 2:14] == 0), "the hole mask changed"
    second = device_atlas(device, spec)
    assert np.array_equal(Snapshot(second).data, before.data)
    for s in stamps:
        second.edit_height(0, [s])
    assert np.array_equal(Snapshot(second).data, after.data)


# ---------------------------------------------------------------------------------------------- F. the plan ring wraps

def held_layers(atlas):
    data = atlas.download_tiles(0, 0, atlas.atlas_size)
    return data, {(c.side, c.lod, c.x, c.y): data[i] for c, i in atlas.tiles()}


@pytest.mark.gpu
def test_plan_ring_wraps_under_a_painting_stroke(device):
    """N frames of one 256-stamp edit (one live stamp, 255 fillers outside the face that are uploaded and change nothing) and one
    HeightBounds.update, nothing synchronised: the stamps alone put N * 256 * sizeof(bt_edit_stamp) bytes into the plan ring, more than
    three times its size, so it wraps at least twice with launches still queued.  Afterwards the layers equal the model, the table equals
    the definition and a fresh build, and a second atlas that synchronises after every call holds the same bytes.

    This guards a race: passing does not prove the wrap correct.  It fails on a wrap that restarts without the wait whenever the device
    lags the host, and it runs the wrap's arithmetic, which nothing else does."""
    spec, [edit] = CASES["f_ring_frame"]
    per_call = MAX_STAMPS * ctypes.sizeof(_ffi.EditStampC)
    frames = 3 * RING_BYTES // per_call + 1
    assert frames * per_call > 3 * RING_BYTES and len(edit["stamps"]) == MAX_STAMPS
    arr = (_ffi.EditStampC * MAX_STAMPS)(*[s._c() for s in edit["stamps"]])
    live = [live_stamp(k) for k in range(frames)]

    def stroke(sync):
        atlas = device_atlas(device, spec)
        hb = bt.HeightBounds(device, 1, 3).build(atlas, 0)
        start = Snapshot(atlas)
        device.synchronize()
        for s in live:
            arr[0] = s._c()
            changed, stats = atlas._edit_result(lambda changed, cap, st: _ffi.lib().bt_atlas_edit_height(atlas._h, 0, 2, arr, MAX_STAMPS, changed, cap, st))
            assert stats["tiles_edited"] >= 1 and stats["tiles_missing"] == 0
            if sync:
                device.synchronize()
            hb.update(atlas, changed)
            if sync:
                device.synchronize()
        return atlas, hb, start

    atlas, hb, start = stroke(False)
    # the model: the fillers change nothing (one frame), so it applies the live stamps only
    with_fillers, without = EM.apply_stamps(start.tiles, 2, edit["stamps"], 2), EM.apply_stamps(start.tiles, 2, edit["stamps"][:1], 2)
    assert all(np.array_equal(with_fillers[k], without[k]) for k in without) and not stamp_boxes(FILLERS, 2, 12)
    primary = start.tiles
    for s in live:
        primary = EM.apply_stamps(primary, 2, [s], 2)
    expected = EM.propagate(primary, 2, False)
    data, held = held_layers(atlas)
    bad = [k for k in held if not np.array_equal(held[k], expected[k])]
    assert not bad, (len(bad), bad[:6])
    assert set(held) == set(start.index) and sum(1 for k in held if not np.array_equal(held[k], start.tiles[k])) == 21
    table = hb.read()
    assert np.array_equal(table, M.build_table(1, 3, held).data)
    fresh = bt.HeightBounds(device, 1, 3).build(atlas, 0)
    assert np.array_equal(table, fresh.read())
    other, other_hb, _ = stroke(True)
    assert np.array_equal(other.download_tiles(0, 0, other.atlas_size), data) and np.array_equal(other_hb.read(), table)

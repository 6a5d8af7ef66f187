"""The model of bt_atlas_label_regions (tests/_regions_model.py) held to a second restatement, to answers worked by hand and to the
definition's invariants; the scenes of tests/_regions_cases.py held to what they are named for; the ctypes mirror held to the header's
stated struct layouts; and the symbol required in the built library.  No GPU."""
import ctypes as C
import re

import numpy as np
import pytest

import _regions_cases as RC
import _regions_model as M
from bevy_terrain_amd import _ffi
from bevy_terrain_amd.tile_atlas import TileAtlas

NONE = M.NONE


def propagate(member, v, max_step=65535, eight=False):
    """the second restatement: every member starts with its own index and takes the smallest label among itself and its linked
    neighbours, whole arrays at a time, until nothing changes"""
    h, w = member.shape
    big = np.int64(1) << 40
    label = np.where(member, np.arange(h * w, dtype=np.int64).reshape(h, w), big)
    shifts = [(0, 1), (1, 0)] + ([(1, 1), (1, -1)] if eight else [])
    while True:
        before = label.copy()
        for dy, dx in shifts:
            a = (slice(0, h - dy), slice(max(0, -dx), w - max(0, dx)))
            b = (slice(dy, h), slice(max(0, dx), w + min(0, dx)))
            linked = member[a] & member[b] & (np.abs(v[a] - v[b]) <= max_step)
            low = np.minimum(label[a], label[b])
            label[a] = np.where(linked, np.minimum(low, label[a]), label[a])  # the two views overlap: a label only ever falls
            label[b] = np.where(linked, np.minimum(low, label[b]), label[b])
        if np.array_equal(before, label):
            return np.where(member, label, NONE).astype(np.uint32)


def plain(mask, **kw):
    mask = np.asarray(mask, dtype=bool)
    v = kw.pop("v", np.zeros(mask.shape, np.int64))
    label = M.labels(mask, np.asarray(v, dtype=np.int64), **kw)
    return label, M.table(label, np.asarray(v, dtype=np.int64))


# ---------------------------------------------------------------------------------------------- by hand

def test_checkerboard_by_hand():
    board = RC.checkerboard(5, 6) != 0
    label, regions = plain(board)
    assert len(regions) == 15 and (regions["area"] == 1).all() and (regions["edges"] == 4).all()
    assert regions["label"].tolist() == np.flatnonzero(board).tolist()
    label, regions = plain(board, eight=True)
    assert len(regions) == 1 and regions[0]["area"] == 15 and regions[0]["edges"] == 60 and regions[0]["label"] == 0
    assert (regions[0]["x_min"], regions[0]["y_min"], regions[0]["x_max"], regions[0]["y_max"]) == (0, 0, 5, 4)


def test_u_by_hand():
    mask = np.array([[1, 0, 1], [1, 0, 1], [1, 1, 1]], bool)
    label, regions = plain(mask)
    assert label.tolist() == [[0, NONE, 0], [0, NONE, 0], [0, 0, 0]]
    assert len(regions) == 1 and regions[0]["area"] == 7 and regions[0]["edges"] == 16  # 12 around the square and 4 more in the notch
    label, regions = plain(mask[:2])  # the arms alone: two regions, labelled by their first cells
    assert label.tolist() == [[0, NONE, 2], [0, NONE, 2]] and regions["area"].tolist() == [2, 2] and regions["edges"].tolist() == [6, 6]


def test_ring_edges_by_hand():
    ring = np.ones((3, 3), bool)
    ring[1, 1] = False
    _, regions = plain(ring)
    assert regions["edges"].tolist() == [16] and regions["area"].tolist() == [8]  # 12 outer, 4 around the hole
    _, regions = plain(np.pad(ring, 1))  # the same with non-members around in place of the window's edge
    assert regions["edges"].tolist() == [16] and (regions[0]["x_min"], regions[0]["y_min"], regions[0]["x_max"], regions[0]["y_max"]) == (1, 1, 3, 3)


def test_v_sum_and_max_step_on_a_ramp_by_hand():
    v = np.array([[10, 11, 12, 14, 15]])
    label, regions = plain(np.ones((1, 5), bool), v=v, max_step=1)
    assert label.tolist() == [[0, 0, 0, 3, 3]]
    assert regions["v_sum"].tolist() == [33, 29] and regions["v_min"].tolist() == [10, 14] and regions["v_max"].tolist() == [12, 15]
    assert regions["edges"].tolist() == [8, 6]  # the edge between 12 and 14 is counted on both sides
    assert plain(np.ones((1, 5), bool), v=v, max_step=2)[0].tolist() == [[0] * 5]
    assert plain(np.ones((1, 5), bool), v=v, max_step=0)[0].tolist() == [[0, 1, 2, 3, 4]]


def test_stats_and_bake_by_hand():
    mask = np.array([[1, 1, 0, 1], [0, 0, 0, 1], [1, 0, 0, 1]], bool)
    label, regions = plain(mask)
    assert regions["area"].tolist() == [2, 3, 1] and regions["label"].tolist() == [0, 3, 8]
    assert M.ids(label).tolist() == [[0, 0, NONE, 1], [NONE, NONE, NONE, 1], [2, NONE, NONE, 1]]
    assert M.stats(mask, regions, region_cap=2) == dict(cells=12, members=6, regions=3, regions_written=2, largest_area=3, largest_label=3, baked=0)
    texels = np.full((3, 4, 4), 9, np.uint8)
    out, baked = M.bake(texels, label, regions, 1, 1, 2, 200)
    assert baked == 3 and out[:, :, 1].tolist() == [[200, 200, 9, 9], [9, 9, 9, 9], [200, 9, 9, 9]] and (out[:, :, [0, 2, 3]] == 9).all()
    both = np.array([[1, 0], [0, 1], [1, 0]], bool)  # two regions of one area: the smaller label is the largest's
    assert M.stats(both, plain(both)[1])["largest_label"] == 0


# ---------------------------------------------------------------------------------------------- the invariants, on random windows and on every scene

def check_invariants(member, v, label, id_, regions, stats, max_step, eight):
    h, w = member.shape
    flat = label.ravel()
    index = np.arange(h * w)
    on = flat != NONE
    assert np.array_equal(on, member.ravel())
    assert (flat[on] <= index[on]).all() and np.array_equal(flat[flat[on]], flat[on])
    assert int(regions["area"].sum()) == stats["members"] == int(member.sum()) and int(regions["v_sum"].sum()) == int(v[member].sum())
    present = np.unique(flat[on])
    assert np.array_equal(regions["label"], present) and stats["regions"] == len(present)
    assert np.array_equal(id_.ravel()[on], np.searchsorted(present, flat[on])) and (id_.ravel()[~on] == NONE).all()
    assert np.array_equal(label, propagate(member, v, max_step, eight))


@pytest.mark.parametrize("seed", range(6))
def test_random_windows_against_the_second_restatement(seed):
    rng = np.random.default_rng(seed)
    h, w = int(rng.integers(1, 40)), int(rng.integers(1, 40))
    member = rng.random((h, w)) < (0.35, 0.45, 0.59, 0.65, 0.9, 0.5)[seed]
    v = rng.integers(0, 6, (h, w)).astype(np.int64)
    for eight in (False, True):
        for max_step in (0, 1, 65535):
            label = M.labels(member, v, max_step, eight)
            regions = M.table(label, v)
            check_invariants(member, v, label, M.ids(label), regions, M.stats(member, regions), max_step, eight)
    # the 8-connected partition is coarser than the 4-connected one: every 4-region lies in one 8-region
    four, eight = M.labels(member, v), M.labels(member, v, eight=True)
    for L in np.unique(four[member]):
        assert len(np.unique(eight[four == L])) == 1
    # the partition of the transposed window is the transpose of the partition
    t = M.labels(member.T.copy(), v.T.copy(), 1, True)
    straight = M.labels(member, v, 1, True)
    pairs = set(zip(straight[member].tolist(), t.T[member].tolist()))
    assert len(pairs) == len(np.unique(straight[member])) == len(np.unique(t[member.T]))


@pytest.mark.parametrize("name", sorted(RC.SCENES))
def test_every_scene_reaches_what_it_is_named_for(name):
    scene = RC.SCENES[name]
    texels, member, label, id_, regions, stats = RC.expected(name)
    reaches = RC.scene_reaches(name)
    missing = [r for r in scene["reach"] if not reaches.get(r)]
    assert not missing, (name, missing, stats)
    check_invariants(member, M.values(texels, scene["channel"]), label, id_, regions, {k: v for k, v in stats.items()}, scene["max_step"], scene["eight"])


def test_scene_reach_details():
    # the U has two local components in its upper block and one region
    assert RC.local_components("u_joined_below", 0, 0) == 2 and RC.local_components("u_joined_below", 0, 1) == 1
    # the serpentine and the spiral cross dozens of seams
    assert RC.seam_links("serpentine") >= 48 * 2 and RC.seam_links("spiral") >= 48
    # the diagonal scenes change their region count with EIGHT
    for pair in ("corner_down_right", "corner_down_left", "seam_diagonals"):
        four, eight = RC.expected(pair + "_four")[5]["regions"], RC.expected(pair + "_eight")[5]["regions"]
        assert four == 2 * eight, pair
    # the spiral is one cell wide: no 2 x 2 square of members
    m = RC.expected("spiral")[1]
    assert not (m[:-1, :-1] & m[1:, :-1] & m[:-1, 1:] & m[1:, 1:]).any() and m.sum() > 96 * 96 // 3
    # every documented case list is used by the GPU tests' parametrisations
    assert len(RC.SCENES) == len(RC.SHAPES + RC.SEAMS + RC.STEPS + RC.SOURCES + RC.SIZES + RC.FIELDS + RC.OTHER_LAYERS)


# ---------------------------------------------------------------------------------------------- the mirror and the library

def test_struct_layouts_match_the_header():
    assert C.sizeof(_ffi.RegionC) == M.REGION_SIZE == TileAtlas.REGION_DTYPE.itemsize == M.REGION_DTYPE.itemsize
    for name, offset in M.REGION_OFFSETS.items():
        assert getattr(_ffi.RegionC, name).offset == offset == TileAtlas.REGION_DTYPE.fields[name][1] == M.REGION_DTYPE.fields[name][1], name
    assert [n for n, _ in _ffi.RegionC._fields_] == list(M.REGION_DTYPE.names) == list(TileAtlas.REGION_DTYPE.names)
    assert C.sizeof(_ffi.RegionsRuleC) == M.RULE_SIZE and C.sizeof(_ffi.RegionsBakeC) == M.BAKE_SIZE and C.sizeof(_ffi.RegionsStatsC) == M.STATS_SIZE
    assert _ffi.RegionsStatsC.edit.offset == M.STATS_SIZE - C.sizeof(_ffi.EditStatsC)
    # the header states the same: the sizes in the structs' closing comments, the offsets in bt_region's field comments
    with open(_ffi.HEADER_PATH) as f:
        header = f.read()
    for struct, size in (("bt_regions_rule", M.RULE_SIZE), ("bt_regions_bake", M.BAKE_SIZE), ("bt_region", M.REGION_SIZE), ("bt_regions_stats", M.STATS_SIZE)):
        assert re.search(r"\} %s; /\* %d bytes \*/" % (struct, size), header), struct
    body = header[header.index("typedef struct bt_region {"):header.index("} bt_region;")]
    stated = {}
    for names, offsets in re.findall(r"u?int\d+_t ([a-z_, ]+);\s*/\* (?:offset )?([\d, ]+):", body):
        stated.update(zip([n.strip() for n in names.split(",")], [int(o) for o in offsets.split(",")]))
    assert stated == M.REGION_OFFSETS
    for name, value in (("NONE", _ffi.REGIONS_NONE), ("MAX_SIDE", _ffi.REGIONS_MAX_SIDE), ("BLOCK", _ffi.REGIONS_BLOCK), ("CHUNK", _ffi.REGIONS_CHUNK)):
        assert re.search(r"#define BT_REGIONS_%s (0x[0-9A-F]+|\d+)u" % name, header) and int(re.search(r"#define BT_REGIONS_%s (0x[0-9A-F]+|\d+)u" % name, header).group(1), 0) == value
    assert (_ffi.REGIONS_FROM_TEXELS, _ffi.REGIONS_INVERT, _ffi.REGIONS_EIGHT) == (M.FROM_TEXELS, M.INVERT, M.EIGHT) == (1, 2, 4)


def test_the_symbol_is_in_the_built_library():
    assert "bt_atlas_label_regions" in _ffi.header_symbols() and "bt_atlas_label_regions" in _ffi.PROTOTYPES
    assert hasattr(_ffi.lib(), "bt_atlas_label_regions")
    assert _ffi.lib().bt_abi_version() == 6

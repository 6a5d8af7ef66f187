"""bt_height_bounds_update branch by branch: the shapes test_gpu_bounds_update.py's scenarios never reach.  The inputs come from
_bounds_update_cases.py, whose reach (trips, form, window mix, walk depths) is asserted on the numpy plan in test_bounds_update_host.py and
here again next to the device's stats.  Held sets are made without a preprocessing job: get_or_allocate_tile + upload_tile holds a tile
with chosen contents; the atlas has no free slot, so releasing a tile and allocating another coordinate evicts it ("parked" coordinates
far below every table take and give back the slots); request_tile of an evicted tile leaves it loading.

After every update: the table equals the definition (_cull_model.build_table of what the atlas holds) and a table freshly built on the
atlas, differed from the definition before, entries_written is exactly the number of affected entries of the numpy plan (every entry has
one writer), and the same update again changes nothing.  T = 16, b = 2."""
import numpy as np
import pytest

import _bounds_update_cases as BC
import _cull_model as M
import bevy_terrain_amd as bt
from bevy_terrain_amd import TileCoordinate
from test_gpu_bounds_update import INVALID, held_layers

pytestmark = pytest.mark.gpu

T, B = BC.T, 2
PARK_LOD = 12  # parked coordinates: below every table of these tests, so neither build nor update looks at them


@pytest.fixture(scope="module")
def device():
    return bt.Device(0)


def new_atlas(device, sides, lod_count, atlas_size):
    model = bt.TerrainModel.sphere((0.0, 0.0, 0.0), 6371000.0, -12000.0, 9000.0) if sides == 6 else bt.TerrainModel.planar((0.0, 0.0, 0.0), 1000.0, 0.0, 250.0)
    cfg = bt.TerrainConfig(lod_count=lod_count, atlas_size=atlas_size, path="terrains/bounds_update_shapes", model=model)
    cfg.add_attachment(bt.AttachmentConfig(name="height", texture_size=T, border_size=B, format=bt.AttachmentFormat.R16))
    return bt.TileAtlas.new(cfg, device)


class Slots:
    """an atlas without a free slot: `initial` held with its contents, the rest parked.  Between two calls the LRU list is empty, so a
    released tile's slot is the next one handed out."""

    def __init__(self, device, sides, lod_count, initial, spare):
        self.atlas = new_atlas(device, sides, lod_count, len(initial) + spare)
        self.held, self.known, self.loading, self.parked, self.parks = set(), set(), set(), [], 0
        for c, layer in initial.items():
            self._take(c, layer)
        for _ in range(spare):
            self._park()

    def _take(self, c, layer):
        _, index = self.atlas.get_or_allocate_tile(TileCoordinate(*c))
        assert index != INVALID
        if layer is not None:
            self.atlas.upload_tile(0, index, layer)
        self.held.add(c)
        self.known.add(c)

    def _park(self):
        c = (0, PARK_LOD, self.parks, 0)
        self.parks += 1
        self.atlas.get_or_allocate_tile(TileCoordinate(*c))
        self.parked.append(c)

    def _free_one(self):
        self.atlas.release_tile(TileCoordinate(*self.parked.pop()))

    def upload(self, c, layer):
        assert c in self.held
        self._take(c, layer)

    def hold(self, c, layer):
        assert c not in self.held and c not in self.loading
        self._free_one()
        self._take(c, layer)

    def evict(self, c):
        assert c in self.held
        self.atlas.release_tile(TileCoordinate(*c))
        self._park()  # takes the released slot: c has no atlas index any more
        self.held.discard(c)

    def load(self, c):
        """requested, never loaded: the atlas knows the tile, it has a slot, and it is not held"""
        if c in self.held:
            self.evict(c)
        elif c not in self.known:
            self.hold(c, None)
            self.evict(c)
        self._free_one()
        self.atlas.request_tile(TileCoordinate(*c))
        self.loading.add(c)

    def apply(self, ops):
        for kind, c, layer in ops:
            getattr(self, kind)(*((c, layer) if layer is not None else (c,)))


def table_index(sides, c):
    n = 1 << c[1]
    return sides * (4 ** c[1] - 1) // 3 + (c[0] * n + c[3]) * n + c[2]


def update_and_check(device, hb, atlas, listed, loading=(), own_of_layers=False):
    """the comparisons of the module docstring -> (stats, the update's Reach, the table before, the expected table)"""
    sides, levels = hb.sides, hb.levels
    held = {k: v for k, v in held_layers(atlas, loading).items() if k[1] != PARK_LOD}
    expected = M.build_table(sides, levels, held, own=BC.own_of(held) if own_of_layers else None).data
    reach = BC.Reach(levels, listed, held.__contains__)
    before = hb.read()
    assert not np.array_equal(before, expected), "the table before the update must differ from the expected one (or the case shows nothing)"
    tiles = [TileCoordinate(*c) for c in listed]
    stats = hb.update(atlas, tiles)
    got = hb.read()
    wrong = np.flatnonzero((got != expected).any(axis=1))
    assert len(wrong) == 0, (len(wrong), wrong[:8], got[wrong[:8]], expected[wrong[:8]])
    fresh = bt.HeightBounds(device, sides, levels).build(atlas, 0)
    assert np.array_equal(got, fresh.read())
    fresh.close()
    reduced = sum(u in held for u in reach.U)
    print(f"levels {levels} sides {sides}: listed {len(reach.U)} windows {reach.window_count} work {reach.work} total {reach.total} stats {stats}")
    assert stats["tiles_listed"] == len(reach.U) and stats["layers_reduced"] == reduced
    assert stats["entries_written"] == reach.total == len(reach.affected)  # one writer per affected entry, no entry without one
    assert stats["launches"] == reach.launches() + (reduced > 0)
    assert hb.update(atlas, tiles) == stats and np.array_equal(hb.read(), got)  # the same update again: nothing changes
    return stats, reach, before, expected


# ------------------------------------------------------------------------------------------- 1. random sparse held sets, small form

@pytest.mark.parametrize("seed", range(len(BC.SPARSE)))
def test_sparse_held_sets(device, seed):
    """three steps of narrowed, moved, evicted, newly held and loading tiles on a random sparse atlas, planar and cube, the atlas as deep
    as the table, shallower or deeper; the list carries a duplicate and a tile below the table"""
    script = BC.sparse_script(seed)
    slots = Slots(device, script.sides, script.lods, script.initial, spare=4 + sum(len(s.ops) for s in script.steps))
    hb = bt.HeightBounds(device, script.sides, script.levels).build(slots.atlas, 0)
    assert np.array_equal(hb.read(), M.build_table(script.sides, script.levels, script.initial).data)
    for step, planned, held in BC.replay(script):
        slots.apply(step.ops)
        stats, reach, _, _ = update_and_check(device, hb, slots.atlas, step.listed, loading=slots.loading)
        now = {k: v for k, v in held_layers(slots.atlas, slots.loading).items() if k[1] != PARK_LOD}
        assert now.keys() == held.keys() == slots.held and all(np.array_equal(now[k], held[k]) for k in now)  # the atlas is what the script says
        assert (reach.total, reach.work, sorted(reach.roots)) == (planned.total, planned.work, sorted(planned.roots))
        assert stats["launches"] <= 2 and reach.small_form
    hb.close()
    slots.atlas.close()


def test_sparse_held_sets_reach():
    """summed over the seeds above, from the plan: an entry whose nearest held ancestor is two or more levels up, an entry without a held
    ancestor beside a held side or quadrant, a fill root inside another's subtree, a listed tile under a root, every step in one launch"""
    seen = {}
    for seed in range(len(BC.SPARSE)):
        for step, reach, held in BC.replay(BC.sparse_script(seed)):
            assert reach.launches() == 1
            for name, hit in BC.sparse_reach(reach, held).items():
                seen[name] = seen.get(name, 0) + hit
    assert set(seen) == {"walks_two", "whole_range_beside_held", "nested_roots", "listed_under_a_root"} and min(seen.values()) >= 2, seen


# ------------------------------------------------------------------------------------------- 2, 3. the full 8-level pyramid

@pytest.fixture(scope="module")
def big(device):
    """the planar atlas of 21 845 held tiles, every range inside BC.BIG_BASE -> (atlas, {coord: atlas index})"""
    coords, layers = BC.big_initial()
    atlas = new_atlas(device, 1, BC.BIG_LEVELS, len(coords))
    index = {}
    for c, layer in zip(coords, layers):
        index[c] = atlas.get_or_allocate_tile(TileCoordinate(*c))[1]
        atlas.upload_tile(0, index[c], layer)
    assert len(set(index.values())) == len(coords) and INVALID not in index.values()
    yield atlas, index
    atlas.close()


def test_second_trips_of_the_small_form(device, big):
    """1104 level-6 tiles with all children held: more than 1024 scatter records, windows, affected entries and level-6 entries in the
    one workgroup.  Every other listed tile's new range reaches beyond its children's at both ends and differs from every other, so its
    entry becomes a value of its own; the tiles between get a flat layer inside their children's union, so their entry is the union
    and the filled own is not.  A skipped second trip of any of the loops leaves some of the last 80 entries wrong."""
    atlas, index = big
    hb = bt.HeightBounds(device, 1, BC.BIG_LEVELS).build(atlas, 0)
    listed = BC.second_trip_list()
    ranges = BC.own_ranges(atlas.download_tiles(0, 0, atlas.atlas_size))
    new, unions = BC.second_trip_layers(np.random.default_rng(21), listed, {c: ranges[i] for c, i in index.items()})
    for c, layer in zip(listed, new):
        atlas.upload_tile(0, index[c], layer)
    stats, reach, before, expected = update_and_check(device, hb, atlas, listed, own_of_layers=True)
    assert BC.SMALL_THREADS < reach.work[6] == stats["tiles_listed"] and BC.SMALL_THREADS < reach.window_count
    assert BC.SMALL_THREADS < stats["entries_written"] <= BC.SMALL_FORM_MAX and stats["launches"] <= 2 and not reach.roots
    at = np.array([table_index(1, c) for c in listed])
    assert (before[at[0::2]] != expected[at[0::2]]).all() and len({tuple(e) for e in expected[at[0::2]]}) == len(listed) // 2
    assert np.array_equal(expected[at[1::2]], unions[1::2]) and (expected[at[1::2]] != BC.own_ranges(new[1::2])).all()
    hb.close()


def test_root_alone(device, big):
    """the root listed, its children held: one entry, and the unite loop passes over every deeper level"""
    atlas, index = big
    hb = bt.HeightBounds(device, 1, BC.BIG_LEVELS).build(atlas, 0)
    root = (0, 0, 0, 0)
    atlas.upload_tile(0, index[root], BC.layer_with(np.random.default_rng(22), 7, 65001))  # beyond BC.BIG_BASE at both ends
    stats, reach, before, expected = update_and_check(device, hb, atlas, [root], own_of_layers=True)
    assert stats["entries_written"] == 1 and reach.work == [1] + [0] * 7 and stats["launches"] <= 2
    assert (before[1:] == expected[1:]).all()
    hb.close()


def test_form_edge(device, big):
    """4096 affected entries, single windows all: the one workgroup with 65 536 bytes of dynamic LDS; 4097: the wide form, twelve
    workgroups of scatter records and a search over 3072 windows at level 7.  The same contents through either form: the same table."""
    atlas, index = big
    small, wide = (bt.HeightBounds(device, 1, BC.BIG_LEVELS).build(atlas, 0) for _ in range(2))
    listed = BC.form_edge_list()
    data = atlas.download_tiles(0, 0, atlas.atlas_size)
    changed = listed[:-1]  # the last tile keeps its contents: leaving it out of the list is correct
    new = BC.moved_layers(np.random.default_rng(23), data[[index[c] for c in changed]])
    for c, layer in zip(changed, new):
        atlas.upload_tile(0, index[c], layer)
    stats, reach, _, _ = update_and_check(device, small, atlas, changed, own_of_layers=True)
    assert stats["entries_written"] == 4096 == BC.SMALL_FORM_MAX and stats["launches"] <= 2 and stats["tiles_listed"] == 3071
    assert reach.window_count * 16 == 65536
    stats, reach, _, _ = update_and_check(device, wide, atlas, listed, own_of_layers=True)
    assert stats["entries_written"] == 4097 and stats["launches"] > 2 and stats["tiles_listed"] == 3072
    assert reach.work[7] == 3072 and len(reach.windows[7]) == 3072
    assert np.array_equal(small.read(), wide.read())
    small.close()
    wide.close()


# ------------------------------------------------------------------------------------------- 4. the wide form on a cube

def test_wide_form_on_a_cube(device):
    """a 6-level cube table over a sparse 4-LOD atlas; listed: roots with two of four children held, held tiles of levels 2 and 3, tiles
    of the last level.  Squares of several shifts and long runs of single windows share a level, five sides are written, one is not."""
    initial, ops, listed = BC.cube_case()
    slots = Slots(device, 6, BC.CUBE_LODS, initial, spare=4 + len(ops))
    hb = bt.HeightBounds(device, 6, BC.CUBE_LEVELS).build(slots.atlas, 0)
    slots.apply(ops)
    stats, reach, before, expected = update_and_check(device, hb, slots.atlas, listed)
    assert stats["entries_written"] > BC.SMALL_FORM_MAX and stats["launches"] > 2 and stats["tiles_listed"] > BC.WIDE_THREADS
    mixes = [{s for _, s, _, _ in level} for level in reach.windows]
    assert any(0 in m and len(m - {0}) >= 2 for m in mixes), mixes
    assert {c[0] for c in reach.affected} == set(range(6)) - {BC.CUBE_UNTOUCHED}
    got = hb.read()
    for level in range(BC.CUBE_LEVELS):  # the untouched side, entry by entry, against the table before
        first = table_index(6, (BC.CUBE_UNTOUCHED, level, 0, 0))
        assert np.array_equal(got[first:first + 4 ** level], before[first:first + 4 ** level])
    hb.close()
    slots.atlas.close()


# ------------------------------------------------------------------------------------------- 5. walk-ups across levels, wide form

def test_walk_up_across_levels(device):
    """an 8-level table over LODs 0 to 2: the fill roots at level 3 own everything down to level 7; entries walk up 1 to 5 levels to a
    held LOD-2 tile, 2 to 6 where the LOD-2 tile was evicted"""
    initial, ops, listed = BC.deep_walk_case()
    slots = Slots(device, 1, 3, initial, spare=4 + len(ops))
    hb = bt.HeightBounds(device, 1, BC.DEEP_LEVELS).build(slots.atlas, 0)
    slots.apply(ops)
    stats, reach, _, _ = update_and_check(device, hb, slots.atlas, listed)
    assert stats["entries_written"] > BC.SMALL_FORM_MAX and stats["launches"] > 2
    depths = reach.depths()
    assert {d for c, d in depths.items() if c[1] >= 3} == {1, 2, 3, 4, 5, 6} and all(r[1] == 3 for r in reach.roots)
    hb.close()
    slots.atlas.close()

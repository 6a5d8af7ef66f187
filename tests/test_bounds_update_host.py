"""CPU checks of bt_height_bounds_update: the entry point's export, the stats struct's size and the NULL-table status, and a small numpy
restatement of the incremental plan (U, ancestors, fill roots, walk-up, bottom-up) against the definition, _cull_model.build_table, on
random sparse held sets with random changes.  The GPU comparisons are in test_gpu_bounds_update.py, which takes its entries_written cap
from here.  The last tests check the inputs of test_gpu_bounds_update_shapes.py (_bounds_update_cases.py): every case reaches the branch
it is named for, on the numpy plan alone."""
import ctypes as C
import os

import numpy as np

import _bounds_model as B
import _bounds_update_cases as BC
import _cull_model as M
from bevy_terrain_amd import _ffi

BT_ERR_INVALID_ARGUMENT = -1


def ancestors(c):
    side, lod, x, y = c
    while lod > 0:
        lod, x, y = lod - 1, x >> 1, y >> 1
        yield (side, lod, x, y)


def children(c):
    side, lod, x, y = c
    return [(side, lod + 1, 2 * x + (k & 1), 2 * y + (k >> 1)) for k in range(4)]


def plan(levels, listed, is_held):
    """-> (U, the ancestors of U outside U, the distinct fill roots): index arithmetic only"""
    U = list(dict.fromkeys(c for c in listed if c[1] < levels))
    in_U = set(U)
    up = list(dict.fromkeys(a for c in U for a in ancestors(c) if a not in in_U))
    roots = list(dict.fromkeys(ch for c in U for ch in children(c) if ch[1] < levels and not is_held(ch)))
    return U, up, roots


def entries_cap(levels, listed, is_held):
    """|U + ancestors(U)| + the whole subtrees, down to levels - 1, below the distinct fill roots"""
    U, up, roots = plan(levels, listed, is_held)
    return len(U) + len(up) + sum((4 ** (levels - c[1]) - 1) // 3 for c in roots)


def subtree(c, levels):
    out, frontier = [], [c]
    while frontier and frontier[0][1] < levels:
        out += frontier
        frontier = [ch for f in frontier for ch in children(f)]
    return out


def incremental_update(table, shadow, listed, own_now):
    """table: M.Table, shadow: {coord: own} of the held tiles it was computed from — both brought up to date in place.
    own_now: {coord: (min, max)} of every tile held now (only the listed ones are looked at).  -> entries recomputed"""
    levels = table.levels
    U, up, roots = plan(levels, listed, lambda c: c in own_now)
    for c in U:  # scatter
        if c in own_now:
            shadow[c] = own_now[c]
        else:
            shadow.pop(c, None)
    affected = set(U) | set(up)
    for r in roots:
        affected |= set(subtree(r, levels))

    def filled(c):  # walk up to the nearest held tile
        while c not in shadow:
            if c[1] == 0:
                return M.WHOLE_RANGE
            c = (c[0], c[1] - 1, c[2] >> 1, c[3] >> 1)
        return shadow[c]

    fill = {c: filled(c) for c in affected}  # no dependency between levels
    for lod in reversed(range(levels)):  # bottom up, children as they stand in the table
        for c in (c for c in affected if c[1] == lod):
            mn, mx = fill[c]
            if lod + 1 < levels:
                for ch in children(c):
                    e = table.data[table.index(*ch)]
                    mn, mx = min(mn, int(e[0])), max(mx, int(e[1]))
            table.data[table.index(*c)] = (mn, mx)
    return len(affected)


def as_layers(own):
    return {c: np.array([[mn, mx], [mx, mn]], np.uint16) for c, (mn, mx) in own.items()}


def random_own(rng, sides, lods, density):
    own = {}
    for side in range(sides):
        for lod in range(lods):
            for y in range(1 << lod):
                for x in range(1 << lod):
                    if rng.random() < density:
                        lo = int(rng.integers(0, 60000))
                        own[(side, lod, x, y)] = (lo, lo + int(rng.integers(0, 5000)))
    return own


def test_symbol_is_declared_everywhere():
    assert "bt_height_bounds_update" in _ffi.header_symbols() and "bt_height_bounds_update" in _ffi.PROTOTYPES
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "integration", "hip.rs")) as f:
        rust = f.read()
    assert "fn bt_height_bounds_update(" in rust and "struct bt_bounds_update_stats" in rust
    assert _ffi.lib().bt_abi_version() == 6


def test_stats_struct_is_24_bytes():
    assert C.sizeof(_ffi.BoundsUpdateStatsC) == 24
    assert _ffi.BoundsUpdateStatsC.entries_written.offset == 16 and _ffi.BoundsUpdateStatsC.launches.offset == 8


def test_null_table_is_refused_without_a_device():
    L = _ffi.lib()
    stats = _ffi.BoundsUpdateStatsC()
    assert L.bt_height_bounds_update(None, None, 0, None, 0, C.byref(stats)) == BT_ERR_INVALID_ARGUMENT
    assert b"NULL" in L.bt_last_error()
    assert L.bt_height_bounds_update(None, None, 0, None, 0, None) == BT_ERR_INVALID_ARGUMENT


def test_incremental_plan_agrees_with_the_definition():
    """a few hundred random sparse held sets; each is changed several times — ranges grow and shrink, tiles flip between held and not
    held — and after every change the table updated from the list of changed tiles equals the table built from scratch"""
    rng = np.random.default_rng(2024)
    shrank = grew = flipped = within_cap = 0
    for case in range(240):
        sides = 6 if case % 8 == 0 else 1
        levels = int(rng.integers(1, 5)) if sides == 1 else int(rng.integers(1, 4))
        lods = int(rng.integers(1, levels + 2))  # the atlas may be shallower or deeper than the table
        own = random_own(rng, sides, lods, rng.choice([0.15, 0.5, 0.9]))
        table = M.build_table(sides, levels, as_layers(own))
        shadow = {c: r for c, r in own.items() if c[1] < levels}
        for step in range(3):
            everything = [(s, l, x, y) for s in range(sides) for l in range(lods) for y in range(1 << l) for x in range(1 << l)]
            picks = [everything[i] for i in rng.choice(len(everything), size=min(len(everything), int(rng.integers(1, 6))), replace=False)]
            for c in picks:
                kind = rng.integers(0, 4)
                if c in own and kind == 0:
                    del own[c]
                    flipped += 1
                elif c in own and kind == 1:  # a narrower range inside the old one
                    lo, hi = own[c]
                    own[c] = (lo + (hi - lo) // 3, hi - (hi - lo) // 3)
                    shrank += 1
                else:
                    flipped += c not in own
                    lo = int(rng.integers(0, 60000))
                    own[c] = (lo, lo + int(rng.integers(0, 5000)))
                    grew += 1
            listed = picks + picks[:1] + [(0, levels + 1, 0, 0)]  # a duplicate and a tile below the table
            written = incremental_update(table, shadow, listed, own)
            expected = M.build_table(sides, levels, as_layers(own))
            assert np.array_equal(table.data, expected.data), (case, step, sides, levels, lods, picks)
            assert shadow == {c: r for c, r in own.items() if c[1] < levels}
            cap = entries_cap(levels, listed, lambda c: c in own)
            assert written <= cap
            within_cap += 1
    assert min(shrank, grew, flipped) > 50 and within_cap == 720


# ---- the inputs of test_gpu_bounds_update_shapes.py: every case reaches the branch it is named for, on the numpy plan alone ------------

def test_vectorised_own_ranges_are_tile_bounds_at_grid_1():
    """the big cases hand build_table own ranges computed for all layers at once: the same numbers as one tile_bounds call per layer,
    and the same table"""
    rng = np.random.default_rng(3)
    coords, layers = BC.big_initial()
    assert len(coords) == len(layers) == 21845 and layers.dtype == np.uint16 and layers.shape[1:] == (BC.T, BC.T)
    sample = np.concatenate([[0, 1, 4, 5, 20, 21, 84, 85, 21844], rng.integers(0, 21845, 48)])
    ranges = BC.own_ranges(layers)
    for i in sample:
        assert tuple(ranges[i]) == tuple(int(v) for v in B.tile_bounds(layers[i], 1)[0][0, 0, 0]), i
    assert ranges[:, 0].min() >= BC.BIG_BASE[0] and ranges[:, 1].max() <= BC.BIG_BASE[1]
    lo, hi = rng.integers(0, 60000, 40), rng.integers(0, 5000, 40)
    hi[:3] = 0  # a flat layer
    made = BC.layers_with(rng, lo, lo + hi)
    assert np.array_equal(BC.own_ranges(made), np.stack([lo, lo + hi], axis=1))
    one = BC.layer_with(rng, 17, 60001)
    assert tuple(B.tile_bounds(one, 1)[0][0, 0, 0]) == (17, 60001)
    held = {c: l for c, l in zip(coords[:85], layers[:85]) if rng.random() < 0.6}
    assert np.array_equal(M.build_table(1, 5, held).data, M.build_table(1, 5, None, own=BC.own_of(held)).data)


def check_one_writer(reach):
    entries = BC.window_entries(reach.windows)
    assert len(entries) == len(set(entries)) == reach.total and set(entries) == reach.affected


def test_sparse_scripts_reach():
    """case 1: the scripts replayed on the numpy plan equal the definition after every step, stay in the one-workgroup form, and between
    them reach the walk-ups, the whole-range entries, the nested roots and the covered listed tiles the GPU test sums up"""
    assert 12 <= len(BC.SPARSE) <= 16
    assert {lv for s, lv, _ in BC.SPARSE if s == 1} == set(range(1, 7)) and {lv for s, lv, _ in BC.SPARSE if s == 6} >= set(range(1, 5))
    assert sum(s == 6 and lv == 5 for s, lv, _ in BC.SPARSE) >= 2 and {d for _, _, d in BC.SPARSE} == {-1, 0, 1}
    seen, kinds, densities = dict(), set(), set()
    for seed in range(len(BC.SPARSE)):
        script = BC.sparse_script(seed)
        densities.add(script.density)
        table = M.build_table(script.sides, script.levels, None, own=BC.own_of(script.initial))
        shadow = {c: r for c, r in BC.own_of(script.initial).items() if c[1] < script.levels}
        assert len(script.steps) == 3
        for step, reach, held in BC.replay(script):
            own = BC.own_of(held)
            before = table.data.copy()
            written = incremental_update(table, shadow, step.listed, own)
            assert np.array_equal(table.data, M.build_table(script.sides, script.levels, None, own=own).data), seed
            assert written == reach.total == len(reach.affected) and reach.small_form and reach.launches() == 1
            check_one_writer(reach)
            assert len(step.listed) == len(set(step.listed)) + 1 and any(c[1] >= script.levels for c in step.listed)
            kinds |= set(step.kinds)
            for name, hit in BC.sparse_reach(reach, held).items():
                seen[name] = seen.get(name, 0) + hit
            seen["differs"] = seen.get("differs", 0) + (not np.array_equal(before, table.data))
    assert densities == set(BC.DENSITIES) and kinds == {"narrow", "move", "evict", "hold", "load"}
    assert all(seen[name] >= 2 for name in ("walks_two", "whole_range_beside_held", "nested_roots", "listed_under_a_root")), seen
    assert seen["differs"] == 3 * len(BC.SPARSE), seen  # every step shows something


def test_second_trip_inputs():
    """case 2: (a) more than 1024 scatter records, windows, affected entries and level-6 entries, at most 4096 in all, no fill root;
    (b) one entry and no work on any deeper level"""
    listed = BC.second_trip_list()
    reach = BC.Reach(BC.BIG_LEVELS, listed, lambda c: True)
    assert len(set(listed)) == len(listed) == 1104 and not reach.roots
    assert BC.SMALL_THREADS < reach.work[6] == len(reach.U) == 1104 and reach.work[7] == 0
    assert BC.SMALL_THREADS < reach.window_count == reach.total <= BC.SMALL_FORM_MAX and reach.launches() == 1
    assert reach.work[:6] == [1, 2, 6, 19, 69, 276]
    check_one_writer(reach)
    coords, layers = BC.big_initial()
    new, unions = BC.second_trip_layers(np.random.default_rng(1), listed, dict(zip(coords, BC.own_ranges(layers))))
    ranges = BC.own_ranges(new)
    wide, flat = ranges[0::2], ranges[1::2]  # both kinds on either side of entry 1024
    assert len({tuple(r) for r in wide}) == 552 and wide[:, 0].max() < BC.BIG_BASE[0] and wide[:, 1].min() > BC.BIG_BASE[1]
    assert (flat[:, 0] == flat[:, 1]).all() and (unions[1::2, 0] < flat[:, 0]).all() and (flat[:, 1] < unions[1::2, 1]).all()
    root = BC.Reach(BC.BIG_LEVELS, [(0, 0, 0, 0)], lambda c: True)
    assert root.total == 1 and root.work == [1] + [0] * 7 and not root.roots


def test_form_edge_arithmetic():
    """case 3: 3072 level-7 tiles and their ancestors are 4097 entries, one more than the one-workgroup form takes; without one of the
    tiles 4096, whose windows (single entries all) are exactly 65 536 bytes"""
    listed = BC.form_edge_list()
    assert len(set(listed)) == 3072 and all(c[1] == 7 for c in listed)
    wide = BC.Reach(BC.BIG_LEVELS, listed, lambda c: True)
    small = BC.Reach(BC.BIG_LEVELS, listed[:-1], lambda c: True)
    assert wide.total == 3 * 1365 + 2 == 4097 == BC.SMALL_FORM_MAX + 1 and not wide.small_form and wide.launches() == 2 + 7
    assert small.total == 4096 == BC.SMALL_FORM_MAX and small.small_form and len(small.U) == 3071
    for reach in (wide, small):
        assert not reach.roots and reach.window_count == reach.total and all(s == 0 for level in reach.windows for _, s, _, _ in level)
        check_one_writer(reach)
    assert small.window_count * 16 == 65536
    assert wide.work == [1, 1, 3, 12, 48, 192, 768, 3072] and -(-len(wide.U) // BC.WIDE_THREADS) == 12
    old = BC.big_initial()[1][:200]
    new = BC.own_ranges(BC.moved_layers(np.random.default_rng(2), old))
    assert (new != BC.own_ranges(old)).all()


def test_cube_case_reach():
    """case 4: the wide form, more than one workgroup of scatter records, a level with single windows and squares of two shifts, five
    sides affected and one untouched"""
    initial, ops, listed = BC.cube_case()
    held, loading = dict(initial), set()
    step = BC.Step()
    step.ops = ops
    BC.apply_step(held, loading, step)
    assert 0.4 < len(initial) / len(BC.pyramid(BC.CUBE_LODS, 6)) < 0.6
    reach = BC.Reach(BC.CUBE_LEVELS, listed, held.__contains__)
    assert reach.total > BC.SMALL_FORM_MAX and reach.launches() > 2 and len(reach.U) > BC.WIDE_THREADS
    check_one_writer(reach)
    mixes = [{s for _, s, _, _ in level} for level in reach.windows]
    assert any(0 in m and len(m - {0}) >= 2 for m in mixes), mixes
    assert any(sum(1 for _, s, _, _ in level if s == 0) > 64 for level in reach.windows)  # a long list for the search
    assert {c[0] for c in reach.affected} == set(range(6)) - {BC.CUBE_UNTOUCHED}
    roots_listed = [c for c in listed if c[1] == 0]
    assert len(roots_listed) >= 2 and all(0 < sum(ch in held for ch in children(c)) < 4 for c in roots_listed)
    assert {c[1] for c in listed} == {0, 2, 3, BC.CUBE_LEVELS - 1}
    last = [c for c in reach.U if c[1] == BC.CUBE_LEVELS - 1]
    under = set(reach.listed_under_a_root())
    assert any(c in under for c in last) and any(c not in under for c in last)
    depths = reach.depths()
    assert {d for d in depths.values()} >= {0, 1, 2, 3, 4}
    table = M.build_table(6, BC.CUBE_LEVELS, None, own=BC.own_of(initial))
    shadow = {c: r for c, r in BC.own_of(initial).items()}
    assert incremental_update(table, shadow, listed, BC.own_of(held)) == reach.total
    assert np.array_equal(table.data, M.build_table(6, BC.CUBE_LEVELS, None, own=BC.own_of(held)).data)


def test_deep_walk_reach():
    """case 5: fill roots at level 3 under an 8-level table; their entries walk up 1 to 5 levels below a held LOD-2 tile and 2 to 6
    below an evicted one"""
    initial, ops, listed = BC.deep_walk_case()
    held, loading = dict(initial), set()
    step = BC.Step()
    step.ops = ops
    BC.apply_step(held, loading, step)
    assert {c[1] for c in initial} == {0, 1, 2} and 0 < sum(c[1] == 2 for c in held) < 16 and all(c[1] == 2 for c in listed)
    reach = BC.Reach(BC.DEEP_LEVELS, listed, held.__contains__)
    assert reach.total > BC.SMALL_FORM_MAX and reach.launches() == 2 + 7
    assert len(reach.roots) == 4 * len(listed) and all(r[1] == 3 for r in reach.roots) and not reach.nested_roots()
    check_one_writer(reach)
    depths = reach.depths()
    below_held = {depths[c] for c in reach.affected if c[1] >= 3 and (0, 2, c[2] >> (c[1] - 2), c[3] >> (c[1] - 2)) in held}
    below_evicted = {depths[c] for c in reach.affected if c[1] >= 3 and (0, 2, c[2] >> (c[1] - 2), c[3] >> (c[1] - 2)) not in held}
    assert below_held == {1, 2, 3, 4, 5} and below_evicted == {2, 3, 4, 5, 6}
    table = M.build_table(1, BC.DEEP_LEVELS, None, own=BC.own_of(initial))
    shadow = dict(BC.own_of(initial))
    assert incremental_update(table, shadow, listed, BC.own_of(held)) == reach.total
    assert np.array_equal(table.data, M.build_table(1, BC.DEEP_LEVELS, None, own=BC.own_of(held)).data)

"""CPU checks of bt_height_bounds_update: the entry point's export, the stats struct's size and the NULL-table status, and a small numpy
restatement of the incremental plan (U, ancestors, fill roots, walk-up, bottom-up) against the definition, _cull_model.build_table, on
random sparse held sets with random changes.  The GPU comparisons are in test_gpu_bounds_update.py, which takes its entries_written cap
from here."""
import ctypes as C
import os

import numpy as np

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
    up = list(dict.fromkeys(a for c in U for a in ancestors(c) if a not in set(U)))
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

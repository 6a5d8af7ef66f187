"""The inputs of test_gpu_bounds_update_shapes.py, built on the CPU: held sets, contents and lists of changed tiles chosen so that
bt_height_bounds_update takes a named branch (a second trip of the one-workgroup form's loops, the edge between the two forms, the wide
form on a cube with mixed windows, walk-ups over several levels), and the numpy restatement of what the host plan makes of a list: the
affected entries, the windows per level and the walk-up depths.  Whether a case reaches its branch is asserted from these alone, in
test_bounds_update_host.py without a GPU and again by the GPU test next to the device's stats.

A tile's contents are a (T, T) uint16 layer, T = 16 (b = 2: the grid-1 reduction takes the whole layer, border included)."""
import numpy as np

import _cull_model as M
import test_bounds_update_host as H  # ancestors, children, plan, subtree: used at call time only (the two modules import each other)

T = 16
SMALL_FORM_MAX = 4096   # kBoundsUpdateSmall: affected entries up to which one workgroup does the table work
SMALL_THREADS = 1024    # kSmallThreads: a loop of the one-workgroup form takes a second trip above this
WIDE_THREADS = 256      # kWideThreads


# ---- contents ---------------------------------------------------------------------------------------------------------------------

def layer_with(rng, lo, hi):
    """a layer whose range is exactly (lo, hi), the two extremes at random texels (border and corners included)"""
    a = rng.integers(lo, hi + 1, (T, T)).astype(np.uint16)
    at = rng.choice(T * T, 2, replace=False)
    a.flat[at[0]], a.flat[at[1]] = lo, hi
    return a


def layers_with(rng, lo, hi):
    """layer_with for arrays lo, hi of n ranges -> (n, T, T)"""
    lo, hi = np.asarray(lo, np.int64), np.asarray(hi, np.int64)
    n = len(lo)
    a = (lo[:, None] + rng.integers(0, 1 << 30, (n, T * T)) % (hi - lo + 1)[:, None]).astype(np.uint16)
    at = rng.integers(0, T * T, n)
    a[np.arange(n), at] = lo
    a[np.arange(n), (at + 1 + rng.integers(0, T * T - 1, n)) % (T * T)] = hi
    return a.reshape(n, T, T)


def own_ranges(layers):
    """the own range of every layer at once: min and max over the whole layer -> (n, 2) int"""
    layers = np.asarray(layers).reshape(len(layers), -1)
    return np.stack([layers.min(axis=1), layers.max(axis=1)], axis=1).astype(np.int64)


def own_of(held):
    """{coord: layer} -> {coord: (min, max)}"""
    if not held:
        return {}
    r = own_ranges(np.stack(list(held.values())))
    return {c: (int(mn), int(mx)) for c, (mn, mx) in zip(held, r)}


def pyramid(levels, sides=1):
    """every coordinate of a full pyramid, level by level, rows first (the order the big atlas allocates in)"""
    return [(s, l, x, y) for l in range(levels) for s in range(sides) for y in range(1 << l) for x in range(1 << l)]


# ---- the plan, restated ---------------------------------------------------------------------------------------------------------------

def affected(levels, listed, is_held):
    """-> (U, up, roots, every affected entry): U + its ancestors + the whole subtrees below the fill roots, each entry once"""
    U, up, roots = H.plan(levels, listed, is_held)
    out = set(U) | set(up)
    for r in roots:
        out |= set(H.subtree(r, levels))
    return U, up, roots, out


def windows(levels, U, up, roots):
    """the windows of every level as (side, shift, x0, y0): a single entry (shift 0) for each tile of U and its ancestors that no fill
    root covers, and for each fill root outside every other root's subtree the square it covers on each level below it"""
    rootset = set(roots)

    def covered(c, itself):
        return (itself and c in rootset) or any(a in rootset for a in H.ancestors(c))

    per = [[] for _ in range(levels)]
    for c in list(U) + list(up):
        if not covered(c, True):
            per[c[1]].append((c[0], 0, c[2], c[3]))
    for r in roots:
        if not covered(r, False):
            for lod in range(r[1], levels):
                s = lod - r[1]
                per[lod].append((r[0], s, r[2] << s, r[3] << s))
    return per


def level_work(per):
    return [sum(4 ** s for _, s, _, _ in level) for level in per]


def window_entries(per):
    """every entry the windows write, with repeats if two windows overlap"""
    return [(side, lod, x0 + dx, y0 + dy) for lod, level in enumerate(per) for side, s, x0, y0 in level for dy in range(1 << s) for dx in range(1 << s)]


def walk_depth(c, is_held):
    """levels from c up to its nearest held ancestor (0: c is held itself), None: there is none and c takes the whole range"""
    depth = 0
    while not is_held(c):
        if c[1] == 0:
            return None
        c, depth = (c[0], c[1] - 1, c[2] >> 1, c[3] >> 1), depth + 1
    return depth


class Reach:
    """what one update reaches, from the plan alone"""

    def __init__(self, levels, listed, is_held):
        self.levels = levels
        self.U, self.up, self.roots, self.affected = affected(levels, listed, is_held)
        self.windows = windows(levels, self.U, self.up, self.roots)
        self.work = level_work(self.windows)
        self.total = sum(self.work)
        self.window_count = sum(len(w) for w in self.windows)
        self.small_form = self.total <= SMALL_FORM_MAX
        self.is_held = is_held

    def depths(self):
        return {c: walk_depth(c, self.is_held) for c in self.affected}

    def nested_roots(self):
        rootset = set(self.roots)
        return [r for r in self.roots if any(a in rootset for a in H.ancestors(r))]

    def listed_under_a_root(self):
        rootset = set(self.roots)
        return [u for u in self.U if u in rootset or any(a in rootset for a in H.ancestors(u))]

    def launches(self):
        """the table kernels' launches (the reduction of the held listed tiles comes on top)"""
        return 1 if self.small_form else 2 + sum(1 for w in self.work[:-1] if w)


# ---- case 1: random sparse held sets, the one-workgroup form --------------------------------------------------------------------------

class Step:
    def __init__(self):
        self.ops = []     # (kind, coord, layer): "upload" new contents of a held tile, "hold" a tile that is not, "evict", "load"
        self.listed = []  # what the update is given
        self.kinds = []


class Script:
    def __init__(self, sides, levels, lods, density, initial, steps):
        self.sides, self.levels, self.lods, self.density, self.initial, self.steps = sides, levels, lods, density, initial, steps


#        (sides, levels, atlas lods - levels)
SPARSE = [(1, 1, 1), (1, 2, 1), (1, 3, 0), (1, 4, -1), (1, 5, 0), (1, 6, 0), (1, 6, -1), (1, 4, 1),
          (6, 1, 1), (6, 2, 0), (6, 3, -1), (6, 4, 0), (6, 5, 0), (6, 5, -1)]
DENSITIES = (0.15, 0.5, 0.9)


def apply_step(held, loading, step):
    """the model of what the ops do to the atlas: held {coord: layer} and the loading set, in place"""
    for kind, c, layer in step.ops:
        if kind in ("upload", "hold"):
            held[c] = layer
        else:
            held.pop(c, None)
            if kind == "load":
                loading.add(c)


def sparse_script(seed):
    sides, levels, delta = SPARSE[seed]
    rng = np.random.default_rng(1000 + seed)
    lods = max(1, levels + delta)
    density = DENSITIES[seed % 3]
    initial = {c: layer_with(rng, lo, lo + int(rng.integers(0, 5000))) for c in pyramid(lods, sides) if rng.random() < density
               for lo in [int(rng.integers(0, 60000))]}
    held, loading, steps = dict(initial), set(), []
    everything = pyramid(lods, sides)
    while len(steps) < 3:
        step = Step()
        picks = [everything[i] for i in rng.choice(len(everything), size=min(len(everything), int(rng.integers(2, 7))), replace=False)]
        for c in list(picks):  # a tile and one below it in the same list: roots inside roots, listed tiles under a root
            below = [d for d in H.children(c) if d[1] < lods]
            if below and rng.random() < 0.4:
                d = below[int(rng.integers(0, 4))]
                picks.append(d)
                deeper = [e for e in H.children(d) if e[1] < lods]
                if deeper and rng.random() < 0.4:
                    picks.append(deeper[int(rng.integers(0, 4))])
        picks = [c for c in dict.fromkeys(picks) if c not in loading] or [c for c in everything if c not in loading][:1]
        loads = 0
        for c in picks:
            kind = int(rng.integers(0, 5))
            if kind == 3:  # at most one tile per step is left loading: it is not picked again
                loads += 1
                kind = 3 if loads == 1 else 4
            lo = int(rng.integers(0, 60000))
            moved = layer_with(rng, lo, lo + int(rng.integers(0, 5000)))
            if c in held:
                mn, mx = own_of({c: held[c]})[c]
                if kind == 0:
                    op = ("upload", c, layer_with(rng, mn + (mx - mn) // 3, mx - (mx - mn) // 3))
                    step.kinds.append("narrow")
                elif kind in (1, 4):
                    op = ("upload", c, moved)
                    step.kinds.append("move")
                else:
                    op = ("evict" if kind == 2 else "load", c, None)
                    step.kinds.append(op[0])
            elif kind == 3:
                op = ("load", c, None)
                step.kinds.append("load")
            else:
                op = ("hold", c, moved)
                step.kinds.append("hold")
            step.ops.append(op)
        step.listed = picks + picks[:1] + [(0, levels + 1, 1, 1)]  # a duplicate and a tile below the table
        after, after_loading = dict(held), set(loading)
        apply_step(after, after_loading, step)
        if np.array_equal(M.build_table(sides, levels, None, own=own_of(held)).data, M.build_table(sides, levels, None, own=own_of(after)).data):
            continue  # the step would show nothing (a narrower range under wider children, say): drawn again
        held, loading = after, after_loading
        steps.append(step)
    return Script(sides, levels, lods, density, initial, steps)


# ---- cases 2 and 3: the full 8-level planar pyramid -------------------------------------------------------------------------------

BIG_LEVELS = 8
BIG_BASE = (20000, 40000)  # every layer the big atlas starts with lies inside


def big_initial(seed=77):
    """-> (coords, layers): 21 845 tiles, every range inside BIG_BASE"""
    rng = np.random.default_rng(seed)
    coords = pyramid(BIG_LEVELS)
    lo = rng.integers(BIG_BASE[0], BIG_BASE[1] - 2000, len(coords))
    return coords, layers_with(rng, lo, lo + rng.integers(0, 2000, len(coords)))


def second_trip_list():
    """case 2(a): the 1104 level-6 tiles below 69 level-4 tiles (more than one row of level 4, so the ancestors fan out)"""
    tops = [(0, 4, i % 16, i // 16) for i in range(69)]
    return [(0, 6, 4 * x + dx, 4 * y + dy) for _, _, x, y in tops for dy in range(4) for dx in range(4)]


def widened_layers(rng, n):
    """ranges that reach beyond BIG_BASE at both ends, all different: an entry whose own is one of these is that range exactly"""
    lo = rng.permutation(np.arange(1000, 1000 + 4 * n, 4))[:n]
    hi = rng.permutation(np.arange(41000, 41000 + 4 * n, 4))[:n]
    return layers_with(rng, lo, hi)


def second_trip_layers(rng, listed, own):
    """new contents for case 2(a), own: {coord: (min, max)} of the atlas as it stands.  Every other tile gets a widened range (the entry
    becomes exactly that range: the scatter and the fill show), the ones between a flat layer strictly inside the union of their
    children's ranges (the entry is that union: only the unite with the children gives it) -> (layers, the children's unions)"""
    layers = widened_layers(rng, len(listed))
    unions = np.array([[min(own[ch][0] for ch in H.children(c)), max(own[ch][1] for ch in H.children(c))] for c in listed])
    middle = (unions[:, 0] + unions[:, 1]) // 2
    layers[1::2] = middle[1::2, None, None]
    return layers, unions


FORM_EDGE_TOPS = [(0, 2, 0, 0), (0, 2, 1, 0), (0, 2, 1, 1)]  # three of the four children of (0, 1, 0, 0)


def form_edge_list():
    """case 3: the 3072 level-7 tiles below FORM_EDGE_TOPS; with their ancestors 3 * 1365 + 2 = 4097 entries, single windows all"""
    return [(0, 7, (x << 5) + dx, (y << 5) + dy) for _, _, x, y in FORM_EDGE_TOPS for dy in range(32) for dx in range(32)]


def moved_layers(rng, old_layers):
    """new contents whose range differs from the old one in both ends, for every layer"""
    old = own_ranges(old_layers)
    lo = rng.integers(2000, 60000, len(old))
    lo = np.where(lo == old[:, 0], lo + 1, lo)
    hi = lo + rng.integers(0, 3000, len(old))
    hi = np.where(hi == old[:, 1], hi + 1, hi)
    return layers_with(rng, lo, hi)


# ---- case 4: the wide form on a cube, mixed windows ----------------------------------------------------------------------------------

CUBE_LEVELS, CUBE_LODS = 6, 4
CUBE_UNTOUCHED = 4  # the side no listed tile lies on


def cube_case(seed=5):
    """-> (initial {coord: layer}, ops, listed).  A sparse cube atlas of 4 LODs, about half of it held.  Listed: the roots of the five
    other sides (their children are partly not held: fill roots at level 1, squares of shifts 0 to 4), the held tiles of levels 2 and 3
    (fill roots at levels 3 and 4), and tiles of the last level, some below a fill root and some not."""
    rng = np.random.default_rng(seed)
    initial = {}
    for c in pyramid(CUBE_LODS, 6):
        keep = rng.random() < 0.5
        if c[1] == 1:  # two children of every root held, two not
            keep = (c[2] + c[3]) % 2 == (c[0] % 2)
        if keep:
            lo = int(rng.integers(10000, 50000))
            initial[c] = layer_with(rng, lo, lo + int(rng.integers(0, 4000)))
    sides = [s for s in range(6) if s != CUBE_UNTOUCHED]
    listed = [(s, 0, 0, 0) for s in sides]
    listed += [c for c in initial if c[0] in sides and c[1] in (2, 3)]
    n = 1 << (CUBE_LEVELS - 1)
    last = [(s, CUBE_LEVELS - 1, int(x), int(y)) for s in sides for x, y in rng.integers(0, n, (24, 2))]
    listed += list(dict.fromkeys(last))
    ops = []
    for c in listed:
        if c in initial:
            lo = int(rng.integers(100, 60000))
            ops.append(("upload", c, layer_with(rng, lo, lo + int(rng.integers(0, 5000)))))
        elif c[1] == 0:
            ops.append(("hold", c, layer_with(rng, 30000, 30100)))
    return initial, ops, listed


# ---- case 5: walk-ups over several levels in the wide form ---------------------------------------------------------------------------

DEEP_LEVELS = 8


def deep_walk_case(seed=9):
    """-> (initial, ops, listed): an atlas of LODs 0 to 2 under an 8-level table, fourteen of the sixteen LOD-2 tiles held.  Listed:
    twelve LOD-2 tiles, eight that get new contents and four that are evicted.  The fill roots are their children at level 3; an entry
    of level l below a held one walks up l - 2 levels (1 to 5), below an evicted one l - 1 (its LOD-1 ancestor is held)."""
    rng = np.random.default_rng(seed)
    finest = [(0, 2, x, y) for y in range(4) for x in range(4)]
    held2 = [finest[i] for i in (0, 1, 2, 4, 5, 6, 7, 8, 10, 11, 12, 13, 14, 15)]
    initial = {}
    for c in pyramid(2) + held2:
        lo = int(rng.integers(10000, 50000))
        initial[c] = layer_with(rng, lo, lo + int(rng.integers(0, 3000)))
    changed, evicted = held2[:8], held2[9:13]
    ops = [("evict", c, None) for c in evicted]
    for c in changed:
        lo = int(rng.integers(100, 60000))
        ops.append(("upload", c, layer_with(rng, lo, lo + int(rng.integers(0, 5000)))))
    return initial, ops, changed + evicted


# ---- what the tests on both sides walk through -----------------------------------------------------------------------------------------

def replay(script):
    """-> per step (step, its Reach, the held tiles after it {coord: layer})"""
    held, loading = dict(script.initial), set()
    for step in script.steps:
        apply_step(held, loading, step)
        now = dict(held)
        yield step, Reach(script.levels, step.listed, now.__contains__), now


def apart(a, b):
    """two tiles on different sides, or in different quadrants of one side"""
    if a[0] != b[0]:
        return True
    return a[1] > 0 and b[1] > 0 and (a[2] >> (a[1] - 1), a[3] >> (a[1] - 1)) != (b[2] >> (b[1] - 1), b[3] >> (b[1] - 1))


def sparse_reach(reach, held):
    """the four conditions case 1 sums over its seeds -> a dict of booleans for one step"""
    depths = reach.depths()
    inside = [h for h in held if h[1] < reach.levels]
    return dict(walks_two=any(d is not None and d >= 2 for d in depths.values()),
                whole_range_beside_held=any(d is None and any(apart(c, h) for h in inside) for c, d in depths.items()),
                nested_roots=bool(reach.nested_roots()),
                listed_under_a_root=bool(reach.listed_under_a_root()))

"""No GPU: the model of the terrain geometry (tests/_geometry_model.py) pinned against things that are not the model, and what
test_gpu_geometry.py assumes of its scenes (tests/_geometry_cases.py).

The model: the strip's slot order against the strip written out as triangles; shared edges of neighbours; full morph lands on the even
grid; every lookup's height against the oracle's tile sample; flat terrains against the closed form; invalid entries give min_height.
The scenes: the union of their traces reaches every value the GPU comparison is there for — coordinate_change_lod up, down and not at all
for either lookup, the second lookup taken and not, morph ratio 0, between and 1, own, ancestor's and no entry, every cube side — and at
most 1 vertex in 1000 is inadmissible (a log2 two doubles away would change one of its bits; both sides use this machine's libm here: the
rule is about the device's).
The long lists of test_gpu_geometry_trips.py: their lengths against 1024, 2048 and the chunk sizes the header's rule gives, tiles one and two
trips apart and on either side of a chunk boundary different in LOD or side and in the model's positions, the oracle's prepass list on the
9-LOD tree longer than 1024, the same cap on inadmissible vertices."""
import numpy as np
import pytest

import _geometry_cases as GC
import _geometry_model as GM
import _oracle as O

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the layouts -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("g", [4, 5, 16])
def test_strip_order(g):
    """a tile's strip, written out: per column the zigzag (col, 0), (col + 1, 0), (col, 1), (col + 1, 1) ... (col + 1, g), with its first and
    its last vertex twice so that consecutive columns are joined by degenerate triangles"""
    strip = []
    for col in range(g):
        zigzag = [(col + (i & 1), i >> 1) for i in range(2 * (g + 1))]
        strip += [zigzag[0]] + zigzag + [zigzag[-1]]
    cx, cy = GM.strip_map(g)
    assert list(zip(cx.tolist(), cy.tolist())) == strip and len(strip) == 2 * g * (g + 2)
    assert set(strip) == {(x, y) for x in range(g + 1) for y in range(g + 1)}  # every grid vertex
    vpr = 2 * (g + 2)
    doubled = [i for i in range(1, len(strip)) if strip[i] == strip[i - 1]]
    assert doubled == sorted([col * vpr + 1 for col in range(g)] + [col * vpr + vpr - 1 for col in range(g)])  # exactly the row ends
    # every triangle of the strip that is not degenerate is a half cell
    for i in range(len(strip) - 2):
        a, b, c = strip[i:i + 3]
        if len({a, b, c}) == 3 and i // vpr == (i + 2) // vpr:
            assert max(p[0] for p in (a, b, c)) - min(p[0] for p in (a, b, c)) == 1 and max(p[1] for p in (a, b, c)) - min(p[1] for p in (a, b, c)) == 1
    # the strip layout is the GRID layout under that map
    c = GC.scene("planar", g) if g in GC.GRIDS else None
    if c is not None:
        strip_v, _, strip_a = GC.expected("planar", g, True, 0, 0)
        grid_v, _, grid_a = GC.expected("planar", g, True, 0, GM.GRID)
        assert grid_v.shape == (len(c.tiles), (g + 1) ** 2) and strip_v.shape == (len(c.tiles), len(strip))
        assert strip_v.tobytes() == grid_v[:, cy * (g + 1) + cx].tobytes() and np.array_equal(strip_a, grid_a[:, cy * (g + 1) + cx])


@pytest.mark.parametrize("g", [4, 5, 12, 16])
def test_neighbours_share_their_edge(g):
    """two tiles of one LOD side by side, NO_MORPH, planar: the vertices along the shared edge have bit-equal world positions"""
    c = GC.scene("planar", g)
    tiles = np.array([(0, 2, 1, 1), (0, 2, 2, 1), (0, 2, 1, 2), (0, 3, 4, 3), (0, 3, 5, 3)], np.uint32)
    _, trace, _ = GM.geometry(c.views[0], c.P, c.entries, c.layers, GC.T, GC.B, tiles, GM.GRID | GM.NO_MORPH)
    world = trace["world"].reshape(len(tiles), g + 1, g + 1, 3)  # [tile][cy][cx]
    assert bits(world[0][:, g]).tobytes() == bits(world[1][:, 0]).tobytes()  # x neighbours
    assert bits(world[0][g, :]).tobytes() == bits(world[2][0, :]).tobytes()  # y neighbours
    assert bits(world[3][:, g]).tobytes() == bits(world[4][:, 0]).tobytes()
    assert (world[0][:, g, 0] > world[0][:, 0, 0]).all()


# ---- morph -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,g", [("planar", 4), ("planar", 5), ("sphere", 12), ("ellipsoid", 16)])
def test_full_morph_lands_on_the_even_grid(kind, g):
    """the far view: morph ratio 1 on every tile below LOD 0, and every vertex of such a tile lies, bit for bit, where a vertex of the even
    grid of that tile lies without morphing; where g is a power of two that is vertex (cx & ~1, cy & ~1)"""
    c = GC.scene(kind, g)
    morphed, trace, _ = GM.geometry(c.views[2], c.P, c.entries, c.layers, GC.T, GC.B, c.tiles, GM.GRID)
    unmorphed, plain, _ = GM.geometry(c.views[2], c.P, c.entries, c.layers, GC.T, GC.B, c.tiles, GM.GRID | GM.NO_MORPH)
    fine = c.tiles[:, 1] > 0
    assert fine.sum() >= 20 and (trace["morph"][fine] == GM.MORPH_ONE).all() and (trace["morph"][~fine] == GM.MORPH_ZERO).all()
    row = g + 1
    even = np.array([cy * row + cx for cy in range(0, row, 2) for cx in range(0, row, 2)])
    for t in np.flatnonzero(fine):
        on_even = {bits(w).tobytes() for w in plain["world"][t][even]}
        assert all(bits(w).tobytes() in on_even for w in trace["world"][t]), (kind, g, t)
    if g & (g - 1) == 0:
        cy, cx = np.divmod(np.arange(row * row), row)
        assert bits(trace["world"][fine]).tobytes() == bits(plain["world"][fine][:, (cy & ~1) * row + (cx & ~1)]).tobytes()
    assert bits(trace["world"][~fine]).tobytes() == bits(plain["world"][~fine]).tobytes()  # LOD 0 never morphs
    assert (morphed["coordinate_uv"][fine] != unmorphed["coordinate_uv"][fine]).any()


# ---- heights -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", list(GC.MODELS))
def test_lookup_heights_equal_the_oracles_tile_sample(kind):
    """per lookup: h = mix(min_height, max_height, the oracle's sample of that layer at that uv); an invalid entry gives min_height"""
    c = GC.scene(kind, 4)
    lo, hi = c.P.min_height, c.P.max_height
    checked = 0
    for view in range(2):
        vertices, trace, _ = GC.expected(kind, 4, True, view, GM.GRID)
        for k, taken in (("0", np.ones_like(trace["second"])), ("1", trace["second"])):
            state, index, uv, h = trace["state" + k][taken], trace["index" + k][taken], trace["uv" + k][taken], trace["h" + k][taken]
            assert (h[state == GM.NO_ENTRY] == lo).all()
            for i in np.flatnonzero(state != GM.NO_ENTRY):
                value = O.sample_tile(O.FORMAT_R16, GC.B, c.layers[int(index[i])], uv[i])[0]
                assert bits(h[i]) == bits(lo * (F(1.0) - value) + hi * value), (kind, view, k, i)
                checked += 1
        # the blended height, and the displacement along the mesh normal
        h0, h1, r = trace["h0"], trace["h1"], vertices["blend_ratio"]
        assert np.array_equal(bits(vertices["height"]), bits(np.where(r > 0, h0 * (F(1.0) - r) + h1 * r, h0)))
        assert np.array_equal(bits(vertices["position"]), bits(trace["world"] + vertices["height"][..., None] * vertices["normal"]))
    assert checked >= 300


@pytest.mark.parametrize("kind", list(GC.MODELS))
def test_flat_terrain_gives_the_closed_form(kind):
    """one flat layer that every entry names: the height is mix(min, max, v / 65535) everywhere; a planar terrain is the plane y = position.y
    + height exactly, a sphere has that radius (within the rounding of binary32 coordinates of this size: 4 m at 9.4e6 m, ulp 1 m)"""
    c = GC.scene(kind, 5)
    raw = 40000
    entries = np.zeros_like(c.entries)  # (atlas index 0, atlas LOD 0) for every node
    layers = {0: np.full((GC.T, GC.T), raw, np.uint16)}
    value = F(raw) / F(65535.0)
    height = c.P.min_height * (F(1.0) - value) + c.P.max_height * value
    for view in c.views:
        v, trace, _ = GM.geometry(view, c.P, entries, layers, GC.T, GC.B, c.tiles, 0)
        assert (trace["state0"] != GM.NO_ENTRY).all()
        assert (np.abs(v["height"] - height) <= np.spacing(height) * 2).all()  # (a blend of two equal heights may round once more)
        centre = np.array(c.model.translation, np.float64)
        if kind == "planar":
            assert np.array_equal(bits(v["position"][..., 1]), bits(F(centre[1]) + v["height"])) and (v["normal"] == (0.0, 1.0, 0.0)).all()
        elif kind == "sphere":
            radius = np.linalg.norm(v["position"].astype(np.float64) - centre, axis=-1)
            assert np.abs(radius - (GC.R + float(height))).max() < 4.0
            assert np.abs(np.linalg.norm(v["normal"].astype(np.float64), axis=-1) - 1.0).max() < 3e-7
        else:  # the ellipsoid: between the two axes, displaced outwards
            radius = np.linalg.norm(v["position"].astype(np.float64) - centre, axis=-1)
            assert (radius > GC.MINOR + float(height) - 4.0).all() and (radius < 6378137.0 + float(height) + 4.0).all()


@pytest.mark.parametrize("kind", ["planar", "sphere"])
def test_nothing_loaded_gives_min_height(kind):
    for view in range(3):
        v, trace, admissible = GC.expected(kind, 4, False, view, 0 if kind == "planar" else GM.GRID)
        lo = GC.scene(kind, 4).P.min_height
        assert (trace["state0"] == GM.NO_ENTRY).all() and (trace["h0"] == lo).all() and (trace["h1"] == lo).all()
        single = v["blend_ratio"] == 0
        assert single.any() and (v["height"][single] == lo).all()
        assert (np.abs(v["height"] - lo) <= 2 * np.spacing(np.abs(lo))).all()  # (mix(lo, lo, r) may round once in each product)


# ---- the scenes of the GPU test ----------------------------------------------------------------------------------------------------------

def test_tables_have_every_kind_of_entry():
    for kind in GC.MODELS:
        _, loaded, entries, coords = GC.table(kind)
        known = coords[:, 1] != GM.INVALID
        depth = coords[known, 1].astype(np.int64) - entries[known, 1].astype(np.int64)
        invalid = entries[known, 1] == GM.INVALID
        assert invalid.any() and (depth[~invalid] == 0).any() and (depth[~invalid] == 1).any() and (depth[~invalid] == 2).any(), kind
        assert set(loaded) <= set(GC.oracle_tiles(kind)) and not set(loaded) & GC.missing(kind)


def test_scenes_reach_every_trace_value():
    reached = {kind: {name: set() for name in ("dir0", "dir1", "second", "morph", "state0", "state1", "side")} for kind in GC.MODELS}
    grids, layouts, stages, unloaded = set(), set(), set(), set()
    inadmissible = total = 0
    for kind, grid, loaded, flags in GC.COMPARED:
        grids.add(grid)
        layouts.add(flags & GM.GRID)
        stages.add(flags & (GM.NO_MORPH | GM.NO_BLEND))
        if not loaded:
            unloaded.add(kind)
        for view in range(3):
            _, trace, admissible = GC.expected(kind, grid, loaded, view, flags)
            inadmissible, total = inadmissible + int((~admissible).sum()), total + admissible.size
            r = reached[kind]
            second = trace["second"]
            r["second"] |= set(np.unique(second).tolist())
            r["dir0"] |= set(np.unique(trace["dir0"]).tolist())
            r["dir1"] |= set(np.unique(trace["dir1"][second]).tolist())
            r["morph"] |= set(np.unique(trace["morph"]).tolist())
            r["state0"] |= set(np.unique(trace["state0"]).tolist())
            r["state1"] |= set(np.unique(trace["state1"][second]).tolist())
            r["side"] |= set(np.unique(trace["side"]).tolist())
    assert grids == set(GC.GRIDS) and layouts == {0, GM.GRID} and stages == {0, GM.NO_MORPH, GM.NO_BLEND, GM.NO_MORPH | GM.NO_BLEND} and unloaded
    for kind, r in reached.items():
        print(kind, r)
        assert r["dir0"] == {GM.UP, GM.NONE, GM.DOWN} and r["dir1"] == {GM.UP, GM.NONE, GM.DOWN}, (kind, r)
        assert r["second"] == {False, True} and r["morph"] == {GM.MORPH_ZERO, GM.MORPH_BETWEEN, GM.MORPH_ONE}, (kind, r)
        assert r["state0"] == {GM.OWN, GM.ANCESTOR, GM.NO_ENTRY} and {GM.OWN, GM.ANCESTOR} <= r["state1"], (kind, r)
        assert r["side"] == ({0} if kind == "planar" else set(range(6))), (kind, r)
    print("vertices", total, "inadmissible", inadmissible)
    assert inadmissible * 1000 <= total


def test_admissibility_flag():
    """a blend log2 planted within two doubles of an f32 rounding boundary is flagged where the f32 matters (inside a blend ring), and
    nothing else is; the same for the morph's"""
    c = GC.scene("planar", 4)
    tiles = c.tiles[:21]
    args = (c.views[0], c.P, c.entries, c.layers, GC.T, GC.B, tiles, GM.GRID)
    logs = {}
    vertices, trace, admissible = GM.geometry(*args, logs=logs)
    assert admissible.all() and set(logs) == {"m", "b"}
    halfway = lambda x: (float(F(x)) + float(np.nextafter(F(x), F(np.inf)))) / 2.0  # between two neighbouring floats: rounds either way
    ring = np.flatnonzero(((vertices["blend_ratio"] > 0) & (vertices["blend_ratio"] < 1)).ravel())
    between = np.flatnonzero((trace["morph"] == GM.MORPH_BETWEEN).ravel())
    assert len(ring) >= 4 and len(between) >= 4
    for key, at in (("b", ring[1]), ("m", between[2])):
        planted = {k: v.copy() for k, v in logs.items()}
        planted[key][at] = np.nextafter(halfway(planted[key][at]), 0.0)  # one double below the boundary
        _, _, flagged = GM.geometry(*args, logs=planted)
        assert not flagged.ravel()[at] and flagged.sum() == flagged.size - 1, (key, at)
        planted[key][at] = float(F(logs[key][at]))  # the middle of its rounding interval
        assert GM.geometry(*args, logs=planted)[2].all()


# ---- the long lists of test_gpu_geometry_trips.py ------------------------------------------------------------------------------------------

def position_rows(vertices):
    """per tile, the bits of every vertex's position"""
    return bits(vertices["position"]).reshape(len(vertices), -1)


def assert_list_conditions(tiles, launches):
    """what makes a vertex written to another trip's slots, or a chunk that began again at the list's head, differ from the expected one in
    more than tile_index: tiles one and two trips apart are of different LOD or side, the tiles on either side of a chunk boundary differ,
    and so do the list's first tile and the first of every later chunk"""
    count = len(tiles)
    for step in (GC.TRIP, 2 * GC.TRIP):
        a, b = tiles[:max(0, count - step)], tiles[step:]
        assert ((a[:, 0] != b[:, 0]) | (a[:, 1] != b[:, 1])).all(), step
    assert sum(launches) == count
    for c in np.cumsum(launches)[:-1]:
        assert (tiles[c - 1] != tiles[c]).any() and (tiles[0] != tiles[c]).any(), c


def test_long_lists_reach_later_trips_and_chunk_boundaries():
    by_hand = {(16, 0): 1213, (32, 0): 321, (32, GM.GRID): 641, (4, 0): 14563}
    for (grid, flags), chunk in by_hand.items():
        slots = (grid + 1) ** 2 if flags & GM.GRID else 2 * grid * (grid + 2)
        assert max(1, (32 << 20) // (slots * 48)) == chunk == GC.chunk_tiles(grid, flags)
    reached = []
    for kind, grid, flags, count, launches in GC.LONG:
        tiles = GC.long_tiles(kind, count)
        assert tiles.shape == (count, 4) and launches == GC.launches_of(grid, flags, count)
        # every tile of the scene, the same number of times +- 1
        rows = GC.long_index(kind, count)
        times = np.bincount(rows, minlength=len(GC.tiles(kind)))
        assert times.max() - times.min() <= 1 and times.min() >= 1 and np.array_equal(tiles, GC.tiles(kind)[rows])
        assert_list_conditions(tiles, launches)
        # what a launch of n tiles reaches: min(n, 1024) workgroups, of which n - 1024 take a second trip and n - 2048 a third
        reached.append(tuple((n, min(n, GC.TRIP), max(0, min(n - GC.TRIP, GC.TRIP)), max(0, n - 2 * GC.TRIP)) for n in launches))
        exp, admissible = GC.long_expected(kind, grid, 0, flags, count)
        assert exp.shape == (count, GC.slots_of(grid, flags)) and np.array_equal(exp["tile_index"][:, 0], np.arange(count))
        position = position_rows(exp)
        for step in (GC.TRIP, 2 * GC.TRIP):  # a tile written by the wrong trip is seen in its positions
            if count > step:
                assert (position[:count - step] != position[step:]).any(axis=1).all(), (kind, grid, step)
        for c in np.cumsum(launches)[:-1]:  # and so is a chunk that began again at the head of the list
            assert (position[0] != position[c]).any() and (position[c - 1] != position[c]).any()
        skipped = int((~admissible).sum())
        print(kind, grid, flags, count, "vertices", admissible.size, "inadmissible", skipped)
        assert skipped * 1000 <= admissible.size
    assert reached == [((2060, 1024, 1024, 12),), ((1025, 1024, 1, 0),), ((1024, 1024, 0, 0),), ((1213, 1024, 189, 0), (87, 87, 0, 0)), ((321, 321, 0, 0), (9, 9, 0, 0)),
                       ((641, 641, 0, 0), (641, 641, 0, 0), (8, 8, 0, 0))]
    assert (16 + 1) ** 2 > 256  # the 1300-tile case: a second trip of the thread loop inside a workgroup's second trip


def test_deep_scene_gives_the_device_form_a_list_longer_than_1024():
    """the oracle's prepass list on the 9-LOD tree at the near view (measured: 1416 tiles on the sphere, LODs 2 .. 8, 1415 on the ellipsoid):
    more than one trip of the device form's 1024 workgroups, fewer than three; the cut capacities of the GPU test lie where they claim"""
    lengths = {}
    for kind in ("sphere", "ellipsoid"):
        c = GC.deep_scene(kind)
        n = lengths[kind] = len(c.tiles)
        assert GC.TRIP < n <= 2 * GC.TRIP and n <= GC.DEEP_KW["geometry_tile_count"] and c.tiles[:, 1].max() < GC.DEEP_LODS
        assert c.indirect[0] == n * 48 and len(np.unique(c.tiles, axis=0)) == n  # (grid 4: 48 strip slots a tile)
        for flags in (0, GM.GRID):
            exp, trace, admissible = GC.deep_expected(kind, flags)
            assert (trace["state0"] == GM.NO_ENTRY).all()
            position = position_rows(exp)
            assert (position[:n - GC.TRIP] != position[GC.TRIP:]).any(axis=1).all()
            print(kind, flags, "tiles", n, "by LOD", np.bincount(c.tiles[:, 1], minlength=GC.DEEP_LODS).tolist(), "inadmissible", int((~admissible).sum()))
            assert (~admissible).sum() * 1000 <= admissible.size
    assert lengths == {"sphere": 1416, "ellipsoid": 1415}
    assert np.bincount(GC.deep_scene("sphere").tiles[:, 1], minlength=GC.DEEP_LODS).tolist() == [0, 0, 27, 190, 266, 235, 233, 233, 232]
    # the cuts: tile c is the first left out
    n, slots = lengths["sphere"], 48
    for capacity, c in GC.cuts(n, slots):
        assert c == min(n, capacity // slots), (capacity, c)
    assert [c for _, c in GC.cuts(n, slots)] == [1100, 1000, 1024, n] and 1000 + GC.TRIP > n >= 1100

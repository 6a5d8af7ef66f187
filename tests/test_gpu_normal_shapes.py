"""The shapes of the surface normals that tests/test_gpu_normals.py leaves out.  The bake (bt_atlas_tile_normals): more than one band of
centre rows per tile (the first window from row 0, an inner window, a short last band against row T - 1), the scalar LDS fill of a T
that is no multiple of 8, halos above 2, a band height set by the LDS budget (to the byte at T = 1024), no window at all (every texel from
HBM), and more tiles than one chunk of the output ring.  The query (bt_tile_tree_sample_normal): borders 1 and 0, where taps fall left of
texel 0 and, without a border, the bilinear pair is clamped at -1 and at T.

Every comparison is the one of tests/test_gpu_normals.py (its helpers and tests/_normal_model.py are imported, not copied): every byte of
a baked map and every bit of a queried normal against the numpy model.

Every bake case proves from its own inputs that it reaches the branch it is named for.  bake_plan() restates the host's plan,
band_windows() the kernel's window, tap_rows() the texture rows a centre row touches (binary32, as the kernel's one window test computes
them), bake_branches() names the branches those reach; test_bake_cases_reach_their_branches asserts them without a GPU, and the GPU cases
again.  A wrong row offset inside a window is visible only if neighbouring texture rows differ: row_roll_share() asserts on the model
alone that the map of the tile with its rows shifted by one differs in at least 0.9 of every centre row's data texels."""
import functools

import numpy as np
import pytest

import _normal_model as NM
import _oracle as O
import bevy_terrain_amd as bt
from test_gpu_normals import assert_bits_equal, make_positions
from test_gpu_raycast import Streamed

F = np.float32
BAND_ROWS = 32       # bt_normal.hip: kBakeBandRows
LDS_BYTES = 40 << 10  # bt_normal.hip: kBakeLdsBytes
CHUNK_BYTES = 32 << 20  # bt_atlas_tile_normals: the maps of one chunk of tiles fit 32 MiB
RING_SLOTS = 3       # bt::StagingRing::kBuffers
ROLL_SHARE = 0.9

# side 100 (scale 50: dist = 50 / (c * 2^lod)), heights 0 .. 25: one 16-bit step is 0.0004, the rasters below move by thousands per texel
MODEL = bt.TerrainModel.planar((0.0, 0.0, 0.0), 100.0, 0.0, 25.0)
OMODEL = O.make_model("planar", (0.0, 0.0, 0.0), 100.0, 0.0, 0.0, 25.0)
# three distinct tiles of a planar terrain: the root and two of its children (the definition's dist halves at LOD 1)
COORDS = [(0, 0, 0, 0), (0, 1, 0, 0), (0, 1, 1, 1)]


@pytest.fixture(scope="module")
def device():
    return bt.Device(0)


# ---------------------------------------------------------------------------------------------- the plan, restated

def bake_plan(T, b):
    """(c, halo, band_rows, bands, lds_bytes) by the rule of bt_atlas_tile_normals; halo None: no window fits the LDS budget"""
    c = T - 2 * b
    halo = T // (2 * c) + 2
    window_rows = LDS_BYTES // (2 * T)
    if window_rows > 2 * halo:
        band_rows = min(BAND_ROWS, window_rows - 2 * halo, c)
    else:
        halo, band_rows = None, min(BAND_ROWS, c)
    bands = -(-c // band_rows)
    lds_bytes = 0 if halo is None else min(band_rows + 2 * halo, T) * 2 * T
    return c, halo, band_rows, bands, lds_bytes


def band_windows(T, b):
    """[(j0, j1, w0, rows)] per band: centre rows [j0, j1) and the texture rows [w0, w0 + rows) the workgroup copies into LDS, as
    tile_normals_kernel computes them (rows == 0: no window)"""
    c, halo, band_rows, bands, _ = bake_plan(T, b)
    out = []
    for band in range(bands):
        j0, j1 = band * band_rows, min((band + 1) * band_rows, c)
        if halo is None:
            out.append((j0, j1, 0, 0))
            continue
        w0 = b + j0 - halo if b + j0 > halo else 0
        out.append((j0, j1, w0, min(b + j1 - 1 + halo, T - 1) - w0 + 1))
    return out


def tap_rows(T, b):
    """(lo, hi) per centre row j: the texture rows its taps and its own texel touch, as the kernel's one window test computes them:
    tap_split in binary32 for the offsets -o and +o, the truncation, the clamp to [0, T - 1], min / max with the texel's own row b + j"""
    c = T - 2 * b
    j = np.arange(c)
    scale, offset, o = F(c) / F(T), F(b) / F(T), F(0.5) / F(c)
    u = ((j.astype(F) + F(0.5)) / F(c)) * scale + offset
    assert u.dtype == F
    first_lo = np.trunc((u - o) * F(T) - F(0.5)).astype(np.int64)
    first_hi = np.trunc((u + o) * F(T) - F(0.5)).astype(np.int64)
    return np.minimum(np.clip(first_lo, 0, T - 1), b + j), np.maximum(np.clip(first_hi + 1, 0, T - 1), b + j)


def rows_outside_their_window(T, b):
    """the centre rows one of whose tap rows lies outside the window of its band (they take the HBM path); every row when there is none"""
    lo, hi = tap_rows(T, b)
    out = []
    for j0, j1, w0, rows in band_windows(T, b):
        out += [j for j in range(j0, j1) if not (lo[j] >= w0 and hi[j] - w0 < rows)]
    return out


def bake_branches(T, b):
    """the names of the kernel lines and plan branches a bake at (T, b) reaches"""
    c, halo, band_rows, bands, lds_bytes = bake_plan(T, b)
    out = {"one_band" if bands == 1 else "several_bands"}
    if c * c < 64:
        out.add("tile_smaller_than_one_wave")
    if halo is None:
        return out | {"no_window"}
    out.add("vector_fill" if T % 8 == 0 else "scalar_fill")
    if b % 2:
        out.add("odd_border")
    windows = band_windows(T, b)
    if b + windows[0][0] <= halo:
        out.add("first_window_starts_at_row_0")       # the `: 0u` of w0
    if b < halo:
        out.add("first_window_clipped_below_row_0")   # ... and rows were cut off
    if b + c - 1 + halo >= T - 1:
        out.add("last_window_ends_at_row_T_minus_1")  # min(.., T - 1) takes T - 1
    if b + c - 1 + halo > T - 1:
        out.add("last_window_clipped_beyond_row_T_minus_1")
    if any(w0 > 0 and w0 + rows < T and rows == band_rows + 2 * halo for _, _, w0, rows in windows):
        out.add("inner_window")
    if bands > 1:
        out.add("short_last_band" if c % band_rows else "bands_divide_c")
    if halo > 2:
        out.add("wide_halo")
    lo, hi = tap_rows(T, b)
    own = b + np.arange(c)
    if (lo < own - 1).any() or (hi > own + 1).any():
        out.add("taps_beyond_the_adjacent_rows")
    if band_rows < min(BAND_ROWS, c):
        out.add("band_rows_set_by_the_lds_budget")
    if lds_bytes == LDS_BYTES:
        out.add("lds_budget_used_to_the_byte")
    return out


# ---------------------------------------------------------------------------------------------- the cases

def Case(T, b, c, halo, band_rows, bands, lds_bytes, reach):
    return dict(T=T, b=b, plan=(c, halo, band_rows, bands, lds_bytes), reach=set(reach))


CASES = {
    # band 0 from row 0, band 1 with rows cut off on neither side, band 2 of 4 rows up to row T - 1
    "three_bands": Case(72, 2, 68, 2, 32, 3, 5184, {"vector_fill", "several_bands", "first_window_starts_at_row_0", "inner_window", "short_last_band",
                                                    "last_window_ends_at_row_T_minus_1"}),
    "scalar_fill": Case(70, 3, 64, 2, 32, 2, 5040, {"scalar_fill", "odd_border", "several_bands", "bands_divide_c"}),
    "scalar_fill_b1": Case(44, 1, 42, 2, 32, 2, 3168, {"scalar_fill", "odd_border", "several_bands", "short_last_band", "first_window_clipped_below_row_0",
                                                       "last_window_clipped_beyond_row_T_minus_1"}),
    "scalar_one_band": Case(20, 2, 16, 2, 16, 1, 800, {"scalar_fill", "one_band"}),
    "wide_halo_bands": Case(136, 34, 68, 3, 32, 3, 10336, {"vector_fill", "wide_halo", "taps_beyond_the_adjacent_rows", "several_bands", "inner_window"}),
    "wide_halo_tiny": Case(64, 30, 4, 10, 4, 1, 3072, {"vector_fill", "wide_halo", "taps_beyond_the_adjacent_rows", "one_band", "tile_smaller_than_one_wave"}),
    "lds_bound": Case(576, 2, 572, 2, 31, 19, 40320, {"vector_fill", "band_rows_set_by_the_lds_budget", "several_bands", "short_last_band", "inner_window"}),
    "lds_full": Case(1024, 2, 1020, 2, 16, 64, 40960, {"vector_fill", "band_rows_set_by_the_lds_budget", "lds_budget_used_to_the_byte", "several_bands",
                                                       "short_last_band", "inner_window"}),
    "lds_full_wide_halo": Case(1024, 448, 128, 6, 8, 16, 40960, {"vector_fill", "wide_halo", "taps_beyond_the_adjacent_rows", "band_rows_set_by_the_lds_budget",
                                                                 "lds_budget_used_to_the_byte", "several_bands", "bands_divide_c", "inner_window"}),
    "no_window": Case(1024, 480, 64, None, 32, 2, 0, {"no_window", "several_bands"}),
}
LAST_BAND_ROWS = {"three_bands": 4, "scalar_fill": 32, "scalar_fill_b1": 10, "lds_bound": 14, "lds_full": 12}  # (1020 = 63 * 16 + 12)
TAP_DISTANCE = {"wide_halo_bands": 2, "wide_halo_tiny": 9}  # texture rows from a centre texel to the farthest row of its taps


def raster(T, seed):
    """(T, T) uint16: three summed sinusoids and noise, 1 .. 65535, about 2 % no-data texels; neighbouring rows differ by thousands"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:T, 0:T].astype(np.float64)
    waves = np.sin(x * 0.37 + seed) + np.sin(y * 0.23 + 1.3 * seed) + np.sin((x + y) * 0.11 + 0.7 * seed)
    v = 0.5 + 0.08 * waves + rng.uniform(-0.22, 0.22, (T, T))
    out = np.clip(np.rint(v * 65535.0), 1, 65535).astype(np.uint16)
    out[rng.random((T, T)) < 0.02] = 0
    return out


def hole_block(T, b):
    """(rows, columns) of the texture: a block of no-data texels across the boundary of bands 0 and 1 (one band: across the tile's middle)"""
    c, _, band_rows, bands, _ = bake_plan(T, b)
    edge = b + (band_rows if bands > 1 else c // 2)
    return slice(max(b, edge - 2), min(b + c, edge + 3)), slice(b + c // 4, b + max(c // 2, c // 4 + 1))


def row_roll_share(texels, b, lod, true_map):
    """per centre row: the share of its data texels at which the model's map of the tile with its texture rows rolled by one differs"""
    c = texels.shape[0] - 2 * b
    rolled = NM.tile_normal_map(OMODEL, np.roll(texels, 1, axis=0), b, lod)
    data = texels[b:b + c, b:b + c] != 0
    differs = (rolled != true_map).any(axis=2) & data
    assert data.sum(axis=1).min() >= 2
    return differs.sum(axis=1) / data.sum(axis=1)


@functools.lru_cache(maxsize=None)
def case_data(name):
    """the three rasters of a case, their maps by the model and the smallest row-roll share: computed once, shared, never written to"""
    T, b = CASES[name]["T"], CASES[name]["b"]
    tiles, maps, share = [], [], 1.0
    for k, coord in enumerate(COORDS):
        texels = raster(T, seed=10 * list(CASES).index(name) + k)
        if k == 1:
            texels[hole_block(T, b)] = 0
        texels[b + k, T - b - 1 - k] = 0  # one no-data texel on (next to) the centre's corner, whatever the noise gave a small centre
        exp = NM.tile_normal_map(OMODEL, texels, b, coord[1])
        share = min(share, float(row_roll_share(texels, b, coord[1], exp).min()))
        for a in (texels, exp):
            a.setflags(write=False)
        tiles.append(texels)
        maps.append(exp)
    return tiles, maps, share


def check_case(name):
    """what makes a case a test of its branch, from the plan and the model alone (asserted without a GPU and again before the GPU run);
    returns the plan and the smallest row-roll share"""
    case = CASES[name]
    T, b = case["T"], case["b"]
    plan = bake_plan(T, b)
    c, halo, band_rows, bands, lds_bytes = plan
    assert plan == case["plan"], (name, plan)
    names = bake_branches(T, b)
    assert case["reach"] <= names, (name, sorted(case["reach"] - names))
    windows = band_windows(T, b)
    assert len(windows) == bands and windows[-1][1] == c
    if name in LAST_BAND_ROWS:
        assert windows[-1][1] - windows[-1][0] == LAST_BAND_ROWS[name]
    for j0, j1, w0, rows in windows:
        assert rows * 2 * T <= LDS_BYTES and rows * 2 * T <= lds_bytes and w0 + rows <= T, (name, j0, w0, rows)
        assert rows * T % 8 == 0 or T % 8  # the 16-byte fill copies whole vectors
    outside = rows_outside_their_window(T, b)
    assert outside == (list(range(c)) if halo is None else []), (name, outside[:8])
    lo, hi = tap_rows(T, b)
    own = b + np.arange(c)
    if name in TAP_DISTANCE:
        assert max((own - lo).max(), (hi - own).max()) == TAP_DISTANCE[name] and (hi - lo).min() >= TAP_DISTANCE[name], (name, set(own - lo), set(hi - own))
    tiles, maps, share = case_data(name)
    assert share >= ROLL_SHARE, (name, share)
    rows, cols = hole_block(T, b)
    assert b <= rows.start < rows.stop <= b + c and b <= cols.start < cols.stop <= b + c
    if bands > 1:
        assert rows.start - b < band_rows <= rows.stop - 1 - b, "the block of no-data texels does not span the boundary of bands 0 and 1"
    for texels, exp in zip(tiles, maps):
        centre = texels[b:b + c, b:b + c]
        assert 0 < (centre == 0).mean() < 0.35 and texels.max() > 50000 and texels[texels > 0].min() < 15000
        assert (exp[centre != 0][:, 2] < 250).mean() > 0.5, "the map is flat"
    return plan, share


@pytest.mark.parametrize("name", list(CASES))
def test_bake_cases_reach_their_branches(name):
    """no GPU: the plan values and branch names of the table, no window beyond the LDS the launch asks for, every centre row's tap rows
    inside its band's window (no window: every row takes the HBM path), and the row-roll condition on the rasters the GPU cases bake"""
    plan, share = check_case(name)
    print(f"{name}: T {CASES[name]['T']} b {CASES[name]['b']} (c, halo, band_rows, bands, lds_bytes) = {plan}, smallest row-roll share {share:.4f}")


def test_no_row_of_these_sizes_leaves_its_window():
    """no GPU: at the texture sizes of the table and every border, a centre row takes the HBM path only where the plan has no window.  A
    (T, b) that fails here reaches the per-texel fallback beside a filled window and belongs into CASES."""
    for T in sorted({case["T"] for case in CASES.values()}):
        for b in range(1, (T + 1) // 2):
            if bake_plan(T, b)[1] is not None:
                assert not rows_outside_their_window(T, b), (T, b)


# ---------------------------------------------------------------------------------------------- the bake on the device

def bake_atlas(device, name):
    """an atlas that holds COORDS with the rasters of the case -> (atlas, [TileCoordinate])"""
    T, b = CASES[name]["T"], CASES[name]["b"]
    cfg = bt.TerrainConfig(lod_count=2, atlas_size=4, path="terrains/normal_shapes", model=MODEL)
    cfg.add_attachment(bt.AttachmentConfig(name="height", texture_size=T, border_size=b, format=bt.AttachmentFormat.R16))
    atlas = bt.TileAtlas.new(cfg, device)
    coords = []
    for coord, texels in zip(COORDS, case_data(name)[0]):
        co, index = atlas.get_or_allocate_tile(bt.TileCoordinate(*coord))
        atlas.upload_tile(0, index, texels)
        coords.append(co)
    return atlas, coords


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_bake_shapes_equal_the_model(device, name):
    """three tiles with different rasters (no-data texels scattered, and a block of them across a band boundary in one), one listed
    twice: every byte of every map"""
    check_case(name)
    T, b = CASES[name]["T"], CASES[name]["b"]
    c = T - 2 * b
    tiles, maps, _ = case_data(name)
    atlas, coords = bake_atlas(device, name)
    order = [0, 1, 2, 1]
    got = atlas.tile_normals(0, [coords[k] for k in order])
    assert got.shape == (4, c, c, 4) and got.dtype == np.uint8
    for n, k in enumerate(order):
        assert np.array_equal(got[n], maps[k]), (name, n, k, np.argwhere((got[n] != maps[k]).any(axis=2))[:6])
        empty = tiles[k][b:b + c, b:b + c] == 0
        assert empty.any() and (got[n][empty] == (128, 128, 255, 0)).all() and (got[n][~empty][:, 3] == 255).all()
    assert not np.array_equal(maps[0], maps[1]) and not np.array_equal(maps[1], maps[2])
    for index, texels in enumerate(tiles):  # a read
        assert np.array_equal(atlas.download_tile(0, index), texels)


# ---------------------------------------------------------------------------------------------- the query at borders 1 and 0

QUERY_CASES = [("planar", 16, 1), ("sphere", 16, 1), ("planar", 16, 0), ("sphere", 16, 0)]


@pytest.fixture(scope="module")
def terrains(device, tmp_path_factory):
    cache = {}

    def get(kind, texture_size, border_size):
        key = (kind, texture_size, border_size)
        if key not in cache:
            s = Streamed(device, tmp_path_factory.mktemp(f"{kind}_{texture_size}_{border_size}"), kind, texture_size=texture_size, border_size=border_size)
            s.height = s.tree.view_state().approximate_height
            cache[key] = s
        return cache[key]

    return get


@pytest.mark.gpu
@pytest.mark.parametrize("kind,texture_size,border_size", QUERY_CASES)
def test_normals_equal_the_model_at_narrow_borders(terrains, kind, texture_size, border_size):
    """test_gpu_normals.test_normals_equal_the_model's comparison (4096 positions of make_positions, a quarter of them on tile borders and
    a hair to either side; normals and up_dot bit for bit) where a tap coordinate t = p * T - 0.5 falls below 0.

    b = 1: t of the left / upper tap lies in (-1, 0) for a position within 0.5 % of a tile's low border: int(t) is 0 and rem is negative,
    the reference's extrapolation.  b = 0: the same for every tap within half a texel of the low border, the pair first, first + 1 is
    clamped at T on the high side, and first is -1 after the truncation exactly where t <= -1: t = uv * T - 1 for the tap at -o, so where
    uv is 0 (or rounds to it), which the positions exactly on a tile border give."""
    s = terrains(kind, texture_size, border_size)
    pts = make_positions(s.omodel, s.view, 4096, seed=11, height=s.height)
    exp_n, exp_d, info = NM.world_normals(s.omodel, s.otree, s.height, texture_size, border_size, s.layers, pts)
    counts = {name: int(info[name].sum()) for name in ("tap_negative", "tap_high", "tap_minus_one")}
    print(f"{kind} T {texture_size} b {border_size}: positions with a tap of negative t / clamped at the high edge / first == -1: {counts}")
    assert counts["tap_negative"] >= 50, counts
    if border_size == 0:
        assert counts["tap_high"] >= 50 and counts["tap_minus_one"] >= 50, counts
    assert (info["ratio"] > 0).sum() >= 300 and (info["ratio"] == 0).sum() >= 1000
    assert len(set(info["lod"][info["layer"] != NM.INVALID])) >= 2
    assert (exp_n != info["N"]).any(axis=1).mean() > 0.9
    if kind != "planar":
        assert len(set(info["side"])) == 6
    got_n, got_d = s.tree.sample_normal(0, pts)
    assert got_n.dtype == np.float32 and got_n.shape == (4096, 3) and got_d.shape == (4096,)
    assert_bits_equal(got_n, exp_n, "normals", info)
    assert_bits_equal(got_d, exp_d, "up_dot", info)


# ---------------------------------------------------------------------------------------------- the chunk ring

@pytest.mark.gpu
def test_bake_chunk_ring(device, terrains):
    """27 tiles of 1020 x 1020 texels: 8 to a chunk, so 4 chunks (8, 8, 8, 3) through the ring of three slots: slot 0 used twice, a short
    last chunk.  The list is layer[i % 3]: period 3 is coprime to 8, so a chunk read from a wrong place of the list, or copied to a wrong
    place of the output, is a wrong tile.  Then calls of two chunks and of exactly three, and the query and the bake in turn on the
    scratch they share (each reallocates it when it is too small), across a trim."""
    name = "lds_full"
    T, b = CASES[name]["T"], CASES[name]["b"]
    c = T - 2 * b
    per_chunk = CHUNK_BYTES // (c * c * 4)
    assert per_chunk == 8 and -(-27 // per_chunk) == 4 > RING_SLOTS and 27 % per_chunk == 3 and -(-9 // per_chunk) == 2 and 24 == RING_SLOTS * per_chunk
    _, maps, _ = case_data(name)
    assert not any(np.array_equal(maps[i], maps[k]) for i, k in ((0, 1), (0, 2), (1, 2)))
    atlas, coords = bake_atlas(device, name)
    listed = [coords[i % 3] for i in range(27)]

    def assert_same(a, e, what):
        assert a.shape == e.shape and all(np.array_equal(a[i], e[i]) for i in range(len(e))), (what, [i for i in range(len(e)) if not np.array_equal(a[i], e[i])])

    got = atlas.tile_normals(0, listed)
    assert got.shape == (27, c, c, 4)
    wrong = [i for i in range(27) if not np.array_equal(got[i], maps[i % 3])]
    assert not wrong, wrong
    assert_same(atlas.tile_normals(0, listed[:9]), got[:9], "two chunks")
    assert_same(atlas.tile_normals(0, listed[:24]), got[:24], "three chunks")
    # the query on a small terrain of the same Device, then the bake: the scratch shrinks and grows
    s = terrains("planar", 16, 1)
    pts = make_positions(s.omodel, s.view, 256, seed=9, height=s.height)
    exp_n, exp_d, _ = NM.world_normals(s.omodel, s.otree, s.height, 16, 1, s.layers, pts)
    first_n, first_d = s.tree.sample_normal(0, pts)
    assert first_n.tobytes() == exp_n.tobytes() and first_d.tobytes() == exp_d.tobytes()
    assert_same(atlas.tile_normals(0, listed), got, "after the query")
    assert device.trim() > 0
    again_n, again_d = s.tree.sample_normal(0, pts)
    assert again_n.tobytes() == first_n.tobytes() and again_d.tobytes() == first_d.tobytes()
    assert_same(atlas.tile_normals(0, listed), got, "after the trim")

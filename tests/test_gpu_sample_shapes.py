"""The sampling path on the device, branch by branch: sample_surface of bt_tile_tree_device.hpp (compute_blend, lookup_tile at lod and
lod - 1, the two tile samples, their blend) through bt_tile_tree_sample_attachment, for both attachment formats and the three models.

The cases are tests/_sample_cases.py's: small terrains (T = 32, b = 2 and T = 20, b = 1; lod_count 4, tree_size 4; an R16 and an Rgba8
attachment in one atlas) whose tiles are preprocessed and saved here, then streamed back with the files of chosen tiles removed, so that
region by region the best loaded tile of a node is its own, its parent, its grandparent or nothing.  The device's best-tile table must equal
the table computed from that loaded set; the 1000 positions of a case are crafted per branch and padded with random ones, and every case
asserts from the second model's trace the minimum counts of _sample_cases.MINIMUM (test_sample_model.py asserts the same without a GPU).
out_vec4 and heights are compared bit for bit, no position excluded, with the CPU oracle and with the second model
(tests/_second_models.py).  The second model restates everything but the closest point on an ellipsoid, which the ellipsoid case takes from
the oracle: there the model is a second opinion on the blend, the lookups and the tile sample only.

compute_blend's f64 log2 is OCML's on the device and libm's on the CPU, at most 1 ulp apart.  _sample_cases keeps a position only when a
log2 two representable doubles away on either side gives the same sample, replaces any other by the next draw, and at most 1 % of the draws
may be replaced.

Then: the batch shapes (one position, one short of / exactly / one over a workgroup of 128, 1000; heights == NULL), and every unorm8 value
in every channel and 4096 unorm16 values through bt_atlas_sample and through the tile tree."""
import ctypes as C
import os

import numpy as np
import pytest

import _sample_cases as SC
import bevy_terrain_amd as bt
from bevy_terrain_amd import _ffi

pytestmark = pytest.mark.gpu

FORMATS = {"height": bt.AttachmentFormat.R16, "albedo": bt.AttachmentFormat.Rgba8}


@pytest.fixture(scope="module")
def device():
    return bt.Device(0)


def two_attachments(cfg, T, b):
    for name, fmt in FORMATS.items():
        cfg.add_attachment(bt.AttachmentConfig(name=name, texture_size=T, border_size=b, format=fmt))
    return cfg


def preprocess_and_save(device, root, model, lods, T, b, heights, colours):
    """both attachments of the whole pyramid, preprocessed on the device and saved under `root` -> the terrain's path"""
    cfg = two_attachments(bt.TerrainConfig(lod_count=lods, atlas_size=6 * 100, path="terrains/sample", model=model), T, b)
    atlas = bt.TileAtlas.new(cfg, device)
    server = bt.AssetServer()
    pre = bt.Preprocessor.new().clear_attachment(0, atlas).clear_attachment(1, atlas)
    for index, sources in enumerate((heights, colours)):
        paths = [f"a{index}_face{s}" for s in range(len(sources))]
        for p, src in zip(paths, sources):
            server.insert(p, src)
        if model.is_spherical():
            pre.preprocess_spherical(bt.SphericalDataset(attachment_index=index, paths=paths, lod_range=range(0, lods)), server, atlas)
        else:
            pre.preprocess_tile(bt.PreprocessDataset(attachment_index=index, path=paths[0], lod_range=range(0, lods)), server, atlas)
    pre.run(atlas)
    pre.save(atlas, root)
    return cfg.path


def stream_one_frame(device, root, path, model, lods, T, b, atlas_size, view_config, view):
    """a fresh streaming atlas and tile tree after one frame at `view`: update -> requests -> loads -> adjust_to_tile_atlas"""
    atlas = bt.TileAtlas.new(two_attachments(bt.TerrainConfig(lod_count=lods, atlas_size=atlas_size, path=path, model=model), T, b), device)
    atlas.load_tile_config(root)
    tree = bt.TileTree.new(atlas, view_config)
    released, requested = tree.update(view)
    tree.apply_requests()
    loaded, failed = atlas.update(root)
    tree.adjust_to_tile_atlas()
    return atlas, tree, requested, loaded, failed


_terrains = {}


@pytest.fixture
def terrain(device, tmp_path_factory):
    """terrain(spec_name) -> (atlas, tree) of that spec, streamed once per module with the spec's missing tiles unloadable, and checked: the
    request list, the load counts, the device's best-tile table == the nearest-loaded-ancestor table of the loaded set, the loaded layers ==
    the CPU oracle's tiles"""
    def get(spec_name):
        if spec_name in _terrains:
            return _terrains[spec_name]
        spec = SC.SPECS[spec_name]
        model = SC.MODELS[spec["kind"]][0]
        root = str(tmp_path_factory.mktemp(spec_name) / "assets")
        path = preprocess_and_save(device, root, model, SC.LODS, spec["T"], spec["b"], *SC.rasters(spec_name))
        for side, lod, x, y in spec["missing"]:
            for name in FORMATS:
                os.remove(os.path.join(root, path, "data", name, f"{side}_{lod}_{x}_{y}.bin"))
        atlas, tree, requested, loaded, failed = stream_one_frame(device, root, path, model, SC.LODS, spec["T"], spec["b"], SC.atlas_size(spec_name),
                                                                  SC.view_config(spec_name)[0], spec["view"])
        tm, exp_requested, exp_loaded, exp_entries, exp_coords = SC.table(spec_name)
        existing = set(SC.oracle_tiles(spec_name))
        assert requested == exp_requested
        assert (loaded, failed) == (2 * len(exp_loaded), 2 * len(set(requested) & spec["missing"])) and failed > 0
        entries, origins, coords, flags = tree.read()
        assert np.array_equal(coords, exp_coords)
        assert np.array_equal(entries, exp_entries) and np.array_equal(entries, SC.nearest_loaded_ancestor(coords, exp_loaded))
        for c in sorted(existing & (set(requested) | spec["missing"])):  # the atlas's own answer, tile by tile
            assert atlas.get_best_tile(bt.TileCoordinate(*c)) == tuple(SC.nearest_loaded_ancestor(np.array([c]), exp_loaded)[0].tolist()), c
        tiles = SC.oracle_tiles(spec_name)
        for c, index in exp_loaded.items():
            assert np.array_equal(atlas.download_tile(0, index), tiles[c][0]) and np.array_equal(atlas.download_tile(1, index), tiles[c][1]), c
        _terrains[spec_name] = (atlas, tree)
        return atlas, tree
    return get


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_bit_equal(ours, expected, what, positions):
    bad = np.flatnonzero((bits(ours) != bits(expected)).reshape(len(ours), -1).any(axis=1))
    assert len(bad) == 0, (what, len(bad), bad[:8].tolist(), positions[bad[:3]].tolist(), ours[bad[:3]].tolist(), expected[bad[:3]].tolist())


@pytest.mark.parametrize("name", list(SC.CASES))
def test_sample_attachment_reaches_and_matches_every_branch(terrain, name):
    c = SC.case(name)
    atlas, tree = terrain(c.spec_name)
    # the batch reaches every branch it is there for (from the second model's trace), within the replacement cap of the log2 caveat
    counts, minimum = SC.reach_counts(c), SC.minimum(c)
    short = {k: (counts[k], m) for k, m in minimum.items() if counts[k] < m}
    assert not short, short
    assert c.replaced * 100 <= c.draws, (c.replaced, c.draws)
    values, heights = tree.sample_attachment(c.attachment, c.positions)
    print(name, "differing rows vs oracle:", int((bits(values) != bits(c.oracle_values)).any(axis=1).sum()), "heights:", int((bits(heights) != bits(c.oracle_heights)).sum()))
    assert_bit_equal(values, c.oracle_values, "out_vec4 vs oracle", c.positions)
    assert_bit_equal(heights, c.oracle_heights, "heights vs oracle", c.positions)
    assert_bit_equal(values, c.model_values, "out_vec4 vs second model", c.positions)
    assert_bit_equal(heights, c.model_heights, "heights vs second model", c.positions)
    # heights = lerp(min_height, max_height, red) for either format; nothing loaded above a node: value exactly 0, height exactly min_height
    model = SC.MODELS[c.spec["kind"]][0]
    lo, hi = np.float32(model.min_height), np.float32(model.max_height)
    assert np.array_equal(heights, (lo + np.float32(hi - lo) * values[:, 0]).astype(np.float32))
    none = np.array([t.lookups[0].depth is None and (len(t.lookups) == 1 or t.lookups[1].depth is None) for t in c.trace])
    assert none.sum() >= 8 and not values[none].any() and (heights[none] == lo).all()
    if c.fmt == SC.RGBA8:
        assert values[~none][:, 1:].any(axis=0).all()


@pytest.mark.parametrize("name", ["planar_r16", "sphere_rgba8"])
def test_batch_shapes_are_prefixes_of_the_whole_batch(terrain, name):
    """count = 1, 127, 128, 129 and 1000 against workgroups of 128 threads: every result is the prefix of the 1000-position result and of the
    oracle's; with heights == NULL (the raw call) out_vec4 is the same and nothing else is written"""
    c = SC.case(name)
    atlas, tree = terrain(c.spec_name)
    whole, whole_heights = tree.sample_attachment(c.attachment, c.positions)
    assert_bit_equal(whole, c.oracle_values, "out_vec4 vs oracle", c.positions)
    assert_bit_equal(whole_heights, c.oracle_heights, "heights vs oracle", c.positions)
    for count in (1, 127, 128, 129, 1000):
        values, heights = tree.sample_attachment(c.attachment, c.positions[:count])
        assert np.array_equal(bits(values), bits(whole[:count])) and np.array_equal(bits(heights), bits(whole_heights[:count])), count
        # heights == NULL; the output buffer has a guard row behind the batch
        positions = np.ascontiguousarray(c.positions[:count])
        out = np.full((count + 1, 4), -7.0, np.float32)
        _ffi.check(_ffi.lib().bt_tile_tree_sample_attachment(tree._h, atlas._h, c.attachment, positions.ctypes.data_as(C.POINTER(C.c_double)), count,
                                                             out.ctypes.data_as(C.POINTER(C.c_float)), None))
        assert np.array_equal(bits(out[:count]), bits(c.oracle_values[:count])) and (out[count] == -7.0).all(), count


# ---------------------------------------------------------------------------------------------- every unorm value

UT, UB = 68, 2  # a centre of 64 x 64


def unorm16_values():
    v = np.unique(np.concatenate([np.round(np.linspace(0, 65535, 4090)).astype(np.int64), [0, 1, 32767, 32768, 65534, 65535]]))
    spare = np.setdiff1d(np.arange(65536), v)[:: 65536 // 64]
    return np.concatenate([v, spare])[:4096].astype(np.uint16)


@pytest.fixture(scope="module")
def root_tile(device, tmp_path_factory):
    """a planar terrain of one tile (lod_count 1: every sample is lod 0, ratio 0, uv = the coordinate) with both attachments, streamed in"""
    model = SC.MODELS["planar"][0]
    root = str(tmp_path_factory.mktemp("unorm") / "assets")
    rng = np.random.default_rng(2)
    path = preprocess_and_save(device, root, model, 1, UT, UB, [rng.integers(1, 65536, (80, 80), dtype=np.uint16)], [rng.integers(1, 256, (80, 80, 4), dtype=np.uint8)])
    atlas, tree, requested, loaded, failed = stream_one_frame(device, root, path, model, 1, UT, UB, 4, bt.TerrainViewConfig(tree_size=2), (0.0, 300.0, 0.0))
    assert (loaded, failed) == (2, 0) and atlas.get_best_tile(bt.TileCoordinate(0, 0, 0, 0)) == (0, 0)
    assert tree.read()[0].tolist()[0] == [0, 0]
    return atlas, tree


def block_centres(block):
    """uv and world positions of the centres of the block x block texel blocks of the 64 x 64 centre, row by row"""
    n = 64 // block
    gy, gx = np.mgrid[0:n, 0:n]
    uv = np.stack([(gx.ravel() * block + block / 2) / 64.0, (gy.ravel() * block + block / 2) / 64.0], axis=1)
    model = SC.MODELS["planar"][0]
    world = np.stack([model.translation[0] + (uv[:, 0] - 0.5) * 1000.0, np.full(len(uv), 40.0), model.translation[2] + (uv[:, 1] - 0.5) * 1000.0], axis=1)
    return uv.astype(np.float32), world


def blocks_layer(values, block, channels):
    """the (68, 68[, 4]) layer whose centre block k (row by row) holds values[k] in every texel; the border something else"""
    n = 64 // block
    centre = np.repeat(np.repeat(values.reshape((n, n) + values.shape[1:]), block, axis=0), block, axis=1)
    layer = np.full((UT, UT) + ((4,) if channels == 4 else ()), 77, values.dtype)
    layer[UB:-UB, UB:-UB] = centre
    return layer


def test_every_unorm8_value_in_every_channel(root_tile):
    """4 x 4 blocks of one byte value per block and channel (channel k of block n holds (n + 64 k) % 256): a sample at a block's centre has
    four equal taps and returns the conversion itself, f32(byte) / f32(255), through bt_atlas_sample and through the tile tree"""
    atlas, tree = root_tile
    n = np.arange(256)
    values = np.stack([(n + 64 * k) % 256 for k in range(4)], axis=1).astype(np.uint8)
    assert all(len(set(values[:, k].tolist())) == 256 for k in range(4))
    atlas.upload_tile(1, 0, blocks_layer(values, 4, 4))
    uv, world = block_centres(4)
    expected = values.astype(np.float32) / np.float32(255.0)
    assert np.array_equal(bits(atlas.sample(1, np.zeros(256, np.uint32), uv)), bits(expected))
    out, heights = tree.sample_attachment(1, world)
    assert np.array_equal(bits(out), bits(expected))
    model = SC.MODELS["planar"][0]  # heights of an Rgba8 attachment: lerp(min_height, max_height, red)
    lo, hi = np.float32(model.min_height), np.float32(model.max_height)
    assert np.array_equal(heights, (lo + np.float32(hi - lo) * expected[:, 0]).astype(np.float32))


def test_4096_unorm16_values(root_tile):
    """2 x 2 blocks, 1024 values a layer, four layers' worth: 0, 1, 32767, 32768, 65534, 65535 and an even spread between"""
    atlas, tree = root_tile
    values = unorm16_values()
    assert len(set(values.tolist())) == 4096 and {0, 1, 32767, 32768, 65534, 65535} <= set(values.tolist())
    uv, world = block_centres(2)
    for part in values.reshape(4, 1024):
        atlas.upload_tile(0, 0, blocks_layer(part, 2, 1))
        expected = np.zeros((1024, 4), np.float32)
        expected[:, 0] = part.astype(np.float32) / np.float32(65535.0)
        assert np.array_equal(bits(atlas.sample(0, np.zeros(1024, np.uint32), uv)), bits(expected))
        out, _ = tree.sample_attachment(0, world)
        assert np.array_equal(bits(out), bits(expected))

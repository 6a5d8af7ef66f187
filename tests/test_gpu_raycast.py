"""bt_tile_tree_raycast on the device: bit equality with the CPU model of its definition (tests/_raycast_model.py on the oracle's
sample_attachment), agreement with bt_tile_tree_sample_attachment independent of that model, the unloaded terrain against the closed
form, the call as a read of the atlas, limits and hostile input.

The terrains are built like test_gpu_tile_tree.py's (smooth raster, R16, 4 LODs, T = 32) and streamed into a tree along a camera path, the
oracle's tree in lock step, so that the entries mix LODs and the tiles requested by the last frame are not loaded yet (their nodes fall
back to an ancestor).  Fixed seeds; no tolerance anywhere: the existing sampling test notes that the device's and libm's f64 log2 may differ
in the last place, which could flip an f32 blend weight within 2^-29 of a rounding boundary — with these seeds no such case occurs."""
import ctypes as C
import math

import numpy as np
import pytest

import _oracle as O
import _raycast_model as RM
import bevy_terrain_amd as bt
from bevy_terrain_amd import _ffi
from test_gpu_tile_tree import build_terrain, camera_path
from test_tile_tree_host import MODELS

pytestmark = pytest.mark.gpu
LODS, T, B = 4, 32, 2
BT_ERR_INVALID_ARGUMENT, BT_ERR_UNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def device():
    return bt.Device(0)


# ---- rays ------------------------------------------------------------------------------------------------------------------------------

def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def make_rays(omodel, view, n, seed):
    """n rays in four equal families: (A) from above towards a ground point, direction not normalised (t in units of it), steep to
    shallow; (B) from mid height, near horizontal (grazing; crossing tile borders and blend rings; on the globe nearly tangent to it);
    (C) origin just above the lowest surface, i.e. under the ground almost everywhere, random direction; (D) just above max_height, level or
    rising (tangent to the globe; leaving the planar terrain's square).  Returns origins, directions, t_min, t_max."""
    rng = np.random.default_rng(seed)
    q = n // 4
    kind = int(omodel.kind)
    pos = np.array([float(omodel.position[i]) for i in range(3)])
    lo, hi = float(omodel.min_height), float(omodel.max_height)
    span = hi - lo
    if kind == 0:
        side = float(omodel.a)
        length = side

        def place(m):  # m ground points over the square and a little beyond, their up vectors
            g = np.column_stack([rng.uniform(-0.52, 0.52, m) * side, np.zeros(m), rng.uniform(-0.52, 0.52, m) * side]) + pos
            return g, np.tile([0.0, 1.0, 0.0], (m, 1))
    else:
        scale = np.array([float(omodel.a), float(omodel.b) if kind == 2 else float(omodel.a), float(omodel.a)])
        length = float(omodel.a) * 0.2
        centre = _unit(np.asarray(view) - pos)

        def place(m):  # m points of the height-0 surface within ~0.35 rad of the view, their (radial) up vectors
            u = _unit(centre + rng.normal(size=(m, 3)) * 0.2)
            return pos + u * scale, u

    def tangent(up):
        return _unit(np.cross(up, _unit(rng.normal(size=up.shape))))

    # A
    g, up = place(q)
    oa = g + up * (hi + rng.uniform(0.2, 1.4, (q, 1)) * span)
    target, tup = place(q)
    if kind != 0:
        tup = _unit(up + tangent(up) * rng.uniform(0.0, 0.12, (q, 1)))  # up to ~0.12 rad away along the surface
        target = pos + tup * scale
    da = (target + tup * lo) - oa
    ta = rng.uniform(0.9, 1.6, q)  # the point of the lowest surface lies at t = 1: hits up to the last coarse round, a few rays end above the ground
    # B
    g, up = place(q)
    ob = g + up * (lo + rng.uniform(0.35, 0.75, (q, 1)) * span)
    db = _unit(tangent(up) + up * rng.uniform(-0.15, 0.05, (q, 1)))
    tb = np.full(q, 0.6 * length)
    # C
    g, up = place(q)
    oc = g + up * (lo + rng.uniform(0.0, 0.1, (q, 1)) * span)
    dc = _unit(rng.normal(size=(q, 3)))
    tc = np.full(q, 0.4 * length)
    # D
    m = n - 3 * q
    g, up = place(m)
    od = g + up * (hi + rng.uniform(0.002, 0.08, (m, 1)) * span)
    dd = _unit(tangent(up) + up * rng.uniform(0.0, 0.3, (m, 1)))
    td = np.full(m, 0.7 * length)
    origins, directions, t_max = np.vstack([oa, ob, oc, od]), np.vstack([da, db, dc, dd]), np.concatenate([ta, tb, tc, td])
    t_min = np.zeros(len(origins))
    t_min[::7] = 0.03 * t_max[::7]  # some rays start beyond their origin
    return origins, directions, t_min, t_max


def assert_mix(model_hits, steps):
    """conditions on the INPUT, from the model's statuses: the test cannot pass on all-miss rays or on hits of one round only"""
    status = model_hits["status"]
    n = len(status)
    for s in (RM.HIT, RM.MISS, RM.INSIDE):
        assert (status == s).sum() * 5 >= n, (s, np.bincount(status, minlength=4))
    if steps == 256:
        rounds = model_hits["step"][status == RM.HIT] // 64
        assert (rounds == 0).any() and ((rounds == 1) | (rounds == 2)).any() and (rounds >= 3).any(), np.bincount(rounds)


def assert_hits_equal(got, exp):
    assert np.array_equal(got["status"], exp["status"]), np.flatnonzero(got["status"] != exp["status"])[:8]
    assert np.array_equal(got["step"], exp["step"]), np.flatnonzero(got["step"] != exp["step"])[:8]
    for name in ("t", "t_above", "position", "height"):  # the bits
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(exp[name])
        assert a.tobytes() == b.tobytes(), (name, np.flatnonzero((a != b).reshape(len(a), -1).any(axis=1))[:8])
    assert not got["_padding"].any()


# ---- terrains --------------------------------------------------------------------------------------------------------------------------

class Streamed:
    """a terrain streamed into a device tree and the oracle's tree in lock step (the loop of test_streaming_loop_entries_and_heights)"""

    def __init__(self, device, tmp_path, kind, frames=12, texture_size=T, border_size=B, model=None):
        self.model, self.omodel = model or MODELS[kind]  # model: a (TerrainModel, oracle model) pair of `kind` other than MODELS'
        root, cfg, tiles = build_terrain(device, tmp_path, self.model, LODS, texture_size, border_size)
        atlas_size = 256 if kind == "planar" else 512
        scfg = bt.TerrainConfig(lod_count=LODS, atlas_size=atlas_size, path=cfg.path, model=self.model)
        scfg.add_attachment(bt.AttachmentConfig(name="height", texture_size=texture_size, border_size=border_size, format=bt.AttachmentFormat.R16))
        self.atlas = bt.TileAtlas.new(scfg, device)
        self.atlas.load_tile_config(root)
        kw = dict(tree_size=4, load_distance=1.2, blend_distance=1.0)
        self.tree = bt.TileTree.new(self.atlas, bt.TerrainViewConfig(**kw))
        self.otree = O.TileTree(self.omodel, LODS, O.make_view_config(**kw))
        stream = O.Stream(atlas_size, 1, existing=list(tiles))
        self.layers = {}
        for pos in camera_path(kind, frames, seed=5):
            assert self.tree.update(pos) == self.otree.update(pos)
            pending = stream.pending_loads()
            assert self.atlas.update(root) == (pending, 0)
            for coord, index in stream.finish_loads(pending):
                self.layers[index] = tiles[coord]
            self.tree.apply_requests()
            self.otree.apply_requests(stream)
            self.tree.adjust_to_tile_atlas()
            self.otree.adjust_to_tile_atlas(stream)
            self.otree.set_approximate_height(self.tree.approximate_height())
            self.view = pos
        entries, _, coords, _ = self.tree.read()
        assert np.array_equal(entries, self.otree.read()[0])
        known = coords[:, 1] != O.INVALID
        assert len(set(entries[known, 1])) >= 3  # the entries mix LODs ...
        assert (entries[known, 1] < coords[known, 1]).any()  # ... and some nodes fall back to an ancestor
        self.sample = RM.sampler(self.otree, texture_size, border_size, self.layers)

    def f(self, pts):
        """f(p) through the EXISTING device call: the model's altitude, the heights of tree.sample_attachment"""
        pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
        return RM.altitude(self.omodel, pts) - self.tree.sample_attachment(0, pts)[1].astype(np.float64)


@pytest.fixture(scope="module")
def terrains(device, tmp_path_factory):
    cache = {}

    def get(kind):
        if kind not in cache:
            cache[kind] = Streamed(device, tmp_path_factory.mktemp(kind), kind)
        return cache[kind]

    return get


# ---- 1. equality with the model ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["planar", "sphere", "ellipsoid"])
@pytest.mark.parametrize("steps,rounds", [(256, 2), (1, 4), (63, 0), (64, 1), (65, 4), (256, 0)])
def test_hits_equal_the_model(terrains, kind, steps, rounds):
    """every ray, no exclusions: status, step, and the bits of t, t_above, position and height.  (steps, refine_rounds) pairs cover
    steps in {1, 63, 64, 65, 256} and refine_rounds in {0, 1, 2, 4}.)"""
    s = terrains(kind)
    n = 200 if steps == 256 else 80
    origins, directions, t_min, t_max = make_rays(s.omodel, s.view, n, seed=100 + steps)
    exp = RM.raycast(s.omodel, s.sample, origins, directions, t_min, t_max, steps, rounds)
    assert_mix(exp, steps)
    got = s.tree.raycast(0, origins, directions, t_min, t_max, steps=steps, refine_rounds=rounds)
    assert_hits_equal(got, exp)


# ---- 2. agreement with the existing API, independent of the model's march ----------------------------------------------------------------

@pytest.mark.parametrize("kind", ["planar", "sphere", "ellipsoid"])
def test_hits_agree_with_sample_attachment(terrains, kind):
    s = terrains(kind)
    steps, rounds = 96, 2
    origins, directions, t_min, t_max = make_rays(s.omodel, s.view, 120, seed=7)
    got = s.tree.raycast(0, origins, directions, t_min, t_max, steps=steps, refine_rounds=rounds)
    hit = got["status"] == _ffi.RAY_HIT
    assert hit.sum() >= 24 and (got["status"] == _ffi.RAY_MISS).sum() >= 24 and (got["status"] == _ffi.RAY_INSIDE).sum() >= 24
    # the reported height is what sample_attachment returns at the reported position, bit for bit; f <= 0 there, f > 0 at p(t_above)
    at_hit = (hit | (got["status"] == _ffi.RAY_INSIDE))
    heights = s.tree.sample_attachment(0, got["position"][at_hit])[1]
    assert heights.tobytes() == np.ascontiguousarray(got["height"][at_hit]).tobytes()
    assert (s.f(got["position"][at_hit]) <= 0.0).all()
    assert np.array_equal(got["position"][at_hit], origins[at_hit] + got["t"][at_hit, None] * directions[at_hit])
    assert (s.f(origins[hit] + got["t_above"][hit, None] * directions[hit]) > 0.0).all()
    assert (got["t_above"][hit] < got["t"][hit]).all()
    # brute force: no coarse step before the hit step is at or under the ground; a MISS has none at all
    dt = (t_max - t_min) / np.float64(steps)
    for r in range(len(origins)):
        last = {_ffi.RAY_HIT: int(got["step"][r]), _ffi.RAY_INSIDE: 0, _ffi.RAY_MISS: steps + 1}[int(got["status"][r])]
        t = t_min[r] + np.arange(steps + 1, dtype=np.float64) * dt[r]
        f = s.f(origins[r][None, :] + t[:, None] * directions[r][None, :])
        assert not (f[:last] <= 0.0).any(), r
        if last <= steps:
            assert f[last] <= 0.0, r
            lo_t = t[last - 1] if last else t_min[r]
            assert lo_t <= got["t_above"][r] <= got["t"][r] <= t[last], r


# ---- 3. nothing loaded -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["planar", "sphere"])
def test_nothing_loaded_is_the_min_height_surface(device, kind):
    model, omodel = MODELS[kind]
    cfg = bt.TerrainConfig(lod_count=LODS, atlas_size=16, path="terrains/none", model=model)
    cfg.add_attachment(bt.AttachmentConfig(name="height", texture_size=T, border_size=B, format=bt.AttachmentFormat.R16))
    atlas = bt.TileAtlas.new(cfg, device)
    tree = bt.TileTree.new(atlas, bt.TerrainViewConfig(tree_size=4))
    pos = np.array([float(omodel.position[i]) for i in range(3)])
    lo = float(omodel.min_height)
    rng = np.random.default_rng(3)
    n = 64
    if kind == "planar":
        origins = pos + np.column_stack([rng.uniform(-400, 400, n), rng.uniform(300, 900, n), rng.uniform(-400, 400, n)])
        d = _unit(np.column_stack([rng.normal(size=n), -np.abs(rng.normal(size=n)) - 0.3, rng.normal(size=n)]))
        exact = (pos[1] + lo - origins[:, 1]) / d[:, 1]
        slack = 64.0 * np.spacing(4000.0)
    else:
        radius = float(omodel.a) + lo
        u = _unit(rng.normal(size=(n, 3)))
        origins = pos + u * (radius + rng.uniform(2.0e4, 3.0e5, (n, 1)))
        d = _unit(-u + rng.normal(size=(n, 3)) * 0.3)
        od = np.einsum("ij,ij->i", origins - pos, d)
        exact = -od - np.sqrt(od ** 2 - (np.einsum("ij,ij->i", origins - pos, origins - pos) - radius ** 2))
        slack = 64.0 * np.spacing(4.0 * 6.4e6)  # tests/test_raycast_model.py derives it
    t_max = 1.5 * exact.max()
    got = tree.raycast(0, origins, d, 0.0, t_max, steps=256, refine_rounds=2)
    assert (got["status"] == _ffi.RAY_HIT).all() and (got["height"] == np.float32(lo)).all()
    assert (got["t_above"] - slack <= exact).all() and (exact <= got["t"] + slack).all()
    assert np.allclose(got["t"] - got["t_above"], t_max / 256 / 4096, rtol=1e-6, atol=0)
    assert np.array_equal(tree.sample_attachment(0, got["position"])[1], got["height"])


# ---- 3b. the ceiling above which a sample fetches nothing ------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["planar", "sphere"])
def test_ground_at_max_height_is_met_at_the_ceiling(device, tmp_path, monkeypatch, kind):
    """every texel 65535: the ground is at max_height, exactly the ceiling above which the kernel skips the fetch.  Rays come straight down in
    steps of a power of two so that (planar: exactly) step 64 lands on the ceiling and steps 0 .. 63 just above it: a kernel that skipped at
    `altitude >= ceiling`, or whose ceiling were a rounding above what the sampling chain returns for value 1, would report a later hit."""
    import _cases as K
    monkeypatch.setattr(K, "smooth_raster", lambda h, w, seed, device=None: np.full((h, w), 65535, np.uint16))
    s = Streamed(device, tmp_path, kind)
    assert all((layer == 65535).all() for layer in s.layers.values())
    pos = np.array([float(s.omodel.position[i]) for i in range(3)])
    hi = float(s.omodel.max_height)
    rng = np.random.default_rng(8)
    n = 48
    delta = 2.0 ** rng.integers(-30 if kind == "planar" else -8, 3, n).astype(np.float64)  # (the sphere's |p| ~ 6.4e6 has an ulp of 1e-9)
    if kind == "planar":
        up = np.tile([0.0, 1.0, 0.0], (n, 1))
        ground = pos + np.column_stack([rng.uniform(-450, 450, n), np.zeros(n), rng.uniform(-450, 450, n)])
    else:
        up = _unit(_unit(np.asarray(s.view) - pos) + rng.normal(size=(n, 3)) * 0.2)
        ground = pos + up * float(s.omodel.a)
    origins = ground + up * (hi + 64.0 * delta)[:, None]
    exp = RM.raycast(s.omodel, s.sample, origins, -up, 0.0, 128.0 * delta, 128, 2)
    assert (exp["status"] == RM.HIT).all() and (exp["height"] == np.float32(hi)).all()
    if kind == "planar":  # exact arithmetic: the sample of step 64 has f == 0, every u_k of both refinement rounds f > 0
        assert (exp["step"] == 64).all() and (exp["t"] == 64.0 * delta).all() and (exp["t_above"] == (64.0 - 1.0 / 4096.0) * delta).all()
        assert (RM.f_values(s.omodel, s.sample, exp["position"]) == 0.0).all()
    else:  # radial rays on the sphere: the same to within the roundings of |p|
        assert (np.abs(exp["step"].astype(np.int64) - 64) <= 1).all()
    got = s.tree.raycast(0, origins, -up, 0.0, 128.0 * delta, steps=128, refine_rounds=2)
    assert_hits_equal(got, exp)
    assert np.array_equal(s.tree.sample_attachment(0, got["position"])[1], got["height"])


# ---- 4. a read ---------------------------------------------------------------------------------------------------------------------------

def test_raycast_is_a_read(device, terrains):
    """like test_gpu_tile_bounds.test_reads_are_not_writes: a raycast against an atlas nothing has written leaves Attachment::written alone,
    so the job with no-data texels that follows takes prev_zero as often as it does without the call; and a raycast on a loaded atlas leaves
    every layer's bytes unchanged"""
    from test_gpu_tile_bounds import holed_job
    counts = []
    for read_first in (False, True):
        atlas, pre = holed_job(device)
        if read_first:
            tree = bt.TileTree.new(atlas, bt.TerrainViewConfig(tree_size=4))
            model = atlas.config.model
            o = np.array(model.translation, dtype=np.float64) + [0.0, float(model.max_height) + 10.0, 0.0]
            hits = tree.raycast(0, [o, o], [(0.0, -1.0, 0.0), (1.0, 0.0, 0.0)], 0.0, float(model.max_height - model.min_height) + 20.0)
            assert list(hits["status"]) == [_ffi.RAY_HIT, _ffi.RAY_MISS] and hits["height"][0] == np.float32(model.min_height)
        pre.run(atlas)
        counts.append(pre.stats()["prev_zero_launches"])
    assert counts[0] > 0 and counts[1] == counts[0], counts
    s = terrains("planar")
    used = max(s.layers) + 1
    before = s.atlas.download_tiles(0, 0, used).copy()
    origins, directions, t_min, t_max = make_rays(s.omodel, s.view, 64, seed=9)
    s.tree.raycast(0, origins, directions, t_min, t_max)
    assert np.array_equal(s.atlas.download_tiles(0, 0, used), before)


# ---- 5. limits and hostile input ---------------------------------------------------------------------------------------------------------

def test_limits_and_hostile_input(device, terrains):
    L = _ffi.lib()
    s = terrains("planar")
    origins, directions, t_min, t_max = make_rays(s.omodel, s.view, 32, seed=21)
    clean = s.tree.raycast(0, origins, directions, t_min, t_max, steps=64, refine_rounds=1)
    rays = np.zeros(32, bt.tile_tree.RAY_DTYPE)
    rays["origin"], rays["direction"], rays["t_min"], rays["t_max"] = origins, directions, t_min, t_max
    hits = np.zeros(32, bt.tile_tree.RAY_HIT_DTYPE)
    hits["step"] = 0x1234
    rp, hp = rays.ctypes.data_as(C.POINTER(_ffi.RayC)), hits.ctypes.data_as(C.POINTER(_ffi.RayHitC))
    tree, atlas = s.tree._h, s.atlas._h
    cap = _ffi.RAYCAST_MAX_SAMPLES
    # the cap counts a ray's samples in whole rounds of 64: 1025 rounds at steps 65536 (255 rays fit), one round up to steps 63, two at steps 64
    refused = {"steps 0": (0, 32, 0, 2), "steps 65537": (0, 32, 65537, 2), "refine_rounds 5": (0, 32, 64, 5), "attachment 1": (1, 32, 64, 1),
               "sample cap, 1025 rounds": (0, cap // (1025 * 64) + 1, 65536, 0), "sample cap, one round of two samples": (0, cap // 64 + 1, 1, 0),
               "sample cap, one full round": (0, cap // 64 + 1, 63, 0), "sample cap, two rounds": (0, cap // 128 + 1, 64, 0)}
    assert cap // (1025 * 64) == 255 and cap // 64 == 262144
    for what, (ai, count, steps, rounds) in refused.items():
        assert L.bt_tile_tree_raycast(tree, atlas, ai, rp, count, steps, rounds, hp) == BT_ERR_INVALID_ARGUMENT, what
        assert L.bt_last_error(), what
    assert L.bt_tile_tree_raycast(tree, atlas, 0, None, 32, 64, 1, hp) == BT_ERR_INVALID_ARGUMENT
    assert L.bt_tile_tree_raycast(tree, atlas, 0, rp, 32, 64, 1, None) == BT_ERR_INVALID_ARGUMENT
    assert L.bt_tile_tree_raycast(None, atlas, 0, rp, 32, 64, 1, hp) == BT_ERR_INVALID_ARGUMENT
    assert L.bt_tile_tree_raycast(tree, None, 0, rp, 32, 64, 1, hp) == BT_ERR_INVALID_ARGUMENT
    assert L.bt_tile_tree_raycast(tree, atlas, 0, rp, 0, 64, 1, hp) == _ffi.BT_OK
    assert L.bt_tile_tree_raycast(tree, atlas, 0, None, 0, 64, 1, None) == _ffi.BT_OK
    assert (hits["step"] == 0x1234).all()  # nothing was touched by any of the above
    # an Rgba8 attachment
    cfg = bt.TerrainConfig(lod_count=2, atlas_size=8, path="terrains/rgba", model=s.model)
    cfg.add_attachment(bt.AttachmentConfig(name="albedo", texture_size=16, border_size=2, format=bt.AttachmentFormat.Rgba8))
    rgba = bt.TileAtlas.new(cfg, device)
    rgba_tree = bt.TileTree.new(rgba, bt.TerrainViewConfig(tree_size=4))
    assert L.bt_tile_tree_raycast(rgba_tree._h, rgba._h, 0, rp, 32, 64, 1, hp) == BT_ERR_UNSUPPORTED
    assert (hits["step"] == 0x1234).all()
    # the smallest march: 2 samples per ray
    assert L.bt_tile_tree_raycast(tree, atlas, 0, rp, 32, 1, 0, hp) == _ffi.BT_OK
    # the largest batch the cap lets through (262144 rays of one round): accepted, and every ray answered like its copy among the 32
    many = np.tile(np.arange(32), cap // 64 // 32)
    big = s.tree.raycast(0, origins[many], directions[many], t_min[many], t_max[many], steps=63, refine_rounds=1)
    small = s.tree.raycast(0, origins, directions, t_min, t_max, steps=63, refine_rounds=1)
    assert len(big) == cap // 64 and big.tobytes() == small[many].tobytes()
    # INVALID rays mixed into a batch leave their neighbours' results unchanged
    bad = {3: ("origin", (np.nan, 0.0, 0.0)), 4: ("direction", (0.0, 0.0, 0.0)), 11: ("direction", (np.inf, 0.0, 0.0)), 12: ("t_max", -np.inf),
           13: ("t_min", np.nan), 30: ("t_max", -1.0), 31: ("origin", (0.0, -np.inf, 0.0))}
    for i, (field, value) in bad.items():
        rays[field][i] = value
    mixed = s.tree.raycast(0, rays["origin"], rays["direction"], rays["t_min"], rays["t_max"], steps=64, refine_rounds=1)
    keep = np.array([i not in bad for i in range(32)])
    assert mixed[keep].tobytes() == clean[keep].tobytes()
    assert (mixed["status"][~keep] == _ffi.RAY_INVALID).all()
    zero = np.zeros(1, bt.tile_tree.RAY_HIT_DTYPE)
    zero["status"] = _ffi.RAY_INVALID
    assert all(mixed[i:i + 1].tobytes() == zero.tobytes() for i in bad)
    # the scratch stays in the context until bt_ctx_trim, and the call works again after it
    assert device.trim() > 0
    again = s.tree.raycast(0, origins, directions, t_min, t_max, steps=64, refine_rounds=1)
    assert again.tobytes() == clean.tobytes()
    # the one-ray convenience
    o = np.array(s.view) + [0.0, 600.0, 0.0]
    found = bt.raycast_terrain(s.tree, s.atlas, o, (0.0, -2.0, 0.0), 2000.0)
    assert found is not None and found[0][0] == o[0] and found[0][2] == o[2]
    assert float(s.tree.sample_attachment(0, [found[0]])[1][0]) >= found[0][1] - float(s.omodel.position[1])
    assert bt.raycast_terrain(s.tree, s.atlas, o, (0.0, 1.0, 0.0), 2000.0) is None

"""bt_tile_tree_raycast without a GPU: the CPU model of its definition (tests/_raycast_model.py, h from the oracle's sample_attachment)
against closed forms, so that model and kernel cannot share a misreading; the statuses; the entry point's NULL-handle refusal.

On a terrain whose tiles all hold one value v the ground is the plane y = position.y + h (planar) or the sphere of radius a + h about the
model's position (sphere), h = f32 lerp(min_height, max_height, v / 65535): the analytic t of the ray / plane or ray / sphere meeting must
lie inside [t_above, t], and t - t_above must be dt / 64^R.

Slack, from the f64 arithmetic alone: f(p) is formed from coordinates of magnitude M (1e3 planar, 6.4e6 sphere) with a handful of roundings,
an absolute error of a few ulp(M) in altitude; a ray that approaches the ground at |cos| >= 0.1 to the vertical turns that into at most
10x as much in t, and t itself (up to a few M) carries its own ulps.  64 ulp(4 M) covers both with room: 1.5e-11 planar, 6e-8 sphere —
thirteen digits below the bracket widths tested."""
import ctypes as C
import math

import numpy as np
import pytest

import _oracle as O
import _raycast_model as RM
from test_tile_tree_host import MODELS

T, B, LODS, VALUE = 16, 2, 3, 40000


def constant_terrain(kind, value=VALUE, load=True):
    """an oracle tree two frames into streaming a terrain whose every tile is `value` (LOD 0 is always loaded, so every position resolves)"""
    _, om = MODELS[kind]
    sides = 1 if kind == "planar" else 6
    existing = [(s, l, x, y) for s in range(sides) for l in range(LODS) for x in range(2 ** l) for y in range(2 ** l)]
    stream = O.Stream(len(existing) + 8, 1, existing=existing if load else [])
    otree = O.TileTree(om, LODS, O.make_view_config(tree_size=4, load_distance=1.2, blend_distance=1.0))
    view = (10.0, 300.0, 3.0) if kind == "planar" else (0.4 * 6.4e6, 0.8 * 6.4e6, 0.45 * 6.4e6)
    layers = {}
    for _ in range(2):
        otree.update(view)
        for _, index in stream.finish_loads(stream.pending_loads()):
            layers[index] = np.full((T, T), value, np.uint16)
        otree.apply_requests(stream)
        otree.adjust_to_tile_atlas(stream)
    h = float(np.float32(om.min_height) + (np.float32(om.max_height) - np.float32(om.min_height)) * (np.float32(value if load else 0) / np.float32(65535.0)))
    return om, RM.sampler(otree, T, B, layers), h, view


def ulp_slack(magnitude):
    return 64.0 * np.spacing(4.0 * magnitude)


@pytest.mark.parametrize("steps,rounds", [(64, 0), (256, 2), (100, 1), (1, 4)])
def test_planar_hits_bracket_the_ray_plane_meeting(steps, rounds):
    om, sample, h, _ = constant_terrain("planar")
    assert float(sample(np.array([[1.0, 2.0, 3.0]]))[0]) == h
    rng = np.random.default_rng(11)
    n = 50
    origins = np.column_stack([rng.uniform(-480, 480, n) + 10.0, rng.uniform(300.0, 900.0, n), rng.uniform(-480, 480, n) + 3.0])
    d = rng.normal(size=(n, 3))
    d[:, 1] = -np.abs(d[:, 1]) - 0.2
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = d[np.abs(d[:, 1]) >= 0.1]
    origins = origins[:len(d)]
    ground = float(om.position[1]) + h
    exact = (ground - origins[:, 1]) / d[:, 1]
    t_max = 1.7 * exact.max()
    hits = RM.raycast(om, sample, origins, d, 0.0, t_max, steps, rounds)
    assert (hits["status"] == RM.HIT).all()
    slack = ulp_slack(1000.0)
    assert (hits["t_above"] - slack <= exact).all() and (exact <= hits["t"] + slack).all()
    width = (t_max / steps) / 64.0 ** rounds
    assert (np.abs((hits["t"] - hits["t_above"]) / width - 1.0) < 1e-9).all()
    assert (hits["height"] == np.float32(h)).all()
    dt = t_max / steps
    assert ((hits["step"] - 1) * dt - slack <= exact).all() and (exact <= hits["step"] * dt + slack).all()
    assert np.allclose(hits["position"][:, 1], ground, atol=width * 1.0 + slack, rtol=0)


@pytest.mark.parametrize("steps,rounds", [(256, 2), (65, 1)])
def test_sphere_hits_bracket_the_ray_sphere_meeting(steps, rounds):
    om, sample, h, view = constant_terrain("sphere")
    radius = float(om.a) + h
    rng = np.random.default_rng(12)
    n = 40
    up = np.asarray(view) / np.linalg.norm(view)
    origins, dirs, exact = [], [], []
    while len(origins) < n:
        u = up + rng.normal(size=3) * 0.05
        u /= np.linalg.norm(u)
        o = u * (radius + rng.uniform(2.0e4, 3.0e5))
        d = -u + rng.normal(size=3) * 0.6
        d /= np.linalg.norm(d)
        # |o + t d|^2 = radius^2: t = -o.d - sqrt((o.d)^2 - (|o|^2 - radius^2)), the first meeting from outside
        od, disc = float(o @ d), float(o @ d) ** 2 - (float(o @ o) - radius ** 2)
        if disc <= 0:
            continue
        t = -od - math.sqrt(disc)
        p = o + t * d
        if t <= 0.0 or abs(float(p @ d)) / radius < 0.1:  # pointing away; grazing: outside the slack's premise
            continue
        origins.append(o), dirs.append(d), exact.append(t)
    origins, dirs, exact = np.array(origins), np.array(dirs), np.array(exact)
    t_max = 1.3 * exact.max()
    hits = RM.raycast(om, sample, origins, dirs, 0.0, t_max, steps, rounds)
    assert (hits["status"] == RM.HIT).all()
    slack = ulp_slack(6.4e6)
    assert (hits["t_above"] - slack <= exact).all() and (exact <= hits["t"] + slack).all()
    width = (t_max / steps) / 64.0 ** rounds
    # t and t_above each carry a few roundings of magnitude ulp(t_max): 8 of them against the width
    assert (np.abs((hits["t"] - hits["t_above"]) - width) <= 8.0 * np.spacing(t_max)).all()
    assert np.allclose(np.linalg.norm(hits["position"], axis=1), radius, atol=width + slack, rtol=0)


def test_nothing_loaded_is_the_min_height_surface():
    om, sample, h, _ = constant_terrain("planar", load=False)
    assert h == float(om.min_height)
    hits = RM.raycast(om, sample, [(10.0, 95.0, 3.0)], [(0.6, -0.8, 0.0)], 0.0, 200.0, 256, 2)
    exact = (float(om.position[1]) + h - 95.0) / -0.8
    assert hits["status"][0] == RM.HIT and hits["t_above"][0] - 1e-11 <= exact <= hits["t"][0] + 1e-11 and hits["height"][0] == np.float32(h)


def test_statuses():
    om, sample, h, _ = constant_terrain("planar")
    top = float(om.position[1]) + float(om.max_height)
    ground = float(om.position[1]) + h
    # above max_height throughout: MISS, and every other field 0
    miss = RM.raycast(om, sample, [(0.0, top + 1.0, 0.0)] * 2, [(1.0, 0.0, 0.0), (0.6, 0.8, 0.0)], 0.0, 5000.0, 256, 2)
    assert (miss["status"] == RM.MISS).all() and not miss["t"].any() and not miss["position"].any() and not miss["step"].any()
    # a ray that stops short of the ground
    assert RM.raycast(om, sample, [(0.0, ground + 100.0, 0.0)], [(0.0, -1.0, 0.0)], 0.0, 99.0, 64, 1)["status"][0] == RM.MISS
    # an origin under the ground: INSIDE at t_min, whatever the direction
    inside = RM.raycast(om, sample, [(0.0, ground - 10.0, 0.0)] * 2, [(0.0, 1.0, 0.0), (1.0, -1.0, 0.0)], 2.5, 500.0, 256, 4)
    assert (inside["status"] == RM.INSIDE).all() and (inside["t"] == 2.5).all() and (inside["t_above"] == 2.5).all() and (inside["step"] == 0).all()
    assert np.array_equal(inside["position"][0], [0.0, ground - 10.0 + 2.5, 0.0]) and (inside["height"] == np.float32(h)).all()
    # a hit exactly on a step is reported at that step: from ground + 32 straight down in 64 steps of 1, f == 0 at step 32
    on_step = RM.raycast(om, sample, [(0.0, ground + 32.0, 0.0)], [(0.0, -1.0, 0.0)], 0.0, 64.0, 64, 0)[0]
    assert on_step["status"] == RM.HIT and on_step["step"] == 32 and on_step["t"] - on_step["t_above"] == 1.0
    # malformed rays
    bad = [((np.nan, 0, 0), (0, -1, 0), 0.0, 1.0), ((0, 0, 0), (0, np.inf, 0), 0.0, 1.0), ((0, 0, 0), (0, 0, 0), 0.0, 1.0),
           ((0, 900, 0), (0, -1, 0), 5.0, 4.0), ((0, 900, 0), (0, -1, 0), 0.0, np.inf), ((0, 900, 0), (0, -1, 0), -np.inf, 1.0),
           ((0, 900, 0), (0, -1, 0), np.nan, 1.0)]
    for o, d, t0, t1 in bad:
        r = RM.raycast(om, sample, [o], [d], t0, t1, 16, 1)[0]
        assert r["status"] == RM.INVALID and r["t"] == 0 and r["step"] == 0, (o, d, t0, t1)
    # t_max == t_min is a valid one-point ray
    assert RM.raycast(om, sample, [(0.0, ground - 1.0, 0.0)], [(0, 1, 0)], 1.0, 1.0, 4, 1)["status"][0] == RM.INSIDE
    # the centre of a sphere: f is NaN there, which is "not hit"
    som, ssample, _, _ = constant_terrain("sphere")
    assert np.isnan(RM.f_values(som, ssample, [(0.0, 0.0, 0.0)])[0])
    assert RM.raycast(som, ssample, [(0.0, 0.0, 0.0)], [(1.0, 0.0, 0.0)], 0.0, 0.0, 1, 0)["status"][0] == RM.MISS


def test_ellipsoid_altitude_is_measured_from_the_projected_point():
    """on the ellipsoid's surface the altitude is 0, and moving out along the model's displacement direction by d gives d"""
    # (centred on the origin: the reference subtracts the translation twice on this path, which shifts a translated ellipsoid's zero level)
    om = O.make_model("ellipsoidal", (0.0, 0.0, 0.0), 6378137.0, 6356752.314245, -12000.0, 9000.0)
    a, b = float(om.a), float(om.b)
    pos = np.array([float(om.position[i]) for i in range(3)])
    rng = np.random.default_rng(5)
    for _ in range(20):
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        surface = pos + u * np.array([a, b, a])
        assert abs(RM.altitude(om, [surface])[0]) < 1e-6
        up = surface - pos  # the geometric normal direction differs from the model's by design; along the radial line the altitude grows monotonically
        far = RM.altitude(om, [surface + up / np.linalg.norm(up) * 5000.0])[0]
        assert 4900.0 < far < 5000.0 + 1e-6


def test_null_handles_are_refused_without_a_device():
    from bevy_terrain_amd import _ffi
    assert "bt_tile_tree_raycast" in _ffi.header_symbols() and "bt_tile_tree_raycast" in _ffi.PROTOTYPES
    assert C.sizeof(_ffi.RayC) == 64 and C.sizeof(_ffi.RayHitC) == 56
    L = _ffi.lib()
    rays, hits = (_ffi.RayC * 1)(), (_ffi.RayHitC * 1)()
    assert L.bt_tile_tree_raycast(None, None, 0, rays, 1, 256, 2, hits) == -1  # BT_ERR_INVALID_ARGUMENT
    assert b"NULL" in L.bt_last_error()
    assert L.bt_tile_tree_raycast(None, None, 0, None, 0, 0, 0, None) == -1  # before the count check
    from bevy_terrain_amd import tile_tree
    assert tile_tree.RAY_DTYPE.itemsize == C.sizeof(_ffi.RayC) and tile_tree.RAY_HIT_DTYPE.itemsize == C.sizeof(_ffi.RayHitC)
    for name, _ in _ffi.RayHitC._fields_:
        assert tile_tree.RAY_HIT_DTYPE.fields[name][1] == getattr(_ffi.RayHitC, name).offset, name

"""The high-precision terrain geometry without a GPU: bt_model_approximation_from_config (host code, f64) byte for byte against the model
of its definition (tests/_hp_model.py), the model's coefficients against central differences of the f64 surface function, the accuracy of
the hp vertex against f64 truth next to the plain vertex's, the model at threshold 0 against _geometry_model, and the reach of the scenes
test_gpu_hp_geometry.py compares (tests/_hp_cases.py), and of the long lists test_gpu_geometry_trips.py sends through the hp calls."""
import ctypes as C

import numpy as np
import pytest

import _geometry_cases as GC
import _geometry_model as GM
import _hp_cases as HC
import _hp_model as HM
import bevy_terrain_amd as bt
from bevy_terrain_amd import _ffi
from bevy_terrain_amd.tile_tree import model_c, view_config_c
from test_tile_tree_host import struct_bytes

BT_ERR_INVALID_ARGUMENT, BT_ERR_UNSUPPORTED = -1, -5

# Measured with the model on the deep scene (_hp_cases.deep_scene: LOD 15 tiles out to the default threshold of 0.001 scales under a view
# 2 m above the ground, BT_GEOMETRY_VIEW_RELATIVE), worst component of |position - f64 truth| in metres over the hp vertices: the series'
# cubic remainder at 6.4 km plus binary32 rounding.  PLAIN: _geometry_model's world position on the same vertices.
HP_ERROR = {"sphere": 2.04e-3, "ellipsoid": 2.34e-3}
PLAIN_ERROR = {"sphere": 0.933, "ellipsoid": 1.035}


def view_positions(kind):
    """views over all six faces, the axis, face-edge and corner positions of test_tile_tree_host, and random ones, about the model's centre"""
    centre = np.array(GC.MODELS[kind][0].translation)
    r = 7.0e6
    pts = [(r, 0, 0), (-r, 0, 0), (0, r, 0), (0, -r, 0), (0, 0, r), (0, 0, -r), (r, r, 0.5 * r), (-r, 0.3 * r, -r), (r, r, r)]
    pts += [(0.9 * r, 0.1 * r, -0.2 * r), (-0.9 * r, 0.3 * r, 0.1 * r), (0.2 * r, 0.1 * r, 0.95 * r), (0.2 * r, -0.3 * r, -0.95 * r), (0.1 * r, 0.92 * r, 0.3 * r), (-0.3 * r, -0.92 * r, 0.2 * r)]
    rng = np.random.default_rng(17)
    d = rng.normal(size=(40, 3))
    pts += list(d / np.linalg.norm(d, axis=1, keepdims=True) * (6371000.0 + rng.uniform(2.0, 5.0e6, size=(40, 1))))
    return [tuple(float(v) for v in centre + np.array(p, np.float64)) for p in pts]


@pytest.mark.parametrize("kind", HC.KINDS)
def test_coefficients_are_byte_equal_to_the_model(kind):
    model = GC.MODELS[kind][0]
    assert C.sizeof(_ffi.ModelApproximationC) == 448 and C.sizeof(_ffi.SideCoefficientsC) == 72
    sides = set()
    for origin_lod, threshold in ((10, 0.001), (3, 0.05), (0, 10.0), (31, 0.0)):
        vc = bt.TerrainViewConfig(origin_lod=origin_lod, precision_threshold_distance=threshold)
        for p in view_positions(kind):
            ours = bt.model_approximation_from_config(model, vc, p)
            exp = HM.approximation(model, vc, p)
            assert struct_bytes(ours) == HM.approximation_bytes(exp), (origin_lod, p)
            assert ours.origin_lod == origin_lod and ours.precision_threshold_distance == np.float32(threshold * (model.scale_vec[0] + model.scale_vec[1]) / 2.0)
            sides.add(HM.coefficients64(model, p)[0])
    assert sides == set(range(6))


def test_from_config_refusals():
    L = _ffi.lib()
    model, vc = model_c(GC.MODELS["sphere"][0]), view_config_c(bt.TerrainViewConfig())
    pos = (C.c_double * 3)(7.0e6, 1.0e5, -2.0e5)
    out = _ffi.ModelApproximationC()
    before = struct_bytes(out)
    call = L.bt_model_approximation_from_config
    assert call(C.byref(model), C.byref(vc), pos, C.byref(out)) == _ffi.BT_OK and struct_bytes(out) != before
    out = _ffi.ModelApproximationC()
    for args in ((None, C.byref(vc), pos, C.byref(out)), (C.byref(model), None, pos, C.byref(out)), (C.byref(model), C.byref(vc), None, C.byref(out)),
                 (C.byref(model), C.byref(vc), pos, None)):
        assert call(*args) == BT_ERR_INVALID_ARGUMENT and L.bt_last_error()
    for bad in (float("nan"), float("inf"), -float("inf")):
        for axis in range(3):
            p = (C.c_double * 3)(7.0e6, 1.0e5, -2.0e5)
            p[axis] = bad
            assert call(C.byref(model), C.byref(vc), p, C.byref(out)) == BT_ERR_INVALID_ARGUMENT
    deep = view_config_c(bt.TerrainViewConfig(origin_lod=32))
    assert call(C.byref(model), C.byref(deep), pos, C.byref(out)) == BT_ERR_INVALID_ARGUMENT and b"origin_lod" in L.bt_last_error()
    planar = model_c(GC.MODELS["planar"][0])
    assert call(C.byref(planar), C.byref(vc), pos, C.byref(out)) == BT_ERR_UNSUPPORTED and b"planar" in L.bt_last_error()
    broken = model_c(GC.MODELS["sphere"][0])
    broken.a = 0.0
    assert call(C.byref(broken), C.byref(vc), pos, C.byref(out)) == BT_ERR_INVALID_ARGUMENT
    assert struct_bytes(out) == before  # no refusal wrote anything
    with pytest.raises(_ffi.BtError):
        bt.model_approximation_from_config(GC.MODELS["planar"][0], bt.TerrainViewConfig(), (1.0, 2.0, 3.0))


@pytest.mark.parametrize("kind", HC.KINDS)
def test_coefficients_agree_with_central_differences(kind):
    """f(s, t) = Coordinate::world_position of the side at height 0, f64.  With step h the central differences carry a truncation error of
    h^2 / 6 f''' (first), h^2 / 12 f'''' (second) and h^2 / 6 (f_sss t + f_stt t) (mixed), and a rounding error of about 2^-52 |f| / h
    resp. 4 * 2^-52 |f| / h^2.  Every derivative of the cube-sphere map up to the fourth is below 64 scales here, so with h = 2^-10 the
    truncation stays below 64 / 6 * h^2 = 1.0e-5 scales and the rounding below 4 * 2^-52 * 2 / h^2 = 1.9e-9 scales: the tolerance is
    2e-5 scales, absolute, for every component; a coefficient that is wrong (a sign, a missing halving, a swapped axis) is wrong by a
    large fraction of a scale."""
    model = GC.MODELS[kind][0]
    tm = HM.tree_model(model)
    h = 2.0 ** -10
    scale = max(model.scale_vec)
    tolerance = 2e-5 * scale
    worst = 0.0
    for p in view_positions(kind)[:15] + view_positions(kind)[-6:]:
        _, st, c64 = HM.coefficients64(model, p)
        for side in range(6):
            s, t = st[side]
            f = lambda ds, dt: tm.world_position(side, np.array([s + ds * h, t + dt * h]), 0.0)
            fd = [f(0, 0) - np.array(p),
                  (f(1, 0) - f(-1, 0)) / (2.0 * h), (f(0, 1) - f(0, -1)) / (2.0 * h),
                  (f(1, 0) - 2.0 * f(0, 0) + f(-1, 0)) / (h * h) / 2.0,
                  (f(1, 1) - f(1, -1) - f(-1, 1) + f(-1, -1)) / (4.0 * h * h),
                  (f(0, 1) - 2.0 * f(0, 0) + f(0, -1)) / (h * h) / 2.0]
            error = np.abs(np.array(fd) - c64[side])
            worst = max(worst, float(error.max()))
            assert (error[0] <= 1e-6).all(), (p, side, error[0])  # the constant: the same point, both in f64
            assert (error <= tolerance).all(), (p, side, HM.NAMES[int(np.argmax(error.max(axis=1)))], error.max(), tolerance)
            assert np.abs(c64[side][1:]).max() > 0.1 * scale  # (the tolerance is small against what it bounds)
    print(kind, "worst difference to central differences %.3g m, tolerance %.3g m" % (worst, tolerance))


@pytest.mark.parametrize("kind", HC.KINDS)
def test_accuracy_against_f64_truth(kind):
    c = HC.deep_scene(kind)
    assert np.float32(c.approximation.precision_threshold_distance) == np.float32(0.001 * (c.model.scale_vec[0] + c.model.scale_vec[1]) / 2.0)
    v, trace, _ = HC.deep_expected(kind, HM.VIEW_RELATIVE | GM.GRID)
    hp = trace["hp"]
    assert hp.sum() > 2500 and (~hp).any() and (v["height"] == 0.0).all()
    assert v["view_distance"][hp].min() < 20.0 and v["view_distance"][hp].max() > 0.95 * float(c.approximation.precision_threshold_distance)
    truth = HM.truth(c.model, c.tiles, v["coordinate_uv"])
    hp_error = np.abs(v["position"].astype(np.float64) - (truth - np.array(c.position))).max(axis=-1)[hp].max()
    plain, _, _ = GM.geometry(c.view, c.P, c.entries, {}, GC.T, GC.B, c.tiles, GM.GRID)
    plain_error = np.abs(plain["position"].astype(np.float64) - HM.truth(c.model, c.tiles, plain["coordinate_uv"])).max(axis=-1)[hp].max()
    print(kind, "hp error %.4g m, plain error %.4g m, ratio %.0f" % (hp_error, plain_error, plain_error / hp_error))
    assert hp_error <= 4.0 * HP_ERROR[kind]
    assert hp_error * 64.0 <= plain_error
    assert 0.5 * PLAIN_ERROR[kind] <= plain_error <= 2.0 * PLAIN_ERROR[kind]  # (the recorded figure is what the plain path still gives)
    # without VIEW_RELATIVE the hp vertex is the series added to the f32 view position: the reference's form, back on the f32 lattice
    absolute, _, _ = HC.deep_expected(kind, GM.GRID)
    wp = np.array(list(c.view.world_position), np.float32)
    for name in GM.FIELDS:
        if name != "position":
            assert absolute[name].tobytes() == v[name].tobytes(), name
    assert np.array_equal(absolute["position"][hp], (wp + v["position"][hp]).astype(np.float32))  # (height 0: position is the base itself)


@pytest.mark.parametrize("kind,grid,flags", [("sphere", 5, 0), ("ellipsoid", 16, GM.GRID | GM.NO_BLEND), ("sphere", 4, GM.NO_MORPH)])
def test_threshold_zero_is_the_plain_geometry(kind, grid, flags):
    c = GC.scene(kind, grid, True)
    for n in range(3):
        exp, _, exp_admissible = GC.expected(kind, grid, True, n, flags)
        got, trace, admissible = HC.expected(kind, grid, 0.0, 10, flags, n)
        assert not trace["hp"].any()
        assert got.tobytes() == exp.tobytes() and np.array_equal(admissible, exp_admissible)


def test_the_compared_scenes_reach_every_branch():
    reach, flags_seen = set(), 0
    for kind, grid, threshold, origin_lod, flags, views in HC.COMPARED:
        flags_seen |= flags | (16 if not flags & GM.GRID else 0) | (32 if not flags & HM.VIEW_RELATIVE else 0)
        split = False
        for n in views:
            v, trace, admissible = HC.expected(kind, grid, threshold, origin_lod, flags, n)
            reach |= set(zip([kind] * trace["hp"].size, trace["hp"].ravel().tolist(), trace["dir_origin"].ravel().tolist(), trace["side"].ravel().tolist()))
            assert (~admissible).sum() * 1000 <= admissible.size, (kind, grid, threshold, n)
            assert np.isfinite(v["position"]).all()
            if threshold == HC.ALL:
                assert trace["hp"].all()
            # hp and other vertices in one tile and in one 64-lane wave of one trip over its grid vertices
            vi = trace["cy"] * (grid + 1) + trace["cx"]
            for k in range(len(vi)):
                for wave in range((grid + 1) ** 2 // 64 + 1):
                    m = vi[k] // 64 == wave
                    split |= bool(trace["hp"][k][m].any() and (~trace["hp"][k][m]).any())
        if threshold == HC.SPLIT:
            assert split, (kind, grid, flags)
    for kind in HC.KINDS:
        for flags in (0, HM.VIEW_RELATIVE):
            v, trace, admissible = HC.deep_expected(kind, flags)
            reach |= set(zip([kind] * trace["hp"].size, trace["hp"].ravel().tolist(), trace["dir_origin"].ravel().tolist(), trace["side"].ravel().tolist()))
            assert (~admissible).sum() * 1000 <= admissible.size
    assert flags_seen == 63  # both layouts, NO_MORPH, NO_BLEND, VIEW_RELATIVE on and off
    for kind in HC.KINDS:
        for hp in (False, True):
            for direction in (GM.UP, GM.NONE, GM.DOWN):
                assert any(r[:3] == (kind, hp, direction) for r in reach), (kind, hp, direction)
        assert {r[3] for r in reach if r[0] == kind and r[1]} == set(range(6))  # hp vertices on all six sides


def test_python_keywords():
    with pytest.raises(ValueError):
        bt.tile_tree._geometry_flags(False, True, True, None, True)
    assert bt.tile_tree._geometry_flags(True, False, True, object(), True) == 1 | 2 | 8 == _ffi.GEOMETRY_GRID | _ffi.GEOMETRY_NO_MORPH | _ffi.GEOMETRY_VIEW_RELATIVE
    assert bt.tile_tree._geometry_flags(False, True, True) == 0


# ---- the long lists of test_gpu_geometry_trips.py ------------------------------------------------------------------------------------------

def test_long_hp_lists():
    from test_geometry_model import assert_list_conditions, position_rows
    for kind, grid, threshold, origin_lod, flags, n, count, launches in HC.LONG:
        tiles = GC.long_tiles(kind, count)
        assert launches == GC.launches_of(grid, flags, count)
        assert_list_conditions(tiles, launches)
        exp, admissible, hp = HC.long_expected(kind, grid, threshold, origin_lod, flags, n, count)
        hp = hp[GC.long_index(kind, count)]
        assert exp.shape == hp.shape == (count, GC.slots_of(grid, flags))
        position = position_rows(exp)
        for step in (GC.TRIP, 2 * GC.TRIP):
            if count > step:
                assert (position[:count - step] != position[step:]).any(axis=1).all(), (kind, grid, step)
                # hp and plain vertices in the later trips too
                assert threshold != HC.SPLIT or (hp[step:].any() and not hp[step:].all() and (hp[step:].any(axis=1) & ~hp[step:].all(axis=1)).any())
        for c in np.cumsum(launches)[:-1]:
            assert (position[0] != position[c]).any() and (position[c - 1] != position[c]).any()
        assert hp.all() if threshold == HC.ALL else (hp.any() and not hp.all())
        print(kind, grid, threshold, count, "vertices", hp.size, "hp", int(hp.sum()), "inadmissible", int((~admissible).sum()))
        assert (~admissible).sum() * 1000 <= admissible.size
    assert [c[6:] for c in HC.LONG] == [(2060, (2060,)), (330, (321, 9))]


def test_long_device_list_mixes_hp_and_plain_vertices():
    """the threshold and origin_lod of the device form's long hp list change nothing in the prepass's list; between one vertex in ten and all
    of them are hp, in the first trip of the 1024 workgroups and in the second, where tiles hold both kinds"""
    for kind in HC.KINDS:
        c = HC.long_device_scene(kind)
        assert np.array_equal(c.tiles, GC.deep_scene(kind).tiles) and len(c.tiles) > GC.TRIP
        assert c.view.origin_lod == HC.LONG_DEVICE_ORIGIN == c.approximation.origin_lod
        for flags in (GM.GRID | HM.VIEW_RELATIVE, 0):
            exp, trace, admissible = HC.long_device_expected(kind, flags)
            share = trace["hp"].mean()
            print(kind, flags, "tiles", len(c.tiles), "hp share %.3f" % share, "inadmissible", int((~admissible).sum()))
            assert 0.1 < share < 1
            assert set(np.unique(trace["dir_origin"][trace["hp"]]).tolist()) == {GM.NONE, GM.DOWN}
            for part in (trace["hp"][:GC.TRIP], trace["hp"][GC.TRIP:]):
                assert part.any() and not part.all()
            assert (trace["hp"][GC.TRIP:].any(axis=1) & ~trace["hp"][GC.TRIP:].all(axis=1)).sum() >= 16
            assert (~admissible).sum() * 1000 <= admissible.size

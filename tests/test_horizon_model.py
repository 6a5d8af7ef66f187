"""The horizon-culling definition (include/bevy_terrain_amd.h) on the CPU: bt_cull_horizon against a float64 restatement, the numpy
model's horizon test against visibility sampled in float64 (it may never drop a tile a sample of which can be seen past the occluding
sphere), the list with either test culling against the unculled one.  The kernels are held to this model bit for bit by
test_gpu_horizon.py."""
import ctypes as C

import numpy as np
import pytest

import _cull_model as M
import _horizon_model as H
import _refine_model as R
import bevy_terrain_amd as bt
from bevy_terrain_amd import _ffi
from bevy_terrain_amd.tile_tree import model_c
from test_cull_model import synthetic_table, visited_tiles

VIEWS = 20
ORIGIN = (0.0, 0.0, 0.0)


def make_model(kind, min_height=-12000.0, max_height=9000.0, position=ORIGIN):
    if kind == "sphere":
        return bt.TerrainModel.sphere(position, 6371000.0, min_height, max_height)
    return bt.TerrainModel.ellipsoid(position, 6378137.0, 6356752.3, min_height, max_height)


def eye_above(model, direction, height):
    """the world position `height` above the model's surface at the local position `direction` (a unit vector): the point(tile, uv, h)
    of the definition, in float64"""
    d = np.asarray(direction, np.float64)
    s = np.asarray(model.scale_vec, np.float64)
    n = d / s
    return np.asarray(model.translation, np.float64) + s * d + height * n / np.linalg.norm(n)


def draw_camera(rng, model, near_ground):
    """(eye, clip_from_world): the eye 1 m .. 1 km above max_height (near_ground) or 10 m .. 1.6e7 m above it, looking anywhere from
    straight down to above the horizon"""
    if not near_ground and model.kind == "spherical" and model.translation == ORIGIN:
        return M.random_camera(rng, "sphere")
    d = rng.normal(size=3)
    d /= np.linalg.norm(d)
    eye = eye_above(model, d, model.max_height + 10.0 ** (rng.uniform(0.0, 3.0) if near_ground else rng.uniform(1.0, 7.2)))
    side = rng.normal(size=3)
    side -= d * np.dot(side, d)
    side /= np.linalg.norm(side)
    pitch = np.radians(rng.uniform(-90.0, 15.0))
    direction = np.cos(pitch) * side + np.sin(pitch) * d
    return eye, M.clip_from_world(eye, direction, np.radians(rng.uniform(30.0, 100.0)), float(rng.choice([1.0, 4.0 / 3.0, 16.0 / 9.0])), up=d)


def horizon_of(model, eye, margin=0.0):
    return H.HorizonView.from_c(bt.cull_horizon(model, tuple(eye), margin))


def visible(view, tiles, cull, horizon, tables):
    """per table of `tables`: the mask of tiles a sample of whose volume — a 9 x 9 x 3 grid of (uv, h), in float64 — can be seen: the
    segment from the eye to it does not enter the open ball of occluder_radius in scaled space"""
    eye, r2 = horizon.eye.astype(np.float64), float(horizon.occluder_radius) ** 2
    t = np.array(list(view.local_from_world_transpose), np.float32).astype(np.float64)
    ranges = []
    for table in tables:
        vmin, vmax = M.raw_range(tiles, table)
        lo, hi = M.heights(cull, vmin).astype(np.float64), M.heights(cull, vmax).astype(np.float64)
        ranges.append((lo, 0.5 * (lo + hi), hi))
    seen = [np.zeros(len(tiles), bool) for _ in tables]
    for v in np.linspace(0.0, 1.0, 9):
        for u in np.linspace(0.0, 1.0, 9):
            rest = np.flatnonzero(~np.logical_and.reduce(seen))  # (a tile seen under every table needs no further sample)
            l, _, n = H.local_surface(view, tiles[rest], (u, v), np.float64)
            g = np.stack([(t[3 * r] * n[:, 0] + t[3 * r + 1] * n[:, 1]) + t[3 * r + 2] * n[:, 2] for r in range(3)], axis=1)
            for k, hs in enumerate(ranges):
                for h in hs:
                    q = l + h[rest, None] * g
                    d = q - eye
                    s = np.clip(-(d @ eye) / np.einsum("ij,ij->i", d, d), 0.0, 1.0)  # the segment's point nearest to the centre
                    c = eye + s[:, None] * d
                    seen[k][rest] |= np.einsum("ij,ij->i", c, c) >= r2
    return seen


def test_model_surface_is_the_frustum_models():
    """the model's world point and normal, computed from its own l, equal _cull_model.surface's bit for bit; l is a unit vector and
    q(tile, uv, 0) is l"""
    rng = np.random.default_rng(8)
    for kind in ("sphere", "ellipsoid"):
        model = make_model(kind, position=(4.0e9, -2.5e8, 1.0e7))
        eye, _ = draw_camera(rng, model, False)
        view = bt.make_view_state(model, bt.TerrainViewConfig(), tuple(eye))
        tiles = visited_tiles(view)
        assert len(tiles) > 100
        for uv in ((0, 0), (1, 0), (0.5, 0.5), (0.25, 1)):
            for dtype, bits in ((np.float32, np.uint32), (np.float64, np.uint64)):
                l, world, normal = H.local_surface(view, tiles, uv, dtype)
                exp_world, exp_normal = M.surface(view, tiles, uv, dtype)
                assert np.array_equal(world.view(bits), exp_world.view(bits)) and np.array_equal(normal.view(bits), exp_normal.view(bits))
                assert l.dtype == dtype and np.allclose(np.linalg.norm(l.astype(np.float64), axis=1), 1.0, atol=3e-7)
                assert np.array_equal(H.scaled_point(view, tiles, uv, 0.0, dtype), l)
        # q is the scaled world point, without the cancellation of a planet far from the origin
        q = H.scaled_point(view, tiles, (0.5, 0.5), 9000.0, np.float64)
        p = M.point(view, tiles, (0.5, 0.5), 9000.0, np.float64)
        wfl = np.array(list(view.world_from_local), np.float32).astype(np.float64)
        assert np.allclose((p - wfl[9:12]) / np.array([wfl[0], wfl[4], wfl[8]]), q, atol=1e-6)


def test_cull_horizon_equals_the_float64_restatement_bit_for_bit():
    assert C.sizeof(_ffi.HorizonViewC) == 24 and _ffi.HorizonViewC.vh.offset == 12 and _ffi.HorizonViewC.margin.offset == 20
    rng = np.random.default_rng(31)
    for k in range(300):
        kind = ("sphere", "ellipsoid")[k % 2]
        position = tuple(rng.normal(size=3) * 10.0 ** rng.uniform(0, 10)) if k % 3 else ORIGIN
        model = make_model(kind, min_height=float(rng.choice([-12000.0, 0.0, 250.0, -1.0e6])), max_height=9000.0, position=position)
        d = rng.normal(size=3)
        eye = eye_above(model, d / np.linalg.norm(d), 10.0 ** rng.uniform(-1, 8) * (-1.0 if k % 11 == 0 else 1.0))
        margin = 0.0 if k % 4 == 0 else 10.0 ** rng.uniform(-3, 5)
        got, exp = bt.cull_horizon(model, tuple(eye), margin), H.horizon_view(model, eye, np.float32(margin))
        fields = np.array([got.eye[0], got.eye[1], got.eye[2], got.vh, got.occluder_radius, got.margin], np.float32)
        expected = np.array([*exp.eye, exp.vh, exp.occluder_radius, exp.margin], np.float32)
        assert np.array_equal(fields.view(np.uint32), expected.view(np.uint32)), (k, fields, expected)
        shortest = min(model.scale_vec)
        assert 0.0 < got.occluder_radius <= 1.0 and float(got.occluder_radius) <= 1.0 + min(model.min_height, 0.0) / shortest
        assert float(got.margin) * shortest >= float(np.float32(margin)) and (got.vh > 0) == (np.linalg.norm(np.array(got.eye[:], np.float64)) > got.occluder_radius)
    # the directed roundings are not the nearest ones throughout
    assert H.round_toward_zero(1.0 - 2.0 ** -26) == np.float32(1.0) - np.float32(2.0 ** -24) and H.round_up(1.0 + 2.0 ** -26) == np.float32(1.0) + np.float32(2.0 ** -23)


def test_cull_horizon_refusals():
    L = _ffi.lib()
    sphere, planar = make_model("sphere"), bt.TerrainModel.planar(ORIGIN, 1000.0, 0.0, 250.0)

    def status(fn):
        with pytest.raises(bt.BtError) as e:
            fn()
        assert str(e.value).split(": ", 2)[2]  # a message
        return e.value.status

    assert status(lambda: bt.cull_horizon(planar, (0.0, 500.0, 0.0))) == -5
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert status(lambda: bt.cull_horizon(sphere, (0.0, bad, 0.0))) == -1
        assert status(lambda: bt.cull_horizon(sphere, (0.0, 7.0e6, 0.0), bad)) == -1
    assert status(lambda: bt.cull_horizon(sphere, (0.0, 7.0e6, 0.0), -1.0)) == -1
    assert status(lambda: bt.cull_horizon(make_model("sphere", min_height=-7.0e6), (0.0, 7.0e6, 0.0))) == -1  # no occluder left
    out, pos = _ffi.HorizonViewC(), (C.c_double * 3)(0.0, 7.0e6, 0.0)
    assert L.bt_cull_horizon(None, pos, 0.0, C.byref(out)) == -1 and L.bt_cull_horizon(C.byref(model_c(sphere)), None, 0.0, C.byref(out)) == -1
    assert L.bt_cull_horizon(C.byref(model_c(sphere)), pos, 0.0, None) == -1
    assert L.bt_tiling_prepass_set_horizon(None, None) == -1 and L.bt_tiling_prepass_set_horizon(None, C.byref(out)) == -1


FAMILIES = ["sphere", "ellipsoid", "sphere_near_ground", "ellipsoid_near_ground"]


@pytest.mark.parametrize("family", FAMILIES)
def test_horizon_culling_is_conservative_and_not_vacuous(family):
    """Over VIEWS random views, with margin 0, with and without a table: no visited tile with a visible sample is horizon-culled (a count
    of zero); every view culls something; of the visited tiles none of whose samples is visible at least a quarter are culled."""
    kind, near_ground = family.split("_")[0], family.endswith("near_ground")
    min_height, max_height = (0.0, 100.0) if near_ground else (-12000.0, 9000.0)
    model = make_model(kind, min_height, max_height)
    rng = np.random.default_rng(4100 + FAMILIES.index(family))
    table = synthetic_table(rng, 6)
    visited_total = hidden_total = culled_total = lost_total = 0
    for k in range(VIEWS):
        eye, _ = draw_camera(rng, model, near_ground)
        view = bt.make_view_state(model, bt.TerrainViewConfig(), tuple(eye))
        cull = M.CullView(np.zeros((0, 4), np.float32), 0.0, min_height, max_height)
        horizon = horizon_of(model, eye)
        assert horizon.vh > 0
        tiles = visited_tiles(view)
        visited_total += len(tiles)
        tables = (None, table)
        for t, seen in zip(tables, visible(view, tiles, cull, horizon, tables)):
            out = H.culled(view, tiles, cull, horizon, t)
            lost = int((out & seen).sum())
            print(family, "view", k, "table" if t is not None else "no table", "visited", len(tiles), "no sample visible", int((~seen).sum()),
                  "culled", int(out.sum()), "visible and culled", lost)
            lost_total += lost
            hidden_total += int((~seen).sum())
            culled_total += int((out & ~seen).sum())
            assert out.sum() > 0, (family, k)
    print(family, "visited", visited_total, "no sample visible", hidden_total, "of them culled", culled_total, "visible and culled", lost_total)
    assert lost_total == 0
    assert visited_total >= 5000
    assert culled_total >= 0.25 * hidden_total


@pytest.mark.parametrize("kind", ["sphere", "ellipsoid"])
def test_list_is_the_unculled_list_without_culled_subtrees(kind):
    model = make_model(kind)
    rng = np.random.default_rng(78)
    table = synthetic_table(rng, 6, levels=3)
    for k in range(6):
        eye, clip = draw_camera(rng, model, k % 3 == 2)
        view = bt.make_view_state(model, bt.TerrainViewConfig(), tuple(eye))
        final, dropped, _ = R.refine(view)
        assert len(dropped) == 0
        horizon = horizon_of(model, eye, 2000.0 if k % 2 else 0.0)
        for planes in (bt.cull_planes(clip), np.zeros((0, 4), np.float32)):
            cull = M.CullView(planes, 3.0 if k % 2 else 0.0, model.min_height, model.max_height)
            # no horizon view: the frustum model's list
            assert np.array_equal(H.refine_culled_horizon(view, cull, None, table)[0], M.refine_culled(view, cull, table)[0])
            passes = []
            got, n_culled, n_visited = H.refine_culled_horizon(view, cull, horizon, table, passes)
            keep = np.ones(len(final), bool)
            chain = final.copy()
            while True:  # a final tile stays unless it or one of its ancestors is culled by either test
                keep &= ~H.culled_either(view, chain, cull, horizon, table)
                up = chain[:, 1] > 0
                if not up.any():
                    break
                chain = np.where(up[:, None], np.stack([chain[:, 0], chain[:, 1] - 1, chain[:, 2] >> 1, chain[:, 3] >> 1], axis=1), chain).astype(np.uint32)
            assert np.array_equal(got, final[keep]), (kind, k)
            assert sum(v for v, _ in passes) == n_visited and n_culled > 0
            assert not M.overflows(passes, len(got), 1 << 20) and M.overflows(passes, len(got), max(v for v, _ in passes) - 1)
            frustum_only = M.refine_culled(view, cull, table)[0]
            assert 0 < len(got) <= len(frustum_only) <= len(final) and {tuple(t) for t in got.tolist()} <= {tuple(t) for t in frustum_only.tolist()}
            if len(planes) == 0:  # horizon culling alone: a strict subset of the unculled list
                assert np.array_equal(frustum_only, final) and len(got) < len(final)
    # what culls nothing: vh <= 0 (the eye inside the occluder), a NaN eye, a NaN vh
    cull = M.CullView(np.zeros((0, 4), np.float32), 0.0, model.min_height, model.max_height)
    inside = horizon_of(model, eye_above(model, (0.0, 1.0, 0.0), model.min_height - 5000.0))
    assert inside.vh < 0
    for nothing in (inside, H.HorizonView(horizon.eye, 0.0, horizon.occluder_radius), H.HorizonView((np.nan, 0.0, 2.0), 3.0, 1.0),
                    H.HorizonView(horizon.eye, np.nan, horizon.occluder_radius), H.HorizonView(horizon.eye, horizon.vh, horizon.occluder_radius, np.nan)):
        got, n_culled, _ = H.refine_culled_horizon(view, cull, nothing)
        assert np.array_equal(got, final) and n_culled == 0

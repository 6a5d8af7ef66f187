"""The cases of tests/_ray_cases.py without a GPU: every case reaches what it is named for, asserted from the CPU models
(_raycast_model, _render_model, _shadow_model) or from the closed forms alone, and the closed forms equal the model over the whole grid
test_gpu_ray_shapes.py runs on the device.  Nothing here runs a kernel."""
from fractions import Fraction

import numpy as np
import pytest

import _cases as K
import _oracle as O
import _ray_cases as RC
import _raycast_model as RM
import _render_model as R
import _shadow_model as S
from test_gpu_raycast import assert_mix, make_rays
from test_render_model import constant_scene, cpu_scene
from test_tile_tree_host import MODELS


def model_ks(origin, t_max, steps, rounds):
    """the k of each refinement round as the model's march finds them (raycast_one's loop, keeping k)"""
    dt = np.float64(t_max) / np.float64(steps)
    t = np.arange(steps + 1, dtype=np.float64) * dt
    below = RM.f_values(RC.OMODEL, RC.constant_sampler, RM._points(origin, RC.DOWN, t)) <= 0.0
    i = int(np.argmax(below))
    assert below.any() and i > 0
    lo, hi, ks = t[i - 1], t[i], []
    for _ in range(rounds):
        u = lo + (hi - lo) * (np.arange(65, dtype=np.float64) / 64.0)
        below = RM.f_values(RC.OMODEL, RC.constant_sampler, RM._points(origin, RC.DOWN, u[1:64])) <= 0.0
        k = int(np.argmax(below)) + 1 if below.any() else 64
        lo, hi = (lo if k == 1 else u[k - 1]), (hi if k == 64 else u[k])
        ks.append(k)
    return ks


# ---- A1 ----------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("steps,rounds", RC.MARCHES)
def test_the_closed_forms_equal_the_model_over_the_grid(steps, rounds):
    """every ray of the march's batch, every byte; and the batch holds what it is named for: hits at lane 63 of a round and lane 0 of the
    next, at the last step inside a partial last round, the first step past `steps` (MISS), k == 1, k == 63 and k == 64 twice in a row"""
    b = RC.a1_batch(steps, rounds)
    got = RM.raycast(RC.OMODEL, RC.constant_sampler, b.origins, b.directions, b.t_min, b.t_max, steps, rounds)
    assert got.tobytes() == b.expected.tobytes(), np.flatnonzero([g.tobytes() != e.tobytes() for g, e in zip(got, b.expected)])[:8]
    grid = b.m >= 0
    assert grid.sum() == len(RC.DELTAS) * len(RC.m_values(steps)) * len(RC.JS) and len(b.m) == grid.sum() + 6 and len(b.m) % 4 != 0
    hit = b.expected["status"] == RM.HIT
    lanes, rounds_of = b.expected["step"][hit] % 64, b.expected["step"][hit] // 64
    if steps >= 64:
        assert ((lanes == 63) & (rounds_of == 0)).any() and ((lanes == 0) & (rounds_of == 1)).any()
    if steps >= 128:
        assert ((lanes == 63) & (rounds_of == 1)).any() and ((lanes == 0) & (rounds_of == 2)).any()
    assert (b.expected["step"][hit] == steps).any() and (b.expected["step"][hit] == 1).any()
    if (steps + 1) % 64:  # the last round is partial: the hit at i == steps is inside it, the lanes after it idle
        assert steps % 64 < 63
    past = grid & (b.m == steps + 1)
    assert past.sum() == 16 and (b.expected["status"][past] == RM.MISS).all()
    inside = grid & (b.m == 0)
    assert (b.expected["status"][inside] == RM.INSIDE).all() and (b.expected["status"][grid & (b.m == 1) & (b.j == 63)] == RM.HIT).all()
    # the rays with t_min == t_max: INSIDE at t_min under and on the ground, MISS above it
    assert list(b.expected["status"][~grid]) == [RM.INSIDE, RM.INSIDE, RM.MISS] * 2 and (b.t_min[~grid] == b.t_max[~grid]).all()
    assert (b.expected["t"][~grid][[0, 1, 3, 4]] == b.t_min[~grid][[0, 1, 3, 4]]).all() and (b.t_min[~grid] > 0.0).all()
    # the k of each refinement round, from the model's own loop
    if rounds:
        seen = set()
        for r in np.flatnonzero(hit & grid & (b.delta == 1.0)):
            ks = model_ks(b.origins[r], b.t_max[r], steps, rounds)
            assert ks == RC.refine_ks(int(b.j[r]), rounds) == RC.exact_march(Fraction(int(b.m[r])) - Fraction(int(b.j[r]), 64), steps, rounds)[4]
            seen.add(tuple(ks))
        firsts = {ks[0] for ks in seen}
        assert {1, 33, 63, 64} <= firsts
        assert rounds < 2 or ((64,) * rounds in seen and (1,) + (64,) * (rounds - 1) in seen)


def test_exact_march_equals_the_closed_form():
    for steps, rounds in RC.MARCHES:
        for m in RC.m_values(steps):
            for j in RC.JS:
                e = RC.expected_hit((0.0, RC.GROUND_Y + (m - j / 64.0), 0.0), 1.0, m, j, steps, rounds)
                status, step, lo, hi, ks, margin = RC.exact_march(Fraction(m) - Fraction(j, 64), steps, rounds)
                assert (status, step, float(hi), float(lo)) == (e["status"], e["step"], e["t"], e["t_above"]), (steps, rounds, m, j)


# ---- A2 ----------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def plane():
    """the all-65535 planar terrain as a scene of the render model"""
    s = constant_scene("planar", value=65535)
    assert s.h == RC.HI
    return s


@pytest.mark.parametrize("case", RC.A2_CAMERAS, ids=lambda c: f"{c[0]}x{c[1]}-{c[2]}-{c[3]}-{float(c[5]):g}")
def test_the_cameras_diverge_by_known_steps_and_equal_the_model(plane, case):
    width, height, steps, rounds, delta, base = case
    c = RC.ortho_camera(width, height, steps, delta, base)
    offsets = RC.pixel_offsets(c, delta)
    exp = RC.expected_planes(c, steps, rounds, delta)
    if (width, height) == (8, 8):
        # the header's pixel formula gives the whole offsets the camera was made for, and all 64 lanes of the block leave at different steps
        assert offsets == [base + (2 * x - 7) + 8 * (7 - 2 * y) for y in range(8) for x in range(8)]
        m = [int(np.ceil(a)) for a in offsets]
        assert len(set(m)) == 64 and max(m) - min(m) == 126 > 64 and exp.margin == 0
    else:
        # no sample that decides anything is within 2^-30 delta of the ground: the roundings of the kernel's points (2^-42) cannot show
        assert exp.margin > Fraction(1, 2 ** 30), float(exp.margin)
        block = exp.step[:8, :8][exp.status[:8, :8] == RM.HIT]
        assert len(set(block.tolist())) >= 32 and block.max() - block.min() > 64
    if exp.stats["miss_pixels"] and ((width, height) == (8, 8) or steps == 200):
        assert (exp.step[exp.status == RM.HIT] == steps).any()  # a pixel is met at the last step, i == steps
    counts = exp.stats
    assert counts["hit_pixels"] >= 8 and (counts["miss_pixels"] >= 4 or counts["inside_pixels"] >= 4), counts
    if rounds:
        firsts = {ks[0] for ks in exp.ks if ks}
        assert firsts == {33} if (width, height) == (8, 8) else len(firsts) >= 8
    got = R.render(plane, c, steps, rounds)
    assert np.array_equal(got.status, exp.status) and got.t.tobytes() == exp.t.tobytes() and got.stats == exp.stats
    assert np.array_equal(got.hits["step"].reshape(height, width), exp.step)
    met = got.status != RM.MISS
    assert (got.normal[met] == np.array([0.0, 1.0, 0.0], np.float32)).all() and (got.rgba[~met] == RC.BACKGROUND).all()


def test_the_cameras_cover_miss_and_inside():
    kinds = set()
    for width, height, steps, rounds, delta, base in RC.A2_CAMERAS:
        st = RC.expected_planes(RC.ortho_camera(width, height, steps, delta, base), steps, rounds, delta).stats
        kinds.add((width, rounds, st["miss_pixels"] > 0, st["inside_pixels"] > 0))
    assert {(8, 0, True, False), (8, 0, False, True), (8, 2, True, False), (8, 2, False, True)} <= kinds


# ---- A3 ----------------------------------------------------------------------------------------------------------------------------------------

def test_the_occlusion_points_equal_the_model():
    points, directions, m, exp = RC.a3_points()
    status, stats = S.occlusion(RC.OMODEL, RC.constant_sampler, points, directions, RC.A3_LIFT * RC.A3_DELTA, RC.A3_STEPS * RC.A3_DELTA, RC.A3_STEPS)
    assert np.array_equal(status, exp)
    # every lane of the first wave leaves the down march at another step; the launch's 140 rays put a direction boundary inside wave 1
    first = S.march_details(RC.OMODEL, RC.constant_sampler, S.shadow_origins(RC.OMODEL, points, RC.A3_LIFT * RC.A3_DELTA), RC.DOWN,
                            RC.A3_STEPS * RC.A3_DELTA, RC.A3_STEPS)[0]
    assert first.tolist() == [0, 0, 0] + list(range(1, 66)) + [-1, -1]
    assert len(points) == 70 and 64 < 70 < 128 and S.occlusion_launches(140, RC.A3_STEPS)[0] == 1
    assert {RM.INSIDE, RM.HIT, RM.MISS} == set(exp[:, 0].tolist()) and set(exp[:, 1].tolist()) == {RM.INSIDE, RM.MISS}
    assert (exp[:, 0] != exp[:, 1]).sum() >= 60 and not np.array_equal(exp.ravel(), exp.T.ravel())  # (a direction-major store would show)


@pytest.mark.parametrize("sun_up", [False, True])
@pytest.mark.parametrize("base", [151, 41])
def test_the_shadow_plane_of_the_exact_pictures_equals_the_model(plane, base, sun_up):
    delta = 0.25
    c = RC.ortho_camera(8, 8, 200, delta, Fraction(base), sun=(0.0, 1.0 if sun_up else -1.0, 0.0))
    exp = RC.expected_planes(c, 200, 0, delta)
    shadow = RC.expected_shadow(exp, RC.pixel_offsets(c, delta), sun_up)
    got = S.render_shadowed(plane, c, 200, 0, RC.SHADOW_LIFT * delta, RC.SHADOW_STEPS * RC.SHADOW_DS * delta, RC.SHADOW_STEPS)
    assert np.array_equal(got.shadow, shadow) and np.array_equal(got.status, exp.status)
    assert ((shadow == S.NONE) == (exp.status == RM.MISS)).all()
    want = {S.NONE, RM.MISS if sun_up else RM.HIT} if base == 151 else {RM.INSIDE, RM.MISS if sun_up else RM.HIT}
    assert set(shadow.ravel().tolist()) == want


# ---- A4 ----------------------------------------------------------------------------------------------------------------------------------------

def test_the_short_launch():
    a = RC.A4
    count, per_launch = R.launches(a.width, a.height, a.steps, a.rounds)
    blocks_x = (a.width + 7) // 8
    assert (count, per_launch, blocks_x) == (2, 60, 61) and per_launch < blocks_x  # a launch holds less than one row of blocks
    c = RC.a4_camera()
    exp = RC.expected_planes(c, a.steps, a.rounds, a.delta)
    assert exp.margin == 0 and exp.stats["launches"] == 2
    assert (exp.status[0] == RM.MISS).all() and (exp.status[1:] == RM.HIT).all() and exp.step[1:, 0].tolist() == list(range(4095, 4082, -2))
    assert all(ks == [33, 64, 64, 64] for ks, s in zip(exp.ks, exp.status.ravel()) if s == RM.HIT)
    assert (exp.t == exp.t[:, :1]).all()  # the rows are constant: only the up vector has a vertical component
    # the model on one pixel of each row (the whole picture would be sixteen million oracle samples)
    origins, directions = R.rays(c)
    for y in range(a.height):
        r = y * a.width + 487 * (y % 2)
        h = RM.raycast_one(RC.OMODEL, RC.constant_sampler, origins[r], directions[r], c.t_min, c.t_max, a.steps, a.rounds)
        assert (h["status"], h["step"], h["t"]) == (exp.status[y, 0], exp.step[y, 0], exp.t[y, 0])
    # the colour the device test expects of a met pixel, unlit: enc8(0.5 * 1.0)
    assert R.enc8(np.float32(0.5) * np.float32(1.0)) == 128 and not c.lighting
    # all but the last few samples of a ray are above the ceiling, where the kernel fetches nothing
    assert min(RC.pixel_offsets(c, a.delta)) > a.steps - 16


# ---- B -----------------------------------------------------------------------------------------------------------------------------------------

def overwritten(scene, make):
    for index in scene.layers:
        scene.layers[index] = make(scene.layers[index])
    scene.sample = RM.sampler(scene.otree, scene.T, scene.B, scene.layers)
    return scene


def test_the_border_0_tile_sample_exceeds_one():
    tile = np.full((32, 32), 30000, np.uint16)
    tile[0] = 65535
    assert abs(float(O.sample_tile(O.FORMAT_R16, 0, tile, (0.5, 0.0))[0]) - 1.2711) < 1e-4
    made = RC.b0_tile(K.smooth_raster(32, 32, seed=1))
    assert float(O.sample_tile(O.FORMAT_R16, 0, made, (0.5, 0.0))[0]) > 1.0 and float(O.sample_tile(O.FORMAT_R16, 0, made, (0.0, 0.5))[0]) > 1.0


@pytest.mark.parametrize("steps,rounds", [(256, 2), (65, 4)])
def test_border_0_rays_hit_above_the_ceiling(steps, rounds):
    s = overwritten(cpu_scene("planar", RC.OMODEL, texture_size=32, border_size=0), RC.b0_tile)
    origins, directions, t_min, t_max = RC.b0_rays(s.omodel)
    assert (RM.altitude(s.omodel, origins) >= RC.ceiling(s.omodel)).all() and (directions[:, 1] >= 0.0).all()  # every sample is above the ceiling
    hits = RM.raycast(s.omodel, s.sample, origins, directions, t_min, t_max, steps, rounds)
    above, miss = RC.hits_above_ceiling(s.omodel, hits)
    print(above, miss)
    assert above >= 8 and miss >= 8


@pytest.mark.parametrize("kind", ["planar", "sphere"])
def test_border_1_rays_meet_the_ground_at_the_ceiling(kind):
    om = MODELS[kind][1]
    s = overwritten(cpu_scene(kind, om, texture_size=32, border_size=1), RC.b1_tile)
    origins, directions, t_min, t_max = RC.b1_rays(om, s.view, s.sample)
    hits = RM.raycast(om, s.sample, origins, directions, t_min, t_max, 128, 2)
    met = RC.met_at_the_ceiling(om, hits)
    print(met, np.bincount(hits["status"], minlength=4))
    # over the plateaus the ground is met at the ceiling; elsewhere it lies lower than these short rays reach
    assert met >= 8 and (hits["status"][:24] == RM.HIT).all() and (hits["status"][24:] == RM.MISS).all()


def test_the_inverted_range_keeps_the_mix():
    om = RC.inverted_models()[1]
    assert float(om.max_height) < float(om.min_height) and RC.ceiling(om) == 0.0  # "above the ceiling" is above the LOWEST ground here
    s = cpu_scene("planar", om)
    s.sample = RM.sampler(s.otree, s.T, s.B, s.layers)
    origins, directions, t_min, t_max = make_rays(RC.geometric_range(om), s.view, 200, seed=356)
    hits = RM.raycast(om, s.sample, origins, directions, t_min, t_max, 256, 2)
    assert_mix(hits, 256)
    hit = hits["status"] == RM.HIT
    assert (RM.altitude(om, hits["position"][hit]) > RC.ceiling(om)).sum() * 2 >= hit.sum()  # a skip "above the ceiling" would drop these

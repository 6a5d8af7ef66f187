"""collide_kernel and sweep_kernel (bt_collide.hip; sphere_contact of bt_collide_device.hpp) on the device, edge by edge, on the cases of
tests/_collide_cases.py (test_collide_cases.py shows without a device that each case reaches what it is named for):

A. contacts on the exact plane against the closed form: every status at its edge (alt == 0, alt == r, a - r == ceiling and one step of
   2^-40 either side), radius 0 (all 64 lanes tie with the foot, which stays), INVALID inputs, workgroups that mix waves that leave early
   with waves that search, counts of 1, 3, 4 and 5.
B. sweeps on the exact plane against the march of the definition in rational arithmetic: a hit at step 1, at step `steps` and first past
   it, a sample exactly at grazing, blocked starts, t_min == t_max, an edge in the upper and in the lower half of every bisection, a
   direction that is neither unit nor vertical.
C. a terrain constant along x on which lanes 8 j + 3 and 8 j + 4 of the winning round tie bit for bit below the foot: the lowest lane
   wins.  Compared with the CPU model (_collide_model), on which the tie is asserted first.
D. the three forms of the ceiling skip (Ground::skip_above): border 0 and an inverted height range, where it is off, and border 1, the
   smallest border at which it is on, met at a - r == ceiling exactly and one ulp above.  Compared with the CPU model.

A and B are closed form, C and D model.  No tolerance anywhere and no excluded sphere or sweep: every comparison is of bytes, the
padding included."""
import numpy as np
import pytest

import _cases as K
import _collide_cases as CC
import _collide_model as CM
import _ray_cases as RC
import bevy_terrain_amd as bt
from test_gpu_ray_shapes import as_scene, overwrite
from test_gpu_raycast import Streamed

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device():
    return bt.Device(0)


def as_device(exp, dtype):
    """records of the model's dtype as the device's (the same fields, and a padding of 0)"""
    out = np.zeros(exp.shape, dtype)
    for name in exp.dtype.names:
        out[name] = as_device(exp[name], dtype[name]) if exp.dtype[name].names else exp[name]
    return out


def assert_same_bytes(got, exp, names=None):
    exp = as_device(exp, got.dtype)
    bad = [i for i in range(len(exp)) if got[i].tobytes() != exp[i].tobytes()]
    assert len(got) == len(exp) and not bad, [(i, names[i] if names else None, got[i], exp[i]) for i in bad[:4]]
    assert got.tobytes() == exp.tobytes()


def flat_terrain(device, tmp_path):
    """terrain P: test_gpu_ray_shapes.plane's way of making every texel 65535, with P's model"""
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(K, "smooth_raster", lambda h, w, seed, device=None: np.full((h, w), 65535, np.uint16))
        s = as_scene(Streamed(device, tmp_path, "planar", model=CC.plane_models()))
    assert all((layer == 65535).all() for layer in s.layers.values())
    return s


@pytest.fixture(scope="module")
def plane(device, tmp_path_factory):
    return flat_terrain(device, tmp_path_factory.mktemp("plane"))


# ---- A: contacts on the exact plane ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R", CC.A_ROUNDS)
def test_contacts_equal_the_closed_form(plane, R):
    b = CC.a_batch()
    got = plane.tree.collide_spheres(0, b.centers, b.radii, refine_rounds=R)
    assert_same_bytes(got, b.expected)
    for count in CC.PICKS:
        sel = CC.picks(len(got), count)
        few = plane.tree.collide_spheres(0, b.centers[sel], b.radii[sel], refine_rounds=R)
        assert len(few) == count
        assert_same_bytes(few, b.expected[sel])
        assert_same_bytes(plane.tree.collide_spheres(0, b.centers[:count], b.radii[:count], refine_rounds=R), b.expected[:count])


# ---- B: sweeps on the exact plane --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R", CC.B_ROUNDS)
@pytest.mark.parametrize("steps,bisections", CC.B_MARCHES)
def test_sweeps_equal_the_exact_march(plane, steps, bisections, R):
    b = CC.b_batch(steps, bisections)
    got = plane.tree.sweep_spheres(0, b.origins, b.directions, b.radii, b.t_min, b.t_max, steps=steps, bisections=bisections, refine_rounds=R)
    assert_same_bytes(got, b.expected, b.names)
    for count in CC.PICKS:
        sel = CC.picks(len(got), count)
        few = plane.tree.sweep_spheres(0, b.origins[sel], b.directions[sel], b.radii[sel], b.t_min[sel], b.t_max[sel], steps=steps, bisections=bisections,
                                       refine_rounds=R)
        assert len(few) == count
        assert_same_bytes(few, b.expected[sel], [b.names[i] for i in sel])


# ---- C: a tie that beats the foot ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def valley(device, tmp_path_factory):
    """terrain V: P's model pair streamed over the smooth raster (as test_collide_cases.py's scene is: the approximate height, and with it
    the LOD of every place, are those of the relief), then every loaded tile replaced by a function of the texel's row"""
    return overwrite(as_scene(Streamed(device, tmp_path_factory.mktemp("valley"), "planar", model=CC.plane_models())), CC.v_tile)


def test_a_tie_below_the_foot_goes_to_the_lowest_lane(valley):
    s = valley
    centers, rounds = CC.c_spheres(s.sample)
    exp = [CC.tie_below_the_foot(s.sample, s.otree, float(s.approximate_height), c, R)[0] for c, R in zip(centers, rounds)]
    assert len(exp) >= 4
    for R in sorted(set(rounds)):
        sel = np.array([i for i, v in enumerate(rounds) if v == R])
        want = np.array([exp[i] for i in sel], dtype=CM.CONTACT_DTYPE)
        got = s.tree.collide_spheres(0, centers[sel], CC.C_RADIUS, refine_rounds=R)
        assert_same_bytes(got, want)
        assert (got["candidate"] % 8 == 4).all() and (got["point"][:, 0] < 0.0).all()


def test_at_radius_0_every_lane_ties_with_the_foot_and_the_foot_stays(valley):
    """the improvement on the foot is strict: 64 lanes with the foot's own d2 leave candidate 0"""
    s = valley
    centers, _ = CC.c_spheres(s.sample)
    for R in (0, 2):
        want = np.array([CC.all_lanes_tie_with_the_foot(s.sample, c, R) for c in centers], dtype=CM.CONTACT_DTYPE)
        assert_same_bytes(s.tree.collide_spheres(0, centers, 0.0, refine_rounds=R), want)


# ---- D: the three forms of the ceiling skip ------------------------------------------------------------------------------------------------------

def model_answers(s, centers, radii, sweeps, march, skip_above):
    """-> the model's contacts and sweep hits at R = 1; march: (steps, bisections); skip_above: whether the border allows the skip"""
    contacts = CM.contacts(s.omodel, s.sample, centers, radii, 1, skip_above=skip_above)
    hits = CM.sweeps(s.omodel, s.sample, sweeps.origins, sweeps.directions, sweeps.radii, sweeps.t_min, sweeps.t_max, *march, 1, skip_above=skip_above)
    return contacts, hits


def test_border_0_searches_above_the_ceiling(device, tmp_path):
    """the skip is off: spheres above the ceiling by more than their radius touch the ridges that border-0 sampling raises above it"""
    s = as_scene(overwrite(Streamed(device, tmp_path, "planar", texture_size=32, border_size=0), RC.b0_tile), 32, 0)
    centers, radii = CC.b0_spheres(s.omodel, s.sample)
    w = CC.b0_sweeps(s.omodel, s.sample)
    off, hits = model_answers(s, centers, radii, w, (16, 4), False)
    on = CM.contacts(s.omodel, s.sample, centers, radii, 1, skip_above=True)
    assert len(centers) <= 64 and CC.skipped_wrongly(s.omodel, centers, radii, off, on) >= 3
    assert len(w.radii) <= 16 and CC.sweep_hits_above(s.omodel, w, hits) >= 1
    assert_same_bytes(s.tree.collide_spheres(0, centers, radii, refine_rounds=1), off)
    assert_same_bytes(s.tree.sweep_spheres(0, w.origins, w.directions, w.radii, w.t_min, w.t_max, steps=16, bisections=4, refine_rounds=1), hits)


def test_border_1_skips_above_the_ceiling_and_not_at_it(device, tmp_path):
    """the skip is on: a - r == ceiling is searched, one ulp above it is FAR"""
    s = as_scene(overwrite(Streamed(device, tmp_path, "planar", texture_size=32, border_size=1), RC.b1_tile), 32, 1)
    centers, radii = CC.b1_spheres(s.omodel, s.view, s.sample)
    w = CC.b1_sweeps(s.omodel, s.view, s.sample)
    contacts, hits = model_answers(s, centers, radii, w, (8, 3), True)
    assert len(centers) <= 64 and CC.b1_pairs(contacts) >= 4
    assert len(w.radii) <= 16 and ((hits["status"] == CM.HIT) & (hits["step"] == 5)).sum() >= 4
    assert_same_bytes(s.tree.collide_spheres(0, centers, radii, refine_rounds=1), contacts)
    assert_same_bytes(s.tree.sweep_spheres(0, w.origins, w.directions, w.radii, w.t_min, w.t_max, steps=8, bisections=3, refine_rounds=1), hits)


def test_an_inverted_range_is_searched_above_its_ceiling(device, tmp_path):
    """max_height < min_height: the skip is off, lerp(min, max, 1.0f) is the LOWEST ground and nearly every sphere is above it"""
    s = as_scene(Streamed(device, tmp_path, "planar", model=RC.inverted_models()))
    centers, radii = CC.b2_spheres(s.omodel, s.sample, s.view)
    w = CC.make_sweeps(RC.geometric_range(s.omodel), s.sample, s.view, n=16)
    contacts, hits = model_answers(s, centers, radii, w, (32, 4), True)  # (the model tests max >= min itself)
    assert len(centers) == 64 and CC.searched_above(s.omodel, centers, radii, contacts) >= 8
    assert (hits["status"] == CM.HIT).sum() >= 3 and CC.sweep_hits_above(s.omodel, w, hits) >= 3
    assert_same_bytes(s.tree.collide_spheres(0, centers, radii, refine_rounds=1), contacts)
    assert_same_bytes(s.tree.sweep_spheres(0, w.origins, w.directions, w.radii, w.t_min, w.t_max, steps=32, bisections=4, refine_rounds=1), hits)

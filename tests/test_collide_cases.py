"""The cases of tests/_collide_cases.py for tests/test_gpu_collide_shapes.py, without a GPU: every case reaches what it is named for, and
the closed forms equal the CPU model of SPHERE CONTACT and SPHERE SWEEP (_collide_model) byte for byte, so that the model and the tables
cannot share a mistake.  Nothing here runs a kernel.

Closed form: sections A and B (contacts and sweeps on the exact plane; the sweeps' march in rational arithmetic).  Model: sections C (a
tie between two lanes that beats the foot, on a sampled atlas) and D (the three forms of the ceiling skip), whose reach conditions are
asserted here on terrains built without a device and again by the device tests on theirs.  Nothing has a tolerance."""
from fractions import Fraction

import numpy as np
import pytest

import _collide_cases as CC
import _collide_model as CM
import _ray_cases as RC
import _raycast_model as RM
from test_ray_cases import overwritten
from test_render_model import cpu_scene


def assert_same_bytes(got, exp, names=None):
    bad = [i for i in range(len(exp)) if got[i].tobytes() != exp[i].tobytes()]
    assert len(got) == len(exp) and not bad, [(i, names[i] if names else None, got[i], exp[i]) for i in bad[:4]]


# ---- A -------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R", CC.A_ROUNDS)
def test_the_contact_table_equals_the_model(R):
    b = CC.a_batch()
    assert_same_bytes(CM.contacts(CC.P_OMODEL, CC.plane_sampler, b.centers, b.radii, R), b.expected)


def test_the_contact_batch_holds_every_edge():
    b = CC.a_batch()
    exp, alt = b.expected, b.centers[:, 1] - CC.P_GROUND_Y
    assert len(exp) == 60 and CM.ceiling(CC.P_OMODEL) == CC.P_H and (np.abs(b.centers[np.isfinite(b.centers).all(axis=1)][:, [0, 2]]) <= 400.0).all()
    counts = np.bincount(exp["status"], minlength=5)
    assert counts[CM.INVALID] == 6 and counts[CM.TOUCHING] >= 10 and counts[CM.NONE] == 5 and counts[CM.BELOW] >= 15 and counts[CM.FAR] >= 10, counts
    # every workgroup of four waves holds waves that leave early and waves that search
    groups = b.searched.reshape(-1, 4)
    assert groups.any(axis=1).all() and (~groups).any(axis=1).all() and len(set(np.argmax(groups, axis=1))) == 4
    valid = exp["status"] != CM.INVALID
    at = valid & (alt == b.radii)
    # alt == r: NONE with depth 0 for r > 0 (not TOUCHING, not FAR), BELOW at r == 0; one step of 2^-40 beyond it FAR, one inside it TOUCHING
    assert (exp["status"][at & (b.radii > 0.0)] == CM.NONE).all() and (exp["depth"][at] == 0.0).all() and (at & (b.radii > 0.0)).sum() == 5
    assert (exp["status"][at & (b.radii == 0.0)] == CM.BELOW).all() and (at & (b.radii == 0.0)).sum() == 1
    assert (exp["status"][valid & (alt == b.radii + 2.0 ** -40)] == CM.FAR).sum() == 6
    assert (exp["status"][valid & (alt == b.radii - 2.0 ** -40) & (alt > 0.0)] == CM.TOUCHING).sum() == 5
    # alt == 0 is BELOW with distance 0; the least altitude above it is searched
    on = valid & (alt == 0.0)
    assert on.sum() == 6 and (exp["status"][on] == CM.BELOW).all() and (exp["distance"][on] == 0.0).all() and (exp["depth"][on] == b.radii[on]).all()
    assert (exp["status"][valid & (alt == 2.0 ** -40) & (b.radii > 0.0)] == CM.TOUCHING).all()
    # a FAR or INVALID record is its status and 76 zero bytes
    for status in (CM.FAR, CM.INVALID):
        zero = np.zeros((), CM.CONTACT_DTYPE)
        zero["status"] = status
        assert all(e.tobytes() == zero.tobytes() for e in exp[exp["status"] == status])
    # the normal of a searched sphere is alt * (1 / alt), which is not always 1
    assert (exp["normal"][b.searched][:, 1] != 1.0).any() and (exp["normal"][b.searched][:, 1] == 1.0).any()
    assert (exp["candidate"] == 0).all()
    for count in CC.PICKS:
        sel = CC.picks(len(exp), count)
        assert len(set(sel)) == count and (count < 4 or (b.searched[sel].any() and not b.searched[sel].all()))


# ---- B -------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R", CC.B_ROUNDS)
@pytest.mark.parametrize("steps,bisections", CC.B_MARCHES)
def test_the_exact_march_equals_the_model(steps, bisections, R):
    b = CC.b_batch(steps, bisections)
    got = CM.sweeps(CC.P_OMODEL, CC.plane_sampler, b.origins, b.directions, b.radii, b.t_min, b.t_max, steps, bisections, R)
    assert_same_bytes(got, b.expected, b.names)


@pytest.mark.parametrize("steps,bisections", CC.B_MARCHES)
def test_the_sweep_batch_holds_every_edge(steps, bisections):
    b = CC.b_batch(steps, bisections)
    exp = {name: e for name, e in zip(b.names, b.expected)}
    row = {name: i for i, name in enumerate(b.names)}
    assert len(exp) == len(b.names) and len(b.names) % 4 != 0

    def of(name, r):
        e = exp[f"{name}, r {r:g}"]
        return int(e["status"]), int(e["step"])

    zero = np.zeros((), CM.SWEEP_DTYPE)
    for r in CC.B_RADII:
        assert of("step 1", r) == (CM.HIT, 1) and of("step `steps`", r) == (CM.HIT, steps)
        assert exp[f"first at steps + 1, r {r:g}"].tobytes() == zero.tobytes()  # MISS: every byte 0
        for name in ("inside, e < 0", "on the ground", "under the ground", "dt == 0, blocked"):
            e, i = exp[f"{name}, r {r:g}"], row[f"{name}, r {r:g}"]
            assert of(name, r) == (CM.INSIDE, 0) and e["t"] == e["t_above"] == b.t_min[i]
            assert e["contact"]["status"] == (CM.TOUCHING if (r > 0.0 and "e < 0" in name or "blocked" in name and r > 0.0) else CM.BELOW), name
        assert exp[f"dt == 0, clear, r {r:g}"].tobytes() == zero.tobytes()
        for name in ("dt == 0, blocked", "dt == 0, clear"):
            assert b.t_min[row[f"{name}, r {r:g}"]] == b.t_max[row[f"{name}, r {r:g}"]] > 0.0
    # a sample exactly at grazing: touching is strict, so the sphere is met one step later than the point
    assert of("grazing at sample `steps`", 0.0) == (CM.HIT, steps) and of("grazing at sample `steps`", 1.5) == (CM.MISS, 0)
    assert of("grazing at sample steps - 1", 1.5) == (CM.HIT, steps)
    assert of("grazing at sample steps - 1", 0.0) == ((CM.HIT, steps - 1) if steps > 1 else (CM.INSIDE, 0))
    # the edge in the upper and in the lower half of the bisections: rho = 0 keeps the lower half every time, 1 - 2^-30 the upper
    if bisections:
        for m in sorted({1, (steps + 1) // 2, steps}):
            e0, e1, e2 = (exp[f"edge m {m} rho {float(rho):g}, r 1.5"] for rho in CC.B_RHOS)
            i0, i2 = row[f"edge m {m} rho 0, r 1.5"], row[f"edge m {m} rho 1, r 1.5"]
            assert e0["step"] == e1["step"] == e2["step"] == m
            width = (b.t_max[i0] - b.t_min[i0]) / steps
            assert e0["t_above"] == b.t_min[i0] + (m - 1) * width and e0["t"] - e0["t_above"] == width / 2.0 ** bisections
            assert e2["t"] == b.t_min[i2] + m * ((b.t_max[i2] - b.t_min[i2]) / steps) or bisections > 30
    hit = b.expected["status"] == CM.HIT
    assert (b.expected["t_above"][hit] < b.expected["t"][hit]).all()
    assert np.isin(b.expected["contact"]["status"][hit], (CM.TOUCHING, CM.BELOW)).all()
    assert (b.expected["contact"]["status"][hit & (b.radii > 0.0)] == CM.TOUCHING).all() and (b.expected["contact"]["status"][hit & (b.radii == 0.0)] == CM.BELOW).all()
    # the oblique sweeps: the point moves with t, by (3 t, 2 t) exactly
    oblique = hit & (b.directions[:, 0] == 3.0)
    assert oblique.sum() >= 3 and (b.expected["t"][oblique] > 0.0).all()
    assert np.array_equal(b.expected["contact"]["point"][oblique][:, [0, 2]], b.origins[oblique][:, [0, 2]] + b.expected["t"][oblique, None] * np.array([3.0, 2.0]))
    assert (b.expected["status"][-4:] == CM.RAY_INVALID).all() and (b.origins[:-4][:, [0, 2]] % 1.0 == 0.0).all()
    assert (np.abs(b.origins[:-4][:, [0, 2]]) + np.abs(b.directions[:-4][:, [0, 2]]) * b.t_max[:-4, None] <= 400.0).all()  # whole x, z; within 400 all the way
    for count in CC.PICKS:
        assert len(set(CC.picks(len(b.names), count))) == count


def test_exact_sweep_against_the_vertical_descent():
    """test_collide_model.test_vertical_descent_onto_flat_ground's closed form, from the rational march"""
    for m, rho in [(1, Fraction(0)), (5, Fraction(5, 16)), (64, Fraction(1, 2)), (37, 1 - Fraction(1, 2 ** 30))]:
        for bisections in (0, 1, 20):
            status, step, lo, hi, seen = CC.exact_sweep(m - 1 + rho, 0, 64, bisections, True)
            k = int(rho * 2 ** bisections) + 1
            assert (status, step, hi, hi - lo) == (CM.HIT, m, m - 1 + Fraction(k, 2 ** bisections), Fraction(1, 2 ** bisections))
            assert len(seen) == m + 1 + bisections + 1


# ---- C -------------------------------------------------------------------------------------------------------------------------------------------

def test_two_lanes_tie_below_the_foot():
    s = overwritten(cpu_scene("planar", CC.P_OMODEL), CC.v_tile)
    probe = np.column_stack([np.array([-3.0, 0.0, 0.125, 77.0]), np.zeros(4), np.full(4, 41.0)])
    assert len(set(s.sample(probe).tolist())) == 1  # the ground does not depend on x
    centers, rounds = CC.c_spheres(s.sample)
    reached = [CC.tie_below_the_foot(s.sample, s.otree, s.approximate_height, c, R)[1] for c, R in zip(centers, rounds)]
    print(reached)
    assert len(reached) >= 4 and len(set(centers[:, 2])) == len(centers) and (centers[:, 0] == 0.0).all()
    assert sum(R == 1 for R in rounds) >= 1 and sum(R == 0 for R in rounds) >= 3
    assert len({lane for lane, _, _ in reached}) >= 3 and len({lod for _, lod, _ in reached}) >= 2
    # the same centres at radius 0: all 64 lanes tie with the foot, which stays
    for c, R in zip(centers, rounds):
        CC.all_lanes_tie_with_the_foot(s.sample, c, R + 1)


# ---- D -------------------------------------------------------------------------------------------------------------------------------------------

def test_border_0_spheres_touch_above_the_ceiling():
    s = overwritten(cpu_scene("planar", RC.OMODEL, texture_size=32, border_size=0), RC.b0_tile)
    centers, radii = CC.b0_spheres(s.omodel, s.sample)
    assert 9 <= len(centers) <= 64
    off = CM.contacts(s.omodel, s.sample, centers, radii, 1, skip_above=False)
    on = CM.contacts(s.omodel, s.sample, centers, radii, 1, skip_above=True)
    print(np.bincount(off["status"], minlength=5), np.bincount(on["status"], minlength=5))
    assert CC.skipped_wrongly(s.omodel, centers, radii, off, on) >= 3
    assert (off["status"] == CM.TOUCHING).sum() >= 3 and (off["status"] == CM.BELOW).sum() >= 3 and (off["status"] == CM.NONE).sum() >= 3
    w = CC.b0_sweeps(s.omodel, s.sample)
    assert 4 <= len(w.radii) <= 16
    hits = CM.sweeps(s.omodel, s.sample, w.origins, w.directions, w.radii, w.t_min, w.t_max, 16, 4, 1, skip_above=False)
    print(np.bincount(hits["status"], minlength=4))
    assert CC.sweep_hits_above(s.omodel, w, hits) >= 1
    skipping = CM.sweeps(s.omodel, s.sample, w.origins, w.directions, w.radii, w.t_min, w.t_max, 16, 4, 1, skip_above=True)
    assert (skipping["step"] > hits["step"]).sum() >= 3  # a skip that stayed on would meet the ground later, below the ceiling


def test_border_1_pairs_straddle_the_ceiling():
    s = overwritten(cpu_scene("planar", RC.OMODEL, texture_size=32, border_size=1), RC.b1_tile)
    centers, radii = CC.b1_spheres(s.omodel, s.view, s.sample)
    assert len(centers) <= 64
    contacts = CM.contacts(s.omodel, s.sample, centers, radii, 1)
    print(np.bincount(contacts["status"], minlength=5))
    assert CC.b1_pairs(contacts) >= 4 and (contacts["status"][1::2] == CM.FAR).all()
    # over the plateaus the foot is at the distance r exactly: NONE with depth 0 unless lower ground nearby is nearer
    assert ((contacts["status"][::2] == CM.NONE) & (contacts["depth"][::2] == 0.0)).sum() >= 4
    w = CC.b1_sweeps(s.omodel, s.view, s.sample)
    hits = CM.sweeps(s.omodel, s.sample, w.origins, w.directions, w.radii, w.t_min, w.t_max, 8, 3, 1)
    print(np.bincount(hits["status"], minlength=4), hits["step"])
    assert len(w.radii) <= 16 and ((hits["status"] == CM.HIT) & (hits["step"] == 5)).sum() >= 4 and (hits["status"] == CM.MISS).sum() >= 4
    a = RM.altitude(s.omodel, w.origins + 4.0 * RC.B1_DELTA * w.directions)
    assert (a - w.radii == RC.ceiling(s.omodel)).all()  # sample 4 is at the ceiling exactly


def test_the_inverted_range_is_searched_above_its_ceiling():
    om = RC.inverted_models()[1]
    s = cpu_scene("planar", om)
    s.sample = RM.sampler(s.otree, s.T, s.B, s.layers)
    centers, radii = CC.b2_spheres(om, s.sample, s.view)
    contacts = CM.contacts(om, s.sample, centers, radii, 1)
    print(np.bincount(contacts["status"], minlength=5))
    assert len(centers) == 64 and CC.searched_above(om, centers, radii, contacts) >= 8 and (contacts["status"] == CM.FAR).sum() == 0
    assert all((contacts["status"] == v).sum() >= 4 for v in (CM.NONE, CM.TOUCHING, CM.BELOW))
    w = CC.make_sweeps(RC.geometric_range(om), s.sample, s.view, n=16)
    hits = CM.sweeps(om, s.sample, w.origins, w.directions, w.radii, w.t_min, w.t_max, 32, 4, 1)
    print(np.bincount(hits["status"], minlength=4))
    assert (hits["status"] == CM.HIT).sum() >= 3 and CC.sweep_hits_above(om, w, hits) >= 3

"""The inputs of tests/test_gpu_collide.py and the conditions they must satisfy, without the package: spheres made from the model's ray hit
positions moved along the up direction by multiples of their radius, sweeps of such spheres, and the counts the batches must reach.
tests/test_collide_model.py asserts the conditions on a terrain built without a device, test_gpu_collide.py on the device's terrain
before the device is asked."""
import types

import numpy as np

import _collide_model as CM
import _raycast_model as RM
from _ray_cases import up_vectors

# the centre is placed k radii above the ray's hit position (which lies at or just under the ground): under it, inside, grazing, clear,
# and so far clear that even the gentle slopes of the globes (a texel is tens of kilometres) move the nearest point off the foot
MULTIPLES = (-1.5, -0.25, 0.0, 0.5, 0.9, 0.99, 1.01, 1.5, 3.0, 0.7, 12.0, 25.0)
RADII = (0.5, 2.0, 8.0, 32.0)
FAR_COUNT, SPHERES = 8, 270  # 270 spheres: 68 workgroups of four waves, the last one half full


def _ranges(omodel):
    lo, hi = float(omodel.min_height), float(omodel.max_height)
    return lo, hi, hi - lo


def _drop(omodel):
    """how far a ray straight down from up_vectors' points lifted by hi + 0.05 span must go to pass the lowest ground (those points lie on
    the sphere of radius a, up to a - b above the ellipsoid)"""
    lo, hi, span = _ranges(omodel)
    return 1.2 * span + (float(omodel.a) - float(omodel.b) if int(omodel.kind) == 2 else 0.0)


def make_spheres(omodel, sample, view, n=SPHERES, seed=31):
    """-> (centers (n, 3), radii (n,)): n - FAR_COUNT - 1 spheres around the ground (three of radius 0), FAR_COUNT above the ceiling by more than their
    radius, and one whose centre has a NaN"""
    rng = np.random.default_rng(seed)
    lo, hi, span = _ranges(omodel)
    m = n - FAR_COUNT - 1
    ground, up = up_vectors(omodel, view, n, rng)
    hits = RM.raycast(omodel, sample, ground[:m] + up[:m] * (hi + 0.05 * span), -up[:m], 0.0, _drop(omodel), 64, 2)
    assert (hits["status"] == RM.HIT).all()
    radii = np.array([RADII[i % len(RADII)] for i in range(n)]) * (1.0 if int(omodel.kind) == 0 else 40.0)  # (a texel of the globes is kilometres wide)
    k = np.array([MULTIPLES[(i // len(RADII)) % len(MULTIPLES)] for i in range(m)])
    centers = np.empty((n, 3))
    centers[:m] = hits["position"] + up[:m] * (k * radii[:m])[:, None]
    for i in (5, 17, 29):  # radius 0: every stencil point is the centre, the foot stays whatever R
        radii[i] = 0.0
        centers[i] = hits["position"][i] + up[i] * (3.0 * RADII[i % len(RADII)] * (1.0 if int(omodel.kind) == 0 else 40.0))
    centers[m:n - 1] = ground[m:n - 1] + up[m:n - 1] * (hi + radii[m:n - 1] * rng.uniform(1.5, 4.0, FAR_COUNT))[:, None]
    centers[n - 1] = centers[0]
    centers[n - 1, 1] = np.nan
    order = rng.permutation(n)  # the kinds mixed through the batch, so that every prefix holds several
    return centers[order], radii[order]


def contact_figures(contacts):
    status = contacts["status"]
    searched = (status == CM.TOUCHING) | (status == CM.NONE)
    candidate = contacts["candidate"][searched]
    return dict(touching=int((status == CM.TOUCHING).sum()), none=int((status == CM.NONE).sum()), below=int((status == CM.BELOW).sum()),
                far=int((status == CM.FAR).sum()), invalid=int((status == CM.INVALID).sum()), foot=int((candidate == 0).sum()),
                round0=int(((candidate >= 1) & (candidate <= 64)).sum()), later=int((candidate > 64).sum()))


def assert_contact_mix(figures, refine_rounds):
    """conditions on the INPUT, from the model's contacts"""
    assert figures["touching"] >= 20 and figures["none"] >= 20 and figures["below"] >= 20, figures
    assert figures["far"] >= 5 and figures["invalid"] >= 1, figures
    # winners: the foot at every R (the spheres of radius 0 at least); with one round only round 0 can win, with more a later round
    # improves on it wherever the ground is not flat
    assert figures["foot"] >= 3, figures
    assert figures["round0" if refine_rounds == 0 else "later"] >= 3, figures


SWEEPS = 36


def make_sweeps(omodel, sample, view, n=SWEEPS, seed=47):
    """-> namespace(origins, directions, radii, t_min, t_max): spheres coming down on the ground steeply and obliquely (HIT), starting in
    touch with it or under it (INSIDE), moving level above the relief (MISS), and four that cannot be marched (INVALID)"""
    rng = np.random.default_rng(seed)
    lo, hi, span = _ranges(omodel)
    scale = 1.0 if int(omodel.kind) == 0 else 40.0
    ground, up = up_vectors(omodel, view, n, rng)
    side = np.cross(up, rng.normal(size=(n, 3)))
    side /= np.linalg.norm(side, axis=1, keepdims=True)
    hits = RM.raycast(omodel, sample, ground + up * (hi + 0.05 * span), -up, 0.0, _drop(omodel), 64, 2)
    assert (hits["status"] == RM.HIT).all()
    surface = hits["position"]
    s = types.SimpleNamespace()
    s.radii = np.array([RADII[i % len(RADII)] for i in range(n)]) * scale
    s.origins, s.directions = np.empty((n, 3)), np.empty((n, 3))
    s.t_min, s.t_max = np.zeros(n), np.empty(n)
    for i in range(n):
        family = i % 4
        if family in (0, 1):  # down from 0.3 .. 0.8 span above the surface point, family 1 with a sideways drift; not normalised
            height = rng.uniform(0.3, 0.8) * span
            s.origins[i] = surface[i] + up[i] * height
            s.directions[i] = (-up[i] + side[i] * (rng.uniform(0.2, 0.8) if family == 1 else 0.0)) * height
            s.t_max[i] = rng.uniform(1.1, 1.5)
        elif family == 2:  # starts within its radius of the ground, or under it
            s.origins[i] = surface[i] + up[i] * (s.radii[i] * rng.choice([-0.5, 0.3, 0.8]))
            s.directions[i] = side[i] + up[i] * rng.uniform(-0.2, 0.2)
            s.t_max[i] = 10.0 * scale
        else:  # level flight above the highest ground
            s.origins[i] = ground[i] + up[i] * (hi + s.radii[i] * rng.uniform(1.2, 2.0))
            s.directions[i] = side[i]
            s.t_max[i] = 20.0 * scale
    s.t_min[::5] = 0.05 * s.t_max[::5]
    s.radii[n - 1] = -1.0
    s.directions[n - 2] = 0.0
    s.origins[n - 3, 2] = np.inf
    s.t_max[n - 4] = np.nan
    return s


def assert_sweep_mix(hits, steps):
    status = hits["status"]
    counts = np.bincount(status, minlength=4)
    assert counts[CM.RAY_INVALID] == 4 and counts[CM.INSIDE] >= 4 and counts[CM.MISS] >= 4, counts
    if steps > 1:
        assert counts[CM.HIT] >= 8, counts
    else:
        assert counts[CM.HIT] >= 1, counts

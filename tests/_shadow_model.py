"""SUN OCCLUSION, bt_tile_tree_sun_occlusion and bt_tile_tree_render_shadowed (include/bevy_terrain_amd.h) written once more on the CPU, out
of the models the tests already have: the altitude direction n(q) as tests/_raycast_model.py's altitude computes it, the shadow ray's
status from _raycast_model.raycast_one at refine_rounds = 0, the picture from tests/_render_model.py plus the header's rule for the shadow
and colour planes, one np.float32 operation at a time.  Nothing of the package under test is imported.

Also here, because the CPU and the GPU tests share them: the two launch rules, the suns and shadow parameters of the test scenes and the
conditions those scenes must satisfy (input_conditions)."""
import types

import numpy as np

import _oracle as O
import _raycast_model as RM
import _render_model as R

F = np.float32
MISS, HIT, INSIDE, INVALID, NONE = RM.MISS, RM.HIT, RM.INSIDE, RM.INVALID, 255  # BT_RAY_*, BT_SHADOW_NONE
SAMPLES_PER_LAUNCH = 1 << 24  # BT_RAYCAST_MAX_SAMPLES


def up_direction(model, pts):
    """n(q) of world points (n, 3): normalize3(transform_vector(m, spherical ? local : (0, 1, 0))), operation by operation as
    _raycast_model.altitude forms its n -> (n, 3) f64"""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    p = [pts[:, 0].copy(), pts[:, 1].copy(), pts[:, 2].copy()]
    pos = [float(model.position[i]) for i in range(3)]
    kind = int(model.kind)
    a, b = float(model.a), float(model.b)
    scale = [a, b, a] if kind == 2 else [a, a, a]
    with np.errstate(all="ignore"):
        if kind == 0:
            up = [np.zeros_like(p[0]), np.ones_like(p[0]), np.zeros_like(p[0])]
        elif kind == 1:
            up = RM._normalize3([(p[i] - pos[i]) / scale[i] for i in range(3)])
        else:
            e = np.array([p[i] - pos[i] for i in range(3)]).T
            s = np.array([O.project_point_ellipsoid((a, a, b), tuple(row)) for row in e]).reshape(-1, 3)
            up = RM._normalize3([(s[:, i] - pos[i]) / scale[i] for i in range(3)])
        n = RM._normalize3([scale[i] * up[i] for i in range(3)])
    return np.stack(n, axis=1)


def shadow_origins(model, points, lift):
    """origin_a = q_a + lift * n_a of finite points (n, 3): one multiply, one add per component"""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return points + np.float64(lift) * up_direction(model, points)


def shadow_rays(model, points, directions, lift):
    """the shadow rays of every (point, direction) pair, point-major -> (origins, directions), (n * k, 3) each; a non-finite point keeps
    a NaN origin (its frame is never computed): INVALID"""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    directions = np.asarray(directions, dtype=np.float64).reshape(-1, 3)
    finite = np.isfinite(points).all(axis=1)
    origins = np.full(points.shape, np.nan)
    if finite.any():
        origins[finite] = shadow_origins(model, points[finite], lift)
    return np.repeat(origins, len(directions), axis=0), np.tile(directions, (len(points), 1))


def occlusion(model, sample, points, directions, lift, distance, steps):
    """SUN OCCLUSION of every pair -> ((n, k) uint8 statuses, the stats but for `launches`)"""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    directions = np.asarray(directions, dtype=np.float64).reshape(-1, 3)
    origins, rays = shadow_rays(model, points, directions, lift)
    status = np.array([RM.raycast_one(model, sample, origins[r], rays[r], 0.0, distance, steps, 0)["status"] for r in range(len(origins))], np.uint8)
    status = status.reshape(len(points), len(directions))
    return status, dict(lit=int((status == MISS).sum()), occluded=int(((status == HIT) | (status == INSIDE)).sum()), invalid=int((status == INVALID).sum()))


def occlusion_launches(rays, steps):
    """(number of launches, rays per launch) of a batch: whole waves of 64 rays at 64 * (steps + 1) worst-case samples each"""
    per_launch = 64 * (SAMPLES_PER_LAUNCH // (64 * (steps + 1)))
    return -(-rays // per_launch), per_launch


def shadowed_launches(width, height, steps, refine_rounds, shadow_steps):
    """_render_model.launches with the shadow ray's samples in a block's worst case"""
    blocks_x = (width + 7) // 8
    blocks = blocks_x * ((height + 7) // 8)
    per_launch = min(blocks, SAMPLES_PER_LAUNCH // (64 * ((steps + 1 + 63 * refine_rounds) + (shadow_steps + 1))))
    if per_launch >= blocks_x:
        per_launch -= per_launch % blocks_x
    return -(-blocks // per_launch), per_launch


def shade_shadowed(c, base, normals, occluded):
    """_render_model.shade with the shadow: k = ambient + (1 - ambient) * (l * sh), sh = occluded ? 0 : 1"""
    base = np.array(base, dtype=np.float32)
    if c.lighting:
        n = [normals[:, k].astype(np.float32) for k in range(3)]
        sun = [F(v) for v in c.sun]
        d = (n[0] * sun[0] + n[1] * sun[1]) + n[2] * sun[2]
        light = np.where(d > F(0.0), d, F(0.0)).astype(np.float32)
        sh = np.where(occluded, F(0.0), F(1.0)).astype(np.float32)
        with np.errstate(all="ignore"):
            k = F(c.ambient) + (F(1.0) - F(c.ambient)) * (light * sh)
        for ch in range(3):
            base[:, ch] = base[:, ch] * k
    return np.stack([R.enc8(base[:, ch]) for ch in range(4)], axis=1)


def render_shadowed(scene, c, steps, refine_rounds, lift, distance, shadow_steps):
    """the five planes and the stats: _render_model.render, the SHADOW PLANE at its hit points, and the colour of the met pixels made
    again with the shadow term"""
    out = R.render(scene, c, steps, refine_rounds)
    met = out.met
    sample = RM.sampler(scene.otree, scene.T, scene.B, scene.layers)
    shadow = np.full(len(met), NONE, np.uint8)
    sun = np.array([np.float64(F(v)) for v in c.sun])  # the exact widening of the camera's f32 sun
    if met.any():
        p = out.hits["position"][met]
        shadow[met] = occlusion(scene.omodel, sample, p, sun, lift, distance, shadow_steps)[0][:, 0]
        occluded = (shadow[met] == HIT) | (shadow[met] == INSIDE)
        if c.albedo is None:
            value = scene.otree.sample_attachment(O.FORMAT_R16, scene.T, scene.B, scene.layers, p)[0][:, 0]
            g = F(0.5) * value.astype(np.float32)
            base = np.stack([g, g, g, np.ones_like(g)], axis=1)
        else:
            base = scene.otree.sample_attachment(O.FORMAT_RGBA8, scene.albedo_T, scene.albedo_B, scene.albedo_layers, p)[0]
        rgba = out.rgba.reshape(-1, 4).copy()
        rgba[met] = shade_shadowed(c, base, out.normal.reshape(-1, 3)[met], occluded)
        out.rgba = rgba.reshape(c.height, c.width, 4)
    out.shadow = shadow.reshape(c.height, c.width)
    out.stats = dict(out.stats, launches=shadowed_launches(c.width, c.height, steps, refine_rounds, shadow_steps)[0])
    return out


def march_details(model, sample, origins, direction, distance, steps):
    """per shadow ray (finite origins (n, 3), one direction): (the step of its first sample at or under the ground, or -1; how many of the
    samples it evaluates lie above the ceiling, where ray_eval fetches nothing)"""
    ceiling = np.float64(F(model.min_height) + (F(model.max_height) - F(model.min_height)) * F(1.0))
    direction = np.asarray(direction, dtype=np.float64)
    t = np.float64(0.0) + np.arange(steps + 1, dtype=np.float64) * ((np.float64(distance) - np.float64(0.0)) / np.float64(steps))
    first, above = [], []
    for o in np.asarray(origins, dtype=np.float64).reshape(-1, 3):
        pts = RM._points(o, direction, t)
        below = RM.f_values(model, sample, pts) <= 0.0
        i = int(np.argmax(below)) if below.any() else -1
        marched = pts if i < 0 else pts[:i + 1]
        first.append(i)
        above.append(int((RM.altitude(model, marched) > ceiling).sum()))
    return np.array(first), np.array(above)


# ---- the scenes of the GPU tests: _render_model.scene_cameras with a low sun and a shadow march ------------------------------------------

SHADOW_STEPS = [1, 48, 200]


def scene_shadow(kind, omodel, view):
    """(sun, lift, distance) for the cameras of _render_model.scene_cameras: a unit sun low over the horizon (11.5 degrees on the planar
    terrain; 1.7 degrees above the VIEW's horizon on the globes, whose relief is a few degrees steep at most: lower, or under the
    horizon, at the hit points further along the sun's azimuth), a lift of 2 % of the height span, and a reach short enough that
    some lit rays stay under the ceiling all the way (on the globes the curvature alone lifts a ray 800 m over 100 km).  The azimuths were
    chosen among five for scenes that meet assert_input_conditions with room; the conditions are asserted, not these numbers."""
    pos = np.array([float(omodel.position[i]) for i in range(3)])
    span = float(omodel.max_height) - float(omodel.min_height)
    if int(omodel.kind) == 0:
        return tuple(R._unit((np.cos(2.8), 0.2, np.sin(2.8)))), 0.02 * span, 600.0
    radial = R._unit(np.asarray(view, dtype=np.float64) - pos)
    east = R._unit(np.cross(radial, (0.0, 0.0, 1.0)))
    north = np.cross(east, radial)
    return tuple(R._unit(east * np.cos(1.5) + north * np.sin(1.5) + radial * 0.03)), 0.02 * span, 1.0e5


def shadow_camera(kind, omodel, view, name="main"):
    """the camera `name` of the scene with the scene's sun -> (camera, lift, distance)"""
    sun, lift, distance = scene_shadow(kind, omodel, view)
    c = R.scene_cameras(kind, omodel, view)[name]
    c.sun = tuple(float(F(v)) for v in sun)
    return c, lift, distance


def boundary_camera(scene):
    """the camera of the two-launch render test on the planar scene: one block wide and 64 blocks tall (8 x 512 pixels), marched with ONE
    primary step, so a pixel meets the ground exactly when its ray's end point p(t_max = 1) lies under it.  The end points form a steep
    plane that dips under the ground below the view position about three rows above the launch boundary (row 504 at 4096 shadow
    steps): only the last rows meet anything, a few of them in the first launch."""
    om = scene.omodel
    x0, z0 = float(scene.view[0]), float(scene.view[2])
    sample = RM.sampler(scene.otree, scene.T, scene.B, scene.layers)
    ground = float(om.position[1]) + float(sample(np.array([[x0, 0.0, z0]]))[0])
    eye = np.array([x0, float(om.position[1]) + float(om.max_height) + 300.0, z0])
    up = np.array([0.0, 200.0, 40.0])
    sy = 1.0 - (2.0 * 500.5) / 512.0  # row 500
    forward = (0.0, (ground - 2.0) - eye[1] - sy * up[1], 0.0)  # (row 500's end points: 2 under the ground below the view)
    sun = scene_shadow("planar", om, scene.view)[0]
    return R.camera(eye, forward, (4.0, 0.0, 0.0), up, 8, 512, 0.0, 1.0, lighting=True, sun=tuple(float(F(v)) for v in sun), ambient=0.25,
                    background=(10, 20, 30, 255))


def input_conditions(scene, kind, steps=96, refine_rounds=2, shadow_steps=48):
    """what the scenes must hold for the comparisons to mean something, from the model alone -> dict of figures (asserted by the tests)"""
    c, lift, distance = shadow_camera(kind, scene.omodel, scene.view)
    sample = RM.sampler(scene.otree, scene.T, scene.B, scene.layers)
    r = R.render(scene, c, steps, refine_rounds)
    hit = (r.hits["status"] == HIT)
    sun = np.array([np.float64(F(v)) for v in c.sun])
    points = r.hits["position"][hit]
    first, above = march_details(scene.omodel, sample, shadow_origins(scene.omodel, points, lift), sun, distance, shadow_steps)
    first0, _ = march_details(scene.omodel, sample, points, sun, distance, shadow_steps)  # lift = 0
    step = np.full(c.height * c.width, -1)
    step[hit] = first
    step = step.reshape(c.height, c.width)
    spans = [len(set(v for v in step[by:by + 8, bx:bx + 8].ravel().tolist() if v >= 0)) for by in range(0, c.height, 8) for bx in range(0, c.width, 8)]
    return dict(hit=int(hit.sum()), occluded=int((first >= 0).sum()), lit=int((first < 0).sum()), steps_in_a_block=max(spans),
                at_step_0=int((first == 0).sum()), at_step_0_without_lift=int((first0 == 0).sum()),
                lit_with_skipped_samples=int(((first < 0) & (above > 0)).sum()), lit_without_skipped_samples=int(((first < 0) & (above == 0)).sum()))


def assert_input_conditions(f):
    """among the main camera's HIT pixels at least 1 / 8 are occluded and 1 / 8 lit; the occluded pixels of one 8 x 8 block leave the
    shadow march at three steps or more; a pixel is decided at step 0 only when the lift is 0 (with the lift none is, without it every
    one: a hit point lies at or under the ground); lit shadow rays with samples above the ceiling (the skip) and without"""
    assert f["occluded"] * 8 >= f["hit"] and f["lit"] * 8 >= f["hit"], f
    assert f["steps_in_a_block"] >= 3, f
    assert f["at_step_0"] == 0 and f["at_step_0_without_lift"] >= 1, f
    assert f["lit_with_skipped_samples"] >= 1 and f["lit_without_skipped_samples"] >= 1, f

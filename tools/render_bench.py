#!/usr/bin/env python3
"""Times bt_tile_tree_render against the same picture composed from the calls a host had before it: bt_tile_tree_raycast on the pixel
rays in batches within its limit, then bt_tile_tree_sample_normal and bt_tile_tree_sample_attachment at the hit points, the grey encoded on
the host.  Prints one JSON line.  Not the headline benchmark (bench.py).

One process, raycast_bench.py's terrains (planar and sphere: synth_fbm_r16 sources, T = 512, 4 LODs, streamed into a tree along a short
camera path); the camera stands above the path's last position and looks down at a slant, 512 x 512 pixels, 256 steps, 2 refinement rounds.
Both forms are asserted to give the same four planes, byte for byte, then timed alternately (median of --repeats calls behind a spin-up; both
end in a synchronisation).

    python tools/render_bench.py [--repeats N] [--size 512]
    rocprofv3 --kernel-trace --stats --output-format csv -- python tools/render_bench.py --trace
        # kernel times: render_kernel beside raycast_kernel + tile_tree_normal_kernel + tile_tree_sample_kernel of the composition, --repeats
        # pictures each per model; the JSON line gives the launches per picture to divide by
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bevy_terrain_amd as bt
import raycast_bench as RB
from bevy_terrain_amd import _ffi

STEPS, ROUNDS = 256, 2
BACKGROUND = (120, 170, 230, 255)


def camera(model, view, size):
    """above the last view position, looking down at a slant: ground from near to far, sky above the horizon / beyond the terrain's edge"""
    pos = np.asarray(model.translation, dtype=np.float64)
    if model.kind == "planar":
        eye = np.array([view[0], pos[1] + model.max_height + 200.0, view[2]])
        return bt.RenderCamera.perspective(eye, (-0.7, -0.45, -0.55), (0.0, 1.0, 0.0), np.radians(60.0), size, size, 0.0, 2500.0, background=BACKGROUND)
    radial = RB.unit(np.asarray(view) - pos)
    east = RB.unit(np.cross(radial, (0.0, 0.0, 1.0)))
    eye = pos + radial * (model.scale_vec[0] + model.max_height + 4.0e5)
    return bt.RenderCamera.perspective(eye, east * 0.8 - radial * 0.6, radial, np.radians(60.0), size, size, 0.0, 3.5e6, background=BACKGROUND)


def enc8(v):
    c = np.where(v > 0.0, np.where(v > 1.0, np.float32(1.0), v), np.float32(0.0)).astype(np.float32)
    return np.floor(np.float32(0.5) + np.float32(255.0) * c).astype(np.uint8)


def compose(tree, cam, spans=None):
    """the picture from the older calls -> the same dict TileTree.render returns (without the stats).  spans (a dict): receives the
    seconds spent in the three groups of library calls and in the host's part"""
    t0 = time.perf_counter()
    origins, directions = bt.render_rays(cam)
    n = len(origins)
    batch = _ffi.RAYCAST_MAX_SAMPLES // (64 * ((STEPS + 1 + 63) // 64))  # bt_tile_tree_raycast counts a ray in whole rounds of 64 samples
    t1 = time.perf_counter()
    hits = np.concatenate([tree.raycast(0, origins[i:i + batch], directions[i:i + batch], cam.t_min, cam.t_max, steps=STEPS, refine_rounds=ROUNDS)
                           for i in range(0, n, batch)])
    t2 = time.perf_counter()
    met = (hits["status"] == _ffi.RAY_HIT) | (hits["status"] == _ffi.RAY_INSIDE)
    points = np.ascontiguousarray(hits["position"][met])
    normals = np.zeros((n, 3), np.float32)
    t3 = time.perf_counter()
    normals[met] = tree.sample_normal(0, points)[0]
    t4 = time.perf_counter()
    values = tree.sample_attachment(0, points)[0]
    t5 = time.perf_counter()
    rgba = np.tile(np.array(cam.background, np.uint8), (n, 1))
    grey = enc8(np.float32(0.5) * values[:, 0])
    rgba[met] = np.stack([grey, grey, grey, np.full_like(grey, 255)], axis=1)
    h, w = cam.height, cam.width
    out = {"t": hits["t"].reshape(h, w), "status": hits["status"].astype(np.uint8).reshape(h, w), "normal": normals.reshape(h, w, 3), "rgba": rgba.reshape(h, w, 4)}
    if spans is not None:
        t6 = time.perf_counter()
        for name, dt in (("raycast", t2 - t1), ("sample_normal", t4 - t3), ("sample_attachment", t5 - t4), ("host", (t1 - t0) + (t3 - t2) + (t6 - t5))):
            spans.setdefault(name, []).append(dt * 1e3)
    return out, -(-n // batch)


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--trace", action="store_true", help="no timing: --repeats pictures of either form per model, for a kernel trace")
    args = ap.parse_args()
    device = bt.Device(0)
    result = {"tool": "render_bench", "size": args.size, "steps": STEPS, "refine_rounds": ROUNDS, "repeats": args.repeats, "texture_size": RB.TEXTURE_SIZE}
    root = tempfile.mkdtemp(prefix="render_bench_")
    try:
        for kind in ("planar", "sphere"):
            model, atlas, tree, view, lods = RB.build(device, kind, os.path.join(root, kind))
            cam = camera(model, view, args.size)
            new = tree.render(cam, steps=STEPS, refine_rounds=ROUNDS)
            old, raycast_calls = compose(tree, cam)
            for plane in ("t", "status", "normal", "rgba"):
                assert np.ascontiguousarray(new[plane]).tobytes() == np.ascontiguousarray(old[plane]).tobytes(), (kind, plane)
            result[f"{kind}_entry_lods"] = lods
            result[f"{kind}_stats"] = new["stats"]
            result[f"{kind}_composition_launches"] = raycast_calls + 2
            if args.trace:
                for _ in range(args.repeats):  # alternating, so both forms see the same clock
                    tree.render(cam, steps=STEPS, refine_rounds=ROUNDS)
                    compose(tree, cam)
                continue
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < 0.3:  # clocks ramp over the first hundreds of milliseconds of work
                tree.render(cam, steps=STEPS, refine_rounds=ROUNDS)
            new_ms, old_ms, spans = [], [], {}
            for _ in range(args.repeats):
                device.synchronize()
                t0 = time.perf_counter()
                tree.render(cam, steps=STEPS, refine_rounds=ROUNDS)
                t1 = time.perf_counter()
                compose(tree, cam, spans)
                t2 = time.perf_counter()
                new_ms.append((t1 - t0) * 1e3)
                old_ms.append((t2 - t1) * 1e3)
            result[f"{kind}_render_wall_ms_median_min_max"] = [round(v, 3) for v in (median(new_ms), min(new_ms), max(new_ms))]
            result[f"{kind}_composition_wall_ms_median_min_max"] = [round(v, 3) for v in (median(old_ms), min(old_ms), max(old_ms))]
            result[f"{kind}_composition_wall_ms_median_by_part"] = {name: round(median(v), 3) for name, v in spans.items()}
            result[f"{kind}_wall_ratio_composition_over_render"] = round(median(old_ms) / median(new_ms), 2)
            tree.close()
    finally:
        shutil.rmtree(root, ignore_errors=True)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Times the sun shadows against what was there before them: bt_tile_tree_render_shadowed beside bt_tile_tree_render of the same camera (the
added cost of the shadow rays), and bt_tile_tree_sun_occlusion beside bt_tile_tree_raycast at refine 0 on identical rays (the shadow
rays of the picture's hit points, built on the host for the older call).  Prints one JSON line.  Not the headline benchmark (bench.py).

One process, raycast_bench.py's terrains (planar and sphere: synth_fbm_r16 sources, T = 512, 4 LODs, streamed into a tree along a short
camera path) under render_bench.py's camera with the light on and a low sun; 512 x 512 pixels, 256 steps, 2 refinement rounds; shadow rays
of 127 steps (two whole rounds of 64 samples for the older call, its best case).  Before anything is timed the shadowed picture is
asserted to be the plain one where lit and the plain one with the sun put out where occluded, and the two queries to give the same statuses.
Each pair is timed alternately (median of --repeats calls behind a spin-up; every call ends in a synchronisation).

    python tools/shadow_bench.py [--repeats N] [--size 512]
    rocprofv3 --kernel-trace --stats --output-format csv -- python tools/shadow_bench.py --trace
        # kernel times, in a run of their own with no counters: render_kernel<true> beside render_kernel<false>, occlusion_kernel beside
        # raycast_kernel, --repeats calls each per model; the JSON line gives the launches per call to divide by
    python tools/shadow_bench.py --summarise DIR/NAME_kernel_trace.csv
        # that trace per kernel and model (the planar terrain's dispatches come first, the sphere's are the second half): total ms
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
import render_bench as RD
from bevy_terrain_amd import _ffi

STEPS, ROUNDS, SHADOW_STEPS = RD.STEPS, RD.ROUNDS, 127


def sun_and_march(model, view):
    """(unit sun, lift, distance): 14 degrees over the horizon on the planar terrain, 1 degree over the view's horizon on the globe (its
    relief is gentle); a lift far above the residual of a (256, 2) march; a reach of the terrain's width / of 300 km on the globe"""
    if model.kind == "planar":
        return RB.unit((-0.55, 0.25, 0.8)), 0.5, 1000.0
    radial = RB.unit(np.asarray(view) - np.asarray(model.translation, dtype=np.float64))
    east = RB.unit(np.cross(radial, (0.0, 0.0, 1.0)))
    north = np.cross(east, radial)
    return RB.unit(east * 0.8 + north * 0.55 + radial * 0.02), 50.0, 3.0e5


def up_direction(model, pts):
    """n(q) of SUN OCCLUSION for the planar and the spherical model, operation by operation (f64 numpy)"""
    if model.kind == "planar":
        return np.tile([0.0, 1.0, 0.0], (len(pts), 1))
    pos, a = model.translation, model.scale_vec[0]
    q = [(pts[:, i] - pos[i]) / a for i in range(3)]
    r = 1.0 / np.sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2])
    n = [a * (q[i] * r) for i in range(3)]
    r = 1.0 / np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
    return np.stack([n[i] * r for i in range(3)], axis=1)


def raycast_occlusion(model, tree, points, sun, lift, distance):
    """the statuses from the older call: the shadow rays built on the host, in batches within its limit -> (statuses, calls)"""
    origins = points + lift * up_direction(model, points)
    directions = np.tile(sun, (len(points), 1))
    batch = _ffi.RAYCAST_MAX_SAMPLES // (64 * ((SHADOW_STEPS + 1 + 63) // 64))
    hits = [tree.raycast(0, origins[i:i + batch], directions[i:i + batch], 0.0, distance, steps=SHADOW_STEPS, refine_rounds=0) for i in range(0, len(points), batch)]
    return np.concatenate(hits)["status"].astype(np.uint8), len(hits)


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def alternate(device, first, second, repeats):
    """median, min, max wall ms of two calls timed in turn"""
    a, b = [], []
    for _ in range(repeats):
        device.synchronize()
        t0 = time.perf_counter()
        first()
        t1 = time.perf_counter()
        second()
        t2 = time.perf_counter()
        a.append((t1 - t0) * 1e3)
        b.append((t2 - t1) * 1e3)
    return [[round(v, 3) for v in (median(x), min(x), max(x))] for x in (a, b)]


def summarise(path):
    """a kernel trace of the --trace run -> {kernel: {model: [dispatches, total ms]}}"""
    import csv
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    out = {}
    for key in ("render_kernel<false>", "render_kernel<true>", "occlusion_kernel", "raycast_kernel"):
        ms = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in rows if key in r["Kernel_Name"]]
        half = len(ms) // 2
        out[key] = {"planar": [half, round(sum(ms[:half]), 3)], "sphere": [len(ms) - half, round(sum(ms[half:]), 3)]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--summarise", metavar="TRACE.csv", help="no GPU work: the kernel trace of a --trace run, per kernel and model")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--trace", action="store_true", help="no timing: --repeats calls of each of the four per model, for a kernel trace")
    args = ap.parse_args()
    if args.summarise:
        print(json.dumps({"tool": "shadow_bench", "kernel_ms": summarise(args.summarise)}), flush=True)
        return
    device = bt.Device(0)
    result = {"tool": "shadow_bench", "size": args.size, "steps": STEPS, "refine_rounds": ROUNDS, "shadow_steps": SHADOW_STEPS, "repeats": args.repeats,
              "texture_size": RB.TEXTURE_SIZE}
    root = tempfile.mkdtemp(prefix="shadow_bench_")
    try:
        for kind in ("planar", "sphere"):
            model, atlas, tree, view, lods = RB.build(device, kind, os.path.join(root, kind))
            sun, lift, distance = sun_and_march(model, view)
            cam = RD.camera(model, view, args.size)
            cam.lighting, cam.sun, cam.ambient = True, tuple(float(np.float32(v)) for v in sun), 0.3
            sun64 = np.array([np.float64(np.float32(v)) for v in sun])
            plain = lambda: tree.render(cam, steps=STEPS, refine_rounds=ROUNDS)
            shadowed = lambda: tree.render_shadowed(cam, lift, distance, SHADOW_STEPS, steps=STEPS, refine_rounds=ROUNDS)
            a, b = plain(), shadowed()
            dark = bt.RenderCamera(cam.origin, cam.forward, cam.right, cam.up, cam.width, cam.height, cam.t_min, cam.t_max, lighting=True, sun=(0.0, 0.0, 0.0),
                                   ambient=cam.ambient, background=cam.background)
            unlit = tree.render(dark, steps=STEPS, refine_rounds=ROUNDS, planes=("rgba",))["rgba"]
            occluded = (b["shadow"] == _ffi.RAY_HIT) | (b["shadow"] == _ffi.RAY_INSIDE)
            for plane in ("t", "status", "normal"):
                assert a[plane].tobytes() == b[plane].tobytes(), (kind, plane)
            assert b["rgba"].tobytes() == np.where(occluded[..., None], unlit, a["rgba"]).tobytes(), kind
            met = (a["status"] == _ffi.RAY_HIT) | (a["status"] == _ffi.RAY_INSIDE)
            origins, directions = bt.render_rays(cam)
            points = np.ascontiguousarray((origins + a["t"].reshape(-1, 1) * directions)[met.ravel()])
            query = lambda: tree.sun_occlusion(0, points, sun64, lift, distance, SHADOW_STEPS)
            older = lambda: raycast_occlusion(model, tree, points, sun64, lift, distance)
            (status, stats), (old_status, raycast_calls) = query(), older()
            assert np.array_equal(status[:, 0], old_status) and np.array_equal(status[:, 0], b["shadow"][met]), kind
            result[f"{kind}_entry_lods"] = lods
            result[f"{kind}_render_stats"] = a["stats"]
            result[f"{kind}_shadowed_launches"] = b["stats"]["launches"]
            result[f"{kind}_shadow_rays"] = len(points)
            result[f"{kind}_occlusion_stats"] = stats
            result[f"{kind}_raycast_calls"] = raycast_calls
            if args.trace:
                for _ in range(args.repeats):  # alternating, so all forms see the same clock
                    plain()
                    shadowed()
                    query()
                    older()
                continue
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < 0.3:  # clocks ramp over the first hundreds of milliseconds of work
                shadowed()
            result[f"{kind}_render_wall_ms_median_min_max"], result[f"{kind}_shadowed_wall_ms_median_min_max"] = alternate(device, plain, shadowed, args.repeats)
            result[f"{kind}_occlusion_wall_ms_median_min_max"], result[f"{kind}_raycast_wall_ms_median_min_max"] = alternate(device, query, older, args.repeats)
            tree.close()
    finally:
        shutil.rmtree(root, ignore_errors=True)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()

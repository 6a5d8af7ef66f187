#!/usr/bin/env python3
"""Times bt_tile_tree_raycast against what a host had before it: the same march driven from Python through
bt_tile_tree_sample_attachment, one call per coarse step and per refinement round for the whole batch.  Prints one JSON line.  Not the
headline benchmark (bench.py).

One process, one terrain per model (planar and sphere: synth_fbm_r16 sources, T = 512, 4 LODs, saved and streamed into a tree along a short
camera path, so rays cross tiles of several LODs and blend rings).  For 1, 64 and 4096 rays at steps 256, refine_rounds 2: the wall time of the
new call and of the baseline (median of --repeats calls behind warm-ups; both end in a synchronisation), and the assertion that both report
the same hits, bit for bit.

    python tools/raycast_bench.py [--repeats N]
    python tools/raycast_bench.py --worst-case        # the measurement behind BT_RAYCAST_MAX_SAMPLES: ellipsoid, every sample in a blend
                                                      # ring (three projections each), no hit, no sample above max_height, every shape
                                                      # of rays x steps the cap lets through at its edge
    rocprofv3 --kernel-trace --stats --output-format csv -- python tools/raycast_bench.py --trace [--steps 255]
                                                      # kernel times: raycast_kernel on 4096 rays beside tile_tree_sample_kernel on exactly the
                                                      # positions the raycast lanes evaluated; the JSON line gives the sample count to divide by
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

import bevy_terrain_amd as bt
from bevy_terrain_amd import _ffi

TEXTURE_SIZE, BORDER, LOD_COUNT, STEPS, ROUNDS = 512, 2, 4, 256, 2
MODELS = {"planar": bt.TerrainModel.planar((10.0, -5.0, 3.0), 1000.0, 0.0, 250.0),
          "sphere": bt.TerrainModel.sphere((0.0, 0.0, 0.0), 6371000.0, -12000.0, 9000.0)}


def unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def altitude(model, pts):
    """the header's altitude for the planar and the spherical model, operation by operation (f64 numpy)"""
    pos, a = model.translation, model.scale_vec[0]
    p = [pts[:, i] for i in range(3)]
    q = [(p[i] - pos[i]) / a for i in range(3)]
    if model.kind == "planar":
        local = [1.0 * q[0], 0.0 * q[1], 1.0 * q[2]]
        up = [np.zeros_like(q[0]), np.ones_like(q[0]), np.zeros_like(q[0])]
    else:
        r = 1.0 / np.sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2])
        local = [q[i] * r for i in range(3)]
        up = local
    n = [a * up[i] for i in range(3)]
    r = 1.0 / np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
    n = [n[i] * r for i in range(3)]
    d = [p[i] - ((a * local[i] + pos[i]) + 0.0 * n[i]) for i in range(3)]
    return (d[0] * n[0] + d[1] * n[1]) + d[2] * n[2]


def build(device, kind, root):
    """preprocess, save, and stream the terrain into a fresh atlas + tree along a descending path"""
    model = MODELS[kind]
    W = 2 ** (LOD_COUNT - 1) * (TEXTURE_SIZE - 2 * BORDER)
    cfg = bt.TerrainConfig(lod_count=LOD_COUNT, atlas_size=6 * 100 if model.is_spherical() else 100, path=f"terrains/raycast_{kind}", model=model)
    cfg.add_attachment(bt.AttachmentConfig(name="height", texture_size=TEXTURE_SIZE, border_size=BORDER, format=bt.AttachmentFormat.R16))
    atlas = bt.TileAtlas.new(cfg, device)
    server, pre, sources = bt.AssetServer(), bt.Preprocessor.new().clear_attachment(0, atlas), []
    if model.is_spherical():
        paths = [f"face{s}" for s in range(6)]
        for s, path in enumerate(paths):
            sources.append(device.synth_fbm_r16(W, W, 40 + s))
            server.insert(path, (sources[-1], W, W))
        pre.preprocess_spherical(bt.SphericalDataset(attachment_index=0, paths=paths, lod_range=range(0, LOD_COUNT)), server, atlas)
    else:
        sources.append(device.synth_fbm_r16(W, W, 40))
        server.insert("src", (sources[-1], W, W))
        pre.preprocess_tile(bt.PreprocessDataset(attachment_index=0, path="src", lod_range=range(0, LOD_COUNT)), server, atlas)
    pre.run(atlas)
    pre.save(atlas, root)
    pre.close()
    for ptr in sources:
        device.free(ptr)
    scfg = bt.TerrainConfig(lod_count=LOD_COUNT, atlas_size=cfg.atlas_size, path=cfg.path, model=model)
    scfg.add_attachment(bt.AttachmentConfig(name="height", texture_size=TEXTURE_SIZE, border_size=BORDER, format=bt.AttachmentFormat.R16))
    streamed = bt.TileAtlas.new(scfg, device)
    streamed.load_tile_config(root)
    tree = bt.TileTree.new(streamed, bt.TerrainViewConfig(tree_size=4, load_distance=1.2, blend_distance=1.0))
    for i in range(8):
        t = i / 7.0
        if kind == "planar":
            view = (10.0 + 300.0 * (1.0 - t), 800.0 * (1.0 - t) + 300.0, 3.0 + 200.0 * (1.0 - t))
        else:
            view = tuple(unit((0.4 + 0.3 * (1.0 - t), 0.8, 0.3)) * (6371000.0 + 3.0e6 * (1.0 - t) ** 2 + 2.0e4))
        tree.update(view)
        streamed.update(root)
        tree.apply_requests()
        tree.adjust_to_tile_atlas()
        tree.approximate_height()
    streamed.update(root)
    tree.adjust_to_tile_atlas()
    entries = tree.read()[0]
    lods = sorted(set(int(v) for v in entries[:, 1] if v != 0xFFFFFFFF))
    return model, streamed, tree, view, lods


def make_rays(model, view, n, seed):
    """half from above towards ground points up to a few tiles away, half from mid height and near horizontal"""
    rng = np.random.default_rng(seed)
    pos = np.asarray(model.translation)
    lo, hi = model.min_height, model.max_height
    half = (n + 1) // 2
    if model.kind == "planar":
        up = np.tile([0.0, 1.0, 0.0], (n, 1))
        ground = pos + np.column_stack([rng.uniform(-480, 480, n), np.zeros(n), rng.uniform(-480, 480, n)])
        reach = 600.0
    else:
        up = unit(unit(np.asarray(view) - pos) + rng.normal(size=(n, 3)) * 0.15)
        ground = pos + up * model.scale_vec[0]
        reach = 0.12 * model.scale_vec[0]
    side = unit(np.cross(up, unit(rng.normal(size=(n, 3)))))
    origins = ground + up * (hi + rng.uniform(0.2, 1.4, (n, 1)) * (hi - lo))
    target = ground + side * rng.uniform(0.0, 0.5, (n, 1)) * reach + up * lo
    directions = target - origins
    t_max = np.full(n, 1.25)
    origins[half:] = ground[half:] + up[half:] * (lo + rng.uniform(0.5, 0.9, (n - half, 1)) * (hi - lo))
    directions[half:] = unit(side[half:] + up[half:] * rng.uniform(-0.15, 0.05, (n - half, 1)))
    t_max[half:] = reach
    return origins, directions, np.zeros(n), t_max


def baseline(model, tree, origins, directions, t_min, t_max, steps, rounds, brackets=None):
    """the march a host drives itself: one bt_tile_tree_sample_attachment call per coarse step for the rays still undecided, one per
    refinement round for the rays that hit.  brackets (a list): receives (rays, lo, hi) as they stand before each refinement round"""
    n = len(origins)
    hits = np.zeros(n, bt.tile_tree.RAY_HIT_DTYPE)
    dt = (t_max - t_min) / np.float64(steps)
    undecided = np.arange(n)
    heights = np.zeros(n, np.float32)

    def below(rays, t):
        pts = origins[rays] + t[:, None] * directions[rays]
        h = tree.sample_attachment(0, pts)[1]
        return (altitude(model, pts) - h.astype(np.float64)) <= 0.0, h

    for i in range(steps + 1):
        if not len(undecided):
            break
        under, h = below(undecided, t_min[undecided] + np.float64(i) * dt[undecided])
        found = undecided[under]
        hits["status"][found] = _ffi.RAY_INSIDE if i == 0 else _ffi.RAY_HIT
        hits["step"][found] = i
        heights[found] = h[under]
        undecided = undecided[~under]
    hit = np.flatnonzero(hits["status"] == _ffi.RAY_HIT)
    lo = t_min + (hits["step"].astype(np.float64) - 1.0) * dt
    hi = t_min + hits["step"].astype(np.float64) * dt
    inside = hits["status"] == _ffi.RAY_INSIDE
    lo[inside] = hi[inside] = t_min[inside]
    k = np.arange(1, 64, dtype=np.float64) / 64.0
    for _ in range(rounds):
        if not len(hit):
            break
        if brackets is not None:
            brackets.append((hit.copy(), lo[hit].copy(), hi[hit].copy()))
        u = lo[hit, None] + (hi[hit] - lo[hit])[:, None] * k[None, :]  # (hits, 63)
        under, h = below(np.repeat(hit, 63), u.reshape(-1))
        under, h = under.reshape(-1, 63), h.reshape(-1, 63)
        first = np.where(under.any(axis=1), under.argmax(axis=1) + 1, 64)  # k*
        rows = np.arange(len(hit))
        ext = np.column_stack([lo[hit], u, hi[hit]])  # u_0 = lo .. u_64 = hi
        heights[hit] = np.where(first < 64, h[rows, np.minimum(first, 63) - 1], heights[hit])
        lo[hit], hi[hit] = ext[rows, first - 1], ext[rows, first]
    decided = hits["status"] != _ffi.RAY_MISS
    hits["t"][decided], hits["t_above"][decided] = hi[decided], lo[decided]
    hits["position"][decided] = origins[decided] + hi[decided, None] * directions[decided]
    hits["height"][decided] = heights[decided]
    return hits


def wall_ms(device, fn, repeats):
    times = []
    for _ in range(repeats):
        device.synchronize()
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def evaluated_positions(origins, directions, t_min, t_max, hits, steps, brackets):
    """every position a lane of raycast_kernel evaluated for these results: whole coarse rounds of 64 steps up to the hit's round (capped at
    `steps`), and u_1 .. u_63 of every refinement round's bracket (`brackets`: what baseline() recorded for the same, identical, hits)"""
    out = []
    dt = (t_max - t_min) / np.float64(steps)
    for r in range(len(origins)):
        status, step = int(hits["status"][r]), int(hits["step"][r])
        last = steps if status == _ffi.RAY_MISS else min((step // 64) * 64 + 63, steps)
        t = t_min[r] + np.arange(last + 1, dtype=np.float64) * dt[r]
        out.append(origins[r] + t[:, None] * directions[r])
    k = np.arange(1, 64, dtype=np.float64) / 64.0
    for rays, lo, hi in brackets:
        u = lo[:, None] + (hi - lo)[:, None] * k[None, :]
        out.append((origins[rays][:, None, :] + u[:, :, None] * directions[rays][:, None, :]).reshape(-1, 3))
    return np.vstack(out)


def spin_up(device, tree, origins, directions, t_min, t_max, seconds=0.3):
    """clocks ramp over the first hundreds of milliseconds of work: keep the device busy before anything is timed"""
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        tree.raycast(0, origins, directions, t_min, t_max, steps=STEPS, refine_rounds=ROUNDS)


def worst_case(device, repeats):
    model = bt.TerrainModel.ellipsoid((100.0, 200.0, -300.0), 6378137.0, 6356752.314245, -12000.0, 9000.0)
    cfg = bt.TerrainConfig(lod_count=8, atlas_size=4, path="terrains/none", model=model)
    cfg.add_attachment(bt.AttachmentConfig(name="height", texture_size=TEXTURE_SIZE, border_size=BORDER, format=bt.AttachmentFormat.R16))
    atlas = bt.TileAtlas.new(cfg, device)
    tree = bt.TileTree.new(atlas, bt.TerrainViewConfig(tree_size=4))  # blend_distance 2.0 (the default)
    centre = unit((0.4, 0.8, 0.3))
    scale = np.asarray(model.scale_vec)
    # nothing is loaded: h = min_height everywhere.  The view sits 2 * scale / 2^1.1 above the rays: target_lod 1.1, blend ratio 0.5 -> both lookups
    tree.update(tuple(np.asarray(model.translation) + centre * scale * (1.0 + 2.0 / 2.0 ** 1.1)))
    result = {}
    rng = np.random.default_rng(1)
    # every shape but the first and the last sits at the cap (count x rounds of 64 samples = 2^24, or the largest count below it): from the most
    # waves of one round each (two active lanes of 64 at steps 1) to the most rounds one wave can be asked for (1025 at steps 65536)
    for count, steps in ((1024, 4095), (262144, 1), (262144, 63), (131072, 64), (65536, 255), (4096, 4095), (255, 65536), (1, 65536)):
        up = unit(centre + rng.normal(size=(count, 3)) * 0.005)
        origins = np.asarray(model.translation) + up * scale + up * -2000.0  # between min_height and max_height, above the (unloaded) ground
        directions = unit(np.cross(up, unit(rng.normal(size=(count, 3)))))
        t_max = np.full(count, 1.0e5)  # level: rises 780 m by the end, still below max_height
        fn = lambda: tree.raycast(0, origins, directions, 0.0, t_max, steps=steps, refine_rounds=0)
        assert (fn()["status"] == _ffi.RAY_MISS).all()
        m = min(64, count)
        spin_up(device, tree, origins[:m], directions[:m], np.zeros(m), t_max[:m])
        ms = wall_ms(device, fn, repeats)
        result[f"ellipsoid_{count}x{steps + 1}_samples"] = count * (steps + 1)
        result[f"ellipsoid_{count}x{steps + 1}_wave_rounds"] = count * ((steps + 64) // 64)
        result[f"ellipsoid_{count}x{steps + 1}_wall_ms_median_min_max"] = [round(v, 3) for v in ms]
    return result


def main():
    global STEPS
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--worst-case", action="store_true")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--steps", type=int, default=STEPS, help="coarse steps of the timed marches (255: 256 samples, four full rounds of 64 lanes)")
    args = ap.parse_args()
    STEPS = args.steps
    device = bt.Device(0)
    result = {"tool": "raycast_bench", "steps": STEPS, "refine_rounds": ROUNDS, "texture_size": TEXTURE_SIZE, "repeats": args.repeats}
    if args.worst_case:
        result.update(worst_case(device, args.repeats))
        print(json.dumps(result), flush=True)
        return
    root = tempfile.mkdtemp(prefix="raycast_bench_")
    try:
        for kind in ("planar", "sphere"):
            model, atlas, tree, view, lods = build(device, kind, os.path.join(root, kind))
            result[f"{kind}_entry_lods"] = lods
            if args.trace:
                o, d, t0, t1 = make_rays(model, view, 4096, seed=4096)
                hits = tree.raycast(0, o, d, t0, t1, steps=STEPS, refine_rounds=ROUNDS)
                brackets = []
                assert baseline(model, tree, o, d, t0, t1, STEPS, ROUNDS, brackets).tobytes() == hits.tobytes()
                pts = evaluated_positions(o, d, t0, t1, hits, STEPS, brackets)
                ceiling = float(np.float32(model.min_height) + (np.float32(model.max_height) - np.float32(model.min_height)) * np.float32(1.0))
                result[f"{kind}_trace_samples"] = len(pts)
                coarse = np.where(hits["status"] == _ffi.RAY_MISS, STEPS // 64 + 1, hits["step"] // 64 + 1)
                result[f"{kind}_trace_lane_slots"] = int((coarse.sum() + ROUNDS * (hits["status"] == _ffi.RAY_HIT).sum()) * 64)  # rounds x 64 lanes
                result[f"{kind}_trace_samples_above_max_height"] = int((altitude(model, pts) > ceiling).sum())
                spin_up(device, tree, o, d, t0, t1)
                for _ in range(args.repeats):  # alternating, so both kernels see the same clock
                    tree.raycast(0, o, d, t0, t1, steps=STEPS, refine_rounds=ROUNDS)
                    tree.sample_attachment(0, pts)
                continue
            for count in (1, 64, 4096):
                o, d, t0, t1 = make_rays(model, view, count, seed=count)
                new = tree.raycast(0, o, d, t0, t1, steps=STEPS, refine_rounds=ROUNDS)
                old = baseline(model, tree, o, d, t0, t1, STEPS, ROUNDS)
                assert new.tobytes() == old.tobytes(), (kind, count, np.flatnonzero(new != old)[:8])
                spin_up(device, tree, o, d, t0, t1)
                new_ms = wall_ms(device, lambda: tree.raycast(0, o, d, t0, t1, steps=STEPS, refine_rounds=ROUNDS), args.repeats)
                old_ms = wall_ms(device, lambda: baseline(model, tree, o, d, t0, t1, STEPS, ROUNDS), max(3, args.repeats // 5))
                result[f"{kind}_{count}_status_miss_hit_inside"] = np.bincount(new["status"], minlength=3).tolist()
                result[f"{kind}_{count}_raycast_ms_median_min_max"] = [round(v, 4) for v in new_ms]
                result[f"{kind}_{count}_baseline_ms_median_min_max"] = [round(v, 3) for v in old_ms]
                result[f"{kind}_{count}_speedup"] = round(old_ms[0] / new_ms[0], 1)
            tree.close()
    finally:
        shutil.rmtree(root, ignore_errors=True)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()

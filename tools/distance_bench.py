#!/usr/bin/env python3
"""Times bt_atlas_distance_field beside a sequential host exact transform with the same tie rule (tools/distance_transform.cpp, compiled here
with -O3, one thread) on the same seeds, and writes profiles/distance.txt.  Not the headline benchmark (bench.py).

One 2048^2 window of bench.py's 16k job (synth_fbm_r16 16384^2, T = 512, lod_count 6; finest mosaic 16256^2) at an odd origin, with three
seed sets: the texels at or below the window's median height (dense: FROM_TEXELS), the rivers of bt_atlas_drainage at RIVER_CELLS cells or
more (sparse: a host plane), and one seed in a corner (a host plane; the outward search's worst case).  Before anything is timed the
device's two planes and its seed count are asserted equal to the host's.

    python tools/distance_bench.py [--repeats N] > distance_bench.json                  wall ms per call of both, median; one JSON line
    rocprofv3 --kernel-trace --output-format csv -d DIR -o distance -- python tools/distance_bench.py --trace [--repeats N]
        # kernel times, in a run of their own with no counters: --repeats calls of each case in turn, nothing else from this file's kernels
    python tools/distance_bench.py --summarise DIR/.../distance_kernel_trace.csv [--repeats N] > distance_kernels.json
        # no GPU work: that trace per case and kernel, median ms per call
    python tools/distance_bench.py --report profiles/distance.txt --json distance_bench.json --kernel-json distance_kernels.json [--note TEXT ...]
        # no GPU work: the two runs as the text file
"""
import argparse
import ctypes as C
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZE, TEXTURE_SIZE, BORDER, LOD_COUNT, ATLAS_SIZE, SEED = 16384, 512, 2, 6, 2048, 42  # bench.py's 16k job
CENTER = TEXTURE_SIZE - 2 * BORDER
MOSAIC = CENTER << (LOD_COUNT - 1)
ORIGIN = (7003, 6997)
SIDE = 2048
RIVER_CELLS = 2000
CASES = ["sea_level", "rivers", "one_corner"]
KERNELS = ("distance_summary_kernel", "distance_carry_kernel", "distance_fill_kernel", "distance_rows_kernel", "distance_finish_kernel")


def host_transform(tmp):
    """tools/distance_transform.cpp compiled into a shared object -> its function"""
    so = os.path.join(tmp, "libdistance_transform.so")
    compiler = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    subprocess.run([compiler, "-O3", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tools", "distance_transform.cpp")], check=True)
    fn = C.CDLL(so).distance_transform
    fn.restype = C.c_uint64
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    return fn


def median(values):
    values = sorted(values)
    return values[len(values) // 2]


def summarise(path, calls):
    """a kernel trace of a --trace run -> {case: {kernel: ms per call}}: a call's dispatches end with its finish launch"""
    import csv
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    groups, current = [], {k: 0.0 for k in KERNELS}
    for r in rows:
        name = r["Kernel_Name"]
        for k in KERNELS:
            if k in name:
                current[k] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
        if "distance_finish_kernel" in name:
            groups.append(current)
            current = {k: 0.0 for k in KERNELS}
    assert len(groups) == calls * len(CASES), (len(groups), calls)
    return {case: {k: round(median([g[k] for g in groups[i * calls:(i + 1) * calls]]), 4) for k in KERNELS} for i, case in enumerate(CASES)}


def report(args):
    result = json.loads([line for line in open(args.json) if line.startswith("{")][-1])
    trace = json.load(open(args.kernel_json))["kernel_ms"] if args.kernel_json else {}
    lines = ["bt_atlas_distance_field - what was measured and what was not",
             "",
             f"1 x MI355X, tools/distance_bench.py, bench.py's 16k job (T = {TEXTURE_SIZE}, {LOD_COUNT} LODs, finest mosaic {MOSAIC}^2), a {SIDE}^2 window at",
             f"({ORIGIN[0]}, {ORIGIN[1]}), median of {result['repeats']} calls.  Wall: the synchronous call, both planes copied out, no bake.  Host:",
             "tools/distance_transform.cpp (columns in two sweeps, then a lower-envelope stack scan per row, the header's tie rule, g++ -O3) on the same",
             "seed plane, one thread, making the seed plane not counted.  The device's planes and its seed count were asserted equal to the",
             "host's before timing.  Kernel times: rocprofv3 --kernel-trace in a run of its own (no counters), median per call.  The row phase",
             "is the outward search; the envelope form was not built.",
             "",
             f"{'case':12s} {'seeds':>9s} {'max dist2':>10s} {'wall ms':>9s} {'host ms':>9s} {'host/wall':>9s} {'summary':>8s} {'carry':>8s} {'fill':>8s} {'rows':>9s} {'finish':>8s}  (kernels: ms)"]
    for case in CASES:
        r, k = result["cases"][case], trace.get(case, {})
        wall, host = r["wall_ms_median_min_max"][0], r["host_ms_median_min_max"][0]
        lines.append(f"{case:12s} {r['stats']['seeds']:9d} {r['stats']['max_dist2']:10d} {wall:9.2f} {host:9.1f} {host / wall:9.3g} "
                     + " ".join(f"{k.get(name, float('nan')):{width}.3f}" for name, width in zip(KERNELS, (8, 8, 8, 9, 8))))
    for note in args.note or []:
        lines += [""] + note.split("\\n")
    with open(args.report, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {args.report}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--trace", action="store_true", help="no timing and no host transform: --repeats calls of each case, for a kernel trace")
    ap.add_argument("--report", metavar="FILE", help="no GPU work: write the text file from --json and --kernel-json")
    ap.add_argument("--json", metavar="FILE")
    ap.add_argument("--kernel-json", metavar="FILE", help="the line --summarise printed")
    ap.add_argument("--summarise", metavar="CSV", help="no GPU work: the kernel trace of a --trace run with the same --repeats as one JSON line")
    ap.add_argument("--note", action="append", help="a paragraph appended to the report")
    args = ap.parse_args()
    if args.summarise:
        print(json.dumps({"tool": "distance_bench", "calls": args.repeats, "kernel_ms": summarise(args.summarise, args.repeats)}), flush=True)
        return
    if args.report:
        return report(args)

    import bevy_terrain_amd as bt

    device = bt.Device(0)
    cfg = bt.TerrainConfig(lod_count=LOD_COUNT, atlas_size=ATLAS_SIZE, path="terrains/bench16k", model=bt.TerrainModel.planar((0.0, 0.0, 0.0), 1000.0, 0.0, 1.0))
    cfg.add_attachment(bt.AttachmentConfig(name="height", texture_size=TEXTURE_SIZE, border_size=BORDER, format=bt.AttachmentFormat.R16))
    atlas = bt.TileAtlas.new(cfg, device)
    src = device.synth_fbm_r16(SIZE, SIZE, SEED)
    bt.Preprocessor.new().clear_attachment(0, atlas).preprocess_tile(
        bt.PreprocessDataset(attachment_index=0, path="synthetic/fbm16k", lod_range=range(0, LOD_COUNT)), bt.AssetServer().insert("synthetic/fbm16k", (src, SIZE, SIZE)), atlas).run(atlas)
    x0, y0 = ORIGIN
    raw, _ = atlas.read_region(0, x0, y0, SIDE, SIDE)
    level = int(np.median(raw))
    accumulation = atlas.drainage(0, x0, y0, SIDE, SIDE)[3]
    corner = np.zeros((SIDE, SIDE), np.uint8)
    corner[0, 0] = 1
    # case -> (the arguments of the call, the seed plane the host is given)
    cases = {"sea_level": (dict(lo=0, hi=level), (raw <= level).astype(np.uint8)),
             "rivers": (dict(seeds=(accumulation >= RIVER_CELLS).astype(np.uint8)), None),
             "one_corner": (dict(seeds=corner), None)}
    call = lambda case, **kw: atlas.distance_field(0, x0, y0, SIDE, SIDE, **cases[case][0], **kw)
    if args.trace:
        for case in CASES:
            for _ in range(args.repeats):
                call(case)
        return
    result = {"tool": "distance_bench", "repeats": args.repeats, "texture_size": TEXTURE_SIZE, "mosaic": MOSAIC, "origin": list(ORIGIN), "side": SIDE, "sea_level": level,
              "river_cells": RIVER_CELLS, "cases": {}}
    tmp = tempfile.mkdtemp(prefix="distance_bench_")
    try:
        transform = host_transform(tmp)
        for case in CASES:
            kw, plane = cases[case]
            plane = np.ascontiguousarray(kw["seeds"] if plane is None else plane)
            host_planes = [np.zeros((SIDE, SIDE), np.uint32) for _ in range(2)]
            host = lambda: transform(plane.ctypes.data, SIDE, SIDE, *[p.ctypes.data for p in host_planes])
            host_ms = []
            for _ in range(3):
                t0 = time.perf_counter()
                seeds = host()
                host_ms.append((time.perf_counter() - t0) * 1e3)
            *planes, stats = call(case)
            for name, got, want in zip(("dist2", "nearest"), planes, host_planes):
                assert got.tobytes() == want.tobytes(), (case, name)
            assert stats["seeds"] == seeds and stats["max_dist2"] == int(host_planes[0].max()), (stats, seeds)
            wall = []
            for _ in range(args.repeats):
                device.synchronize()
                t0 = time.perf_counter()
                *_, stats = call(case)
                wall.append((time.perf_counter() - t0) * 1e3)
            stats = {k: v for k, v in stats.items() if k not in ("edit", "changed")}
            result["cases"][case] = dict(stats=stats, wall_ms_median_min_max=[round(v, 3) for v in (median(wall), min(wall), max(wall))],
                                         host_ms_median_min_max=[round(v, 1) for v in (median(host_ms), min(host_ms), max(host_ms))])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()

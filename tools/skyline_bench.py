#!/usr/bin/env python3
"""Times bt_atlas_skyline beside a sequential host hull walk with the same tie rule (tools/skyline_hull.cpp, compiled here with -O3, one
thread) on the same window, and writes profiles/skyline.txt.  Not the headline benchmark (bench.py).

One 2048^2 window of bench.py's 16k job (synth_fbm_r16 16384^2, T = 512, lod_count 6; finest mosaic 16256^2) at an odd origin, with three
direction sets: one oblique direction, 16 and 64 azimuths round the compass (axes, diagonals and obliques among them; 64 directions are
four batches of 16 at this size), each with a sun from TileAtlas.sun_directions.  Before anything is timed the device's four planes and
its sums are asserted equal to the host's.

    python tools/skyline_bench.py [--repeats N] > skyline_bench.json                  wall ms per call of both, median; one JSON line
    rocprofv3 --kernel-trace --output-format csv -d DIR -o skyline -- python tools/skyline_bench.py --trace [--repeats N]
        # kernel times, in a run of their own with no counters: --repeats calls of each case in turn, nothing else from this file's kernels
    python tools/skyline_bench.py --summarise DIR/.../skyline_kernel_trace.csv [--repeats N] > skyline_kernels.json
        # no GPU work: that trace per case and kernel, median ms per call
    python tools/skyline_bench.py --report profiles/skyline.txt --json skyline_bench.json --kernel-json skyline_kernels.json [--note TEXT ...]
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
CELL_SIZE, RAW_UNIT = 30.0, 1.0  # metres: a cell's width, the height of one raw unit (suns of 3 to 30 raw units a cell: shadows on this terrain)
CASES = {"one_oblique": 1, "round_16": 16, "round_64": 64}
BATCH = 16  # directions in flight at 2^22 cells
KERNELS = ("viewshed_transpose_kernel", "skyline_walk_kernel", "skyline_finish_kernel")


def directions(case):
    from bevy_terrain_amd import TileAtlas
    n = CASES[case]
    if n == 1:
        rows = TileAtlas.sun_directions(0.0, 20.0, CELL_SIZE, RAW_UNIT)
        rows[0, :2] = (3, 1)
        return rows
    azimuth = np.arange(n) * 360.0 / n
    elevation = 5.0 + 40.0 * np.sin(np.pi * (np.arange(n) + 0.5) / n)  # a day's arc, turned round the whole compass
    return TileAtlas.sun_directions(azimuth, elevation, CELL_SIZE, RAW_UNIT)


def host_hull(tmp):
    """tools/skyline_hull.cpp compiled into a shared object -> its function"""
    so = os.path.join(tmp, "libskyline_hull.so")
    compiler = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    subprocess.run([compiler, "-O3", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tools", "skyline_hull.cpp")], check=True)
    fn = C.CDLL(so).skyline_hull
    fn.restype = C.c_uint64
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return fn


def median(values):
    values = sorted(values)
    return values[len(values) // 2]


def summarise(path, calls):
    """a kernel trace of a --trace run -> {case: {kernel: ms per call}}: a call's dispatches end with the finish launch of its last batch"""
    import csv
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    finishes = [-(-n // BATCH) for n in CASES.values() for _ in range(calls)]  # per call, in order
    groups, current, seen = [], {k: 0.0 for k in KERNELS}, 0
    for r in rows:
        name = r["Kernel_Name"]
        for k in KERNELS:
            if k in name:
                current[k] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
        if "skyline_finish_kernel" in name:
            seen += 1
            if seen == finishes[len(groups)]:
                groups.append(current)
                current, seen = {k: 0.0 for k in KERNELS}, 0
    assert len(groups) == calls * len(CASES), (len(groups), calls)
    return {case: {k: round(median([g[k] for g in groups[i * calls:(i + 1) * calls]]), 4) for k in KERNELS} for i, case in enumerate(CASES)}


def report(args):
    result = json.loads([line for line in open(args.json) if line.startswith("{")][-1])
    trace = json.load(open(args.kernel_json))["kernel_ms"] if args.kernel_json else {}
    lines = ["bt_atlas_skyline - what was measured and what was not",
             "",
             f"1 x MI355X, tools/skyline_bench.py, bench.py's 16k job (T = {TEXTURE_SIZE}, {LOD_COUNT} LODs, finest mosaic {MOSAIC}^2), a {SIDE}^2 window at",
             f"({ORIGIN[0]}, {ORIGIN[1]}), median of {result['repeats']} calls.  Wall: the synchronous call with the mask and the count copied out (the",
             "steps and rise planes, 6 bytes a cell and direction, stay on the device), no bake; wall all: with all four planes copied out.  Host:",
             "tools/skyline_hull.cpp (the header's hull walk line by line on the row-major window, g++ -O3), one thread, all four planes, median",
             f"of {result['host_repeats']}.  The device's four planes, lit and sum_steps were asserted equal to the host's before timing.  Kernel times:",
             "rocprofv3 --kernel-trace in a run of its own (no counters), median per call, the batches of a call summed.",
             "",
             f"{'case':12s} {'dirs':>4s} {'lines':>7s} {'max steps':>9s} {'wall ms':>9s} {'wall all':>9s} {'host ms':>9s} {'host/wall':>9s} {'wins':>6s} {'transpose':>9s} {'walk':>9s} {'finish':>8s}  (kernels: ms)"]
    for case in CASES:
        r, k = result["cases"][case], trace.get(case, {})
        wall, full, host = r["wall_ms_median_min_max"][0], r["wall_all_planes_ms_median_min_max"][0], r["host_ms_median_min_max"][0]
        lines.append(f"{case:12s} {r['stats']['directions']:4d} {r['stats']['lines']:7d} {r['stats']['max_steps']:9d} {wall:9.2f} {full:9.2f} {host:9.1f} {host / wall:9.3g} "
                     f"{'device' if wall < host else 'host':>6s} " + " ".join(f"{k.get(name, float('nan')):{width}.3f}" for name, width in zip(KERNELS, (9, 9, 8))))
    for note in args.note or []:
        lines += [""] + note.split("\\n")
    with open(args.report, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {args.report}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--trace", action="store_true", help="no timing and no host walk: --repeats calls of each case, for a kernel trace")
    ap.add_argument("--report", metavar="FILE", help="no GPU work: write the text file from --json and --kernel-json")
    ap.add_argument("--json", metavar="FILE")
    ap.add_argument("--kernel-json", metavar="FILE", help="the line --summarise printed")
    ap.add_argument("--summarise", metavar="CSV", help="no GPU work: the kernel trace of a --trace run with the same --repeats as one JSON line")
    ap.add_argument("--note", action="append", help="a paragraph appended to the report")
    args = ap.parse_args()
    if args.summarise:
        print(json.dumps({"tool": "skyline_bench", "calls": args.repeats, "kernel_ms": summarise(args.summarise, args.repeats)}), flush=True)
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
    call = lambda case, **kw: atlas.skyline(0, x0, y0, SIDE, SIDE, directions(case), **kw)
    if args.trace:
        for case in CASES:
            for _ in range(args.repeats):
                call(case, steps=False, rise=False)
        return
    raw, _ = atlas.read_region(0, x0, y0, SIDE, SIDE)
    raw = np.ascontiguousarray(raw)
    host_repeats = 3
    result = {"tool": "skyline_bench", "repeats": args.repeats, "host_repeats": host_repeats, "texture_size": TEXTURE_SIZE, "mosaic": MOSAIC, "origin": list(ORIGIN), "side": SIDE,
              "cases": {}}
    tmp = tempfile.mkdtemp(prefix="skyline_bench_")
    try:
        hull = host_hull(tmp)
        for case, n in CASES.items():
            rows = np.ascontiguousarray(directions(case), dtype=np.int64)
            host_planes = [np.zeros((n, SIDE, SIDE), np.uint16), np.zeros((n, SIDE, SIDE), np.int32), np.zeros((SIDE, SIDE), np.uint64), np.zeros((SIDE, SIDE), np.uint8)]
            host_ms = []
            for _ in range(host_repeats if n <= 16 else 1):
                t0 = time.perf_counter()
                sum_steps = hull(raw.ctypes.data, SIDE, SIDE, rows.ctypes.data, n, *[p.ctypes.data for p in host_planes])
                host_ms.append((time.perf_counter() - t0) * 1e3)
            *planes, stats = call(case)
            for name, got, want in zip(("steps", "rise", "mask", "count"), planes, host_planes):
                assert got.tobytes() == want.tobytes(), (case, name)
            assert stats["sum_steps"] == sum_steps and stats["lit"] == int(host_planes[3].sum(dtype=np.int64)) and stats["max_steps"] == int(host_planes[0].max()), stats
            assert stats["launches"] == 2 + 2 * -(-n // BATCH), stats
            del planes, host_planes
            timed = {}
            for key, kw in (("wall", dict(steps=False, rise=False)), ("wall_all_planes", {})):
                wall = []
                for _ in range(args.repeats if key == "wall" or n <= 16 else 2):
                    device.synchronize()
                    t0 = time.perf_counter()
                    *_, stats = call(case, **kw)
                    wall.append((time.perf_counter() - t0) * 1e3)
                timed[key + "_ms_median_min_max"] = [round(v, 3) for v in (median(wall), min(wall), max(wall))]
            stats = {k: v for k, v in stats.items() if k not in ("edit", "changed")}
            result["cases"][case] = dict(stats=stats, host_ms_median_min_max=[round(v, 1) for v in (median(host_ms), min(host_ms), max(host_ms))], **timed)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()

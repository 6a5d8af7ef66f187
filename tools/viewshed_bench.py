#!/usr/bin/env python3
"""Times bt_atlas_viewshed beside a sequential host walk of the same lines (tools/viewshed_lines.cpp, compiled here with -O3, one thread)
on the same gathered heights, and writes profiles/viewshed.txt.  Not the headline benchmark (bench.py).

Four cases on bench.py's 16k job (synth_fbm_r16 16384^2, T = 512, lod_count 6; finest mosaic 16256^2): windows of 1024^2 and 2048^2 at an
odd origin, with 1 and with 16 observers.  Before anything is timed the device's three planes and its sample count are asserted equal to
the host's, wherever the host runs: always at 1024^2, and at 2048^2 when eight times its 1024^2 time stays under a minute.

    python tools/viewshed_bench.py [--repeats N] > viewshed_bench.json                  wall ms per call of both, median; one JSON line
    rocprofv3 --kernel-trace --output-format csv -d DIR -o viewshed -- python tools/viewshed_bench.py --trace [--repeats N]
        # kernel times, in a run of their own with no counters: --repeats calls of each case in turn, nothing else
    python tools/viewshed_bench.py --summarise DIR/.../viewshed_kernel_trace.csv [--repeats N] > viewshed_kernels.json
        # no GPU work: that trace per case and kernel, median ms per call
    python tools/viewshed_bench.py --report profiles/viewshed.txt --json viewshed_bench.json --kernel-json viewshed_kernels.json [--note TEXT ...]
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
CASES = [(1024, 1), (1024, 16), (2048, 1), (2048, 16)]  # (side, observers)
EYE_HEIGHT, TARGET_HEIGHT = 200, 30
KERNELS = ("viewshed_transpose_kernel", "viewshed_walk", "viewshed_finish_kernel")
HOST_LIMIT_S = 60.0


def case_name(case):
    return f"{case[0]}x{case[0]}_{case[1]}obs"


def observers_of(side, count):
    """the first in the middle, the others scattered by a fixed rule; (count, 4) uint32"""
    rng = np.random.default_rng(7)
    xy = np.concatenate([[[side // 2, side // 2]], rng.integers(0, side, (count - 1, 2))]).astype(np.uint32)
    return np.concatenate([xy, np.full((count, 1), EYE_HEIGHT, np.uint32), np.zeros((count, 1), np.uint32)], axis=1)


def host_walk(tmp):
    """tools/viewshed_lines.cpp compiled into a shared object -> its function"""
    so = os.path.join(tmp, "libviewshed_lines.so")
    compiler = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    subprocess.run([compiler, "-O3", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tools", "viewshed_lines.cpp")], check=True)
    fn = C.CDLL(so).viewshed_lines
    fn.restype = C.c_uint64
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    return fn


def median(values):
    values = sorted(values)
    return values[len(values) // 2]


def summarise(path, calls):
    """a kernel trace of a --trace run -> {case: {kernel: [ms per call, dispatches per call]}}: a call's dispatches end with its finish launch"""
    import csv
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    groups, current = [], {k: [0.0, 0] for k in KERNELS}
    for r in rows:
        name = r["Kernel_Name"]
        for k in KERNELS:
            if k in name:
                current[k][0] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
                current[k][1] += 1
        if "viewshed_finish_kernel" in name:
            groups.append(current)
            current = {k: [0.0, 0] for k in KERNELS}
    assert len(groups) == calls * len(CASES), (len(groups), calls)
    return {case_name(case): {k: [round(median([g[k][0] for g in groups[i * calls:(i + 1) * calls]]), 4), median([g[k][1] for g in groups[i * calls:(i + 1) * calls]])]
                              for k in KERNELS} for i, case in enumerate(CASES)}


def report(args):
    result = json.loads([line for line in open(args.json) if line.startswith("{")][-1])
    trace = json.load(open(args.kernel_json))["kernel_ms"] if args.kernel_json else {}
    lines = ["bt_atlas_viewshed - what was measured and what was not",
             "",
             f"1 x MI355X, tools/viewshed_bench.py, bench.py's 16k job (T = {TEXTURE_SIZE}, {LOD_COUNT} LODs, finest mosaic {MOSAIC}^2), windows at",
             f"({ORIGIN[0]}, {ORIGIN[1]}), eye height {EYE_HEIGHT}, target height {TARGET_HEIGHT}, no radius, median of {result['repeats']} calls.  Wall: the synchronous call, host",
             "arrays out (clearance and count copied out).  Host: tools/viewshed_lines.cpp (the same lines walked with the same DDA, g++ -O3) on",
             "the texels bt_atlas_read_region returned, one thread, the read not counted.  The device's planes and its sample count were",
             "asserted equal to the host's before timing wherever the host ran.  Kernel times: rocprofv3 --kernel-trace in a run of its own",
             "(no counters), median per call, the sum over a call's dispatches.  Samples/s: line samples over the walk kernels' time.",
             "",
             f"{'case':16s} {'samples':>14s} {'wall ms':>10s} {'host ms':>11s} {'host/wall':>9s} {'transpose ms':>12s} {'walk ms':>10s} {'finish ms':>9s} {'Gsamples/s':>10s}"]
    for case in CASES:
        name = case_name(case)
        r, k = result["cases"][name], trace.get(name, {})
        host = r.get("host_ms_median_min_max")
        walk = k.get("viewshed_walk", [float("nan"), 0])[0]
        lines.append(f"{name:16s} {r['stats']['samples']:14d} {r['wall_ms_median_min_max'][0]:10.2f} " + (f"{host[0]:11.1f} {host[0] / r['wall_ms_median_min_max'][0]:9.3g}" if host else f"{'not run':>11s} {'':9s}")
                     + f" {k.get('viewshed_transpose_kernel', [float('nan')])[0]:12.3f} {walk:10.3f} {k.get('viewshed_finish_kernel', [float('nan')])[0]:9.3f} {r['stats']['samples'] / walk / 1e6:10.2f}")
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
        print(json.dumps({"tool": "viewshed_bench", "calls": args.repeats, "kernel_ms": summarise(args.summarise, args.repeats)}), flush=True)
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
    call = lambda side, observers, **kw: atlas.viewshed(0, x0, y0, side, side, observers, target_height=TARGET_HEIGHT, **kw)
    if args.trace:
        for side, count in CASES:
            for _ in range(args.repeats):
                call(side, observers_of(side, count))
        return
    result = {"tool": "viewshed_bench", "repeats": args.repeats, "texture_size": TEXTURE_SIZE, "mosaic": MOSAIC, "origin": list(ORIGIN), "cases": {}}
    tmp = tempfile.mkdtemp(prefix="viewshed_bench_")
    try:
        walk = host_walk(tmp)
        host_s = {}  # observers -> seconds of the 1024^2 host walk
        for side, count in CASES:
            observers = observers_of(side, count)
            host_ms = None
            if side == 1024 or 8.0 * host_s[count] < HOST_LIMIT_S:
                raw, _ = atlas.read_region(0, x0, y0, side, side)
                host_planes = [np.zeros((side, side), t) for t in (np.uint32, np.uint8, np.uint64)]
                host = lambda: walk(raw.ctypes.data, side, side, observers.ctypes.data, count, TARGET_HEIGHT, *[p.ctypes.data for p in host_planes])
                t0 = time.perf_counter()
                samples = host()
                host_ms = [(time.perf_counter() - t0) * 1e3]
                *planes, stats = call(side, observers, mask=True)
                for name, got, want in zip(("clearance", "count", "mask"), planes, host_planes):
                    assert got.tobytes() == want.tobytes(), (side, count, name)
                assert stats["samples"] == samples, (stats, samples)
                if side == 1024:
                    host_s[count] = host_ms[0] / 1e3
                    for _ in range(2 if host_ms[0] < 5e3 else 0):  # twice more where it is cheap
                        t0 = time.perf_counter()
                        host()
                        host_ms.append((time.perf_counter() - t0) * 1e3)
            wall = []
            for _ in range(args.repeats):
                device.synchronize()
                t0 = time.perf_counter()
                *_, stats = call(side, observers)
                wall.append((time.perf_counter() - t0) * 1e3)
            entry = dict(stats=stats, wall_ms_median_min_max=[round(v, 3) for v in (median(wall), min(wall), max(wall))])
            if host_ms:
                entry["host_ms_median_min_max"] = [round(v, 1) for v in (median(host_ms), min(host_ms), max(host_ms))]
            result["cases"][case_name((side, count))] = entry
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()

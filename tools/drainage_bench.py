#!/usr/bin/env python3
"""Times bt_atlas_drainage beside a sequential host analysis (tools/drainage_flood.cpp: priority-flood, a breadth-first search and a
topological accumulation, compiled here with -O3, one thread) on the same gathered heights, and writes profiles/drainage.txt.  Not the
headline benchmark (bench.py).

One scene on bench.py's 16k job (synth_fbm_r16 16384^2, T = 512, lod_count 6; finest mosaic 16256^2): a 2048 x 2048 window at an odd
origin.  Before anything is timed the device's four planes are asserted equal to the host's.

    python tools/drainage_bench.py [--repeats N] > drainage_bench.json                wall ms per call of both, median; sweeps; one JSON line
    rocprofv3 --kernel-trace --output-format csv -d DIR -o drainage -- python tools/drainage_bench.py --trace [--repeats N]
        # kernel times, in a run of their own with no counters: --repeats calls, nothing else
    python tools/drainage_bench.py --summarise DIR/.../drainage_kernel_trace.csv [--repeats N] > drainage_kernels.json
        # no GPU work: that trace per kernel, median ms per call
    python tools/drainage_bench.py --report profiles/drainage.txt --json drainage_bench.json --kernel-json drainage_kernels.json [--note TEXT ...]
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
WINDOW = (7003, 6997, 2048, 2048)
KERNELS = ("drain_prepare_kernel", "FillRule", "drain_flat_seed_kernel", "FlatRule", "drain_direction_kernel", "AccumulateRule", "drain_finish_kernel")


def host_analysis(tmp):
    """tools/drainage_flood.cpp compiled into a shared object -> its function"""
    so = os.path.join(tmp, "libdrainage_flood.so")
    compiler = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    subprocess.run([compiler, "-O3", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tools", "drainage_flood.cpp")], check=True)
    fn = C.CDLL(so).drainage_flood
    fn.restype = C.c_uint32
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return fn


def median(values):
    values = sorted(values)
    return values[len(values) // 2]


def summarise(path, calls):
    """a kernel trace of a --trace run -> {kernel: [ms per call, dispatches per call]}: a call's dispatches are those from its prepare launch to the next"""
    import csv
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    groups = []
    for r in rows:
        name = r["Kernel_Name"]
        if "drain_prepare_kernel" in name:
            groups.append({k: [0.0, 0] for k in KERNELS})
        if not groups:
            continue
        for k in KERNELS:
            if k in name and (k.startswith("drain_") or "relax_kernel" in name):  # the rules: relax_kernel<Rule> of bt_relax.hpp
                groups[-1][k][0] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
                groups[-1][k][1] += 1
    assert len(groups) == calls, (len(groups), calls)
    return {k: [round(median([g[k][0] for g in groups]), 4), median([g[k][1] for g in groups])] for k in KERNELS}


def report(args):
    result = json.loads([line for line in open(args.json) if line.startswith("{")][-1])
    trace = json.load(open(args.kernel_json))["kernel_ms"] if args.kernel_json else {}
    s, wall, host = result["stats"], result["wall_ms_median_min_max"], result["host_ms_median_min_max"]
    lines = ["bt_atlas_drainage - what was measured and what was not",
             "",
             f"1 x MI355X, tools/drainage_bench.py, bench.py's 16k job (T = {TEXTURE_SIZE}, {LOD_COUNT} LODs, finest mosaic {MOSAIC}^2), a {WINDOW[2]} x {WINDOW[3]} window at",
             f"({WINDOW[0]}, {WINDOW[1]}), median of {result['repeats']} calls.  Wall: the synchronous call, host arrays out (all four planes copied out).  Host:",
             "tools/drainage_flood.cpp (priority-flood, breadth-first search, topological accumulation; g++ -O3) on the texels",
             "bt_atlas_read_region returned, one thread, the read not counted.  The device's four planes were asserted equal to the host's",
             "before timing.  Kernel times: rocprofv3 --kernel-trace in a run of its own (no counters), median per call, the sum over a",
             "call's dispatches.",
             "",
             f"cells {s['cells']}  outlets {s['outlets']}  filled {s['filled']}  flats {s['flats']}  max flat distance {s['max_flat_distance']}  max accumulation {s['max_accumulation']}",
             f"sweeps: fill {s['sweeps_fill']}, flat {s['sweeps_flat']}, accumulate {s['sweeps_accumulate']}; launches {s['launches']}",
             f"wall ms    {wall[0]:9.2f} ({wall[1]:.2f} .. {wall[2]:.2f})",
             f"host ms    {host[0]:9.2f} ({host[1]:.2f} .. {host[2]:.2f})",
             f"host / wall (above 1: the device call is faster): {host[0] / wall[0]:.3g}",
             "",
             f"{'kernel':38s}  ms per call  dispatches"]
    for k in KERNELS:
        ms, n = trace.get(k, [float("nan"), 0])
        name = k if k.startswith("drain_") else "relax_kernel<" + k + ">"
        lines.append(f"{name:38s}  {ms:11.3f}  {n:10d}")
    for note in args.note or []:
        lines += [""] + note.split("\\n")
    with open(args.report, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {args.report}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--trace", action="store_true", help="no timing and no host analysis: --repeats calls, for a kernel trace")
    ap.add_argument("--report", metavar="FILE", help="no GPU work: write the text file from --json and --kernel-json")
    ap.add_argument("--json", metavar="FILE")
    ap.add_argument("--kernel-json", metavar="FILE", help="the line --summarise printed")
    ap.add_argument("--summarise", metavar="CSV", help="no GPU work: the kernel trace of a --trace run with the same --repeats as one JSON line")
    ap.add_argument("--note", action="append", help="a paragraph appended to the report")
    args = ap.parse_args()
    if args.summarise:
        print(json.dumps({"tool": "drainage_bench", "calls": args.repeats, "kernel_ms": summarise(args.summarise, args.repeats)}), flush=True)
        return
    if args.report:
        return report(args)

    import bevy_terrain_amd as bt
    from bevy_terrain_amd import _ffi

    if os.environ.get("BT_LIB"):  # another build of the library, e.g. tools/libbevy_terrain_amd_dbg.so (make -C bevy_terrain_amd/csrc debug) with BT_DRAIN_ROUNDS set
        _ffi.LIB_PATH = os.environ["BT_LIB"]
        result_lib = {"lib": os.environ["BT_LIB"], "BT_DRAIN_ROUNDS": os.environ.get("BT_DRAIN_ROUNDS")}
    else:
        result_lib = {}
    device = bt.Device(0)
    cfg = bt.TerrainConfig(lod_count=LOD_COUNT, atlas_size=ATLAS_SIZE, path="terrains/bench16k", model=bt.TerrainModel.planar((0.0, 0.0, 0.0), 1000.0, 0.0, 1.0))
    cfg.add_attachment(bt.AttachmentConfig(name="height", texture_size=TEXTURE_SIZE, border_size=BORDER, format=bt.AttachmentFormat.R16))
    atlas = bt.TileAtlas.new(cfg, device)
    src = device.synth_fbm_r16(SIZE, SIZE, SEED)
    bt.Preprocessor.new().clear_attachment(0, atlas).preprocess_tile(
        bt.PreprocessDataset(attachment_index=0, path="synthetic/fbm16k", lod_range=range(0, LOD_COUNT)), bt.AssetServer().insert("synthetic/fbm16k", (src, SIZE, SIZE)), atlas).run(atlas)
    x0, y0, w, h = WINDOW
    call = lambda: atlas.drainage(0, x0, y0, w, h)
    if args.trace:
        for _ in range(args.repeats):
            call()
        return
    result = {"tool": "drainage_bench", "repeats": args.repeats, "texture_size": TEXTURE_SIZE, "mosaic": MOSAIC, "window": list(WINDOW), **result_lib}
    tmp = tempfile.mkdtemp(prefix="drainage_bench_")
    try:
        analyse = host_analysis(tmp)
        raw, _ = atlas.read_region(0, x0, y0, w, h)
        host_planes = [np.zeros((h, w), t) for t in (np.uint16, np.uint32, np.uint8, np.uint32)]

        def host():
            return analyse(raw.ctypes.data, None, None, w, h, *[p.ctypes.data for p in host_planes])

        outflow = host()
        *planes, stats = call()
        for name, got, want in zip(("filled", "flat", "direction", "accumulation"), planes, host_planes):
            assert got.tobytes() == want.tobytes(), name
        assert stats["outflow"] == outflow
        wall, host_ms = [], []
        for _ in range(args.repeats):
            device.synchronize()
            t0 = time.perf_counter()
            *_, stats = call()
            wall.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            host()
            host_ms.append((time.perf_counter() - t0) * 1e3)
        result.update(stats=stats, wall_ms_median_min_max=[round(v, 3) for v in (median(wall), min(wall), max(wall))],
                      host_ms_median_min_max=[round(v, 3) for v in (median(host_ms), min(host_ms), max(host_ms))])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Times bt_atlas_path_field beside a host Dijkstra (tools/path_dijkstra.cpp: std::priority_queue, compiled here with -O3) on the same
gathered heights, and writes profiles/path.txt.  Not the headline benchmark (bench.py).

Three scenes on bench.py's 16k job (synth_fbm_r16 16384^2, T = 512, lod_count 6; finest mosaic 16256^2):
    open     a 2048 x 2048 window at an odd origin, one goal in its middle, the walking cost of examples/pathfinding.py without a grade limit
    masked   the same with a random host mask over 15 % of the cells
    maze     a 1024 x 1024 window under the serpentine maze of tests/_path_cases.py (every odd row a wall with one gap, alternately at
             either end; as a host mask): one corridor half a million cells long
Before anything is timed the device's field is asserted bit-equal to the host search's.

    python tools/path_bench.py [--repeats N] > path_bench.json                      wall ms per call of both, median; sweeps; one JSON line
    rocprofv3 --kernel-trace --output-format csv -d DIR -o path -- python tools/path_bench.py --trace [--repeats N]
        # kernel times, in a run of their own with no counters: --repeats calls per scene, nothing else
    python tools/path_bench.py --summarise DIR/.../path_kernel_trace.csv [--repeats N] > path_kernels.json
        # no GPU work: that trace per scene and kernel, median ms per call
    python tools/path_bench.py --report profiles/path.txt --json path_bench.json --kernel-json path_kernels.json [--repeats N] [--note TEXT ...]
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
SCENES = ("open", "masked", "maze")


def serpentine(n):
    wall = np.zeros((n, n), dtype=np.uint8)
    for i, y in enumerate(range(1, n, 2)):
        wall[y, :] = 1
        wall[y, n - 1 if i % 2 == 0 else 0] = 0
    return wall


def scenes():
    """name -> (x0, y0, w, h, goals, mask)"""
    big = (7003, 6997, 2048, 2048)
    mask = (np.random.default_rng(15).random((2048, 2048)) < 0.15).astype(np.uint8)
    mask[1024, 1024] = 0
    return {"open": big + ([(1024, 1024, 0.0)], None), "masked": big + ([(1024, 1024, 0.0)], mask), "maze": (5001, 9003, 1024, 1024, [(0, 0, 0.0)], serpentine(1024))}


def host_search(tmp):
    """tools/path_dijkstra.cpp compiled into a shared object -> its function"""
    so = os.path.join(tmp, "libpath_dijkstra.so")
    compiler = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    subprocess.run([compiler, "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tools", "path_dijkstra.cpp")], check=True)
    fn = C.CDLL(so).path_dijkstra
    fn.restype = C.c_uint32
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    return fn


def median(values):
    values = sorted(values)
    return values[len(values) // 2]


def summarise(path, calls):
    """a kernel trace of a --trace run -> {scene: {kernel: ms per call}}: a call's dispatches are those from its prepare launch to the next"""
    import csv
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    groups = []
    for r in rows:
        name = r["Kernel_Name"]
        if "path_prepare_kernel" in name:
            groups.append({"relax_ms": 0.0, "relax_dispatches": 0, "prepare_ms": 0.0, "next_ms": 0.0})
        if not groups:
            continue
        ms = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
        if "relax_kernel" in name and "PathRule" in name:  # relax_kernel<PathRule> of bt_relax.hpp
            groups[-1]["relax_ms"] += ms
            groups[-1]["relax_dispatches"] += 1
        elif "path_prepare_kernel" in name:
            groups[-1]["prepare_ms"] += ms
        elif "path_next_kernel" in name:
            groups[-1]["next_ms"] += ms
    assert len(groups) == calls * len(SCENES), (len(groups), calls)
    out = {}
    for i, scene in enumerate(SCENES):
        part = groups[i * calls:(i + 1) * calls]
        out[scene] = {k: round(median([g[k] for g in part]), 4) for k in part[0]}
    return out


def report(args):
    result = json.loads([line for line in open(args.json) if line.startswith("{")][-1])
    trace = summarise(args.kernel_trace, args.repeats) if args.kernel_trace else json.load(open(args.kernel_json))["kernel_ms"] if args.kernel_json else {}
    lines = ["bt_atlas_path_field (DESIGN.md 3.20) - what was measured and what was not",
             "",
             f"1 x MI355X, tools/path_bench.py, bench.py's 16k job (T = {TEXTURE_SIZE}, {LOD_COUNT} LODs, finest mosaic {MOSAIC}^2), median of {result['repeats']} calls.",
             "Wall: the synchronous call, host arrays in and out (both planes copied out).  Host search: tools/path_dijkstra.cpp",
             "(std::priority_queue, g++ -O3) on the texels bt_atlas_read_region returned, one thread, the read not counted.  The",
             "device's field was asserted bit-equal to the host search's before timing.  Kernel times: rocprofv3 --kernel-trace in",
             f"a run of its own ({args.repeats} calls per scene, no counters), median per call, the sum over a call's dispatches.",
             "",
             "scene    window       cells      reachable  sweeps  launches  wall ms (min .. max)       host Dijkstra ms   relax kernels ms  (dispatches)  prepare ms  next ms"]
    for scene in SCENES:
        r = result[scene]
        t = trace.get(scene, {})
        wall, host = r["wall_ms_median_min_max"], r["host_dijkstra_ms_median_min_max"]
        lines.append(f"{scene:8s} {r['window'][2]:4d} x {r['window'][3]:<5d} {r['stats']['cells']:9d}  {r['stats']['reachable']:9d}  {r['stats']['sweeps']:6d}  {r['stats']['launches']:8d}  "
                     f"{wall[0]:8.2f} ({wall[1]:.2f} .. {wall[2]:.2f})   {host[0]:8.2f}           "
                     f"{t.get('relax_ms', float('nan')):10.3f}  ({t.get('relax_dispatches', 0):6d})     {t.get('prepare_ms', float('nan')):8.4f}  {t.get('next_ms', float('nan')):8.4f}")
    lines += ["", "host Dijkstra / wall (above 1: the device call is faster): " +
              ", ".join(f"{s} {result[s]['host_dijkstra_ms_median_min_max'][0] / result[s]['wall_ms_median_min_max'][0]:.3g}" for s in SCENES)]
    for note in args.note or []:
        lines += [""] + note.split("\\n")
    with open(args.report, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {args.report}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--trace", action="store_true", help="no timing and no host search: --repeats calls per scene, for a kernel trace")
    ap.add_argument("--report", metavar="FILE", help="no GPU work: write the text file from --json and --kernel-trace")
    ap.add_argument("--json", metavar="FILE")
    ap.add_argument("--kernel-trace", metavar="CSV")
    ap.add_argument("--kernel-json", metavar="FILE", help="the line --summarise printed, instead of --kernel-trace")
    ap.add_argument("--summarise", metavar="CSV", help="no GPU work: the kernel trace of a --trace run with the same --repeats, per scene, as one JSON line")
    ap.add_argument("--note", action="append", help="a paragraph appended to the report")
    args = ap.parse_args()
    if args.summarise:
        print(json.dumps({"tool": "path_bench", "calls_per_scene": args.repeats, "kernel_ms": summarise(args.summarise, args.repeats)}), flush=True)
        return
    if args.report:
        return report(args)

    import bevy_terrain_amd as bt
    from bevy_terrain_amd import _ffi

    if os.environ.get("BT_LIB"):  # another build of the library, e.g. tools/libbevy_terrain_amd_dbg.so (make -C bevy_terrain_amd/csrc debug) with BT_PATH_ROUNDS set
        _ffi.LIB_PATH = os.environ["BT_LIB"]
        result_lib = {"lib": os.environ["BT_LIB"], "BT_PATH_ROUNDS": os.environ.get("BT_PATH_ROUNDS")}
    else:
        result_lib = {}
    device = bt.Device(0)
    cfg = bt.TerrainConfig(lod_count=LOD_COUNT, atlas_size=ATLAS_SIZE, path="terrains/bench16k", model=bt.TerrainModel.planar((0.0, 0.0, 0.0), 1000.0, 0.0, 1.0))
    cfg.add_attachment(bt.AttachmentConfig(name="height", texture_size=TEXTURE_SIZE, border_size=BORDER, format=bt.AttachmentFormat.R16))
    atlas = bt.TileAtlas.new(cfg, device)
    src = device.synth_fbm_r16(SIZE, SIZE, SEED)
    bt.Preprocessor.new().clear_attachment(0, atlas).preprocess_tile(
        bt.PreprocessDataset(attachment_index=0, path="synthetic/fbm16k", lod_range=range(0, LOD_COUNT)), bt.AssetServer().insert("synthetic/fbm16k", (src, SIZE, SIZE)), atlas).run(atlas)
    cost = bt.PathCost(min_height=0.0, max_height=100.0, cell_size=1000.0 / MOSAIC, grade_weight=2.0, climb_weight=3.0, descend_weight=0.5)
    result = {"tool": "path_bench", "repeats": args.repeats, "texture_size": TEXTURE_SIZE, "mosaic": MOSAIC, **result_lib}
    tmp = tempfile.mkdtemp(prefix="path_bench_")
    try:
        search = None if args.trace else host_search(tmp)
        for name, (x0, y0, w, h, goals, mask) in scenes().items():
            call = lambda: atlas.path_field(0, x0, y0, w, h, cost, goals, blocked=mask)
            if args.trace:
                for _ in range(args.repeats):
                    call()
                continue
            raw, _ = atlas.read_region(0, x0, y0, w, h)
            goal_arr = (_ffi.PathGoalC * len(goals))(*[_ffi.PathGoalC(*g) for g in goals])
            cost_c = cost._c()
            host_D = np.zeros((h, w), np.float32)

            def host():
                return search(raw.ctypes.data, mask.ctypes.data if mask is not None else None, w, h, C.addressof(cost_c), C.addressof(goal_arr), len(goals), host_D.ctypes.data)

            reachable = host()
            field, _, stats = call()
            assert field.view(np.uint32).tobytes() == host_D.view(np.uint32).tobytes() and stats["reachable"] == reachable, name
            wall, host_ms = [], []
            for _ in range(args.repeats):
                device.synchronize()
                t0 = time.perf_counter()
                _, _, stats = call()
                wall.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                host()
                host_ms.append((time.perf_counter() - t0) * 1e3)
            result[name] = {"window": [x0, y0, w, h], "stats": stats, "wall_ms_median_min_max": [round(v, 3) for v in (median(wall), min(wall), max(wall))],
                            "host_dijkstra_ms_median_min_max": [round(v, 3) for v in (median(host_ms), min(host_ms), max(host_ms))]}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()

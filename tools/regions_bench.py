#!/usr/bin/env python3
"""Times bt_atlas_label_regions beside a sequential two-pass host labeller with the same rule (tools/regions_label.cpp, compiled here with
-O3, one thread) and beside a device-to-device copy of the bytes of its planes, and writes profiles/regions.txt.  Not the headline
benchmark (bench.py).

One 2048^2 window: the whole finest mosaic of a synth_fbm_r16 terrain (T = 516, border 2, lod_count 3).  Four scenes: the texels at or
below the window's median height (sea_level: FROM_TEXELS), uniform noise at density 0.59 under 4-connectivity (noise_59: a host plane), a
one-cell-wide spiral (spiral: a host plane; about 2 M cells in one corridor, the case the union-find form is for), and a checkerboard under
4-connectivity (checkerboard: 2^21 regions of one cell).  Before anything is timed both planes, the whole table and the counts of the
device are asserted equal to the host's.

    python tools/regions_bench.py [--repeats N] > regions_bench.json                  wall ms per call of both, median; one JSON line
    rocprofv3 --kernel-trace --output-format csv -d DIR -o regions -- python tools/regions_bench.py --trace [--repeats N]
        # kernel times, in a run of their own with no counters: --repeats calls of each scene in turn, nothing else from this file's kernels
    python tools/regions_bench.py --summarise DIR/.../regions_kernel_trace.csv [--repeats N] > regions_kernels.json
        # no GPU work: that trace per scene and kernel, median ms per call
    python tools/regions_bench.py --report profiles/regions.txt --json regions_bench.json --kernel-json regions_kernels.json [--note TEXT ...]
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

SIDE, TEXTURE_SIZE, BORDER, LOD_COUNT, SEED = 2048, 516, 2, 3, 42
CASES = ["sea_level", "noise_59", "spiral", "checkerboard"]
KERNELS = ("regions_local_kernel", "regions_seam_kernel", "regions_flatten_kernel", "regions_scan_kernel", "regions_emit_kernel", "regions_finish_kernel")
REGION_DTYPE = np.dtype([("label", "<u4"), ("area", "<u4"), ("x_min", "<u2"), ("y_min", "<u2"), ("x_max", "<u2"), ("y_max", "<u2"), ("v_min", "<u2"), ("v_max", "<u2"),
                         ("edges", "<u4"), ("v_sum", "<u8")])


def host_labeller(tmp):
    """tools/regions_label.cpp compiled into a shared object -> its function"""
    so = os.path.join(tmp, "libregions_label.so")
    compiler = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    subprocess.run([compiler, "-O3", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tools", "regions_label.cpp")], check=True)
    fn = C.CDLL(so).regions_label
    fn.restype = C.c_uint32
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    return fn


def spiral(side):
    """one cell wide, one cell apart: the rings 0, 2, 4, ... from the edge inwards, each opened after its first cell and joined to the next"""
    plane = np.zeros((side, side), np.uint8)
    rings = range(0, side // 2 - 1, 2)
    for k in rings:
        a, b = k, side - 1 - k
        plane[a, a:b + 1] = plane[b, a:b + 1] = 1
        plane[a:b + 1, a] = plane[a:b + 1, b] = 1
        if k != rings[-1]:
            plane[a + 1, a] = 0      # the ring is cut below its first cell ...
            plane[a + 2, a + 1] = 1  # ... and its end turns inwards to the next ring's first cell
    return plane


def copy_ms(nbytes, repeats):
    """a device-to-device copy of nbytes, median ms"""
    import torch
    src, dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    times = []
    for _ in range(repeats + 2):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        dst.copy_(src)
        end.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(end))
    return median(times[2:])


def median(values):
    values = sorted(values)
    return values[len(values) // 2]


def summarise(path, calls):
    """a kernel trace of a --trace run -> {scene: {kernel: ms per call}}: a call's dispatches end with its finish launch"""
    import csv
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    groups, current = [], {k: 0.0 for k in KERNELS}
    for r in rows:
        name = r["Kernel_Name"]
        for k in KERNELS:
            if k in name:
                current[k] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
        if "regions_finish_kernel" in name:
            groups.append(current)
            current = {k: 0.0 for k in KERNELS}
    assert len(groups) == calls * len(CASES), (len(groups), calls)
    return {case: {k: round(median([g[k] for g in groups[i * calls:(i + 1) * calls]]), 4) for k in KERNELS} for i, case in enumerate(CASES)}


def report(args):
    result = json.loads([line for line in open(args.json) if line.startswith("{")][-1])
    trace = json.load(open(args.kernel_json))["kernel_ms"] if args.kernel_json else {}
    copy = result["copy_ms_of_the_planes"]
    lines = ["bt_atlas_label_regions - what was measured and what was not",
             "",
             f"1 x MI355X, tools/regions_bench.py, a synth_fbm_r16 terrain (T = {TEXTURE_SIZE}, {LOD_COUNT} LODs), the whole finest mosaic as a {SIDE}^2 window, median of",
             f"{result['repeats']} calls.  Wall: the synchronous call, both planes and the whole table copied out, no bake.  Host: tools/regions_label.cpp (two passes",
             "over a union-find by index, g++ -O3) on the same member plane and values, one thread, making the member plane not counted.  The",
             "device's planes, its table and its counts were asserted equal to the host's before timing.  Kernel times: rocprofv3 --kernel-trace in a",
             f"run of its own (no counters), median per call.  Floor: a device-to-device copy of the two planes' bytes ({2 * SIDE * SIDE * 4 >> 20} MiB) takes {copy:.3f} ms.",
             "",
             f"{'scene':13s} {'members':>9s} {'regions':>9s} {'largest':>9s} {'wall ms':>9s} {'host ms':>9s} {'host/wall':>9s} {'local':>8s} {'seams':>8s} {'flatten':>8s} {'scan':>8s} {'emit':>8s} {'finish':>8s} {'kernels':>8s} {'/copy':>6s}  (kernels: ms)"]
    for case in CASES:
        r, k = result["cases"][case], trace.get(case, {})
        wall, host = r["wall_ms_median_min_max"][0], r["host_ms_median_min_max"][0]
        total = sum(k.values()) if k else float("nan")
        lines.append(f"{case:13s} {r['stats']['members']:9d} {r['stats']['regions']:9d} {r['stats']['largest_area']:9d} {wall:9.2f} {host:9.1f} {host / wall:9.3g} "
                     + " ".join(f"{k.get(name, float('nan')):8.3f}" for name in KERNELS) + f" {total:8.3f} {total / copy:6.1f}")
    for note in args.note or []:
        lines += [""] + note.split("\\n")
    with open(args.report, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {args.report}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--trace", action="store_true", help="no timing and no host labeller: --repeats calls of each scene, for a kernel trace")
    ap.add_argument("--report", metavar="FILE", help="no GPU work: write the text file from --json and --kernel-json")
    ap.add_argument("--json", metavar="FILE")
    ap.add_argument("--kernel-json", metavar="FILE", help="the line --summarise printed")
    ap.add_argument("--summarise", metavar="CSV", help="no GPU work: the kernel trace of a --trace run with the same --repeats as one JSON line")
    ap.add_argument("--note", action="append", help="a paragraph appended to the report")
    args = ap.parse_args()
    if args.summarise:
        print(json.dumps({"tool": "regions_bench", "calls": args.repeats, "kernel_ms": summarise(args.summarise, args.repeats)}), flush=True)
        return
    if args.report:
        return report(args)

    import bevy_terrain_amd as bt

    device = bt.Device(0)
    tiles = (4 ** LOD_COUNT - 1) // 3
    cfg = bt.TerrainConfig(lod_count=LOD_COUNT, atlas_size=tiles, path="terrains/regions_bench", model=bt.TerrainModel.planar((0.0, 0.0, 0.0), 1000.0, 0.0, 1.0))
    cfg.add_attachment(bt.AttachmentConfig(name="height", texture_size=TEXTURE_SIZE, border_size=BORDER, format=bt.AttachmentFormat.R16))
    atlas = bt.TileAtlas.new(cfg, device)
    assert (TEXTURE_SIZE - 2 * BORDER) << (LOD_COUNT - 1) == SIDE
    src = device.synth_fbm_r16(SIDE, SIDE, SEED)
    bt.Preprocessor.new().clear_attachment(0, atlas).preprocess_tile(
        bt.PreprocessDataset(attachment_index=0, path="synthetic/fbm2k", lod_range=range(0, LOD_COUNT)), bt.AssetServer().insert("synthetic/fbm2k", (src, SIDE, SIDE)), atlas).run(atlas)
    raw, _ = atlas.read_region(0, 0, 0, SIDE, SIDE)
    level = int(np.median(raw))
    rng = np.random.default_rng(59)
    board = ((np.add.outer(np.arange(SIDE), np.arange(SIDE)) % 2) == 0).astype(np.uint8)
    # scene -> (the arguments of the call, the member plane the host is given)
    cases = {"sea_level": (dict(lo=0, hi=level), (raw <= level).astype(np.uint8)),
             "noise_59": (dict(members=(rng.random((SIDE, SIDE)) < 0.59).astype(np.uint8)), None),
             "spiral": (dict(members=spiral(SIDE)), None),
             "checkerboard": (dict(members=board), None)}
    call = lambda case, **kw: atlas.label_regions(0, 0, 0, SIDE, SIDE, **cases[case][0], **kw)
    if args.trace:
        for case in CASES:
            for _ in range(args.repeats):
                call(case)
        return
    result = {"tool": "regions_bench", "repeats": args.repeats, "texture_size": TEXTURE_SIZE, "side": SIDE, "sea_level": level, "cases": {}}
    result["copy_ms_of_the_planes"] = round(copy_ms(2 * SIDE * SIDE * 4, args.repeats), 4)
    tmp = tempfile.mkdtemp(prefix="regions_bench_")
    try:
        labeller = host_labeller(tmp)
        for case in CASES:
            kw, plane = cases[case]
            plane = np.ascontiguousarray(kw["members"] if plane is None else plane)
            host_planes = [np.zeros((SIDE, SIDE), np.uint32) for _ in range(2)]
            host_table = np.zeros(SIDE * SIDE, REGION_DTYPE)
            host = lambda: labeller(plane.ctypes.data, raw.ctypes.data, SIDE, SIDE, 65535, 0, *[p.ctypes.data for p in host_planes], host_table.ctypes.data, SIDE * SIDE)
            host_ms = []
            for _ in range(3):
                t0 = time.perf_counter()
                regions = host()
                host_ms.append((time.perf_counter() - t0) * 1e3)
            *planes, table, stats = call(case)
            for name, got, want in zip(("label", "id"), planes, host_planes):
                assert got.tobytes() == want.tobytes(), (case, name)
            assert stats["regions"] == regions == len(table) and table.tobytes() == host_table[:regions].tobytes(), (case, stats, regions)
            assert stats["members"] == int(plane.astype(bool).sum()) and stats["largest_area"] == int(host_table["area"][:regions].max())
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

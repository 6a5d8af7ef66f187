#!/usr/bin/env python3
"""Times bt_atlas_rasterize_shapes beside a sequential host rasteriser with the same rules (tools/shapes_raster.cpp, compiled here with
-O3, one thread) on the same lists, and writes profiles/shapes.txt.  Not the headline benchmark (bench.py).

One 2048^2 window: the whole finest mosaic of a synthetic R16 terrain (synth_fbm_r16 2048^2, T = 516, border 2, lod_count 3), with three
lists, all ADD so that every call writes: 64 polygons of 1024 vertices, 2048 strokes of 64 vertices at a half-width of 3 cells, and one
polygon of 2^16 vertices around the whole window, where every block walks every edge.  Before anything is timed the device's two planes,
its texels and its covered count are asserted equal to the host's.  The floor: the same call with one four-vertex polygon over the same
U (ADD 0), which is the gather and the write-back any edit of that rectangle pays, with next to no raster.

    python tools/shapes_bench.py [--repeats N] > shapes_bench.json                       wall ms per call of both, median; one JSON line
    rocprofv3 --kernel-trace --output-format csv -d DIR -o shapes -- python tools/shapes_bench.py --trace [--repeats N]
        # kernel times, in a run of their own with no counters: --repeats calls of each case in turn and of the floor
    python tools/shapes_bench.py --summarise DIR/.../shapes_kernel_trace.csv [--repeats N] > shapes_kernels.json
        # no GPU work: that trace per case, the raster kernel and the other kernels of a call (gather + write-back), median ms per call
    python tools/shapes_bench.py --report profiles/shapes.txt --json shapes_bench.json --kernel-json shapes_kernels.json [--note TEXT ...]
        # no GPU work: the two runs as the text file
"""
import argparse
import ctypes as C
import json
import math
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
CASES = ["polygons_64x1024", "strokes_2048x64", "one_polygon_65536", "floor"]


def ring(n, cx, cy, radius, wobble=0.0, lobes=7):
    return [(cx + radius * (1.0 + wobble * math.sin(lobes * 2 * math.pi * k / n)) * math.cos(2 * math.pi * k / n),
             cy + radius * (1.0 + wobble * math.sin(lobes * 2 * math.pi * k / n)) * math.sin(2 * math.pi * k / n)) for k in range(n)]


def lists():
    """case -> the shapes, floats in cells"""
    rng = np.random.default_rng(SEED)
    polygons = [dict(polygon=ring(1024, 128 + 256 * (k % 8) + 20 * math.sin(k), 128 + 256 * (k // 8) + 20 * math.cos(k), 150.0, 0.2), op="add", value=100) for k in range(64)]
    strokes = []
    for _ in range(2048):
        x, y, heading = rng.uniform(0, SIDE), rng.uniform(0, SIDE), rng.uniform(0, 2 * math.pi)
        points = []
        for _ in range(64):
            points.append((x, y))
            heading += rng.normal(0.0, 0.25)
            x, y = x + 6.0 * math.cos(heading), y + 6.0 * math.sin(heading)
        strokes.append(dict(stroke=points, half_width=3.0, op="add", value=50))
    around = [dict(polygon=ring(1 << 16, SIDE / 2, SIDE / 2, SIDE / 2 - 2.5, 0.001, 31), op="add", value=10)]
    floor = [dict(polygon=[(-1.0, -1.0), (SIDE, -1.0), (SIDE, SIDE), (-1.0, SIDE)], op="add", value=0)]
    return {"polygons_64x1024": polygons, "strokes_2048x64": strokes, "one_polygon_65536": around, "floor": floor}


def host_raster(tmp):
    """tools/shapes_raster.cpp compiled into a shared object -> its function"""
    so = os.path.join(tmp, "libshapes_raster.so")
    compiler = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    subprocess.run([compiler, "-O3", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tools", "shapes_raster.cpp")], check=True)
    fn = C.CDLL(so).shapes_raster
    fn.restype = C.c_uint64
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    return fn


def median(values):
    values = sorted(values)
    return values[len(values) // 2]


def summarise(path, calls):
    """a kernel trace of a --trace run -> {case: {"raster": ms, "gather_and_write_back": ms}} per call: a call's dispatches begin with its gather"""
    import csv
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    groups = []
    for r in rows:
        name, ms = r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
        if "edit_gather_kernel" in name:
            groups.append({"raster": 0.0, "gather_and_write_back": 0.0})
        if not groups:
            continue  # (the preprocess, before the first call)
        groups[-1]["raster" if "shapes_raster_kernel" in name else "gather_and_write_back"] += ms
    groups = [g for g in groups if g["raster"] > 0.0]
    assert len(groups) == calls * len(CASES), (len(groups), calls)
    return {case: {k: round(median([g[k] for g in groups[i * calls:(i + 1) * calls]]), 4) for k in ("raster", "gather_and_write_back")} for i, case in enumerate(CASES)}


def report(args):
    result = json.loads([line for line in open(args.json) if line.startswith("{")][-1])
    trace = json.load(open(args.kernel_json))["kernel_ms"] if args.kernel_json else {}
    lines = ["bt_atlas_rasterize_shapes - what was measured and what was not",
             "",
             f"1 x MI355X, tools/shapes_bench.py, a synthetic R16 terrain (T = {TEXTURE_SIZE}, {LOD_COUNT} LODs), the whole finest mosaic as a {SIDE}^2 window, median of",
             f"{result['repeats']} calls.  Wall: the synchronous call with both planes copied out and the write-back; dry: the same with BT_SHAPES_DRY_RUN.  Host:",
             "tools/shapes_raster.cpp (row-wise edge lists for polygons, per-segment boxes for strokes, g++ -O3) on the same list and texels, one thread.",
             "The device's planes, texels and covered count were asserted equal to the host's before timing.  Kernel times: rocprofv3 --kernel-trace",
             "in a run of its own (no counters), median per call: the raster kernel, and beside it every other kernel of the call (the gather of U and",
             "the write-back's region copy, ancestors and aprons), which is the floor any edit of that rectangle pays.  floor: one four-vertex polygon",
             "over the same U.",
             "",
             f"{'case':20s} {'vertices':>9s} {'covered':>9s} {'wall ms':>9s} {'dry ms':>9s} {'host ms':>9s} {'host/wall':>9s} {'raster':>9s} {'gather+write':>13s} {'raster/floor':>13s}  (kernels: ms)"]
    for case in CASES:
        r, k = result["cases"][case], trace.get(case, {})
        wall, dry, host = r["wall_ms_median_min_max"][0], r["dry_ms_median_min_max"][0], r["host_ms_median_min_max"][0]
        raster, rest = k.get("raster", float("nan")), k.get("gather_and_write_back", float("nan"))
        lines.append(f"{case:20s} {r['vertices']:9d} {r['stats']['covered']:9d} {wall:9.2f} {dry:9.2f} {host:9.1f} {host / wall:9.3g} {raster:9.3f} {rest:13.3f} {raster / rest:13.3g}")
    for note in args.note or []:
        lines += [""] + note.split("\\n")
    with open(args.report, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {args.report}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--trace", action="store_true", help="no timing and no host raster: --repeats calls of each case, for a kernel trace")
    ap.add_argument("--report", metavar="FILE", help="no GPU work: write the text file from --json and --kernel-json")
    ap.add_argument("--json", metavar="FILE")
    ap.add_argument("--kernel-json", metavar="FILE", help="the line --summarise printed")
    ap.add_argument("--summarise", metavar="CSV", help="no GPU work: the kernel trace of a --trace run with the same --repeats as one JSON line")
    ap.add_argument("--note", action="append", help="a paragraph appended to the report")
    args = ap.parse_args()
    if args.summarise:
        print(json.dumps({"tool": "shapes_bench", "calls": args.repeats, "kernel_ms": summarise(args.summarise, args.repeats)}), flush=True)
        return
    if args.report:
        return report(args)

    import bevy_terrain_amd as bt

    device = bt.Device(0)
    tiles = (4 ** LOD_COUNT - 1) // 3
    cfg = bt.TerrainConfig(lod_count=LOD_COUNT, atlas_size=tiles, path="terrains/shapes_bench", model=bt.TerrainModel.planar((0.0, 0.0, 0.0), 1000.0, 0.0, 1.0))
    cfg.add_attachment(bt.AttachmentConfig(name="height", texture_size=TEXTURE_SIZE, border_size=BORDER, format=bt.AttachmentFormat.R16))
    atlas = bt.TileAtlas.new(cfg, device)
    src = device.synth_fbm_r16(SIDE, SIDE, SEED)
    bt.Preprocessor.new().clear_attachment(0, atlas).preprocess_tile(
        bt.PreprocessDataset(attachment_index=0, path="synthetic/fbm2k", lod_range=range(0, LOD_COUNT)), bt.AssetServer().insert("synthetic/fbm2k", (src, SIDE, SIDE)), atlas).run(atlas)
    packed = {case: bt.TileAtlas.pack_shapes(shapes) for case, shapes in lists().items()}
    call = lambda case, **kw: atlas.rasterize_shapes(0, 0, 0, SIDE, SIDE, packed[case], **kw)
    if args.trace:
        for case in CASES:
            for _ in range(args.repeats):
                call(case, count=False, last=False)
        return
    result = {"tool": "shapes_bench", "repeats": args.repeats, "texture_size": TEXTURE_SIZE, "side": SIDE, "cases": {}}
    tmp = tempfile.mkdtemp(prefix="shapes_bench_")
    try:
        raster = host_raster(tmp)
        for case in CASES:
            vertices, entries = packed[case]
            texels, _ = atlas.read_region(0, 0, 0, SIDE, SIDE)
            host_planes = [np.zeros((SIDE, SIDE), np.uint8), np.zeros((SIDE, SIDE), np.uint16)]
            host_ms = []
            for _ in range(3):
                host_texels = texels.copy()
                t0 = time.perf_counter()
                covered = raster(vertices.ctypes.data, entries.ctypes.data, len(entries), SIDE, SIDE, host_texels.ctypes.data, 2, 0, *[p.ctypes.data for p in host_planes])
                host_ms.append((time.perf_counter() - t0) * 1e3)
            *planes, stats = call(case)
            for name, got, want in zip(("count", "last"), planes, host_planes):
                assert got.tobytes() == want.tobytes(), (case, name)
            after, _ = atlas.read_region(0, 0, 0, SIDE, SIDE)
            assert after.tobytes() == host_texels.tobytes(), (case, "texels")
            assert stats["covered"] == covered and stats["written"] == int((after != texels).sum()), (stats, covered)
            wall, dry = [], []
            for times, kw in ((wall, {}), (dry, dict(dry_run=True))):
                for _ in range(args.repeats):
                    device.synchronize()
                    t0 = time.perf_counter()
                    *_, stats = call(case, **kw)
                    times.append((time.perf_counter() - t0) * 1e3)
            stats = {k: v for k, v in stats.items() if k not in ("edit", "changed")}
            result["cases"][case] = dict(stats=stats, vertices=len(vertices), wall_ms_median_min_max=[round(v, 3) for v in (median(wall), min(wall), max(wall))],
                                         dry_ms_median_min_max=[round(v, 3) for v in (median(dry), min(dry), max(dry))],
                                         host_ms_median_min_max=[round(v, 1) for v in (median(host_ms), min(host_ms), max(host_ms))])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()

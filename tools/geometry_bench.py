#!/usr/bin/env python3
"""Times bt_tile_tree_build_geometry (the device form of the terrain geometry) on the final tile lists of refine_bench.py's scripted camera
paths at grid 16, and writes profiles/geometry.txt.  Not the headline benchmark (bench.py).

Terrains: raycast_bench.py's (planar 1000 m / 0..250 m and sphere 6371 km / -12..9 km, T = 512, 4 LODs, streamed along a short camera
path), each with a tile tree of the default view configuration (grid 16: 576 strip slots = 27648 bytes a tile).  Per path the 64 views
of refine_bench.scripted_paths(): bt_tiling_prepass_run, then bt_tile_tree_build_geometry into one buffer sized for the longest list.

    python tools/geometry_bench.py --profile [--commit HASH] [--out profiles/geometry.txt]
        starts `rocprofv3 --kernel-trace --output-format csv -- python tools/geometry_bench.py --trace` as a child (kernel tracing
        only, no counters), reads geometry_kernel's launches from its kernel trace, pairs them with the tile counts the child prints,
        and writes the table: time per launch, bytes written (tiles x 27648), rate, fraction of the HBM peak
    python tools/geometry_bench.py --trace
        the child's part alone: the launches, and one JSON line with the final tiles per launch
    --high-precision (with either): on the sphere path every view's list is also built by bt_tile_tree_build_geometry_hp (the approximation
        and the view of the same position, the default precision_threshold_distance), the same number of launches right after the plain
        ones; the table gains the hp instantiation's times beside the plain one's and the number of hp vertices of the last view
"""
import argparse
import csv
import datetime
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md (tools/workloads.py)
GRID = 16
REPEATS = 3  # launches per view: the median of them is the view's time
VERTEX_BYTES = 48


def launches(high_precision=False):
    """the child: prepass + geometry for every view of both paths, REPEATS geometry launches per view (high_precision: and REPEATS of the hp
    form on the sphere) -> the JSON line"""
    import bevy_terrain_amd as bt
    import raycast_bench as RB
    import refine_bench as RF

    device = bt.Device(0)
    result = {"tool": "geometry_bench", "grid": GRID, "repeats": REPEATS, "paths": {}}
    root = tempfile.mkdtemp(prefix="geometry_bench_")
    try:
        for (name, _, positions, _), kind in zip(RF.scripted_paths(), ("planar", "sphere")):
            model, atlas, _, _, lods = RB.build(device, kind, root)
            cfg = bt.TerrainViewConfig(tree_size=4, load_distance=1.2, grid_size=GRID)
            tree = bt.TileTree.new(atlas, cfg)
            tree.update(positions[-1])
            tree.adjust_to_tile_atlas()
            prepass = bt.TilingPrepass(device, cfg.geometry_tile_count)
            views = [bt.make_view_state(model, cfg, p) for p in positions]
            hp = high_precision and kind == "sphere"
            approximations = [bt.model_approximation_from_config(model, cfg, p) for p in positions] if hp else [None] * len(positions)
            counts = []
            for v in views:
                prepass.run(v)
                counts.append(len(prepass.read()[0]))
            slots = tree.vertices_per_tile()
            capacity = max(counts) * slots
            buffer = device.malloc(capacity * VERTEX_BYTES)
            for v, a in zip(views[:4], approximations[:4]):  # warm
                prepass.run(v)
                tree.build_geometry(prepass, 0, v, vertices=buffer, vertex_capacity=capacity)
                if hp:
                    tree.build_geometry(prepass, 0, v, vertices=buffer, vertex_capacity=capacity, approximation=a)
            device.synchronize()
            for v, a in zip(views, approximations):
                prepass.run(v)
                for _ in range(REPEATS if hp else 0):  # (first, so that the closing check below reads the plain form's vertices)
                    tree.build_geometry(prepass, 0, v, vertices=buffer, vertex_capacity=capacity, approximation=a)
                if hp and v is views[-1]:
                    device.synchronize()
                    threshold = a.precision_threshold_distance
                    hp_vertices = int((device.download(buffer, (counts[-1], slots), bt.TERRAIN_VERTEX_DTYPE)["view_distance"] < threshold).sum())
                for _ in range(REPEATS):
                    tree.build_geometry(prepass, 0, v, vertices=buffer, vertex_capacity=capacity)
                device.synchronize()
            # what the last launch wrote is the host form's answer for that list
            tiles = prepass.read()[0]
            known = tiles[:, 1] < atlas.config.lod_count
            built = device.download(buffer, (len(tiles), slots), bt.TERRAIN_VERTEX_DTYPE)
            host = tree.tile_geometry(0, tiles[known], views[-1])  # (refuses tiles below the terrain's last LOD; its tile_index counts the shorter list)
            assert known.any() and all(built[known][f].tobytes() == host[f].tobytes() for f in bt.TERRAIN_VERTEX_DTYPE.names if f != "tile_index")
            device.free(buffer)
            chunk = max(1, (32 << 20) // (slots * VERTEX_BYTES))  # the host form: one launch per 32 MiB of vertices
            result["paths"][name] = {"kind": kind, "entry_lods": lods, "tiles": counts, "slots_per_tile": slots, "warm_launches": 4,
                                     "host_launches": -(-int(known.sum()) // chunk)}
            if hp:
                result["paths"][name].update(hp=True, hp_vertices_last_view=hp_vertices, precision_threshold_distance=float(threshold))
            tree.close()
            del atlas
            device.trim()
    finally:
        shutil.rmtree(root, ignore_errors=True)
    print(json.dumps(result), flush=True)


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def profile(commit, out_path, high_precision=False):
    work = tempfile.mkdtemp(prefix="geometry_profile_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", work, "-o", "geometry", "--", sys.executable, os.path.abspath(__file__), "--trace"] + (["--high-precision"] if high_precision else [])
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
        if done.returncode != 0:
            sys.stderr.write(done.stderr[-4000:])
            raise SystemExit(done.returncode)
        line = json.loads([l for l in done.stdout.splitlines() if l.startswith("{")][-1])
        traces = glob.glob(os.path.join(work, "**", "*kernel_trace.csv"), recursive=True)
        assert len(traces) == 1, traces
        with open(traces[0], newline="") as f:
            rows = [(r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3) for r in csv.DictReader(f) if "geometry_kernel" in r["Kernel_Name"]]
        is_hp = lambda name: "geometry_kernel<true>" in name or "geometry_kernelILb1E" in name  # the kHighPrecision instantiation
        us = [t for name, t in rows if not is_hp(name)]
        hp_us = [t for name, t in rows if is_hp(name)]
    finally:
        shutil.rmtree(work, ignore_errors=True)
    if not commit:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stdout=subprocess.PIPE, text=True).stdout.strip() or "unknown"
        except OSError:
            commit = "unknown"
    lines = ["Terrain geometry: bt_tile_tree_build_geometry (geometry_kernel), 1 x MI355X, one lease",
             "========================================================================================", "",
             f"Date {datetime.date.today().isoformat()}; commit {commit}.  Tool: tools/geometry_bench.py --profile (a child under `rocprofv3 --kernel-trace`,",
             f"kernel tracing only).  Grid {GRID}: {line['paths'][next(iter(line['paths']))]['slots_per_tile']} strip slots x {VERTEX_BYTES} B a tile; {REPEATS} launches per view, the median taken;",
             "bytes = final tiles x slots x 48 (what the kernel writes; it reads 16 B a tile, the entries and at most 8 texels a vertex from L2).",
             f"Fraction: of the {HBM_PEAK_GBS / 1000:.0f} TB/s HBM peak.", ""]
    at = hp_at = 0
    for name, p in line["paths"].items():
        at += p["warm_launches"]
        rows, hp_rows = [], []
        for tiles in p["tiles"]:
            t = median(us[at:at + REPEATS])
            at += REPEATS
            rows.append((tiles, t, tiles * p["slots_per_tile"] * VERTEX_BYTES))
        if p.get("hp"):
            hp_at += p["warm_launches"]
            for tiles in p["tiles"]:
                hp_rows.append((tiles, median(hp_us[hp_at:hp_at + REPEATS]), tiles * p["slots_per_tile"] * VERTEX_BYTES))
                hp_at += REPEATS
        at += p["host_launches"]  # the closing check's
        rate = lambda r: r[2] / (r[1] * 1e-6) / 1e9  # GB/s
        total_bytes, total_us = sum(r[2] for r in rows), sum(r[1] for r in rows)
        big, small = max(rows, key=lambda r: r[0]), min(rows, key=lambda r: r[0])
        lines += [f"{name} ({p['kind']}, entry LODs {p['entry_lods']}): {len(rows)} views, final tiles {small[0]} .. {big[0]}",
                  f"  all views      {total_us:9.1f} us  {total_bytes / 1e6:9.1f} MB  {total_bytes / (total_us * 1e-6) / 1e9:7.1f} GB/s  {100.0 * total_bytes / (total_us * 1e-6) / 1e9 / HBM_PEAK_GBS:5.1f} % of peak",
                  f"  longest list   {big[1]:9.1f} us  {big[2] / 1e6:9.1f} MB  {rate(big):7.1f} GB/s  {100.0 * rate(big) / HBM_PEAK_GBS:5.1f} % of peak   ({big[0]} tiles)",
                  f"  shortest list  {small[1]:9.1f} us  {small[2] / 1e6:9.1f} MB  {rate(small):7.1f} GB/s  {100.0 * rate(small) / HBM_PEAK_GBS:5.1f} % of peak   ({small[0]} tiles)",
                  f"  median view    {median([r[1] for r in rows]):9.1f} us  ({median([r[0] for r in rows])} tiles)", ""]
        if hp_rows:
            hp_total = sum(r[1] for r in hp_rows)
            hp_big = max(hp_rows, key=lambda r: r[0])
            lines[-1:] = [f"  high precision (bt_tile_tree_build_geometry_hp, geometry_kernel<true>, threshold {p['precision_threshold_distance']:.0f} m; {p['hp_vertices_last_view']} hp vertices in the last view):",
                          f"  all views      {hp_total:9.1f} us  ({hp_total / total_us:5.2f} x the plain form on the same lists)",
                          f"  longest list   {hp_big[1]:9.1f} us  ({hp_big[1] / big[1]:5.2f} x)",
                          f"  median view    {median([r[1] for r in hp_rows]):9.1f} us", ""]
    assert at == len(us) and hp_at == len(hp_us), (at, len(us), hp_at, len(hp_us))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--high-precision", action="store_true")
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geometry.txt"))
    args = ap.parse_args()
    if args.profile:
        profile(args.commit, args.out, args.high_precision)
    else:
        launches(args.high_precision)


if __name__ == "__main__":
    main()

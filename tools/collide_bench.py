#!/usr/bin/env python3
"""Times bt_tile_tree_collide_spheres beside what a caller could do before it existed: the same 8 x 8 stencils through
bt_tile_tree_sample_attachment, one call for the feet and one per round, the ground points, the minimum and the next window taken on the
host in numpy; and writes profiles/collide.txt.  Not the headline benchmark (bench.py).  No speed-up is promised: both numbers and their
ratio are recorded.

The terrain: synth_fbm_r16 4096^2, T = 512, 4 LODs, planar 1000 wide and 100 high, every tile loaded, a tree of size 8 over it.  The
spheres: a grid of 128 x 128 (16384) of radius 2 at 0.75 radii above the ground under them, refine_rounds 2 (three rounds).  Before
anything is timed the host's distances and winners are compared with the device's (the host repeats the definition for the planar model).

    python tools/collide_bench.py [--repeats N] > collide_bench.json                 wall ms per call of both, median; one JSON line
    rocprofv3 --kernel-trace --output-format csv -d DIR -o collide -- python tools/collide_bench.py --trace [--repeats N]
        # kernel times, in a run of their own with no counters: --repeats calls of each path, nothing else
    python tools/collide_bench.py --summarise DIR/.../collide_kernel_trace.csv [--repeats N] > collide_kernels.json
    python tools/collide_bench.py --report profiles/collide.txt --json collide_bench.json --kernel-json collide_kernels.json [--note TEXT ...]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZE, TEXTURE_SIZE, BORDER, LOD_COUNT, SEED = 4096, 512, 2, 4, 42
SIDE, MAX_HEIGHT, GRID, RADIUS, ROUNDS = 1000.0, 100.0, 128, 2.0, 2
LANE = np.arange(64)
SX = (2.0 * (LANE & 7).astype(np.float64) - 7.0) / 7.0
SY = (2.0 * (LANE >> 3).astype(np.float64) - 7.0) / 7.0


def median(values):
    values = sorted(values)
    return values[len(values) // 2]


def ground(tree, q):
    """G(q) of the planar model at the origin: ((q.x / side) * side, h, (q.z / side) * side) and h, through the existing call"""
    h = tree.sample_attachment(0, q)[1]
    return np.column_stack([SIDE * (q[:, 0] / SIDE) + 0.0, (SIDE * (0.0 * (q[:, 1] / SIDE)) + 0.0) + h.astype(np.float64), SIDE * (q[:, 2] / SIDE) + 0.0]), h


def host_contacts(tree, centers, r, rounds):
    """the definition's search with bt_tile_tree_sample_attachment as its only device call: rounds + 2 calls.  Spheres above the ground
    and under the ceiling only (no status): -> distance, candidate"""
    n = len(centers)
    g0, _ = ground(tree, centers)
    d = g0 - centers
    best = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    candidate = np.zeros(n, np.uint32)
    ox, oy, w = np.zeros(n), np.zeros(n), r
    for k in range(rounds + 1):
        x, y = ox[:, None] + w * SX[None, :], oy[:, None] + w * SY[None, :]
        q = np.stack([centers[:, None, 0] + (x * 1.0 + y * 0.0), centers[:, None, 1] + (x * 0.0 + y * 0.0), centers[:, None, 2] + (x * 0.0 + y * 1.0)], axis=2)
        g, _ = ground(tree, q.reshape(-1, 3))
        d = g.reshape(n, 64, 3) - centers[:, None, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        lane = np.argmin(d2, axis=1)
        rows = np.arange(n)
        better = d2[rows, lane] < best
        best = np.where(better, d2[rows, lane], best)
        candidate = np.where(better, 64 * k + lane + 1, candidate).astype(np.uint32)
        ox, oy = np.where(better, x[rows, lane], ox), np.where(better, y[rows, lane], oy)
        w = w * (2.0 / 7.0)
    return np.sqrt(best), candidate


def summarise(path, calls):
    """a kernel trace of a --trace run -> ms per call: the collide kernel's, and the sum of the sample kernel's launches of one host search"""
    import csv
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    ms = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
    last = max(i for i, r in enumerate(rows) if "collide_kernel" in r["Kernel_Name"])
    collide = [ms(r) for r in rows if "collide_kernel" in r["Kernel_Name"]]
    sample = [ms(r) for r in rows[last + 1:] if "tile_tree_sample_kernel" in r["Kernel_Name"]]  # (the host searches run after the device calls)
    per_search = ROUNDS + 2
    assert len(collide) == calls and len(sample) == calls * per_search, (len(collide), len(sample), calls)
    return {"collide_kernel_ms": round(median(collide), 4), "sample_kernels_ms_per_search": round(median([sum(sample[i * per_search:(i + 1) * per_search]) for i in range(calls)]), 4),
            "sample_launches_per_search": per_search}


def report(args):
    result = json.loads([line for line in open(args.json) if line.startswith("{")][-1])
    kernels = json.load(open(args.kernel_json)) if args.kernel_json else {}
    wall, host = result["collide_wall_ms_median_min_max"], result["host_wall_ms_median_min_max"]
    lines = ["bt_tile_tree_collide_spheres (DESIGN.md 3.21) - what was measured and what was not",
             "",
             f"1 x MI355X, tools/collide_bench.py: {result['spheres']} spheres of radius {RADIUS:g}, refine_rounds {ROUNDS} ({ROUNDS + 1} rounds of 64 ground points each),",
             f"planar terrain {SIZE}^2 texels, T = {TEXTURE_SIZE}, {LOD_COUNT} LODs, all tiles loaded; median of {5 * result['repeats']} calls, of {result['repeats']} host searches.",
             "Wall: the synchronous call, host arrays in and out.  Host search: the same stencils through bt_tile_tree_sample_attachment,",
             f"{ROUNDS + 2} calls (the feet, then one per round), positions, ground points, minimum and next window in numpy on one thread.",
             f"Before timing: {result['equal_candidates']} of {result['spheres']} winners equal, largest distance difference {result['max_distance_difference']:.3g}.",
             "Kernel times: rocprofv3 --kernel-trace in a run of its own, no counters, median per call.",
             "",
             f"bt_tile_tree_collide_spheres   wall {wall[0]:9.3f} ms ({wall[1]:.3f} .. {wall[2]:.3f})   kernel {kernels.get('collide_kernel_ms', float('nan')):9.4f} ms (one launch)",
             f"host search over sample calls  wall {host[0]:9.3f} ms ({host[1]:.3f} .. {host[2]:.3f})   kernels {kernels.get('sample_kernels_ms_per_search', float('nan')):9.4f} ms "
             f"({kernels.get('sample_launches_per_search', ROUNDS + 2)} launches)",
             "",
             f"host search / collide call, wall: {host[0] / wall[0]:.3g}" +
             (f"; kernels: {kernels['sample_kernels_ms_per_search'] / kernels['collide_kernel_ms']:.3g}" if kernels else "")]
    for note in args.note or []:
        lines += [""] + note.split("\\n")
    with open(args.report, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {args.report}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--trace", action="store_true", help="no timing: --repeats calls of the device call, then --repeats host searches, for a kernel trace")
    ap.add_argument("--report", metavar="FILE", help="no GPU work: write the text file from --json and --kernel-json")
    ap.add_argument("--json", metavar="FILE")
    ap.add_argument("--kernel-json", metavar="FILE", help="the line --summarise printed")
    ap.add_argument("--summarise", metavar="CSV", help="no GPU work: the kernel trace of a --trace run with the same --repeats as one JSON line")
    ap.add_argument("--note", action="append", help="a paragraph appended to the report")
    args = ap.parse_args()
    if args.summarise:
        print(json.dumps(dict(tool="collide_bench", calls=args.repeats, **summarise(args.summarise, args.repeats))), flush=True)
        return
    if args.report:
        return report(args)

    import bevy_terrain_amd as bt
    from bevy_terrain_amd import _ffi

    device = bt.Device(0)
    tile_count = (4 ** LOD_COUNT - 1) // 3
    cfg = bt.TerrainConfig(lod_count=LOD_COUNT, atlas_size=tile_count, path="terrains/collide_bench", model=bt.TerrainModel.planar((0.0, 0.0, 0.0), SIDE, 0.0, MAX_HEIGHT))
    cfg.add_attachment(bt.AttachmentConfig(name="height", texture_size=TEXTURE_SIZE, border_size=BORDER, format=bt.AttachmentFormat.R16))
    atlas = bt.TileAtlas.new(cfg, device)
    src = device.synth_fbm_r16(SIZE, SIZE, SEED)
    bt.Preprocessor.new().clear_attachment(0, atlas).preprocess_tile(
        bt.PreprocessDataset(attachment_index=0, path="synthetic/fbm4k", lod_range=range(0, LOD_COUNT)), bt.AssetServer().insert("synthetic/fbm4k", (src, SIZE, SIZE)), atlas).run(atlas)
    tree = bt.TileTree.new(atlas, bt.TerrainViewConfig(tree_size=8, load_distance=1.2, blend_distance=1.0))
    tree.update((0.0, MAX_HEIGHT + 50.0, 0.0))
    tree.adjust_to_tile_atlas()

    span = np.linspace(-0.45 * SIDE, 0.45 * SIDE, GRID)
    centers = np.array([(x, 0.0, z) for z in span for x in span])
    centers[:, 1] = tree.sample_attachment(0, centers)[1].astype(np.float64) + 0.75 * RADIUS
    device_call = lambda: tree.collide_spheres(0, centers, RADIUS, refine_rounds=ROUNDS)
    host_call = lambda: host_contacts(tree, centers, RADIUS, ROUNDS)
    if args.trace:
        for _ in range(args.repeats):
            device_call()
        for _ in range(args.repeats):
            host_call()
        return
    got = device_call()
    distance, candidate = host_call()
    searched = (got["status"] == _ffi.CONTACT_TOUCHING) | (got["status"] == _ffi.CONTACT_NONE)
    assert searched.all(), np.bincount(got["status"])
    difference = float(np.abs(got["distance"] - distance).max())
    assert difference <= 1e-9, difference
    # each path in a loop of its own after a warm-up (alternated, the device call pays for the host search's 100 MB of hipMalloc / hipFree);
    # the device call is short, so it is timed five times as often
    def timed(call, warm, calls):
        for _ in range(warm):
            call()
        out = []
        for _ in range(calls):
            device.synchronize()
            t0 = time.perf_counter()
            call()
            out.append((time.perf_counter() - t0) * 1e3)
        return out

    wall, host = timed(device_call, 3, 5 * args.repeats), timed(host_call, 1, args.repeats)
    trio = lambda v: [round(x, 3) for x in (median(v), min(v), max(v))]
    print(json.dumps({"tool": "collide_bench", "repeats": args.repeats, "spheres": len(centers), "radius": RADIUS, "refine_rounds": ROUNDS,
                      "touching": int((got["status"] == _ffi.CONTACT_TOUCHING).sum()), "equal_candidates": int((got["candidate"] == candidate).sum()),
                      "max_distance_difference": difference, "collide_wall_ms_median_min_max": trio(wall), "host_wall_ms_median_min_max": trio(host)}), flush=True)


if __name__ == "__main__":
    main()

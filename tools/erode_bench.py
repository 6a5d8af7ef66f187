#!/usr/bin/env python3
"""Times bt_atlas_erode_height and writes profiles/erosion.txt.  Not the headline benchmark (bench.py).

A 2048 x 2048 window (the whole finest mosaic of a planar atlas, T = 260, b = 2, lod_count 4, preprocessed from synth_fbm_r16 2048^2) at 1,
64 and 512 steps, the parameters of the issue's prototype, no host planes (the call only enqueues; the context is synchronised).

    python tools/erode_bench.py [--repeats N] > erode_bench.json
        # wall ms per call, median; and, in the same process, a device-to-device copy of the bytes one step must move
    rocprofv3 --kernel-trace --output-format csv -d DIR -o erode -- python tools/erode_bench.py --trace
        # kernel times, in a run of their own with no counters: one call per step count, nothing else
    python tools/erode_bench.py --summarise DIR/.../erode_kernel_trace.csv > erode_kernels.json
        # no GPU work: the step kernel's dispatches of that trace
    python tools/erode_bench.py --report profiles/erosion.txt --json erode_bench.json --kernel-json erode_kernels.json [--note TEXT ...]
        # no GPU work: the two runs as the text file
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TEXTURE_SIZE, BORDER, LOD_COUNT, SEED = 260, 2, 4, 42
CENTER = TEXTURE_SIZE - 2 * BORDER
MOSAIC = CENTER << (LOD_COUNT - 1)  # 2048
STEPS = (1, 64, 512)
STEP_BYTES_PER_CELL = 7 * 4 + 7 * 4 + 1  # 7 planes read, 7 written, the activity byte


def median(values):
    values = sorted(values)
    return values[len(values) // 2]


def make_atlas(bt, device):
    model = bt.TerrainModel.planar((0.0, 0.0, 0.0), 2048.0, 0.0, 200.0)
    config = (bt.TerrainConfig(lod_count=LOD_COUNT, atlas_size=(4 ** LOD_COUNT - 1) // 3, path="terrains/erode_bench", model=model)
              .add_attachment(bt.AttachmentConfig(name="height", texture_size=TEXTURE_SIZE, border_size=BORDER, format=bt.AttachmentFormat.R16)))
    atlas = bt.TileAtlas.new(config, device)
    ptr = device.synth_fbm_r16(MOSAIC, MOSAIC, SEED)
    source = device.download(ptr, (MOSAIC, MOSAIC), np.uint16)
    device.free(ptr)
    server = bt.AssetServer().insert("height", source)
    (bt.Preprocessor.new().clear_attachment(0, atlas)
     .preprocess_tile(bt.PreprocessDataset(attachment_index=0, path="height", lod_range=range(0, LOD_COUNT)), server, atlas).run(atlas))
    return atlas


def params(bt, steps):
    return bt.ErosionParams(min_height=0.0, max_height=200.0, cell_size=1.0, dt=0.05, rain=0.5, evaporation=0.3, gravity=9.81, capacity=0.05, erode=0.3, deposit=0.3,
                            min_tilt=0.05, min_depth=0.01, steps=steps)


def copy_ms(repeats):
    """a device-to-device copy that reads and writes what one step reads and writes: 7 float planes and the byte plane, median ms"""
    import torch
    cells = MOSAIC * MOSAIC
    src = torch.zeros(cells * 29, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    times, burst = [], 20  # a burst per pair of events: one copy is tens of microseconds
    for _ in range(repeats + 3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(burst):
            dst.copy_(src)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / burst)
    return median(times[3:]), cells * 29 * 2


def bench(args):
    import bevy_terrain_amd as bt
    device = bt.Device(0)
    atlas = make_atlas(bt, device)
    if args.trace:
        for steps in STEPS:
            atlas.erode_height(0, 0, 0, MOSAIC, MOSAIC, params(bt, steps))
            device.synchronize()
        return
    wall = {}
    for steps in STEPS:
        times = []
        for _ in range(args.repeats + 1):
            device.synchronize()
            t0 = time.perf_counter()
            changed, stats, _, _ = atlas.erode_height(0, 0, 0, MOSAIC, MOSAIC, params(bt, steps))
            device.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        wall[str(steps)] = dict(wall_ms=round(median(times[1:]), 3), sim_launches=stats["sim_launches"], edit_launches=stats["edit"]["launches"], changed=len(changed))
    ms, moved = copy_ms(args.repeats)
    print(json.dumps(dict(window=[MOSAIC, MOSAIC], repeats=args.repeats, wall=wall, copy_ms=round(ms, 4), copy_bytes_moved=moved, step_bytes=MOSAIC * MOSAIC * STEP_BYTES_PER_CELL)))


def summarise(path):
    import csv
    rows = [r for r in csv.DictReader(open(path))]
    out = {}
    for kernel in ("erode_step_kernel", "erode_init_kernel", "erode_finish_kernel"):
        ms = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in rows if kernel in r["Kernel_Name"]]
        out[kernel] = dict(dispatches=len(ms), median_ms=round(median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), total_ms=round(sum(ms), 3))
    assert out["erode_step_kernel"]["dispatches"] == sum(STEPS), out
    return out


def report(args):
    result = json.loads([line for line in open(args.json) if line.startswith("{")][-1])
    kernels = json.load(open(args.kernel_json))
    step = kernels["erode_step_kernel"]
    lines = ["bt_atlas_erode_height (DESIGN.md 3.23) - what was measured and what was not",
             "",
             f"1 x MI355X, tools/erode_bench.py: a {MOSAIC} x {MOSAIC} window (the finest mosaic of a planar atlas, T = {TEXTURE_SIZE}, {LOD_COUNT} LODs, fBm heights),",
             f"the parameters of the issue's prototype, no host planes.  Wall: the call and a synchronise of the context, median of {result['repeats']} calls.",
             "Kernel times: rocprofv3 --kernel-trace in a run of its own (one call per step count, no counters).  The copy: torch's",
             "device-to-device copy of 29 bytes per cell (7 float planes and a byte plane, read and written), timed with events in",
             "the process of the wall times.  One lease, one card, its clocks as they were: the figures are not comparable across",
             "leases to better than a few per cent and say nothing about another card.",
             "",
             "steps   wall ms   per step ms   launches (simulation + write-back)"]
    for steps in STEPS:
        w = result["wall"][str(steps)]
        lines.append(f"{steps:5d} {w['wall_ms']:9.3f} {w['wall_ms'] / steps:13.4f}   {w['sim_launches']} + {w['edit_launches']}")
    lines += ["",
              f"erode_step_kernel: {step['dispatches']} dispatches, median {step['median_ms']} ms, min {step['min_ms']}, max {step['max_ms']}",
              f"erode_init_kernel: median {kernels['erode_init_kernel']['median_ms']} ms; erode_finish_kernel: median {kernels['erode_finish_kernel']['median_ms']} ms",
              f"a step moves {result['step_bytes'] / 1e6:.1f} MB (57 bytes per cell: 7 planes read, 7 written, the activity byte); the copy moves {result['copy_bytes_moved'] / 1e6:.1f} MB in "
              f"{result['copy_ms']} ms ({result['copy_bytes_moved'] / result['copy_ms'] / 1e9:.2f} TB/s)",
              f"step kernel / copy = {step['median_ms'] / result['copy_ms']:.2f}: a step takes that many copies' time; the copy is {100.0 * result['copy_ms'] / step['median_ms']:.0f} % of it",
              ""]
    lines += list(args.note or [])
    open(args.report, "w").write("\n".join(lines).rstrip("\n") + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--summarise")
    ap.add_argument("--report")
    ap.add_argument("--json")
    ap.add_argument("--kernel-json")
    ap.add_argument("--note", action="append")
    args = ap.parse_args()
    if args.summarise:
        print(json.dumps(summarise(args.summarise)))
    elif args.report:
        report(args)
    else:
        bench(args)


if __name__ == "__main__":
    main()

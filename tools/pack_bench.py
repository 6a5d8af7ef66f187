#!/usr/bin/env python3
"""Measures the packed tile format on this project's own data and writes profiles/pack.txt.  Not the headline benchmark (bench.py).

Workloads: the atlas of bench.py's 16k job (bt_synth_fbm_r16 16384^2, T = 512, b = 2, lod_count 6: 1365 R16 tiles), and the Rgba8
attachment of tools/workloads.py's config 2 twice: with its own source (uniform noise, the worst case) and with a colour ramp of the
heights (examples/_sources.py).  First every unpacked layer is asserted equal to its source.

    python tools/pack_bench.py [--repeats N] > pack_bench.json
        # ratios in total and per LOD, the width histogram, wall times of the raw and the packed save and load on one directory, and a
        # device-to-device copy of the raw bytes
    rocprofv3 --kernel-trace --output-format csv -d DIR -o pack -- python tools/pack_bench.py --trace
        # kernel times, in a run of their own with no counters: one pack and one unpack of every layer of the 16k atlas
    python tools/pack_bench.py --summarise DIR/.../pack_kernel_trace.csv > pack_kernels.json
    python tools/pack_bench.py --report profiles/pack.txt --json pack_bench.json --kernel-json pack_kernels.json [--note TEXT ...]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ("pack_measure_kernel", "pack_scan_kernel", "pack_emit_kernel", "pack_decode_kernel")


def median(values):
    values = sorted(values)
    return values[len(values) // 2]


def job16k(bt, device):
    import bench as B
    src = device.synth_fbm_r16(B.SIZE, B.SIZE, B.SEED)
    cfg = bt.TerrainConfig(lod_count=B.LOD_COUNT, atlas_size=B.ATLAS_SIZE, path="terrains/pack16k", model=bt.TerrainModel.planar((0.0, 0.0, 0.0), 1000.0, 0.0, 1.0))
    cfg.add_attachment(bt.AttachmentConfig(name="height", texture_size=B.TEXTURE_SIZE, border_size=B.BORDER, format=bt.AttachmentFormat.R16))
    atlas = bt.TileAtlas.new(cfg, device)
    server = bt.AssetServer().insert("src", (src, B.SIZE, B.SIZE))
    bt.Preprocessor.new().clear_attachment(0, atlas).preprocess_tile(bt.PreprocessDataset(attachment_index=0, path="src", lod_range=range(0, B.LOD_COUNT)), server, atlas).run(atlas)
    device.synchronize()
    device.free(src)
    return cfg, atlas


def albedo4k(bt, device, ramp):
    import _sources
    import workloads as W
    h, noise = W.config2_sources(device)
    heights = device.download(h, (4096, 4096), np.uint16)
    device.free(h)
    source = _sources.albedo_of(heights) if ramp else noise
    cfg = W.planar_cfg(4, 128, "terrains/pack4k_ramp" if ramp else "terrains/pack4k_noise", [("albedo", bt.AttachmentFormat.Rgba8)])
    atlas = bt.TileAtlas.new(cfg, device)
    server = bt.AssetServer().insert("src", np.ascontiguousarray(source))
    bt.Preprocessor.new().clear_attachment(0, atlas).preprocess_tile(bt.PreprocessDataset(attachment_index=0, path="src", lod_range=range(0, 4)), server, atlas).run(atlas)
    device.synchronize()
    return cfg, atlas


def measure(bt, device, name, cfg, atlas, repeats, directory):
    tiles = atlas.tiles()
    layers = [layer for _, layer in tiles]
    a = cfg.attachments[0]
    tile_bytes = a.texture_size * a.texture_size * a.format.pixel_size()
    data, offsets = atlas.pack_tiles(0, layers)
    twin = bt.TileAtlas.new(cfg, device)
    twin.unpack_tiles(0, layers, data, offsets)
    for first in range(0, max(layers) + 1, 64):  # every unpacked layer equals its source
        n = min(64, max(layers) + 1 - first)
        assert np.array_equal(twin.download_tiles(0, first, n), atlas.download_tiles(0, first, n)), (name, first)
    sizes = np.diff(offsets.astype(np.int64))
    per_lod = {}
    for (coord, _), size in zip(tiles, sizes):
        raw, packed, count = per_lod.get(coord.lod, (0, 0, 0))
        per_lod[coord.lod] = (raw + tile_bytes, packed + int(size), count + 1)
    bits = 16 if a.format == bt.AttachmentFormat.R16 else 8
    histogram = np.zeros(bits + 1, np.int64)
    view = np.frombuffer(data, np.uint8)
    W = (1 if bits == 16 else 4) * a.texture_size * ((a.texture_size + 63) // 64)
    for lo in offsets[:-1]:
        histogram += np.bincount(view[int(lo) + 16:int(lo) + 16 + W], minlength=bits + 1)
    # wall times on one directory: the raw and the packed save, the raw and the packed load
    where = os.path.join(directory, name)
    atlas.save_tile_config(where)
    folder = atlas.attachment_directory(where, 0)
    wall = {k: [] for k in ("save_attachment", "save_tiles_packed", "load_tiles", "load_tiles_packed", "pack_tiles", "unpack_tiles")}

    def timed(key, fn):
        device.synchronize()
        t0 = time.perf_counter()
        fn()
        device.synchronize()
        wall[key].append((time.perf_counter() - t0) * 1e3)

    loader = bt.TileAtlas.new(cfg, device)
    loader.load_tile_config(where)
    for _ in range(repeats + 1):
        timed("save_attachment", lambda: atlas.save_attachment(0, folder))
        timed("save_tiles_packed", lambda: atlas.save_tiles_packed(0, folder))
        timed("load_tiles", lambda: loader.load_tiles(0, where))
        timed("load_tiles_packed", lambda: loader.load_tiles_packed(0, folder))
        timed("pack_tiles", lambda: atlas.pack_tiles(0, layers, capacity=int(offsets[-1])))
        timed("unpack_tiles", lambda: twin.unpack_tiles(0, layers, data, offsets))
    for c, layer in tiles[::97]:
        assert np.array_equal(loader.download_tile(0, loader.get_tile(c)[1]), atlas.download_tile(0, layer)), (name, c)
    raw_total = tile_bytes * len(tiles)
    return dict(tiles=len(tiles), format=a.format.name, raw_bytes=raw_total, packed_bytes=int(offsets[-1]), ratio=round(raw_total / int(offsets[-1]), 4),
                per_lod={str(l): dict(tiles=c, raw=r, packed=p, ratio=round(r / p, 4)) for l, (r, p, c) in sorted(per_lod.items())},
                width_histogram=histogram.tolist(), wall_ms={k: round(median(v[1:]), 3) for k, v in wall.items()})


def copy_ms(nbytes, repeats):
    import torch
    src = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    times, burst = [], 10
    for _ in range(repeats + 3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(burst):
            dst.copy_(src)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / burst)
    return median(times[3:])


def bench(args):
    import bevy_terrain_amd as bt
    device = bt.Device(0)
    cfg, atlas = job16k(bt, device)
    if args.trace:
        layers = [layer for _, layer in atlas.tiles()]
        data, offsets = atlas.pack_tiles(0, layers)
        twin = bt.TileAtlas.new(cfg, device)
        twin.unpack_tiles(0, layers, data, offsets)
        device.synchronize()
        return
    import bench as B
    directory = tempfile.mkdtemp(dir=B.ram_directory())
    try:
        out = {"fbm16k_r16": measure(bt, device, "fbm16k_r16", cfg, atlas, args.repeats, directory)}
        out["copy_ms_of_raw_bytes"] = round(copy_ms(out["fbm16k_r16"]["raw_bytes"], args.repeats), 4)
        del atlas
        for name, ramp in (("config2_albedo_noise", False), ("config2_albedo_ramp", True)):
            cfg, atlas = albedo4k(bt, device, ramp)
            out[name] = measure(bt, device, name, cfg, atlas, args.repeats, directory)
            del atlas
        out["directory"] = "RAM-backed" if B.ram_directory() else "the default temporary directory"
        out["repeats"] = args.repeats
        print(json.dumps(out))
    finally:
        shutil.rmtree(directory, ignore_errors=True)


def summarise(path):
    import csv
    rows = [r for r in csv.DictReader(open(path))]
    out = {}
    for kernel in KERNELS:
        ms = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in rows if kernel in r["Kernel_Name"]]
        out[kernel] = dict(dispatches=len(ms), total_ms=round(sum(ms), 4), median_ms=round(median(ms), 4), max_ms=round(max(ms), 4))
    return out


def report(args):
    result = json.loads([line for line in open(args.json) if line.startswith("{")][-1])
    kernels = json.load(open(args.kernel_json))
    main = result["fbm16k_r16"]
    lines = ["Packed tile files (DESIGN.md 3.28) - what was measured",
             "",
             "1 x MI355X, tools/pack_bench.py.  Every unpacked layer was first asserted equal to its source.  Wall: the call and a synchronise of",
             f"the context, median of {result['repeats']} calls, all four file calls on one directory ({result['directory']}).  Kernel times: rocprofv3",
             "--kernel-trace in a run of its own (one pack and one unpack of the 16k atlas's 1365 layers, 22 chunks of 64 tiles, no counters).",
             "One lease, one card, its clocks as they were.",
             ""]
    for name in ("fbm16k_r16", "config2_albedo_noise", "config2_albedo_ramp"):
        r = result[name]
        lines.append(f"{name}: {r['tiles']} {r['format']} tiles of 512 x 512, raw {r['raw_bytes']} bytes, packed {r['packed_bytes']} bytes, ratio {r['ratio']}")
        for lod, v in r["per_lod"].items():
            lines.append(f"  lod {lod}: {v['tiles']:5d} tiles, raw {v['raw']:11d}, packed {v['packed']:11d}, ratio {v['ratio']}")
        groups = sum(r["width_histogram"])
        lines.append("  widths (share of the groups): " + ", ".join(f"{w}: {100.0 * n / groups:.1f} %" for w, n in enumerate(r["width_histogram"]) if n))
        w = r["wall_ms"]
        lines.append(f"  wall ms: save_attachment {w['save_attachment']}, save_tiles_packed {w['save_tiles_packed']}; load_tiles {w['load_tiles']}, load_tiles_packed {w['load_tiles_packed']}; "
                     f"pack_tiles {w['pack_tiles']}, unpack_tiles {w['unpack_tiles']} (host memory in and out)")
        lines.append("")
    passes = kernels["pack_emit_kernel"]["dispatches"]  # chunks; the binding's pack_tiles sizes first, so measure and scan ran twice per chunk
    encode = sum(kernels[k]["total_ms"] / kernels[k]["dispatches"] * passes for k in KERNELS[:3])
    lines.append(f"kernels, the 16k atlas ({main['raw_bytes'] / 1e6:.0f} MB raw):")
    for k in KERNELS:
        lines.append(f"  {k}: {kernels[k]['dispatches']} dispatches, total {kernels[k]['total_ms']} ms, median {kernels[k]['median_ms']}, max {kernels[k]['max_ms']}")
    copy = result["copy_ms_of_raw_bytes"]
    lines.append(f"  encode (measure + scan + emit, once per chunk) {encode:.3f} ms, decode {kernels['pack_decode_kernel']['total_ms']} ms; a device-to-device copy of the same raw bytes {copy} ms "
                 f"({2 * main['raw_bytes'] / copy / 1e9:.2f} TB/s moved): encode = {encode / copy:.1f} copies, decode = {kernels['pack_decode_kernel']['total_ms'] / copy:.1f} copies")
    lines.append("")
    lines += list(args.note or [])
    open(args.report, "w").write("\n".join(lines).rstrip("\n") + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
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

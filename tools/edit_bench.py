#!/usr/bin/env python3
"""Times bt_atlas_edit_height on bench.py's 16k job (synth_fbm_r16 16384^2, T = 512, lod_count 6, 1365 tiles); prints one JSON line.  Not the
headline benchmark (bench.py).

Per case (one SMOOTH ADD stamp of radius 4 / 32 / 256 / 2048 texels across a four-tile corner of the finest LOD, and 64 stamps of radius
32): device time per call from a device-event pair around `--calls` back-to-back calls (no synchronise in between; the plan ring of the
context serves the calls in flight) after a spin-up of the same calls, the median of `--repeats` such windows (and the windows themselves, `*_windows`); `launches` and
`changed_count` of the call; host time per call (the planning + enqueue, a host clock around the same window ended by a synchronise).
Successive calls of a window use the same stamps: the texels saturate after some calls, the work does not change.

Then the smoothing brush (bt_atlas_smooth_height): one SMOOTH stamp of strength 0.5 at the same corner and radii, kernel_radius 1 and 2, the
same windows (rows `smooth_r{radius}_k{kernel_radius}`; the ADD rows above are their yardstick, taken in the same run), and what a host
would do for the same tile set without the call: download the changed tiles, (filter on the host: left out), bt_atlas_write_region of the
stamp's box (wall time, `download_write_region_wall_ms`, with its two legs).

Next to them what a host can do without the call: (a) re-running the kept preprocess queue (bench.py's headline step) and (b) a
download_tiles / upload_tile round trip of the same changed tile set, the host patching left out (wall time, it is synchronous).

    python tools/edit_bench.py [--calls N] [--repeats N]

--bounds: instead of the above, what keeping a 6-level bt_height_bounds table current costs after a stamp of radius 32 and of radius 2048:
per call the stamp alone, stamp + bt_height_bounds_update(changed) and stamp + bt_height_bounds_build, each as device time (the event pair
around the window; the build synchronises inside, so its window holds its host work too) and as wall time of the window ended by a
synchronise; the update's stats.

--paint: instead of the above, a 16k-class Rgba8 job (the same tiling: T = 512, lod_count 6, 1365 tiles, from a 4096^2 random source) and on
it, for a radius-32 and a radius-2048 stamp at the same corner: bt_atlas_paint per call (rows `paint_r{radius}`) beside bt_atlas_write_region
of the stamp's box with the texels bt_atlas_read_region returned (rows `write_region_r{radius}`; the same plan; a tenth of the calls for the
large box), their ratio, and bt_atlas_read_region of a 4096^2 rectangle beside bt_atlas_download_tiles of the layers it covers (wall time,
both are synchronous; row `read_region_4096`).

--splat: instead of the above, the 16k height job with a second, Rgba8 attachment of the same tiling and on it bt_atlas_splat_from_height: a
whole-face derive in both modes (rows `splat_face_colour`, eight rules, and `splat_face_weights`, four; a tenth of the calls per window; with
the bytes of heights read plus target texels written over the call's time, `GB_per_s`) and a box of the radius-32 stamp's footprint (row
`splat_box`); beside them, in the same process, bt_atlas_paint with a stamp of the same footprint (`paint_face`, `paint_box`: the same plan
behind another first step) and the host loop the call replaces: bt_atlas_read_region of the heights, bt_atlas_tile_normals of the tiles, the
rules in numpy, bt_atlas_write_region of the result (wall time with its legs, `host_loop_box` and `host_loop_2048` for a 2048^2 box).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bevy_terrain_amd as bt

SIZE, TEXTURE_SIZE, BORDER, LOD_COUNT, ATLAS_SIZE, SEED = 16384, 512, 2, 6, 2048, 42  # bench.py's 16k job
CENTER = TEXTURE_SIZE - 2 * BORDER


def cases():
    corner = (16 * CENTER + 0.25, 16 * CENTER - 0.5)  # where four finest tiles meet, mid-terrain
    out = {f"r{r}": [bt.EditStamp(corner, float(r), 0.01)] for r in (4, 32, 256, 2048)}
    out["64_stamps_r32"] = [bt.EditStamp((corner[0] + 97.0 * (k % 8) - 340.0, corner[1] + 97.0 * (k // 8) - 340.0), 32.0, 0.01) for k in range(64)]
    return out


def median(values):
    values = sorted(values)
    return values[len(values) // 2]


def bounds_mode(device, atlas, args, result):
    """stamp, stamp + update, stamp + build: the same windows as the edit cases, the build's with a tenth of the calls (it is synchronous).
    The calls go to the C entry points with arrays made once, as a renderer's would: `changed` passes from the edit to the update as it is."""
    import ctypes as C

    from bevy_terrain_amd import _ffi

    L = _ffi.lib()
    hb = bt.HeightBounds(device, 1, LOD_COUNT).build(atlas, 0)
    cap = atlas.atlas_size
    changed = (_ffi.TileCoordinateC * cap)()
    edit_stats, update_stats = _ffi.EditStatsC(), _ffi.BoundsUpdateStatsC()
    all_cases = cases()
    for name in ("r32", "r2048"):
        stamps = (_ffi.EditStampC * len(all_cases[name]))(*[s._c() for s in all_cases[name]])

        def stamp():
            _ffi.check(L.bt_atlas_edit_height(atlas._h, 0, LOD_COUNT - 1, stamps, len(stamps), changed, cap, C.byref(edit_stats)))

        def stamp_update():
            stamp()
            _ffi.check(L.bt_height_bounds_update(hb._h, atlas._h, 0, changed, edit_stats.changed_count, C.byref(update_stats)))

        def stamp_build():
            stamp()
            _ffi.check(L.bt_height_bounds_build(hb._h, atlas._h, 0))

        stamp_update()
        row = {"changed_count": edit_stats.changed_count,
               "update_stats": {field: getattr(update_stats, field) for field, _ in _ffi.BoundsUpdateStatsC._fields_ if field != "_pad"}}
        for label, call, calls in (("stamp", stamp, args.calls), ("stamp_update", stamp_update, args.calls), ("stamp_build", stamp_build, max(args.calls // 10, 1))):
            for _ in range(max(calls // 4, 1)):
                call()
            device_ms, host_ms, wall_ms = [], [], []
            for _ in range(args.repeats):
                device.synchronize()
                t0 = time.perf_counter()
                device.timer_begin()
                for _ in range(calls):
                    call()
                host_ms.append((time.perf_counter() - t0) * 1e3 / calls)  # planning + enqueue (the build: everything, it synchronises)
                device_ms.append(device.timer_end() / calls)
                wall_ms.append((time.perf_counter() - t0) * 1e3 / calls)  # timer_end has waited for the window
            row[label] = {"device_ms_per_call": round(median(device_ms), 4), "host_ms_per_call": round(median(host_ms), 4),
                          "wall_ms_per_call": round(median(wall_ms), 4), "calls_per_window": calls}
        result[name] = row
    hb.close()


def window(device, call, calls, repeats):
    """(device ms per call, host ms per call, the device windows): an event pair around `calls` back-to-back calls after a spin-up"""
    for _ in range(max(calls // 4, 1)):
        call()
    device_ms, host_ms = [], []
    for _ in range(repeats):
        device.synchronize()
        t0 = time.perf_counter()
        device.timer_begin()
        for _ in range(calls):
            call()
        host_ms.append((time.perf_counter() - t0) * 1e3 / calls)
        device_ms.append(device.timer_end() / calls)
    return median(device_ms), median(host_ms), [round(v, 4) for v in device_ms]


def paint_mode(device, args, result):
    import numpy as np

    cfg = bt.TerrainConfig(lod_count=LOD_COUNT, atlas_size=ATLAS_SIZE, path="terrains/bench16k_albedo",
                           model=bt.TerrainModel.planar((0.0, 0.0, 0.0), 1000.0, 0.0, 1.0))
    cfg.add_attachment(bt.AttachmentConfig(name="albedo", texture_size=TEXTURE_SIZE, border_size=BORDER, format=bt.AttachmentFormat.Rgba8))
    atlas = bt.TileAtlas.new(cfg, device)
    src = np.random.default_rng(SEED).integers(0, 256, size=(4096, 4096, 4), dtype=np.uint8)
    src[..., 0] |= 1
    pre = bt.Preprocessor.new().clear_attachment(0, atlas).preprocess_tile(
        bt.PreprocessDataset(attachment_index=0, path="albedo", lod_range=range(0, LOD_COUNT)), bt.AssetServer().insert("albedo", src), atlas)
    pre.run(atlas)
    index = {c: i for c, i in atlas.tiles()}
    assert len(index) == 1365, len(index)
    result["tiles"] = len(index)
    corner = (16 * CENTER + 0.25, 16 * CENTER - 0.5)
    size = CENTER << (LOD_COUNT - 1)
    for r in (32, 2048):
        stamps = [bt.PaintStamp(corner, float(r), (0.8, 0.3, 0.2, 1.0), opacity=0.05)]
        changed, stats = atlas.paint(0, stamps)
        device_ms, host_ms, windows = window(device, lambda: atlas.paint(0, stamps), args.calls, args.repeats)
        result[f"paint_r{r}"] = {"device_ms_per_call": round(device_ms, 4), "host_ms_per_call": round(host_ms, 4), "device_ms_windows": windows,
                                 "launches": stats["launches"], "changed_count": stats["changed_count"], "tiles_edited": stats["tiles_edited"]}
        lo = [max(0, int(np.floor(corner[i] - r))) for i in range(2)]
        hi = [min(size - 1, int(np.ceil(corner[i] + r))) for i in range(2)]
        w, h = hi[0] - lo[0] + 1, hi[1] - lo[1] + 1
        region, missing = atlas.read_region(0, lo[0], lo[1], w, h)
        assert missing == 0
        calls = args.calls if r == 32 else max(args.calls // 10, 5)
        changed, stats = atlas.write_region(0, region, lo[0], lo[1])
        region_ms, region_host_ms, windows = window(device, lambda: atlas.write_region(0, region, lo[0], lo[1]), calls, args.repeats)
        result[f"write_region_r{r}"] = {"device_ms_per_call": round(region_ms, 4), "host_ms_per_call": round(region_host_ms, 4), "device_ms_windows": windows,
                                        "box": [w, h], "calls_per_window": calls, "launches": stats["launches"], "changed_count": stats["changed_count"]}
        result[f"paint_over_write_region_r{r}"] = round(device_ms / region_ms, 3)
    # read-back: a 4096^2 rectangle against the whole layers it covers
    x0, y0, n = int(corner[0]) - 2048, int(corner[1]) - 2048, 4096
    layers = sorted(index[c] for c in index if c.lod == LOD_COUNT - 1 and x0 // CENTER <= c.x <= (x0 + n - 1) // CENTER and y0 // CENTER <= c.y <= (y0 + n - 1) // CENTER)
    # the C entry points into buffers made and touched once, as an editor's would be: no allocation, no page faults inside the windows
    import ctypes as C

    from bevy_terrain_amd import _ffi

    L = _ffi.lib()
    rect = np.zeros((n, n, 4), np.uint8)
    tiles = np.zeros((len(layers), TEXTURE_SIZE, TEXTURE_SIZE, 4), np.uint8)
    rect.fill(1), tiles.fill(1)

    def read():
        _ffi.check(L.bt_atlas_read_region(atlas._h, 0, 0, LOD_COUNT - 1, x0, y0, n, n, rect.ctypes.data_as(C.c_void_p), 0, None))

    def download():
        for k, i in enumerate(layers):
            _ffi.check(L.bt_atlas_download_tiles(atlas._h, 0, i, 1, tiles[k].ctypes.data_as(C.c_void_p), tiles[k].nbytes))

    read(), download()
    read_ms, download_ms = [], []
    for _ in range(args.repeats):
        device.synchronize()
        t0 = time.perf_counter()
        read()
        t1 = time.perf_counter()
        download()
        read_ms.append((t1 - t0) * 1e3)
        download_ms.append((time.perf_counter() - t1) * 1e3)
    first = layers.index(next(i for c, i in index.items() if (c.lod, c.x, c.y) == (LOD_COUNT - 1, x0 // CENTER, y0 // CENTER)))  # the rectangle's top-left tile
    assert np.array_equal(rect[:CENTER - y0 % CENTER, :CENTER - x0 % CENTER], tiles[first][BORDER + y0 % CENTER:BORDER + CENTER, BORDER + x0 % CENTER:BORDER + CENTER])
    rect_bytes, layer_bytes = rect.nbytes, tiles.nbytes
    result["read_region_4096"] = {"wall_ms": round(median(read_ms), 3), "GB_per_s": round(rect_bytes / median(read_ms) / 1e6, 2), "bytes": rect_bytes,
                                  "wall_ms_windows": [round(v, 3) for v in read_ms],
                                  "download_tiles_wall_ms": round(median(download_ms), 3), "download_tiles_GB_per_s": round(layer_bytes / median(download_ms) / 1e6, 2),
                                  "download_tiles_bytes": layer_bytes, "layers": len(layers),
                                  "note": "wall time of the C calls (both synchronous) into buffers allocated and touched beforehand"}
    pre.close()


def splat_mode(device, args, result):
    import math

    import numpy as np

    F = np.float32
    cfg = bt.TerrainConfig(lod_count=LOD_COUNT, atlas_size=ATLAS_SIZE, path="terrains/bench16k_splat",
                           model=bt.TerrainModel.planar((0.0, 0.0, 0.0), 1000.0, -50.0, 450.0))
    cfg.add_attachment(bt.AttachmentConfig(name="height", texture_size=TEXTURE_SIZE, border_size=BORDER, format=bt.AttachmentFormat.R16))
    cfg.add_attachment(bt.AttachmentConfig(name="albedo", texture_size=TEXTURE_SIZE, border_size=BORDER, format=bt.AttachmentFormat.Rgba8))
    atlas = bt.TileAtlas.new(cfg, device)
    src = device.synth_fbm_r16(SIZE, SIZE, SEED)
    pre = bt.Preprocessor.new().clear_attachment(0, atlas).preprocess_tile(
        bt.PreprocessDataset(attachment_index=0, path="synthetic/fbm16k", lod_range=range(0, LOD_COUNT)),
        bt.AssetServer().insert("synthetic/fbm16k", (src, SIZE, SIZE)), atlas)
    pre.run(atlas)
    index = {c: i for c, i in atlas.tiles()}
    assert len(index) == 1365, len(index)
    result["tiles"] = len(index)
    R, inf = bt.SplatRule, math.inf
    colour = [R(height=(-inf, 110.0), height_fade=20.0, colour=(0.1, 0.3, 0.7)), R(height=(110.0, 140.0), height_fade=15.0, colour=(0.8, 0.75, 0.5)),
              R(height=(140.0, 230.0), height_fade=30.0, slope=(0.0, 30.0), slope_fade=0.05, colour=(0.3, 0.6, 0.2)),
              R(height=(180.0, 260.0), height_fade=30.0, slope=(10.0, 40.0), slope_fade=0.05, colour=(0.1, 0.4, 0.15), weight=0.75),
              R(height=(230.0, 330.0), height_fade=30.0, colour=(0.5, 0.45, 0.4)), R(slope=(40.0, 90.0), slope_fade=0.1, colour=(0.35, 0.3, 0.3), weight=4.0),
              R(height=(300.0, inf), height_fade=25.0, slope=(0.0, 50.0), slope_fade=0.1, colour=(1.0, 1.0, 1.0), weight=2.0),
              R(height=(200.0, 210.0), height_fade=5.0, colour=(0.6, 0.5, 0.3), weight=0.25)]
    weights = colour[:4]
    size = CENTER << (LOD_COUNT - 1)
    corner = (16 * CENTER + 0.25, 16 * CENTER - 0.5)
    lo = [max(0, int(np.floor(corner[i] - 32.0))) for i in range(2)]
    hi = [min(size - 1, int(np.ceil(corner[i] + 32.0))) for i in range(2)]
    box = (lo[0], lo[1], hi[0] - lo[0] + 1, hi[1] - lo[1] + 1)
    few = max(args.calls // 10, 5)

    def row(call, calls, stats, **more):
        device_ms, host_ms, windows = window(device, call, calls, args.repeats)
        return dict({"device_ms_per_call": round(device_ms, 4), "host_ms_per_call": round(host_ms, 4), "device_ms_windows": windows, "calls_per_window": calls,
                     "launches": stats["launches"], "changed_count": stats["changed_count"], "tiles_edited": stats["tiles_edited"]}, **more)

    for name, mode, rules in (("splat_face_colour", "colour", colour), ("splat_face_weights", "weights", weights)):
        changed, stats = atlas.splat_from_height(0, 1, rules, mode=mode)
        r = row(lambda: atlas.splat_from_height(0, 1, rules, mode=mode), few, stats, rules=len(rules))
        r["bytes_heights_read_plus_target_written"] = size * size * 6
        r["GB_per_s"] = round(size * size * 6 / r["device_ms_per_call"] / 1e6, 1)
        result[name] = r
    changed, stats = atlas.splat_from_height(0, 1, colour, mode="colour", rect=box)
    result["splat_box"] = row(lambda: atlas.splat_from_height(0, 1, colour, mode="colour", rect=box), args.calls, stats, box=list(box[2:]), rules=len(colour))
    # the paint brush on the same footprints: the same plan behind another first step
    for name, stamp, calls in (("paint_face", bt.PaintStamp((size / 2.0, size / 2.0), 2.0 * size, (0.8, 0.3, 0.2, 1.0), opacity=0.05, falloff="hard"), few),
                               ("paint_box", bt.PaintStamp(corner, 32.0, (0.8, 0.3, 0.2, 1.0), opacity=0.05), args.calls)):
        changed, stats = atlas.paint(1, [stamp])
        result[name] = row(lambda: atlas.paint(1, [stamp]), calls, stats)
    result["splat_over_paint_face"] = round(result["splat_face_colour"]["device_ms_per_call"] / result["paint_face"]["device_ms_per_call"], 3)
    result["splat_over_paint_box"] = round(result["splat_box"]["device_ms_per_call"] / result["paint_box"]["device_ms_per_call"], 3)

    # the host loop the call replaces
    def band(x, lo_, hi_, fade):
        if fade > 0:
            r_, q_ = np.clip((x - F(lo_ - fade)) / F(fade), 0, 1), np.clip((F(hi_ + fade) - x) / F(fade), 0, 1)
        else:
            r_, q_ = (x >= lo_).astype(F), (x <= hi_).astype(F)
        return (r_ * r_ * (F(3) - F(2) * r_)) * (q_ * q_ * (F(3) - F(2) * q_))

    def host_loop(x0, y0, w, h):
        t0 = time.perf_counter()
        heights, missing = atlas.read_region(0, x0, y0, w, h)
        t1 = time.perf_counter()
        tiles = [c for c in index if c.lod == LOD_COUNT - 1 and x0 // CENTER <= c.x <= (x0 + w - 1) // CENTER and y0 // CENTER <= c.y <= (y0 + h - 1) // CENTER]
        normals = atlas.tile_normals(0, tiles)
        t2 = time.perf_counter()
        steep = np.zeros((h, w), F)
        for c, n in zip(tiles, normals):
            ox, oy = c.x * CENTER, c.y * CENTER
            xa, xb, ya, yb = max(x0, ox), min(x0 + w, ox + CENTER), max(y0, oy), min(y0 + h, oy + CENTER)
            steep[ya - y0:yb - y0, xa - x0:xb - x0] = F(1) - (n[ya - oy:yb - oy, xa - ox:xb - ox, 2].astype(F) * F(2.0 / 255.0) - F(1))
        world = F(-50.0) + F(500.0) * (heights.astype(F) / F(65535.0))
        total, acc = np.zeros((h, w), F), np.zeros((h, w, 3), F)
        for rule in colour:
            s_lo, s_hi = rule.steep()
            wk = F(rule.weight) * band(world, rule.height[0], rule.height[1], rule.height_fade) * band(steep, s_lo, s_hi, rule.slope_fade)
            total += wk
            acc += wk[..., None] * np.array(rule.colour, F)
        out = np.zeros((h, w, 4), np.uint8)
        with np.errstate(invalid="ignore", divide="ignore"):
            out[..., :3] = np.floor(F(0.5) + F(255) * np.clip(acc / total[..., None], 0, 1))
        out[..., 3] = 255
        out[total <= 0] = (0, 0, 0, 255)
        out[..., 0] |= (out[..., :3] == 0).all(axis=-1).astype(np.uint8)
        out[heights == 0] = 0
        t3 = time.perf_counter()
        atlas.write_region(1, out, x0, y0)
        device.synchronize()
        t4 = time.perf_counter()
        return [(t4 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t4 - t3) * 1e3]

    for name, rect, repeats in (("host_loop_box", box, args.repeats), ("host_loop_2048", (int(corner[0]) - 1024, int(corner[1]) - 1024, 2048, 2048), 2)):
        host_loop(*rect)
        legs = [host_loop(*rect) for _ in range(repeats)]
        total, read, normals, rules_ms, write = (round(median([leg[i] for leg in legs]), 3) for i in range(5))
        result[name] = {"wall_ms": total, "read_region_ms": read, "tile_normals_ms": normals, "numpy_rules_ms": rules_ms, "write_region_ms": write, "box": list(rect[2:])}
    pre.close()
    device.free(src)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--bounds", action="store_true", help="time stamp + bt_height_bounds_update and stamp + bt_height_bounds_build")
    ap.add_argument("--paint", action="store_true", help="time bt_atlas_paint beside bt_atlas_write_region, and bt_atlas_read_region, on an Rgba8 job")
    ap.add_argument("--splat", action="store_true", help="time bt_atlas_splat_from_height beside bt_atlas_paint and the host loop it replaces")
    args = ap.parse_args()
    device = bt.Device(0)
    if args.splat:
        result = {"tool": "edit_bench --splat", "texture_size": TEXTURE_SIZE, "lod_count": LOD_COUNT, "calls_per_window": args.calls, "windows": args.repeats,
                  "note": "device ms per call: event pair around back-to-back calls, median of the windows; host loops: wall time"}
        splat_mode(device, args, result)
        print(json.dumps(result), flush=True)
        return
    if args.paint:
        result = {"tool": "edit_bench --paint", "texture_size": TEXTURE_SIZE, "lod_count": LOD_COUNT, "calls_per_window": args.calls, "windows": args.repeats,
                  "note": "device ms per call: event pair around back-to-back calls, median of the windows"}
        paint_mode(device, args, result)
        print(json.dumps(result), flush=True)
        return
    cfg = bt.TerrainConfig(lod_count=LOD_COUNT, atlas_size=ATLAS_SIZE, path="terrains/bench16k",
                           model=bt.TerrainModel.planar((0.0, 0.0, 0.0), 1000.0, 0.0, 1.0))
    cfg.add_attachment(bt.AttachmentConfig(name="height", texture_size=TEXTURE_SIZE, border_size=BORDER, format=bt.AttachmentFormat.R16))
    atlas = bt.TileAtlas.new(cfg, device)
    src = device.synth_fbm_r16(SIZE, SIZE, SEED)
    pre = bt.Preprocessor.new().clear_attachment(0, atlas).preprocess_tile(
        bt.PreprocessDataset(attachment_index=0, path="synthetic/fbm16k", lod_range=range(0, LOD_COUNT)),
        bt.AssetServer().insert("synthetic/fbm16k", (src, SIZE, SIZE)), atlas)
    pre.run(atlas, keep_queue=True)
    index = {c: i for c, i in atlas.tiles()}
    assert len(index) == 1365, len(index)
    result = {"tool": "edit_bench", "tiles": len(index), "texture_size": TEXTURE_SIZE, "lod_count": LOD_COUNT, "calls_per_window": args.calls,
              "windows": args.repeats, "note": "device ms per call: event pair around back-to-back calls, median of the windows"}

    if args.bounds:
        bounds_mode(device, atlas, args, result)
        print(json.dumps(result), flush=True)
        pre.close()
        device.free(src)
        return

    # (a) the kept queue again: the whole terrain, whatever the footprint
    for _ in range(3):
        pre.run(atlas, keep_queue=True)
    windows = []
    for _ in range(args.repeats):
        device.synchronize()
        device.timer_begin()
        for _ in range(20):
            pre.run(atlas, keep_queue=True, sync=False)
        windows.append(device.timer_end() / 20)
    result["rerun_kept_queue_device_ms"] = round(median(windows), 4)

    for name, stamps in cases().items():
        changed, stats = atlas.edit_height(0, stamps)
        for _ in range(args.calls // 4):  # spin-up: code objects, scratch growth, clocks
            atlas.edit_height(0, stamps)
        device_ms, host_ms = [], []
        for _ in range(args.repeats):
            device.synchronize()
            t0 = time.perf_counter()
            device.timer_begin()
            for _ in range(args.calls):
                atlas.edit_height(0, stamps)
            host_ms.append((time.perf_counter() - t0) * 1e3 / args.calls)  # planning + enqueue: nothing has been waited for yet
            device_ms.append(device.timer_end() / args.calls)
        # (b) the same tile set by hand: download, (patch on the host), upload — synchronous calls
        layers = [index[c] for c in changed]
        tiles = [atlas.download_tile(0, i) for i in layers]
        round_trip = []
        for _ in range(args.repeats):
            device.synchronize()
            t0 = time.perf_counter()
            tiles = [atlas.download_tile(0, i) for i in layers]
            for i, t in zip(layers, tiles):
                atlas.upload_tile(0, i, t)
            round_trip.append((time.perf_counter() - t0) * 1e3)
        result[name] = {"stamps": len(stamps), "device_ms_per_call": round(median(device_ms), 4), "host_ms_per_call": round(median(host_ms), 4),
                        "device_ms_windows": [round(v, 4) for v in device_ms], "host_ms_windows": [round(v, 4) for v in host_ms],
                        "launches": stats["launches"], "changed_count": stats["changed_count"], "tiles_edited": stats["tiles_edited"],
                        "download_upload_round_trip_wall_ms": round(median(round_trip), 3)}
    smooth_cases(device, atlas, index, args, result)
    print(json.dumps(result), flush=True)
    pre.close()
    device.free(src)


def smooth_cases(device, atlas, index, args, result):
    import numpy as np

    corner = (16 * CENTER + 0.25, 16 * CENTER - 0.5)
    size = CENTER << (LOD_COUNT - 1)
    for r in (4, 32, 256, 2048):
        stamps = [bt.SmoothStamp(corner, float(r), 0.5)]
        for k in (1, 2):
            changed, stats = atlas.smooth_height(0, stamps, k)
            for _ in range(args.calls // 4):
                atlas.smooth_height(0, stamps, k)
            device_ms, host_ms = [], []
            for _ in range(args.repeats):
                device.synchronize()
                t0 = time.perf_counter()
                device.timer_begin()
                for _ in range(args.calls):
                    atlas.smooth_height(0, stamps, k)
                host_ms.append((time.perf_counter() - t0) * 1e3 / args.calls)
                device_ms.append(device.timer_end() / args.calls)
            result[f"smooth_r{r}_k{k}"] = {"device_ms_per_call": round(median(device_ms), 4), "host_ms_per_call": round(median(host_ms), 4),
                                           "device_ms_windows": [round(v, 4) for v in device_ms], "host_ms_windows": [round(v, 4) for v in host_ms],
                                           "launches": stats["launches"], "changed_count": stats["changed_count"], "tiles_edited": stats["tiles_edited"]}
        # the same tile set by hand: download the changed tiles, (filter), write the stamp's box back through write_region
        lo = [max(0, int(np.floor(corner[i] - r))) for i in range(2)]
        hi = [min(size - 1, int(np.ceil(corner[i] + r))) for i in range(2)]
        layers = [index[c] for c in changed]
        region = np.zeros((hi[1] - lo[1] + 1, hi[0] - lo[0] + 1), np.uint16)
        for c in changed:  # the box's texels as they stand, from the finest tiles' centres: the round trip leaves the terrain as it is
            if c.lod != LOD_COUNT - 1:
                continue
            ox, oy = c.x * CENTER, c.y * CENTER
            xa, xb, ya, yb = max(lo[0], ox), min(hi[0] + 1, ox + CENTER), max(lo[1], oy), min(hi[1] + 1, oy + CENTER)
            if xa < xb and ya < yb:
                tile = atlas.download_tile(0, index[c])
                region[ya - lo[1]:yb - lo[1], xa - lo[0]:xb - lo[0]] = tile[BORDER + ya - oy:BORDER + yb - oy, BORDER + xa - ox:BORDER + xb - ox]
        legs = []
        for _ in range(args.repeats):
            device.synchronize()
            t0 = time.perf_counter()
            for i in layers:
                atlas.download_tile(0, i)
            t1 = time.perf_counter()
            atlas.write_region(0, region, lo[0], lo[1])
            device.synchronize()
            legs.append(((time.perf_counter() - t0) * 1e3, (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3))
        total, down, up = (round(median([leg[i] for leg in legs]), 3) for i in range(3))
        result[f"smooth_r{r}_by_hand"] = {"download_write_region_wall_ms": total, "download_ms": down, "write_region_ms": up, "tiles": len(layers)}


if __name__ == "__main__":
    main()

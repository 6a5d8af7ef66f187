"""Shared builders: run the same preprocess job through the product (HIP, via the mirrored reference
API) and through the oracle, and compare every tile byte for byte."""
import numpy as np

import _oracle as O
import bevy_terrain_amd as bt

FMT = {O.FORMAT_R16: bt.AttachmentFormat.R16, O.FORMAT_RGBA8: bt.AttachmentFormat.Rgba8}


def variant_bits():
    """BT_VARIANT_* of include/bevy_terrain_amd.h, parsed from the text: {name without the prefix: bit} (bt_run_stats.variants)"""
    import re

    from bevy_terrain_amd import _ffi

    text = open(_ffi.HEADER_PATH).read()
    return {m.group(1): int(m.group(2), 0) for m in re.finditer(r"\bBT_VARIANT_([A-Z0-9_]+)\s*=\s*(0x[0-9a-fA-F]+|\d+)u?", text)}


def variants(stats):
    """the names of the variants a run launched, from Preprocessor.stats()"""
    return {name for name, bit in variant_bits().items() if stats["variants"] & bit}


def random_raster(fmt, h, w, seed, holes=0.0):
    rng = np.random.default_rng(seed)
    if fmt == O.FORMAT_R16:
        src = rng.integers(1, 65536, size=(h, w), dtype=np.uint16)
        if holes:
            src[rng.random(src.shape) < holes] = 0
    else:
        src = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
        src[..., 0] = np.maximum(src[..., 0], 1)
        if holes:
            src[..., 0][rng.random(src.shape[:2]) < holes] = 0
    return src


def smooth_raster(h, w, seed, device=None):
    """fBm heightmap in [1, 65535]; large sizes come from the HIP generator (which the GPU tests check
    against the integer numpy model), small ones from the model itself."""
    if device is not None:
        ptr = device.synth_fbm_r16(w, h, seed)
        out = device.download(ptr, (h, w), np.uint16)
        device.free(ptr)
        return out
    import _model as M
    return M.fbm_u16(w, h, seed)


def product_planar(device, src, lod_count, T, b, fmt, atlas_size=128, generic=False, mips=1, reference_dispatch=False, **ds):
    cfg = bt.TerrainConfig(lod_count=lod_count, atlas_size=atlas_size, path="terrains/test",
                           model=bt.TerrainModel.planar((0, 0, 0), 1000.0, 0.0, 1.0))
    cfg.add_attachment(bt.AttachmentConfig(name="att", texture_size=T, border_size=b, format=FMT[fmt],
                                           mip_level_count=mips))
    atlas = bt.TileAtlas.new(cfg, device)
    server = bt.AssetServer().insert("src", src)
    pre = bt.Preprocessor.new().clear_attachment(0, atlas).preprocess_tile(
        bt.PreprocessDataset(attachment_index=0, path="src", lod_range=range(0, lod_count), **ds), server, atlas)
    pre.run(atlas, generic=generic, reference_dispatch=reference_dispatch)
    return atlas, pre


def oracle_planar(src, lod_count, T, b, fmt, atlas_size=128, threads=8, **ds):
    a = O.OracleAtlas(lod_count, atlas_size, False, [(T, b, 1, fmt)])
    a.clear_attachment(0).preprocess_tile(0, src, (0, lod_count), **ds).run(threads)
    return a


def reference_kernels(oracle_atlas):
    """Checker for the BASELINE configs and smoke(): the oracle's queue driver with every Split / Downsample / Stitch task
    executed by the REFERENCE'S OWN WGSL (oracle/_ref, see tests/_wgslref.py) instead of the hand-written kernels.  The
    built library travels to the GPU box; its absence is an error, not a silent fallback."""
    import _wgslref as W

    assert W.available(), "oracle/_ref/libbt_wgslref.so missing: run `make -C oracle/wgsl_ref` where /root/reference exists"
    return W.attach(oracle_atlas)


def assert_atlas_equal(atlas, oracle, attachment=0):
    ours = atlas.tiles()
    theirs = oracle.tiles()
    # the integer tile-index contract: same coordinates at the same atlas indices
    assert [((c.side, c.lod, c.x, c.y), i) for c, i in ours] == theirs
    n = len(ours)
    if n == 0:
        return 0
    used = max(i for _, i in ours) + 1
    guard = min(2, atlas.config.atlas_size - used)  # the layers behind the last tile: nothing may have written them (zero since bt_atlas_create)
    data = atlas.download_tiles(attachment, 0, used + guard)
    assigned = {i for _, i in ours}
    stray = [i for i in range(used + guard) if i not in assigned and data[i].any()]
    assert not stray, f"layers {stray[:5]} hold no tile and are not zero"
    bad = []
    for coord, idx in theirs:
        exp = oracle.tile(attachment, idx)
        if not np.array_equal(data[idx], exp):
            diff = np.argwhere(data[idx] != exp)
            bad.append((coord, len(diff), tuple(diff[0]), data[idx][tuple(diff[0])], exp[tuple(diff[0])]))
    assert not bad, f"{len(bad)}/{n} tiles differ, first: {bad[:3]}"
    return n


def prior_pattern(fmt, T, layer):
    """Previous contents of atlas layer `layer` for overlay tests: non-zero everywhere (R16 and Rgba8 channel 0 in the upper half,
    [0x8000, 0xFFFF] / [0x80, 0xFF]), different per layer and per texel (a hash of (layer, y, x)).  A job whose source keeps its values
    (channel 0) in the lower half cannot compute a pattern value, so a texel that holds one was kept, not blended."""
    y, x = np.mgrid[0:T, 0:T].astype(np.uint64)
    m = np.uint64(0xFFFFFFFF)
    h = (np.uint64((layer + 1) * 0x9E3779B1 & 0xFFFFFFFF)) ^ (y * np.uint64(0x85EBCA77) & m) ^ (x * np.uint64(0xC2B2AE3D) & m)
    h ^= h >> np.uint64(15)
    h = h * np.uint64(0x2C1B3C6D) & m
    h ^= h >> np.uint64(13)
    if fmt == O.FORMAT_R16:
        return ((h & np.uint64(0xFFFF)) | np.uint64(0x8000)).astype(np.uint16)
    out = np.stack([(h >> np.uint64(8 * k)) & np.uint64(0xFF) for k in range(4)], axis=-1).astype(np.uint8)
    out[..., 0] |= 0x80
    return out


def low_half(src, fmt):
    """the source with its values (R16) / channel 0 (Rgba8) moved into the lower half, no-data (0) kept: blends of it stay below
    prior_pattern's values"""
    src = src.copy()
    plane = src if fmt == O.FORMAT_R16 else src[..., 0]
    plane[...] = np.where(plane == 0, 0, (plane >> 1) | 1)  # 1 .. 0x7FFF / 1 .. 0x7F
    return src


def kept_texels(fresh, primed, prior, b):
    """centre texels of one tile where the job had no data: the oracle run onto zeros left 0 there and the run onto `prior` kept it"""
    c = slice(b, fresh.shape[0] - b)
    f, p, q = fresh[c, c], primed[c, c], prior[c, c]
    if f.ndim == 3:
        return (f[..., 0] == 0) & (p == q).all(axis=-1)
    return (f == 0) & (p == q)

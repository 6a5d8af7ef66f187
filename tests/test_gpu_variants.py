"""Which kernel variant produced the tiles: every plan and kernel variant the launch planner (fused_plan, bt_fused_plan.cpp) can choose, pinned by a
small job that must report EXACTLY its variants (bt_run_stats.variants) and match the oracle tile for tile — on a fresh atlas, re-run onto the
written atlas (no-data texels fetch their previous value), through the streamed pipeline and onto a fresh atlas primed with non-zero
previous contents (the fetch must read the right texel of the right layer).  A planner change (a threshold, the size of
MainShared in bt_fused_args.hpp) that moves a case to another variant fails here and has to be moved on purpose; a variant without a case fails on the CPU
(test_every_variant_has_a_case)."""

import numpy as np
import pytest

import _cases as K
import _model as M
import _oracle as O
import bevy_terrain_amd as bt
from bevy_terrain_amd import _ffi

R16, RGBA8 = O.FORMAT_R16, O.FORMAT_RGBA8
MAIN_ROWS = 8  # kMainRows: centre rows of a fused_main chunk


# Variants no job reaches through the API, with the reason
UNREACHABLE = {
    "MAIN_REG_528": "no longer reported: the library has no fused_main<512, 528> with register staging.  Every R16 raster is 16-byte aligned in base and "
                    "pitch (the library pads what it uploads and copies an unaligned borrowed device raster into a padded buffer: bt_preprocessor_preprocess_tile), "
                    "so T = 512 at pitch 528 takes the LDS-DMA instance (MAIN_DMA_528); an unaligned one would take MAIN_REG_PITCH",
}


def case(name, variants, fmt, T, b, lods, size, *, lod_lo=0, rect=None, nodata=(), second=None, first_job=None):
    """variants: the exact BT_VARIANT_* set; size: (W, H) of the source or six (W, H) of a cube job; rect: ((tlx, tly), (brx, bry));
    nodata: placements of no-data texels besides a sparse random scatter ("skipped", "apron", "chunks", "corners");
    second: (T, b) of a second R16 attachment with its own job in the same queue; first_job: an earlier job of the same queue on the
    coarsest LOD alone (from a source of one tile), so that the main job's atlas indices are not the fresh layout"""
    return pytest.param(dict(variants=frozenset(variants), fmt=fmt, T=T, b=b, lods=lods, size=size, lod_lo=lod_lo, rect=rect, nodata=nodata,
                             second=second, first_job=first_job), id=name)


def _m(T, b, lods, ratio):
    """source side for a source-to-tile ratio"""
    return int(round((T - 2 * b) * (1 << (lods - 1)) * ratio))


CASES = [
    # fused_direct (Rgba8): the row-step variant follows the source-to-tile ratio of the rows (raster.height)
    case("direct-skips-1.03", {"DIRECT_SKIPS", "STITCH_LAUNCH"}, RGBA8, 512, 2, 3, (_m(512, 2, 3, 1.03),) * 2, nodata=("skipped",)),
    case("direct-plain-1.015", {"DIRECT", "STITCH_LAUNCH"}, RGBA8, 512, 2, 2, (_m(512, 2, 2, 1.015),) * 2, nodata=("skipped",)),
    case("direct-skips-1.9", {"DIRECT_SKIPS", "STITCH_LAUNCH"}, RGBA8, 512, 2, 2, (_m(512, 2, 2, 1.9),) * 2, nodata=("skipped",)),
    case("direct-skips-aniso-0.8x1.3", {"DIRECT_SKIPS", "STITCH_LAUNCH"}, RGBA8, 512, 2, 2, (_m(512, 2, 2, 0.8), _m(512, 2, 2, 1.3)), nodata=("skipped",)),
    case("direct-rep-0.9995", {"DIRECT_REP", "STITCH_LAUNCH"}, RGBA8, 512, 2, 2, (1015, 1015)),
    case("direct-plain-1.0", {"DIRECT", "STITCH_LAUNCH"}, RGBA8, 512, 2, 2, (1016, 1016)),
    case("direct-rep-aniso-1.4x0.8", {"DIRECT_REP", "STITCH_LAUNCH"}, RGBA8, 512, 2, 2, (_m(512, 2, 2, 1.4), _m(512, 2, 2, 0.8))),
    # six faces from 0.8 to 1.4 of the grid: both flags, the kRep instance runs (faces whose rows skip source rows too)
    case("direct-rep-cube-mixed", {"DIRECT_REP", "STITCH_LAUNCH"}, RGBA8, 256, 2, 2,
         tuple((_m(256, 2, 2, r), _m(256, 2, 2, r)) for r in (0.8, 1.4, 1.0, 1.1, 0.9, 1.25)), nodata=("skipped",)),
    # a dataset rectangle: the ratio is the source over HALF the mosaic (bry - tly = 0.5): 900 / 1016
    case("direct-rep-rect", {"DIRECT_REP", "STITCH_LAUNCH"}, RGBA8, 512, 2, 3, (900, 900), lod_lo=1, rect=((0.0, 0.0), (0.5, 0.5))),
    # fused_main (R16, T <= 512, even b <= 8)
    case("main-dma-528-1.0", {"MAIN_DMA_528", "STITCH_LAUNCH"}, R16, 512, 2, 2, (1016, 1016), nodata=("apron", "chunks")),
    case("main-dma-pitch-1.23", {"MAIN_DMA_PITCH", "STITCH_LAUNCH"}, R16, 512, 2, 3, (_m(512, 2, 3, 1.23),) * 2, nodata=("apron", "chunks")),
    case("main-apron-global-1.3", {"MAIN_APRON_GLOBAL", "STITCH_LAUNCH"}, R16, 512, 2, 3, (_m(512, 2, 3, 1.3),) * 2, nodata=("apron", "chunks")),
    case("main-single-buffer-1.41", {"MAIN_SINGLE_BUFFER", "STITCH_LAUNCH"}, R16, 512, 2, 3, (_m(512, 2, 3, 1.41),) * 2, nodata=("apron", "chunks")),
    case("main-dma-pitch-T256-1.9", {"MAIN_DMA_PITCH", "STITCH_LAUNCH"}, R16, 256, 2, 3, (_m(256, 2, 3, 1.9),) * 2, nodata=("apron", "chunks")),
    case("main-reg-pitch-T128-1.0", {"MAIN_REG_PITCH", "STITCH_LAUNCH"}, R16, 128, 2, 3, (496, 496), nodata=("apron", "chunks")),
    case("main-unstaged-T128-5", {"MAIN_UNSTAGED", "STITCH_LAUNCH"}, R16, 128, 2, 3, (_m(128, 2, 3, 5.0),) * 2, nodata=("corners",)),
    # fused_tail below three fused LODs: the closed form of the fresh layout, or the grids
    case("tail-regular-r16", {"MAIN_REG_PITCH", "TAIL_REGULAR"}, R16, 128, 2, 4, (992, 992), nodata=("apron",)),
    case("tail-irregular-r16", {"MAIN_REG_PITCH", "TAIL_IRREGULAR"}, R16, 128, 2, 4, (992, 992), first_job=True),
    case("tail-regular-rgba8", {"DIRECT", "TAIL_REGULAR"}, RGBA8, 128, 2, 4, (992, 992)),
    case("tail-irregular-rgba8", {"DIRECT", "TAIL_IRREGULAR"}, RGBA8, 128, 2, 4, (992, 992), first_job=True),
    # the batched split + stitch of the finest LOD, fused_tail below it
    case("hybrid-b10", {"HYBRID", "TAIL_REGULAR"}, R16, 512, 10, 3, (1968, 1968), nodata=("apron",)),
    case("hybrid-T1024", {"HYBRID", "TAIL_REGULAR"}, R16, 1024, 2, 2, (2040, 2040)),
    # the batched kernels for the whole queue: an odd border, and a qualifying job queued with one that does not (second attachment)
    case("generic-odd-b", {"GENERIC"}, R16, 128, 3, 3, (500, 500)),
    case("generic-mixed-queue", {"GENERIC"}, R16, 128, 2, 3, (496, 496), second=(128, 3)),
]


def _rows_read(mosaic_rows, c, lods, lo, hi, dim):
    """the source rows (both of the bilinear pair) that the given finest-LOD mosaic rows read (split.wgsl's axis, tests/_model.py)"""
    n = 1 << (lods - 1)
    x0, x1, _ = M._axis_params(n * c, c, n, lo, hi, dim)
    rows = np.asarray(sorted(mosaic_rows), dtype=np.int64)
    rows = rows[(rows >= 0) & (rows < n * c)]
    return np.union1d(x0[rows], x1[rows])


def _place_nodata(src, fmt, cfg, c, b, lods, rect, seed):
    """no-data texels where the variants read in their own way, plus a sparse random scatter"""
    rng = np.random.default_rng(seed)
    H, W = src.shape[:2]
    (tlx, tly), (brx, bry) = rect or ((0.0, 0.0), (1.0, 1.0))
    n = 1 << (lods - 1)
    plane = src if fmt == R16 else src[..., 0]
    plane[rng.random((H, W)) < 0.005] = 0
    bands = [k * c + d for k in range(1, n) for d in range(-b, b)]  # the apron rows of every finest tile boundary
    cols = slice(int(rng.integers(0, 7)), None, 23)
    for kind in cfg["nodata"]:
        if kind == "skipped":  # source rows the chain of row starts passes over (read as the second row of a pair only)
            x0, x1, _ = M._axis_params(n * c, c, n, tly, bry, H)
            rows = np.setdiff1d(np.arange(x0.min(), x0.max() + 1), x0)
            assert len(rows) or H <= n * c, "a source finer than the grid passes over rows"
            plane[rows, cols] = 0
        elif kind == "apron":
            plane[_rows_read(bands, c, lods, tly, bry, H), cols] = 0
        elif kind == "chunks":  # the first and last row of every chunk of kMainRows centre rows: the staging buffer's boundaries
            chunk = [ty * c + r for ty in range(n) for r0 in range(0, c, MAIN_ROWS) for r in (r0, min(c, r0 + MAIN_ROWS) - 1)]
            plane[_rows_read(chunk, c, lods, tly, bry, H), cols] = 0
        elif kind == "corners":  # the apron corners fused_corner writes: the source around every interior tile corner
            rows = _rows_read(bands, c, lods, tly, bry, H)
            xs = _rows_read(bands, c, lods, tlx, brx, W)
            plane[np.ix_(rows, xs)] = 0
        else:
            raise ValueError(kind)


def _sources(cfg):
    fmt, T, b, lods = cfg["fmt"], cfg["T"], cfg["b"], cfg["lods"]
    sizes = cfg["size"] if isinstance(cfg["size"][0], tuple) else (cfg["size"],)
    out = []
    for k, (W, H) in enumerate(sizes):
        src = K.random_raster(fmt, H, W, seed=1000 * T + 10 * W + k)
        _place_nodata(src, fmt, cfg, T - 2 * b, b, lods, cfg["rect"], seed=W + k)
        out.append(src)
    return out


def _names(mask, bits):
    return sorted(name for name, bit in bits.items() if mask & bit)


def test_every_variant_has_a_case():
    """CPU: the union of the table's variants and UNREACHABLE is every BT_VARIANT_* of the header, bit for bit"""
    bits = K.variant_bits()
    assert len(bits) == 15 and len(set(bits.values())) == len(bits) and all(v & (v - 1) == 0 for v in bits.values()), bits
    covered = set().union(*(p.values[0]["variants"] for p in CASES))
    assert covered <= set(bits), covered - set(bits)
    assert not covered & set(UNREACHABLE), covered & set(UNREACHABLE)
    assert covered | set(UNREACHABLE) == set(bits), set(bits) - covered - set(UNREACHABLE)
    # the names the header spells (the Python binding reads them through the stats dict)
    assert "variants" in {f[0] for f in _ffi.RunStatsC._fields_} and "reserved" not in {f[0] for f in _ffi.RunStatsC._fields_}


@pytest.fixture(scope="module")
def device():
    return bt.Device(0)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CASES)
def test_variant_matches_the_oracle(device, tmp_path, cfg):
    bits = K.variant_bits()
    fmt, T, b, lods, lod_lo, rect = cfg["fmt"], cfg["T"], cfg["b"], cfg["lods"], cfg["lod_lo"], cfg["rect"]
    cube = isinstance(cfg["size"][0], tuple)
    srcs = _sources(cfg)
    ds = dict(top_left=rect[0], bottom_right=rect[1]) if rect else {}
    atlas_size = 16 if T > 512 else 128 if lods > 3 else 64
    attachments = [(T, b, 1, fmt)] + ([(cfg["second"][0], cfg["second"][1], 1, R16)] if cfg["second"] else [])
    first = K.random_raster(fmt, T - 2 * b, T - 2 * b, seed=5) if cfg["first_job"] else None
    second = K.random_raster(R16, 500, 500, seed=6, holes=0.01) if cfg["second"] else None

    def run_oracle(prior=None):
        """prior: {(attachment, layer): texels} the atlas holds before the queue runs (else the atlas's zeros)"""
        oracle = O.OracleAtlas(lods, atlas_size, cube, attachments)
        for (i, layer), texels in (prior or {}).items():
            oracle.set_tile(i, layer, texels)
        for i in range(len(attachments)):
            oracle.clear_attachment(i)
        if first is not None:
            oracle.preprocess_tile(0, first, (0, 1))
        if cube:
            oracle.preprocess_spherical(0, srcs, (lod_lo, lods))
        else:
            oracle.preprocess_tile(0, srcs[0], (lod_lo, lods), **ds)
        if second is not None:
            oracle.preprocess_tile(1, second, (0, lods))
        return oracle.run(16)

    oracle = fresh = run_oracle()

    server = bt.AssetServer()
    for k, s in enumerate(srcs):
        server.insert(f"s{k}", s)
    if first is not None:
        server.insert("first", first)
    if second is not None:
        server.insert("second", second)
    model = {} if cube else dict(model=bt.TerrainModel.planar((0, 0, 0), 1000.0, 0.0, 1.0))
    tc = bt.TerrainConfig(lod_count=lods, atlas_size=atlas_size, path="terrains/variants", **model)
    for k, (t, bb, _, f) in enumerate(attachments):
        tc.add_attachment(bt.AttachmentConfig(name=f"a{k}", texture_size=t, border_size=bb, format=K.FMT[f]))

    def queue(atlas, root=None, defer=False):
        pre = bt.Preprocessor.new()
        for i in range(len(attachments)):
            pre.clear_attachment(i, atlas, root)
        if first is not None:
            pre.preprocess_tile(bt.PreprocessDataset(attachment_index=0, path="first", lod_range=range(0, 1)), server, atlas, defer_upload=defer)
        if cube:
            pre.preprocess_spherical(bt.SphericalDataset(attachment_index=0, paths=[f"s{k}" for k in range(6)], lod_range=range(lod_lo, lods)),
                                     server, atlas, defer_upload=defer)
        else:
            pre.preprocess_tile(bt.PreprocessDataset(attachment_index=0, path="s0", lod_range=range(lod_lo, lods), **ds), server, atlas, defer_upload=defer)
        if second is not None:
            pre.preprocess_tile(bt.PreprocessDataset(attachment_index=1, path="second", lod_range=range(0, lods)), server, atlas, defer_upload=defer)
        return pre

    def check(atlas, oracle=oracle):
        n = sum(K.assert_atlas_equal(atlas, oracle, attachment=i) for i in range(len(attachments)))
        assert n > 0
        return n

    masks = []
    atlas = bt.TileAtlas.new(tc, device)
    pre = queue(atlas)
    pre.run(atlas, keep_queue=True)  # 1. a fresh atlas: the previous value of a no-data texel is the atlas's 0
    masks.append(pre.stats()["variants"])
    n = check(atlas)
    pre.run(atlas)  # 2. the kept queue again, onto the written atlas: no-data texels fetch their previous value
    masks.append(pre.stats()["variants"])
    assert check(atlas) == n
    atlas2 = bt.TileAtlas.new(tc, device)  # 3. the streamed pipeline (banded where the plan allows it)
    pre2 = queue(atlas2, str(tmp_path), defer=True)
    pre2.run_streamed(atlas2, str(tmp_path))
    masks.append(pre2.stats()["variants"])
    assert check(atlas2) == n
    want = sum(bits[v] for v in cfg["variants"])
    assert masks == [want] * 3, f"launched {[_names(m, bits) for m in masks]}, the table says {sorted(cfg['variants'])}"

    # 4. a fresh atlas whose every layer the queue writes holds non-zero previous contents (tests/_cases.prior_pattern, uploaded by the
    # host): no launch may take the previous value as 0, and a no-data texel keeps ITS layer's texel — which steps 1 and 2 cannot tell
    # from 0 (step 2's previous values are the zeros step 1 left at the no-data texels)
    prior = {(i, idx): K.prior_pattern(attachments[i][3], attachments[i][0], idx + 4096 * i)
             for i in range(len(attachments)) for _, idx in fresh.tiles()}
    primed = run_oracle(prior)
    atlas3 = bt.TileAtlas.new(tc, device)
    for (i, idx), texels in prior.items():
        atlas3.upload_tile(i, idx, texels)
    pre3 = queue(atlas3)
    pre3.run(atlas3)
    assert pre3.stats()["variants"] == want, f"launched {_names(pre3.stats()['variants'], bits)} onto the primed atlas"
    assert check(atlas3, primed) == n
    assert pre3.stats()["prev_zero_launches"] == 0
    # not vacuous: the finest tiles of the main job (per face of a cube job) keep the pattern at no-data centre texels the fresh run left 0
    kept = {}
    for (side, lod, _, _), idx in fresh.tiles():
        if lod == lods - 1:
            k = K.kept_texels(fresh.tile(0, idx), primed.tile(0, idx), prior[(0, idx)], b)
            kept[side] = kept.get(side, 0) + int(k.sum())
    assert len(kept) == (6 if cube else 1) and min(kept.values()) >= 16, f"no-data centre texels that keep the previous value, per side: {kept}"

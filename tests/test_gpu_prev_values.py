"""Kept previous values and the host's bookkeeping behind FusedArgs::prev_zero.

A finest-tile texel whose source sample has no data keeps the atlas's previous value (split.wgsl:34-42).  A fused launch whose finest
layers nothing has written since bt_atlas_create takes that value as 0 without reading it (prev_zero, decided by fused_begin_run from
Attachment::written).  That is only right if every path that puts bytes into level 0 marks its layers written, and only fast if no read
does.  Every writer below primes a fresh atlas (and the oracle, OracleAtlas.set_tile) with non-zero previous contents, then one small fused
job with no-data texels inside and across finest-tile seams runs onto it: the tiles equal the oracle's, no launch is flagged, and the
no-data centre texels hold what the writer put there.  The reads at the end must leave the flag on."""

import ctypes as C
import os

import numpy as np
import pytest

import _cases as K
import _oracle as O
import bevy_terrain_amd as bt
from bevy_terrain_amd import _ffi

R16, RGBA8 = O.FORMAT_R16, O.FORMAT_RGBA8
T, B, LODS, W, ATLAS = 128, 2, 3, 496, 32  # 21 tiles; source : mosaic = 1.0 -> fused_main (register staging, pitch 128) / fused_direct
VARIANT = {R16: "MAIN_REG_PITCH", RGBA8: "DIRECT"}
MIN_KEPT = 16  # no-data centre texels per primed finest tile that must hold the previous value


def _source(fmt, seed=3):
    """values (channel 0) in the lower half — prior_pattern's values cannot come out of a blend — and no-data rows and columns across the
    finest-tile seams (mosaic rows / columns 124, 248, 372 at ratio 1.0) besides a sparse scatter"""
    src = K.low_half(K.random_raster(fmt, W, W, seed=seed, holes=0.01), fmt)
    plane = src if fmt == R16 else src[..., 0]
    plane[118:131, 20:300] = 0
    plane[200:420, 244:253] = 0
    plane[365:380, 360:480] = 0
    return src


def _base(fmt):
    """a full-data source for the earlier job an overlay is laid onto"""
    src = K.low_half(K.random_raster(fmt, W, W, seed=99), fmt)
    (src if fmt == R16 else src[..., 0])[...] |= 1
    return src


class Job:
    """the same preprocess job on the product and on the oracle; prior: {(attachment, layer): texels} the atlas holds beforehand"""

    def __init__(self, device, fmt, attachments=1):
        self.device, self.fmt = device, fmt
        self.src = _source(fmt)
        self.attachments = [(T, B, 1, fmt)] * attachments
        self.tc = bt.TerrainConfig(lod_count=LODS, atlas_size=ATLAS, path="terrains/prev",
                                   model=bt.TerrainModel.planar((0, 0, 0), 1000.0, 0.0, 1.0))
        for k in range(attachments):
            self.tc.add_attachment(bt.AttachmentConfig(name=f"a{k}", texture_size=T, border_size=B, format=K.FMT[fmt]))
        self.base = _base(fmt)
        self.server = bt.AssetServer().insert("src", self.src).insert("base", self.base)
        self.fresh = self.oracle()
        self.layers = [i for _, i in self.fresh.tiles()]
        self.finest = [i for c, i in self.fresh.tiles() if c[1] == LODS - 1]

    def oracle(self, prior=None, base_first=False):
        o = O.OracleAtlas(LODS, ATLAS, False, self.attachments)
        for (a, layer), texels in (prior or {}).items():
            o.set_tile(a, layer, texels)
        o.clear_attachment(0)
        if base_first:
            o.preprocess_tile(0, self.base, (0, LODS))
        return o.preprocess_tile(0, self.src, (0, LODS)).run(16)

    def pattern(self, layers=None, attachment=0):
        return {(attachment, i): K.prior_pattern(self.fmt, T, i + 4096 * attachment) for i in (self.layers if layers is None else layers)}

    def atlas(self):
        return bt.TileAtlas.new(self.tc, self.device)

    def queue(self, atlas, root=None, defer=False, base_first=False):
        pre = bt.Preprocessor.new().clear_attachment(0, atlas, root)
        if base_first:
            pre.preprocess_tile(bt.PreprocessDataset(attachment_index=0, path="base", lod_range=range(0, LODS)), self.server, atlas, defer_upload=defer)
        return pre.preprocess_tile(bt.PreprocessDataset(attachment_index=0, path="src", lod_range=range(0, LODS)), self.server, atlas, defer_upload=defer)

    def check(self, atlas, pre, prior, flagged=0, oracle=None):
        """tiles == the oracle's run onto `prior`; `flagged` launches took prev_zero; a primed finest tile keeps its previous texels at the
        job's no-data centre texels, an unprimed one keeps 0 there"""
        stats = pre.stats()
        assert VARIANT[self.fmt] in K.variants(stats), K.variants(stats)
        primed = oracle or self.oracle(prior)
        assert K.assert_atlas_equal(atlas, primed) == len(self.layers)  # (first: a wrong flag shows as the texels it lost)
        assert stats["prev_zero_launches"] == flagged
        data = atlas.download_tiles(0, 0, max(self.layers) + 1)
        c = slice(B, T - B)
        for i in self.finest:
            fresh = self.fresh.tile(0, i)[c, c]
            nodata = (fresh if fresh.ndim == 2 else fresh[..., 0]) == 0  # the run onto zeros left 0 there
            assert nodata.sum() >= MIN_KEPT, (i, int(nodata.sum()))
            if (0, i) in prior:
                kept = K.kept_texels(self.fresh.tile(0, i), data[i], prior[(0, i)], B)
                assert kept.sum() == nodata.sum(), f"layer {i}: {int(nodata.sum() - kept.sum())} no-data centre texels lost the previous value"
            else:
                assert not data[i][c, c][nodata].any(), f"layer {i} (not primed): a no-data centre texel is not 0"
        return primed


def _write_through(device, ptr, tile_bytes, prior):
    for (_, layer), texels in prior.items():
        texels = np.ascontiguousarray(texels)
        _ffi.check(_ffi.lib().bt_memcpy_h2d(device._h, C.c_void_p(ptr + layer * tile_bytes), texels.ctypes.data_as(C.c_void_p), texels.nbytes))


@pytest.fixture(scope="module")
def device():
    return bt.Device(0)


@pytest.fixture(scope="module", params=[R16, RGBA8], ids=["r16", "rgba8"])
def job(request, device):
    return Job(device, request.param)


@pytest.mark.gpu
def test_the_fresh_job_is_flagged(job):
    """the baseline every row below departs from: onto a fresh atlas the fused launch takes prev_zero and the tiles still equal the oracle's"""
    atlas = job.atlas()
    pre = job.queue(atlas)
    pre.run(atlas)
    job.check(atlas, pre, {}, flagged=1, oracle=job.fresh)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["one", "all"])
def test_upload_tile(job, which):
    """bt_atlas_upload_tile into one finest layer (the rest fresh: the launch is still not flagged, the fresh tiles keep 0) or into all"""
    prior = job.pattern([job.finest[1]] if which == "one" else None)
    atlas = job.atlas()
    for (a, i), texels in prior.items():
        atlas.upload_tile(a, i, texels)
    pre = job.queue(atlas)
    pre.run(atlas)
    job.check(atlas, pre, prior)


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["attachment_storage", "mip_storage_0"])
def test_writes_through_a_storage_pointer(device, job, how):
    """the caller writes level 0 through the pointer bt_atlas_attachment_storage / bt_atlas_mip_storage(level 0) hands out"""
    atlas = job.atlas()
    if how == "attachment_storage":
        ptr, tile_bytes, _ = atlas.attachment_storage(0)
    else:
        p, tb = C.c_void_p(), C.c_uint64()
        _ffi.check(_ffi.lib().bt_atlas_mip_storage(atlas._h, 0, 0, C.byref(p), C.byref(tb)))
        ptr, tile_bytes = p.value, tb.value
    prior = job.pattern()
    _write_through(device, ptr, tile_bytes, prior)
    pre = job.queue(atlas)
    pre.run(atlas)
    job.check(atlas, pre, prior)


def _saved_pattern(job, root):
    """the primed oracle's tiles as `.bin` files + config.tc under root (the tiles the job allocates, holding the pattern)"""
    prior = job.pattern()
    o = O.OracleAtlas(LODS, ATLAS, False, job.attachments)
    for (a, i), texels in prior.items():
        o.set_tile(a, i, texels)
    o.clear_attachment(0).preprocess_tile(0, job.src, (0, LODS))  # allocates the tiles (not run)
    directory = os.path.join(root, "terrains/prev", "data", "a0")
    os.makedirs(directory, exist_ok=True)
    o.save_attachment(0, directory)
    o.save_tile_config(os.path.join(root, "terrains/prev", "config.tc"))
    return prior


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["load_tiles", "update"])
def test_loaded_tiles(job, tmp_path, how):
    """tiles read from files: bt_atlas_load_tile_config + bt_atlas_load_tiles, or request_tile + the streaming loads of bt_atlas_update"""
    root = str(tmp_path)
    prior = _saved_pattern(job, root)
    atlas = job.atlas()
    coords = [bt.TileCoordinate(*c) for c, _ in job.fresh.tiles()]  # in atlas-index order: the loads take the slots the job would
    atlas.load_tile_config(root)
    if how == "load_tiles":
        atlas.load_tiles(0, root, coords)
    else:
        for c in coords:
            atlas.request_tile(c)
        assert atlas.update(root) == (len(coords), 0)
    pre = job.queue(atlas)
    pre.run(atlas)
    job.check(atlas, pre, prior)


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["generic_run", "same_queue"])
def test_earlier_job(job, how):
    """a full-data job that ran before onto the same tiles — an earlier run of the batched kernels (BT_RUN_GENERIC), or the first job of the
    same queue (fused, flagged: only it) — and the overlay keeps the earlier job's texels where it has no data"""
    base_oracle = O.OracleAtlas(LODS, ATLAS, False, job.attachments)
    base_oracle.clear_attachment(0).preprocess_tile(0, job.base, (0, LODS)).run(16)
    assert [i for _, i in base_oracle.tiles()] == job.layers
    prior = {(0, i): base_oracle.tile(0, i) for i in job.layers}
    atlas = job.atlas()
    if how == "generic_run":
        pre = bt.Preprocessor.new().clear_attachment(0, atlas).preprocess_tile(
            bt.PreprocessDataset(attachment_index=0, path="base", lod_range=range(0, LODS)), job.server, atlas)
        pre.run(atlas, generic=True)
        assert K.variants(pre.stats()) == {"GENERIC"}
        K.assert_atlas_equal(atlas, base_oracle)
        pre = job.queue(atlas)
        pre.run(atlas)
        job.check(atlas, pre, prior)
    else:
        pre = job.queue(atlas, base_first=True)
        pre.run(atlas)
        job.check(atlas, pre, prior, flagged=1, oracle=job.oracle(base_first=True))


@pytest.mark.gpu
def test_streamed_run(job, tmp_path):
    """the overlay through the streamed pipeline (bt_preprocessor_run_streamed) onto a primed atlas"""
    prior = job.pattern()
    atlas = job.atlas()
    for (a, i), texels in prior.items():
        atlas.upload_tile(a, i, texels)
    pre = job.queue(atlas, str(tmp_path), defer=True)
    st = pre.run_streamed(atlas, str(tmp_path))
    assert st["streamed"]
    job.check(atlas, pre, prior)


@pytest.mark.gpu
def test_sharded_run_over_emulated_ranks(device):
    """every emulated rank's atlas primed (tests/test_shard.py's harness: BT_RUN_SHARD_LOCAL per rank, the pieces by hand, BT_RUN_SHARD_FINISH
    on rank 0): no rank's launch is flagged and every finest piece and the finished atlas equal the primed oracle's"""
    from test_shard import _emulate_ranks

    T6, b6, lods6, world = 64, 2, 6, 2
    src = K.random_raster(R16, 1100, 1100, seed=35, holes=0.01)
    src[500:530, :] = 0
    fresh = K.oracle_planar(src, lods6, T6, b6, R16, atlas_size=2048, threads=16)
    layers = [i for _, i in fresh.tiles()]
    prior = {i: K.prior_pattern(R16, T6, i) for i in layers}
    primed = O.OracleAtlas(lods6, 2048, False, [(T6, b6, 1, R16)])
    for i, texels in prior.items():
        primed.set_tile(0, i, texels)
    primed.clear_attachment(0).preprocess_tile(0, src, (0, lods6)).run(16)
    jobs = []

    def make_job():
        cfg = bt.TerrainConfig(lod_count=lods6, atlas_size=2048, path="t", model=bt.TerrainModel.planar((0, 0, 0), 1.0, 0.0, 1.0))
        cfg.add_attachment(bt.AttachmentConfig(name="h", texture_size=T6, border_size=b6))
        atlas = bt.TileAtlas.new(cfg, device)
        for i, texels in prior.items():
            atlas.upload_tile(0, i, texels)
        pre = bt.Preprocessor.new().preprocess_tile(bt.PreprocessDataset(path="s", lod_range=range(0, lods6)), bt.AssetServer().insert("s", src), atlas)
        jobs.append((atlas, pre))
        return atlas, pre

    pieces = _emulate_ranks(device, world, make_job, len(layers), primed, lods6 - 1, T6, b6)
    assert len({p["owner_rank"] for p in pieces}) == world
    assert all(pre.stats()["prev_zero_launches"] == 0 for _, pre in jobs)
    finest = [i for c, i in fresh.tiles() if c[1] == lods6 - 1]
    data = jobs[0][0].download_tiles(0, 0, max(layers) + 1)
    kept = sum(int(K.kept_texels(fresh.tile(0, i), data[i], prior[i], b6).sum()) for i in finest)
    assert kept >= MIN_KEPT * 4


@pytest.mark.gpu
def test_two_attachments_are_flagged_on_their_own(device):
    """Attachment::written is per attachment: priming attachment 1 leaves attachment 0's job flagged; priming attachment 0 unflags it"""
    job = Job(device, R16, attachments=2)
    for primed_attachment, flagged in ((1, 1), (0, 0)):
        prior = job.pattern(attachment=primed_attachment)
        atlas = job.atlas()
        for (a, i), texels in prior.items():
            atlas.upload_tile(a, i, texels)
        pre = job.queue(atlas)
        pre.run(atlas)
        job.check(atlas, pre, {k: v for k, v in prior.items() if k[0] == 0}, flagged=flagged,
                  oracle=job.fresh if flagged else None)
        if primed_attachment == 1:  # attachment 1 holds the pattern untouched
            data = atlas.download_tiles(1, 0, max(job.layers) + 1)
            assert all(np.array_equal(data[i], prior[(1, i)]) for i in job.layers)


@pytest.mark.gpu
def test_reads_are_not_writes(device, tmp_path):
    """downloads, download_mip at levels 1 AND 0, sample, generate_mipmaps, save_attachment and a tile tree's sample_attachment /
    approximate_height on a fresh atlas: the job after them still takes prev_zero (and still equals the oracle)"""
    job = Job(device, R16)
    job.tc = bt.TerrainConfig(lod_count=LODS, atlas_size=ATLAS, path="terrains/prev", model=job.tc.model)
    job.tc.add_attachment(bt.AttachmentConfig(name="a0", texture_size=T, border_size=B, format=bt.AttachmentFormat.R16, mip_level_count=2))
    atlas = job.atlas()
    assert not atlas.download_tiles(0, 0, ATLAS).any()
    assert not atlas.download_tile(0, job.finest[0]).any()
    with pytest.raises(ValueError, match="no storage"):  # (mip levels >= 1 are allocated by the first generate_mipmaps / load)
        atlas.download_mip(0, 1, job.finest[0])
    assert not atlas.download_mip(0, 0, job.finest[0]).any()
    assert not atlas.sample(0, job.finest[:2], [(0.5, 0.5), (0.25, 0.75)]).any()
    atlas.generate_mipmaps(0)
    assert not atlas.download_mip(0, 1, job.finest[0]).any()
    atlas.save_attachment(0, str(tmp_path))
    tree = bt.TileTree(atlas, atlas.model, LODS, bt.TerrainViewConfig())  # (no update: its requests would take atlas slots)
    tree.sample_attachment(0, np.array([[120.0, 0.0, -75.0], [500.0, 0.0, 500.0]]))
    tree.approximate_height()
    pre = job.queue(atlas)
    pre.run(atlas)
    job.check(atlas, pre, {}, flagged=1, oracle=job.fresh)


@pytest.mark.gpu
def test_a_fresh_atlas_then_a_new_stream(job):
    """bt_atlas_create zeroes the layers with a memset queued on the context's stream, and a prev_zero launch leaves no-data texels unwritten
    on the strength of it.  bt_ctx_set_stream waits for the outgoing stream, so a job run on the new stream finds the zeros.  (A pass here
    cannot prove that no race is left: an unordered memset usually finishes first anyway.)"""
    import torch

    dev = bt.Device(0)
    other = torch.cuda.Stream(device=0)
    try:
        atlas = bt.TileAtlas.new(job.tc, dev)
        _ffi.check(_ffi.lib().bt_ctx_set_stream(dev._h, C.c_void_p(other.cuda_stream)))
        assert _ffi.lib().bt_ctx_stream(dev._h) == other.cuda_stream
        pre = job.queue(atlas)
        pre.run(atlas)
        job.check(atlas, pre, {}, flagged=1, oracle=job.fresh)
        pre.close()
        atlas.close()
    finally:
        dev.synchronize()
        dev.close()

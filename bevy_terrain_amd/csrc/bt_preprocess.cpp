// Preprocessor (preprocessor.rs): the source rasters and the task queue of a job (the integer tile-index contract: which tile gets which
// atlas index, in which order), its argument checks, and the save of what its runs wrote.  The queue's launches are bt_run.cpp's.
#include <unistd.h>

#include <cmath>
#include <cstring>

#include "bt_tile_io.hpp"

using namespace bt;

namespace {

void release_rasters(bt_preprocessor* p) {
    // kernels of an asynchronous run may still read these buffers; the hipFree this parking replaces synchronised implicitly
    bool synced = false;
    for (Raster& r : p->rasters)
        if (r.owned && r.dev.data && !synced) {
            hipStreamSynchronize(p->ctx->stream);
            synced = true;
        }
    for (Raster& r : p->rasters)
        if (r.owned && r.dev.data) p->ctx->park_raster((void*)r.dev.data, r.alloc_bytes);  // kept for the next queue's rasters (bt_ctx::spare_rasters)
    p->rasters.clear();
}

struct TileRange {
    uint32_t lx, ly, ux, uy;
};

// PreprocessDataset::overlapping_tiles (preprocessor.rs:58-66): f32 maths; `as_uvec2` saturates (negative -> 0).
// The range is clamped to the face (tiles x, y >= 2^lod do not exist; upstream a bottom_right > 1 would invent them).
TileRange overlapping_tiles(const bt_preprocess_dataset& d, uint32_t lod) {
    const float n = float(1u << lod);
    auto sat = [&](float v) -> uint32_t { return !(v > 0.0f) ? 0u : (v >= n ? uint32_t(1u << lod) : uint32_t(v)); };
    return {sat(d.top_left[0] * n), sat(d.top_left[1] * n), sat(std::ceil(d.bottom_right[0] * n)), sat(std::ceil(d.bottom_right[1] * n))};
}

bt_status add_raster(bt_preprocessor* p, const bt_atlas* a, uint32_t ai, const bt_raster* src, int32_t* index) {
    if (!src || !src->data || !src->width || !src->height) {
        set_error("source raster missing");
        return BT_ERR_INVALID_ARGUMENT;
    }
    const uint32_t fmt = a->attachments[ai].meta.format;
    if (fmt != BT_FORMAT_R16 && fmt != BT_FORMAT_RGBA8) {
        set_error("attachment format %u is not processed (reference: preprocessing.wgsl:73-90 has no branch for it)", fmt);
        return BT_ERR_UNSUPPORTED;
    }
    if (src->format != fmt) {
        set_error("raster format %u != attachment format %u", src->format, fmt);
        return BT_ERR_INVALID_ARGUMENT;
    }
    const uint32_t px = fmt == BT_FORMAT_R16 ? 2 : 4;
    const uint64_t pitch = src->row_pitch ? src->row_pitch : uint64_t(src->width) * px;
    if (pitch < uint64_t(src->width) * px || pitch % px) {
        set_error("row_pitch %llu: must hold %u texels of %u bytes and be a multiple of the texel size", (unsigned long long)pitch, src->width, px);
        return BT_ERR_INVALID_ARGUMENT;
    }
    Raster r;
    r.format = fmt;
    r.owned = false;
    r.dev = {src->data, src->width, src->height, pitch};
    if (src->on_device > BT_RASTER_HOST_DEFERRED) {
        set_error("bt_raster.on_device = %u", src->on_device);
        return BT_ERR_INVALID_ARGUMENT;
    }
    // fused_main moves the source in 16-byte pieces (LDS-DMA, or 16-byte register loads): base and pitch must be multiples of 16 bytes, else
    // it stages texel by texel — a 16380-texel-wide R16 raster ran 3 x slower than the 16384-wide one (0.81 vs 0.27 ms).  So the library pads
    // what it uploads itself, and copies a BORROWED device raster whose base or pitch is not 16-byte aligned into a padded buffer of its own
    // (0.5 GB: 0.15 ms) when the queue first runs — the caller's memory is read then, as before.  Deferred host rasters keep the caller's pitch
    // (their bands travel as plain 1-D copies).
    const uint64_t row_bytes = uint64_t(src->width) * px, padded_pitch = (row_bytes + 15u) & ~uint64_t(15);
    const bool r16 = fmt == BT_FORMAT_R16;
    auto take_buffer = [&](uint64_t need, void** dev) -> bt_status {
        uint64_t kept_bytes = 0;
        if (void* kept = p->ctx->take_spare_raster(need, &kept_bytes)) {  // a buffer an earlier queue released
            *dev = kept;
            r.alloc_bytes = kept_bytes;
        } else {
            BT_HIP(hipMalloc(dev, need));
            r.alloc_bytes = need;
        }
        return BT_OK;
    };
    if (src->on_device == 1u && r16 && ((reinterpret_cast<uintptr_t>(src->data) | pitch) & 15u) != 0) {
        void* dev = nullptr;
        BT_HIP(hipSetDevice(p->ctx->device));
        if (bt_status st = take_buffer(padded_pitch * src->height, &dev)) return st;
        r.dev_src = src->data;  // copied (device to device, row by row) by the first run of the queue
        r.dev_src_pitch = pitch;
        r.pending = true;
        r.dev = {dev, src->width, src->height, padded_pitch};
        r.owned = true;
    } else if (src->on_device != 1u) {
        void* dev = nullptr;
        BT_HIP(hipSetDevice(p->ctx->device));
        // the caller's buffer ends with the last texel of the last row, not with a whole pitch
        const uint64_t bytes = pitch * (src->height - 1) + row_bytes;
        const bool pad = r16 && (pitch & 15u) != 0;  // (deferred rasters too: their windows / bands then travel as pitched copies)
        const uint64_t dev_pitch = pad ? padded_pitch : pitch;
        if (bt_status st = take_buffer(dev_pitch * src->height, &dev)) return st;
        if (src->on_device == BT_RASTER_HOST_DEFERRED) {  // copied when the queue runs; the caller keeps the rows alive until then
            r.host = src->data;
            r.host_bytes = bytes;
            r.host_pitch = pitch;
            r.pending = true;
        } else {
            hipError_t e = pad ? hipMemcpy2DAsync(dev, dev_pitch, src->data, pitch, row_bytes, src->height, hipMemcpyHostToDevice, p->ctx->stream)
                               : hipMemcpyAsync(dev, src->data, bytes, hipMemcpyHostToDevice, p->ctx->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(p->ctx->stream);
            if (e != hipSuccess) {
                hipFree(dev);
                return hip_fail(e, "raster upload");
            }
        }
        r.dev.data = dev;
        r.dev.pitch = dev_pitch;
        r.owned = true;
    }
    *index = int32_t(p->rasters.size());
    p->rasters.push_back(r);
    return BT_OK;
}

Task make_task(TaskType type, const bt_atlas_tile& tile, const bt_preprocess_dataset& d, uint32_t job) {
    Task t{};
    t.type = type;
    t.coord = tile.coordinate;
    t.atlas_index = tile.atlas_index;
    t.attachment_index = d.attachment_index;
    t.tl[0] = d.top_left[0];
    t.tl[1] = d.top_left[1];
    t.br[0] = d.bottom_right[0];
    t.br[1] = d.bottom_right[1];
    t.raster = -1;
    t.job = job;
    return t;
}

void push_barrier(bt_preprocessor* p, uint32_t job) {
    Task t{};
    t.type = kBarrier;
    t.raster = -1;
    t.job = job;
    p->queue.push_back(t);
}

// Preprocessor::split_and_downsample (preprocessor.rs:234-269)
bt_status split_and_downsample(bt_preprocessor* p, bt_atlas* a, const bt_preprocess_dataset& d, int32_t raster, uint32_t job) {
    uint32_t lod = d.lod_end - 1;
    TileRange r = overlapping_tiles(d, lod);
    for (uint32_t x = r.lx; x < r.ux; x++)
        for (uint32_t y = r.ly; y < r.uy; y++) {
            bt_atlas_tile tile;
            if (bt_status s = bt_atlas_get_or_allocate_tile(a, {d.side, lod, x, y}, &tile)) return s;
            Task t = make_task(kSplit, tile, d, job);
            t.raster = raster;
            p->queue.push_back(t);
        }
    while (lod > d.lod_begin) {
        lod--;
        push_barrier(p, job);
        r = overlapping_tiles(d, lod);
        for (uint32_t x = r.lx; x < r.ux; x++)
            for (uint32_t y = r.ly; y < r.uy; y++) {
                bt_atlas_tile tile;
                if (bt_status s = bt_atlas_get_or_allocate_tile(a, {d.side, lod, x, y}, &tile)) return s;
                Task t = make_task(kDownsample, tile, d, job);
                bt_tile_coordinate ch[4];
                tile_children(tile.coordinate, ch);
                for (int i = 0; i < 4; i++) bt_atlas_get_tile(a, ch[i], &t.rel[i]);
                p->queue.push_back(t);
            }
    }
    return BT_OK;
}

// Preprocessor::stitch_and_save_layer (preprocessor.rs:271-288)
bt_status stitch_and_save_layer(bt_preprocessor* p, bt_atlas* a, const bt_preprocess_dataset& d, uint32_t lod, uint32_t job) {
    const TileRange r = overlapping_tiles(d, lod);
    for (int pass = 0; pass < 2; pass++) {
        for (uint32_t x = r.lx; x < r.ux; x++)
            for (uint32_t y = r.ly; y < r.uy; y++) {
                bt_atlas_tile tile;
                if (bt_status s = bt_atlas_get_or_allocate_tile(a, {d.side, lod, x, y}, &tile)) return s;
                Task t = make_task(pass == 0 ? kStitch : kSave, tile, d, job);
                if (pass == 0) {
                    bt_tile_coordinate nb[8];
                    tile_neighbours(tile.coordinate, a->config.spherical != 0, nb);
                    for (int i = 0; i < 8; i++) bt_atlas_get_tile(a, nb[i], &t.rel[i]);
                }
                p->queue.push_back(t);
            }
        if (pass == 0) push_barrier(p, job);
    }
    return BT_OK;
}

bt_status check_dataset(const bt_atlas* a, uint32_t ai, uint32_t lod_begin, uint32_t lod_end) {
    if (ai >= a->attachments.size()) {
        set_error("attachment_index %u out of range", ai);
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (lod_end <= lod_begin || lod_end > 31) {
        set_error("lod_range %u..%u", lod_begin, lod_end);
        return BT_ERR_INVALID_ARGUMENT;
    }
    const AttachmentMeta& m = a->attachments[ai].meta;
    if (lod_end - lod_begin > 1 && (m.center_size & 1u)) {
        // downsample.wgsl:18-20 indexes child_tiles[0..4) with center_size/2; odd sizes run out of bounds upstream
        set_error("center_size %u must be even to downsample", m.center_size);
        return BT_ERR_UNSUPPORTED;
    }
    if (m.center_size < m.border_size) {
        // stitch.wgsl:79-88 then reads a neighbour's apron (q = p +- c lands outside its centre) while that apron is being
        // written by the same pass: undefined upstream, refused here
        set_error("center_size %u < border_size %u", m.center_size, m.border_size);
        return BT_ERR_UNSUPPORTED;
    }
    if ((uint64_t(m.texture_size) * m.pixel_size) % 4u) {
        set_error("texture row must be a whole number of 32-bit entries");
        return BT_ERR_UNSUPPORTED;
    }
    return BT_OK;
}

}  // namespace

extern "C" {

bt_status bt_preprocessor_create(bt_ctx* ctx, bt_preprocessor** out) {
    if (!ctx || !out) return BT_ERR_INVALID_ARGUMENT;
    *out = new bt_preprocessor();
    (*out)->ctx = ctx;
    return BT_OK;
}

void bt_preprocessor_destroy(bt_preprocessor* p) {
    if (!p) return;
    hipSetDevice(p->ctx->device);
    release_rasters(p);
    fused_release(p);
    for (hipEvent_t e : p->events) hipEventDestroy(e);
    for (hipEvent_t e : p->event_pool) hipEventDestroy(e);
    if (p->shard_local_done) hipEventDestroy(p->shard_local_done);
    if (p->shard_exchange_done) hipEventDestroy(p->shard_exchange_done);
    if (p->tasks_dev) hipFree(p->tasks_dev);
    if (p->rasters_dev) hipFree(p->rasters_dev);
    delete p;
}

bt_status bt_preprocessor_clear_attachment(bt_preprocessor* p, bt_atlas* a, uint32_t ai, const char* directory) {
    if (!p || !a || ai >= a->attachments.size()) return BT_ERR_INVALID_ARGUMENT;
    a->existing_tiles.clear();  // for ALL attachments, like :292; the slots (tile_states) stay assigned
    if (directory) {
        // reset_directory (preprocessor.rs:18-22)
        unlink((std::string(directory) + "/../../config.tc").c_str());
        remove_tree(directory);
        return make_dirs(directory);
    }
    return BT_OK;
}

// Preprocessor::preprocess_tile (preprocessor.rs:298-312)
bt_status bt_preprocessor_preprocess_tile(bt_preprocessor* p, bt_atlas* a, const bt_preprocess_dataset* d, const bt_raster* src) {
    if (!p || !a || !d) return BT_ERR_INVALID_ARGUMENT;
    if (bt_status s = check_dataset(a, d->attachment_index, d->lod_begin, d->lod_end)) return s;
    if (d->side >= 6u) {  // a cube has six sides (coordinate.rs:17-40: the side tables); a planar terrain uses side 0
        set_error("dataset side %u", d->side);
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (!(d->bottom_right[0] > d->top_left[0]) || !(d->bottom_right[1] > d->top_left[1])) {
        set_error("empty dataset rectangle");
        return BT_ERR_INVALID_ARGUMENT;
    }
    int32_t raster;
    if (bt_status s = add_raster(p, a, d->attachment_index, src, &raster)) return s;
    const uint32_t job = p->jobs++;
    p->compiled = false;
    p->saves_recorded = false;
    if (bt_status s = split_and_downsample(p, a, *d, raster, job)) return s;
    push_barrier(p, job);
    for (uint32_t lod = d->lod_begin; lod < d->lod_end; lod++)
        if (bt_status s = stitch_and_save_layer(p, a, *d, lod, job)) return s;
    return BT_OK;
}

// Preprocessor::preprocess_spherical (preprocessor.rs:314-343)
bt_status bt_preprocessor_preprocess_spherical(bt_preprocessor* p, bt_atlas* a, const bt_spherical_dataset* sd, const bt_raster sources[6]) {
    if (!p || !a || !sd || !sources) return BT_ERR_INVALID_ARGUMENT;
    if (bt_status s = check_dataset(a, sd->attachment_index, sd->lod_begin, sd->lod_end)) return s;
    const uint32_t job = p->jobs++;
    p->compiled = false;
    p->saves_recorded = false;
    bt_preprocess_dataset side[6];
    int32_t raster[6];
    for (uint32_t s = 0; s < 6; s++) {
        side[s] = {sd->attachment_index, s, {0.0f, 0.0f}, {1.0f, 1.0f}, sd->lod_begin, sd->lod_end};
        if (bt_status rc = add_raster(p, a, sd->attachment_index, &sources[s], &raster[s])) return rc;
    }
    for (uint32_t s = 0; s < 6; s++)
        if (bt_status rc = split_and_downsample(p, a, side[s], raster[s], job)) return rc;
    push_barrier(p, job);
    for (uint32_t lod = sd->lod_begin; lod < sd->lod_end; lod++)
        for (uint32_t s = 0; s < 6; s++)
            if (bt_status rc = stitch_and_save_layer(p, a, side[s], lod, job)) return rc;
    return BT_OK;
}

uint32_t bt_preprocessor_task_counts(const bt_preprocessor* p, uint32_t counts[5]) {
    if (!p) return 0;
    if (counts) {
        memset(counts, 0, 5 * sizeof(uint32_t));
        for (const Task& t : p->queue) counts[t.type]++;
    }
    return uint32_t(p->queue.size());
}

bt_status bt_preprocessor_save(bt_preprocessor* p, bt_atlas* a, const char* assets_root) {
    if (!p || !a || !assets_root) return BT_ERR_INVALID_ARGUMENT;
    // exactly the tiles of the Save tasks that have run (select_ready_tasks -> tile_atlas.save, preprocessor.rs:378-380)
    const std::string terrain = std::string(assets_root) + "/" + a->config.path;
    for (uint32_t ai = 0; ai < a->attachments.size(); ai++) {
        std::vector<std::pair<uint32_t, bt_tile_coordinate>> tiles;
        for (const AtlasTileAttachment& t : a->to_save) {
            if (t.attachment_index != ai || t.atlas_index == BT_INVALID_ATLAS_INDEX) continue;
            // after a distributed sharded run a rank writes its share only: the finest tiles it computed, and of the lower
            // LODs (complete on every rank) every world-th tile — each file has exactly one writer
            if (p->shard_world > 1 && p->shard_distributed && shard_holder(p, ai, t.coordinate.lod, t.atlas_index) != p->shard_rank) continue;
            tiles.push_back({t.atlas_index, t.coordinate});
        }
        if (tiles.empty()) continue;
        // AtlasAttachment::new: path = "assets/{path}/data/{name}" (tile_atlas.rs:175)
        const std::string dir = terrain + "/data/" + a->attachments[ai].cfg.name;
        if (bt_status s = save_tiles(a, ai, dir.c_str(), std::move(tiles))) return s;
    }
    a->to_save.clear();
    p->saves_recorded = false;
    if (p->shard_world > 1 && p->shard_distributed && p->shard_rank != 0) return BT_OK;  // config.tc: rank 0
    if (bt_status s = make_dirs(terrain)) return s;
    return bt_atlas_save_tile_config(a, (terrain + "/config.tc").c_str());
}

bt_status bt_preprocessor_last_run_stats(const bt_preprocessor* p, bt_run_stats* out) {
    if (!p || !out) return BT_ERR_INVALID_ARGUMENT;
    *out = p->stats;
    return BT_OK;
}

}  // extern "C"

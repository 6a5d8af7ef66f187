// Packed tiles, the host half (the format: PACKED TILES in the header; the kernels: bt_pack.hip): the bound and the validator, which need
// no device; bt_atlas_pack_tiles / bt_atlas_unpack_tiles; the "{coord}.btp" save and load paths; and bt_atlas_update's packed form.
// Every path works in chunks of at most kPackChunk tiles or 32 MiB of raw texels through the context's staging ring, and only packed
// bytes (with, on the way in, the strip offsets the validator has walked anyway) are copied between host and device.
#include <sys/stat.h>

#include <cstdio>
#include <cstring>

#include "bt_tile_io.hpp"

namespace bt {
namespace {

uint64_t pad8(uint64_t v) { return (v + 7u) & ~uint64_t(7); }

// The validator.  strip_off (optional): the offset of every strip's payload from the stream's first byte, appended
bt_status packed_check(const uint8_t* p, uint64_t size, uint32_t* format, uint32_t* texture_size, std::vector<uint64_t>* strip_off) {
    const char* who = "bt_packed_tile_check";
    if (size < 16u) {
        set_error("%s: %llu bytes, a stream has at least 16", who, (unsigned long long)size);
        return BT_ERR_IO;
    }
    if (memcmp(p, "BTP1", 4) != 0) {
        set_error("%s: the magic is not 'BTP1'", who);
        return BT_ERR_IO;
    }
    const uint32_t fmt = p[4], rows = p[5], T = uint32_t(p[6]) | uint32_t(p[7]) << 8;
    const uint64_t payload = uint64_t(p[8]) | uint64_t(p[9]) << 8 | uint64_t(p[10]) << 16 | uint64_t(p[11]) << 24;
    if (format) *format = fmt;
    if (texture_size) *texture_size = T;
    if (fmt != BT_FORMAT_R16 && fmt != BT_FORMAT_RGBA8) {
        set_error("%s: format %u is not R16 or Rgba8", who, fmt);
        return fmt == BT_FORMAT_RG16 || fmt == BT_FORMAT_RGB8 ? BT_ERR_UNSUPPORTED : BT_ERR_IO;
    }
    if (rows != BT_PACK_STRIP_ROWS) {
        set_error("%s: strips of %u rows, this version reads %u", who, rows, BT_PACK_STRIP_ROWS);
        return rows ? BT_ERR_UNSUPPORTED : BT_ERR_IO;
    }
    if (T == 0) {
        set_error("%s: texture_size 0", who);
        return BT_ERR_IO;
    }
    if (p[12] | p[13] | p[14] | p[15]) {
        set_error("%s: bytes 12-15 are not zero", who);
        return BT_ERR_IO;
    }
    const PackShape s = PackShape::of(fmt, T);
    if (size < s.head) {
        set_error("%s: %llu bytes do not hold the %u width bytes of a %u-texel tile", who, (unsigned long long)size, s.W, T);
        return BT_ERR_IO;
    }
    const uint8_t* widths = p + 16;
    const uint32_t per_strip = BT_PACK_STRIP_ROWS * s.planes * s.gpr;
    uint64_t words = 0;
    for (uint32_t i = 0; i < s.W; i++) {
        if (strip_off && i % per_strip == 0) strip_off->push_back(s.head + 8u * words);
        if (widths[i] > s.bits) {
            set_error("%s: width %u of group %u, a value has %u bits", who, widths[i], i, s.bits);
            return BT_ERR_IO;
        }
        words += widths[i];
    }
    for (uint32_t i = 16u + s.W; i < s.head; i++)
        if (p[i]) {
            set_error("%s: padding byte %u is not zero", who, i);
            return BT_ERR_IO;
        }
    if (payload != 8u * words) {
        set_error("%s: the payload field says %llu bytes, the widths add up to %llu", who, (unsigned long long)payload, (unsigned long long)(8u * words));
        return BT_ERR_IO;
    }
    if (size != s.head + payload) {
        set_error("%s: %llu bytes, header, widths and payload take %llu", who, (unsigned long long)size, (unsigned long long)(s.head + payload));
        return BT_ERR_IO;
    }
    return BT_OK;
}

// the attachment a packed call works on
bt_status pack_attachment(const char* who, const bt_atlas* a, uint32_t ai, PackShape* s) {
    if (ai >= a->attachments.size()) {
        set_error("%s: attachment %u of %zu", who, ai, a->attachments.size());
        return BT_ERR_INVALID_ARGUMENT;
    }
    const AttachmentMeta& m = a->attachments[ai].meta;
    const bool known = (m.format == BT_FORMAT_R16 || m.format == BT_FORMAT_RGBA8) && m.texture_size <= 65535u;
    if (known) *s = PackShape::of(m.format, m.texture_size);
    if (!known || s->bound() - s->head > 0xFFFFFFFFull) {  // (the payload field has 32 bits)
        set_error("%s: an attachment of format %u and texture_size %u cannot be packed", who, m.format, m.texture_size);
        return BT_ERR_UNSUPPORTED;
    }
    return BT_OK;
}

uint32_t chunk_tiles(const PackShape& s) { return uint32_t(std::max<uint64_t>(1, std::min<uint64_t>(kPackChunk, (32ull << 20) / s.tile_bytes))); }
// what a chunk needs of a staging buffer: the streams at their bound, and on the way in the two tables behind them
uint64_t chunk_staging(const PackShape& s) { return uint64_t(chunk_tiles(s)) * (s.bound() + 8u * (1u + s.strips)) + 16u; }

// the device scratch of a chunk: the streams, and behind them the strip offsets (u64) and the strip sizes (u32)
struct ChunkScratch {
    uint8_t* streams;
    uint64_t* strip_off;
    uint32_t* strip_bytes;
    uint64_t* starts;       // device, kPackChunk + 1
    uint64_t* starts_host;  // its pinned twin
};
bt_status chunk_scratch(bt_ctx* ctx, const PackShape& s, ChunkScratch* c) {
    const uint64_t n = uint64_t(chunk_tiles(s)) * s.strips;
    const uint64_t streams = align256(chunk_staging(s)), offs = align256(8u * n), sizes = align256(4u * n);
    if (bt_status st = ctx->pack.reserve(ctx, streams + offs + sizes)) return st;
    if (bt_status st = ctx->pack_words.reserve(ctx, 8u * (kPackChunk + 1u), true)) return st;
    c->streams = static_cast<uint8_t*>(ctx->pack.dev);
    c->strip_off = reinterpret_cast<uint64_t*>(c->streams + streams);
    c->strip_bytes = reinterpret_cast<uint32_t*>(c->streams + streams + offs);
    c->starts = static_cast<uint64_t*>(ctx->pack_words.dev);
    c->starts_host = static_cast<uint64_t*>(ctx->pack_words.host);
    return BT_OK;
}

// Packs `count` layers (at most a chunk) on the device; on return starts_host[0 .. count] are the streams' starts in the chunk's output.
// emit: the streams are written too.  to_ring >= 0: and copied into that staging buffer (which the caller has waited for).  Synchronous
bt_status pack_chunk(bt_atlas* a, uint32_t ai, const PackShape& s, const uint32_t* layers, uint32_t count, bool emit, int to_ring, const ChunkScratch& c) {
    const Attachment& at = a->attachments[ai];
    hipStream_t stream = a->ctx->stream;
    PackTiles tiles{};
    tiles.count = count;
    for (uint32_t i = 0; i < count; i++) tiles.layers[i] = layers[i];
    if (bt_status st = launch_pack_measure(stream, at.meta.format, s, at.level0, tiles, c.strip_bytes)) return st;
    if (bt_status st = launch_pack_scan(stream, s, count, c.strip_bytes, c.starts, c.strip_off)) return st;
    if (emit)
        if (bt_status st = launch_pack_emit(stream, at.meta.format, s, at.level0, tiles, c.starts, c.strip_off, c.streams)) return st;
    BT_HIP(hipMemcpyAsync(c.starts_host, c.starts, 8u * (count + 1u), hipMemcpyDeviceToHost, stream));
    BT_HIP(hipStreamSynchronize(stream));
    if (emit && to_ring >= 0) {
        StagingRing& ring = a->ctx->staging;
        const hipError_t e = hipMemcpyAsync(ring.buffer(uint32_t(to_ring)), c.streams, c.starts_host[count], hipMemcpyDeviceToHost, stream);
        const bt_status recorded = ring.record(uint32_t(to_ring), stream);
        if (e != hipSuccess) return hip_fail(e, "packed tile download");
        if (recorded) return recorded;
        return ring.wait(uint32_t(to_ring));
    }
    return BT_OK;
}

// Decodes a chunk whose validated streams lie in staging buffer k, stream i at starts[i], all below `extent` (a multiple of 8); strip_off:
// per stream and strip, from the buffer's first byte.  The two tables go behind the streams, ONE copy carries all of it, one launch
// decodes it; the buffer's event is recorded behind the launch
bt_status decode_chunk(bt_atlas* a, uint32_t ai, const PackShape& s, uint32_t k, const std::vector<uint32_t>& layers, const std::vector<uint64_t>& starts,
                       const std::vector<uint64_t>& strip_off, uint64_t extent, const ChunkScratch& c) {
    const Attachment& at = a->attachments[ai];
    StagingRing& ring = a->ctx->staging;
    hipStream_t stream = a->ctx->stream;
    uint8_t* pinned = static_cast<uint8_t*>(ring.buffer(k));
    const uint32_t count = uint32_t(layers.size());
    memcpy(pinned + extent, starts.data(), 8u * count);
    memcpy(pinned + extent + 8u * count, strip_off.data(), 8u * strip_off.size());
    const uint64_t total = extent + 8u * count + 8u * strip_off.size();
    PackTiles tiles{};
    tiles.count = count;
    for (uint32_t i = 0; i < count; i++) {
        tiles.layers[i] = layers[i];
        at.mark_written(layers[i], 1);
    }
    const hipError_t e = hipMemcpyAsync(c.streams, pinned, total, hipMemcpyHostToDevice, stream);
    bt_status launched_ok = BT_OK;
    if (e == hipSuccess)
        launched_ok = launch_pack_decode(stream, at.meta.format, s, at.level0, tiles, c.streams, reinterpret_cast<const uint64_t*>(c.streams + extent),
                                         reinterpret_cast<const uint64_t*>(c.streams + extent + 8u * count));
    const bt_status recorded = ring.record(k, stream);  // (behind a failed copy too)
    if (e != hipSuccess) return hip_fail(e, "packed tile upload");
    return launched_ok ? launched_ok : recorded;
}

// a stream that is valid and is one of this attachment's; *mismatch: valid, but of another format or size
bt_status check_for(const uint8_t* p, uint64_t size, const PackShape& s, uint32_t format, std::vector<uint64_t>* strip_off, bool* mismatch) {
    uint32_t fmt = 0, T = 0;
    *mismatch = false;
    const size_t before = strip_off ? strip_off->size() : 0;
    if (bt_status st = packed_check(p, size, &fmt, &T, strip_off)) {
        if (strip_off) strip_off->resize(before);
        return st;
    }
    if (fmt != format || T != s.T) {
        if (strip_off) strip_off->resize(before);
        *mismatch = true;
        set_error("a packed tile of format %u and texture_size %u for an attachment of format %u and texture_size %u", fmt, T, format, s.T);
        return BT_ERR_INVALID_ARGUMENT;
    }
    return BT_OK;
}

uint32_t held_layer(const bt_atlas* a, const bt_tile_coordinate& c) {
    if (is_invalid(c) || !a->existing_tiles.count(c)) return BT_INVALID_ATLAS_INDEX;
    const auto it = a->tile_states.find(c);
    return it != a->tile_states.end() && it->second.atlas_index < a->config.atlas_size ? it->second.atlas_index : BT_INVALID_ATLAS_INDEX;
}

std::string packed_path(const std::string& dir, const bt_tile_coordinate& c) {
    char name[64];
    bt_tile_name(c, name, sizeof name);
    return dir + "/" + name + ".btp";
}

}  // namespace

// bt_atlas_update under BT_TILE_FILES_PACKED: the batches of bt_atlas_update, each attachment's files of a batch read into staging buffer 0,
// checked, and decoded by one launch
bt_status update_packed(bt_atlas* a, const char* assets_root, uint32_t max_loads, uint32_t* loaded, uint32_t* failed) {
    BT_HIP(hipSetDevice(a->ctx->device));
    std::vector<PackShape> shapes(a->attachments.size());
    uint64_t largest = 0, staging = 32ull << 20;
    const PackShape* widest = nullptr;
    for (uint32_t ai = 0; ai < a->attachments.size(); ai++) {
        if (bt_status s = pack_attachment("bt_atlas_update", a, ai, &shapes[ai])) return s;
        if (!widest || chunk_staging(shapes[ai]) > chunk_staging(*widest)) widest = &shapes[ai];
        largest = std::max(largest, shapes[ai].tile_bytes);
        staging = std::max(staging, chunk_staging(shapes[ai]));
    }
    if (!widest) return BT_OK;
    const uint32_t chunk = uint32_t(std::max<uint64_t>(1, std::min<uint64_t>(kPackChunk, (32ull << 20) / std::max<uint64_t>(largest, 1))));
    StagingRing& ring = a->ctx->staging;
    if (bt_status s = ring.reserve(staging)) return s;
    ChunkScratch scratch{};
    for (const PackShape& s : shapes)  // (the scratch only grows: after the loop it holds every attachment's chunk)
        if (bt_status st = chunk_scratch(a->ctx, s, &scratch)) return st;
    std::vector<std::vector<uint32_t>> mip_layers(a->attachments.size());
    uint32_t budget = max_loads ? max_loads : 0xFFFFFFFFu, done = 0, bad = 0;
    bt_status rc = BT_OK;
    while (!a->to_load.empty() && budget && rc == BT_OK) {
        std::vector<AtlasTileAttachment> batch;
        while (!a->to_load.empty() && budget && batch.size() < chunk) {
            batch.push_back(a->to_load.front());
            a->to_load.pop_front();
            budget--;
        }
        std::vector<bool> ok(batch.size(), false);
        for (uint32_t ai = 0; ai < a->attachments.size() && rc == BT_OK; ai++) {
            const PackShape& s = shapes[ai];
            const Attachment& at = a->attachments[ai];
            const uint64_t bound = s.bound();
            std::vector<uint32_t> layers;
            std::vector<uint64_t> starts, strip_off;
            uint64_t extent = 0;
            if ((rc = ring.wait(0)) != BT_OK) break;
            uint8_t* pinned = static_cast<uint8_t*>(ring.buffer(0));
            for (size_t k = 0; k < batch.size(); k++) {
                const AtlasTileAttachment& t = batch[k];
                if (t.attachment_index != ai) continue;
                const std::string path = packed_path(std::string(assets_root) + "/" + a->config.path + "/data/" + at.cfg.name, t.coordinate);
                FILE* f = fopen(path.c_str(), "rb");
                if (!f) continue;  // the tile stays Loading, as with a missing `.bin`
                const size_t got = fread(pinned + extent, 1, bound, f);
                const bool longer = got == bound && fgetc(f) != EOF;
                fclose(f);
                bool mismatch;
                const size_t strips_before = strip_off.size();
                if (longer || check_for(pinned + extent, got, s, at.meta.format, &strip_off, &mismatch) != BT_OK) continue;
                for (size_t i = strips_before; i < strip_off.size(); i++) strip_off[i] += extent;
                ok[k] = true;
                layers.push_back(t.atlas_index);
                starts.push_back(extent);
                extent += got;  // (a valid stream's size is a multiple of 8)
            }
            if (!layers.empty()) rc = decode_chunk(a, ai, s, 0, layers, starts, strip_off, extent, scratch);
        }
        if (rc == BT_OK) rc = ring.wait(0);
        for (size_t k = 0; k < batch.size(); k++) {
            if (!ok[k]) {
                bad++;
                continue;
            }
            if (rc != BT_OK) continue;
            const AtlasTileAttachment& t = batch[k];
            // loaded_tile_attachment (:347-359); a slot that was reused for another tile meanwhile is ignored
            auto it = a->tile_states.find(t.coordinate);
            if (it == a->tile_states.end() || it->second.atlas_index != t.atlas_index || it->second.loading == 0) continue;
            if (--it->second.loading == 0) a->state_version++;
            mip_layers[t.attachment_index].push_back(t.atlas_index);
            done++;
        }
    }
    for (uint32_t ai = 0; ai < a->attachments.size() && rc == BT_OK; ai++) rc = mip_filled_layers(a, ai, mip_layers[ai]);
    if (loaded) *loaded = done;
    if (failed) *failed = bad;
    return rc;
}

}  // namespace bt

using namespace bt;

extern "C" {

bt_status bt_packed_tile_bound(uint32_t format, uint32_t texture_size, uint64_t* bytes) {
    if (!bytes) {
        set_error("bt_packed_tile_bound: NULL bytes");
        return BT_ERR_INVALID_ARGUMENT;
    }
    *bytes = 0;
    if (format == BT_FORMAT_RG16 || format == BT_FORMAT_RGB8) {
        set_error("bt_packed_tile_bound: format %u is not packed", format);
        return BT_ERR_UNSUPPORTED;
    }
    if ((format != BT_FORMAT_R16 && format != BT_FORMAT_RGBA8) || texture_size == 0 || texture_size > 65535u) {
        set_error("bt_packed_tile_bound: format %u, texture_size %u", format, texture_size);
        return BT_ERR_INVALID_ARGUMENT;
    }
    const PackShape s = PackShape::of(format, texture_size);
    *bytes = s.bound();
    return BT_OK;
}

bt_status bt_packed_tile_check(const void* bytes, uint64_t size, uint32_t* format, uint32_t* texture_size) {
    if (!bytes) {
        set_error("bt_packed_tile_check: NULL bytes");
        return BT_ERR_INVALID_ARGUMENT;
    }
    return packed_check(static_cast<const uint8_t*>(bytes), size, format, texture_size, nullptr);
}

bt_status bt_atlas_pack_tiles(bt_atlas* a, uint32_t ai, const uint32_t* layers, uint32_t count, void* dst_host, uint64_t dst_bytes, uint64_t* offsets) {
    if (!a || !offsets || (count && !layers)) {
        set_error("bt_atlas_pack_tiles: NULL %s", !a ? "atlas" : !offsets ? "offsets" : "layers");
        return BT_ERR_INVALID_ARGUMENT;
    }
    offsets[0] = 0;
    PackShape s;
    if (bt_status st = pack_attachment("bt_atlas_pack_tiles", a, ai, &s)) return st;
    for (uint32_t i = 0; i < count; i++)
        if (layers[i] >= a->config.atlas_size) {
            set_error("bt_atlas_pack_tiles: layer %u of %u", layers[i], a->config.atlas_size);
            return BT_ERR_INVALID_ARGUMENT;
        }
    if (!count) return BT_OK;
    BT_HIP(hipSetDevice(a->ctx->device));
    StagingRing& ring = a->ctx->staging;
    ChunkScratch scratch;
    if (bt_status st = chunk_scratch(a->ctx, s, &scratch)) return st;
    if (dst_host)
        if (bt_status st = ring.reserve(std::max<uint64_t>(32ull << 20, chunk_staging(s)))) return st;
    const uint32_t chunk = chunk_tiles(s);
    bool overflow = false;
    for (uint32_t lo = 0; lo < count; lo += chunk) {
        const uint32_t n = std::min(chunk, count - lo);
        const bool emit = dst_host && !overflow;
        if (emit)
            if (bt_status st = ring.wait(0)) return st;
        if (bt_status st = pack_chunk(a, ai, s, layers + lo, n, emit, emit ? 0 : -1, scratch)) return st;
        for (uint32_t i = 0; i < n; i++) offsets[lo + i + 1u] = offsets[lo] + scratch.starts_host[i + 1u];
        if (!emit) continue;
        if (offsets[lo + n] > dst_bytes)
            overflow = true;
        else
            memcpy(static_cast<uint8_t*>(dst_host) + offsets[lo], ring.buffer(0), scratch.starts_host[n]);
    }
    if (overflow) {
        set_error("bt_atlas_pack_tiles: the streams take %llu bytes, dst_host holds %llu", (unsigned long long)offsets[count], (unsigned long long)dst_bytes);
        return BT_ERR_OVERFLOW;
    }
    return BT_OK;
}

bt_status bt_atlas_unpack_tiles(bt_atlas* a, uint32_t ai, const uint32_t* layers, uint32_t count, const void* src_host, const uint64_t* offsets) {
    if (!a || (count && (!layers || !src_host || !offsets))) {
        set_error("bt_atlas_unpack_tiles: NULL %s", !a ? "atlas" : !layers ? "layers" : !src_host ? "src_host" : "offsets");
        return BT_ERR_INVALID_ARGUMENT;
    }
    PackShape s;
    if (bt_status st = pack_attachment("bt_atlas_unpack_tiles", a, ai, &s)) return st;
    if (!count) return BT_OK;
    const Attachment& at = a->attachments[ai];
    const uint8_t* src = static_cast<const uint8_t*>(src_host);
    // everything is refused before anything is touched
    std::vector<uint32_t> sorted(layers, layers + count);
    std::sort(sorted.begin(), sorted.end());
    for (uint32_t i = 0; i < count; i++) {
        if (sorted[i] >= a->config.atlas_size) {
            set_error("bt_atlas_unpack_tiles: layer %u of %u", sorted[i], a->config.atlas_size);
            return BT_ERR_INVALID_ARGUMENT;
        }
        if (i && sorted[i] == sorted[i - 1u]) {
            set_error("bt_atlas_unpack_tiles: layer %u is listed twice", sorted[i]);
            return BT_ERR_INVALID_ARGUMENT;
        }
        if (offsets[i + 1u] < offsets[i]) {
            set_error("bt_atlas_unpack_tiles: offsets[%u] is below offsets[%u]", i + 1u, i);
            return BT_ERR_INVALID_ARGUMENT;
        }
    }
    std::vector<uint64_t> strip_rel;  // per stream and strip, from the stream's first byte
    for (uint32_t i = 0; i < count; i++) {
        bool mismatch;
        if (bt_status st = check_for(src + offsets[i], offsets[i + 1u] - offsets[i], s, at.meta.format, &strip_rel, &mismatch)) return st;
    }
    BT_HIP(hipSetDevice(a->ctx->device));
    StagingRing& ring = a->ctx->staging;
    ChunkScratch scratch;
    if (bt_status st = chunk_scratch(a->ctx, s, &scratch)) return st;
    if (bt_status st = ring.reserve(std::max<uint64_t>(32ull << 20, chunk_staging(s)))) return st;
    const uint32_t chunk = chunk_tiles(s);
    bt_status rc = BT_OK;
    for (uint32_t lo = 0, c = 0; lo < count && rc == BT_OK; lo += chunk, c++) {
        const uint32_t n = std::min(chunk, count - lo), k = c % StagingRing::kBuffers;
        if ((rc = ring.wait(k)) != BT_OK) break;
        uint8_t* pinned = static_cast<uint8_t*>(ring.buffer(k));
        std::vector<uint32_t> chunk_layers(layers + lo, layers + lo + n);
        std::vector<uint64_t> starts, strip_off;
        uint64_t extent = 0;
        for (uint32_t i = 0; i < n; i++) {
            const uint64_t size = offsets[lo + i + 1u] - offsets[lo + i];
            memcpy(pinned + extent, src + offsets[lo + i], size);
            starts.push_back(extent);
            for (uint32_t t = 0; t < s.strips; t++) strip_off.push_back(extent + strip_rel[uint64_t(lo + i) * s.strips + t]);
            extent += size;
        }
        rc = decode_chunk(a, ai, s, k, chunk_layers, starts, strip_off, extent, scratch);
    }
    const bt_status drained = ring.drain();
    if (rc == BT_OK) rc = drained;
    if (rc != BT_OK) return rc;
    return mip_filled_layers(a, ai, sorted);
}

bt_status bt_atlas_save_tiles_packed(bt_atlas* a, uint32_t ai, const char* directory, const bt_tile_coordinate* coords, uint32_t count) {
    if (!a || !directory || (count && !coords)) {
        set_error("bt_atlas_save_tiles_packed: NULL %s", !a ? "atlas" : !directory ? "directory" : "coords");
        return BT_ERR_INVALID_ARGUMENT;
    }
    PackShape s;
    if (bt_status st = pack_attachment("bt_atlas_save_tiles_packed", a, ai, &s)) return st;
    TileSaver::Tiles tiles;
    if (!coords) {  // every existing tile that holds a slot, as bt_atlas_save_attachment
        for (const bt_tile_coordinate& c : a->existing_tiles)
            if (held_layer(a, c) != BT_INVALID_ATLAS_INDEX) tiles.push_back({held_layer(a, c), c});
    } else {
        for (uint32_t i = 0; i < count; i++) {
            const uint32_t layer = held_layer(a, coords[i]);
            if (layer == BT_INVALID_ATLAS_INDEX) {
                set_error("bt_atlas_save_tiles_packed: tile %u_%u_%u_%u is not in the atlas", coords[i].side, coords[i].lod, coords[i].x, coords[i].y);
                return BT_ERR_INVALID_ARGUMENT;
            }
            tiles.push_back({layer, coords[i]});
        }
    }
    if (bt_status st = make_dirs(directory)) return st;
    if (tiles.empty()) return BT_OK;
    std::sort(tiles.begin(), tiles.end(), [](const auto& l, const auto& r) { return l.first != r.first ? l.first < r.first : CoordLess()(l.second, r.second); });
    tiles.erase(std::unique(tiles.begin(), tiles.end(), [](const auto& l, const auto& r) { return l.first == r.first && operator_eq(l.second, r.second); }), tiles.end());
    BT_HIP(hipSetDevice(a->ctx->device));
    StagingRing& ring = a->ctx->staging;
    ChunkScratch scratch;
    if (bt_status st = chunk_scratch(a->ctx, s, &scratch)) return st;
    if (bt_status st = ring.reserve(std::max<uint64_t>(32ull << 20, chunk_staging(s)))) return st;
    const uint32_t chunk = chunk_tiles(s);
    bt_status rc = BT_OK;
    {
        FileWriters writers(ctx_io_threads(a->ctx), StagingRing::kBuffers);
        for (size_t lo = 0, c = 0; lo < tiles.size() && rc == BT_OK; lo += chunk, c++) {
            const uint32_t n = uint32_t(std::min<size_t>(chunk, tiles.size() - lo)), k = uint32_t(c % StagingRing::kBuffers);
            writers.wait_buffer(k);  // the files of the chunk that was here are written
            if ((rc = ring.wait(k)) != BT_OK) break;
            uint32_t layers[kPackChunk];
            for (uint32_t i = 0; i < n; i++) layers[i] = tiles[lo + i].first;
            if ((rc = pack_chunk(a, ai, s, layers, n, true, int(k), scratch)) != BT_OK) break;
            std::vector<FileWriters::Job> jobs;
            for (uint32_t i = 0; i < n; i++)
                jobs.push_back({packed_path(directory, tiles[lo + i].second), static_cast<const uint8_t*>(ring.buffer(k)) + scratch.starts_host[i],
                                size_t(scratch.starts_host[i + 1u] - scratch.starts_host[i]), k});
            writers.push(std::move(jobs));
        }
        for (uint32_t k = 0; k < StagingRing::kBuffers; k++) writers.wait_buffer(k);
        const bt_status written = writers.status();
        if (rc == BT_OK) rc = written;
    }
    return rc;
}

bt_status bt_atlas_load_tiles_packed(bt_atlas* a, uint32_t ai, const char* directory, const bt_tile_coordinate* coords, uint32_t count) {
    if (!a || !directory || (count && !coords)) {
        set_error("bt_atlas_load_tiles_packed: NULL %s", !a ? "atlas" : !directory ? "directory" : "coords");
        return BT_ERR_INVALID_ARGUMENT;
    }
    PackShape s;
    if (bt_status st = pack_attachment("bt_atlas_load_tiles_packed", a, ai, &s)) return st;
    const Attachment& at = a->attachments[ai];
    std::vector<bt_tile_coordinate> all;
    if (!coords) {
        for (const bt_tile_coordinate& c : a->existing_tiles) all.push_back(c);
        std::sort(all.begin(), all.end(), CoordLess());
        coords = all.data();
        count = uint32_t(all.size());
    }
    if (!count) return BT_OK;
    BT_HIP(hipSetDevice(a->ctx->device));
    constexpr uint32_t kBuffers = StagingRing::kBuffers;
    StagingRing& ring = a->ctx->staging;
    ChunkScratch scratch;
    if (bt_status st = chunk_scratch(a->ctx, s, &scratch)) return st;
    if (bt_status st = ring.reserve(std::max<uint64_t>(32ull << 20, chunk_staging(s)))) return st;
    const uint32_t chunk = chunk_tiles(s);
    const uint64_t bound = s.bound();
    std::vector<uint32_t> layers;
    bt_status rc = BT_OK;
    {
        // files -> the pinned buffers (reader threads, each file at the size the directory reports) -> one copy and one decode launch per
        // chunk on the context's stream: chunk c + 1 is read while chunk c is checked and decoded
        FileWriters readers(ctx_io_threads(a->ctx), kBuffers);
        const uint32_t chunks = (count + chunk - 1) / chunk;
        std::vector<std::vector<uint32_t>> index(kBuffers);
        std::vector<std::vector<uint64_t>> starts(kBuffers);
        std::vector<uint64_t> extents(kBuffers, 0);
        std::vector<uint32_t> firsts(kBuffers, 0);
        auto decode = [&](uint32_t c) -> bt_status {  // chunk c has been queued for reading: wait for its files, check them, enqueue its decode
            const uint32_t k = c % kBuffers;
            readers.wait_buffer(k);
            if (bt_status st = readers.status()) return st;
            const uint8_t* pinned = static_cast<const uint8_t*>(ring.buffer(k));
            std::vector<uint64_t> strip_off;
            for (size_t t = 0; t < index[k].size(); t++) {
                const uint64_t size = (t + 1 < starts[k].size() ? starts[k][t + 1] : extents[k]) - starts[k][t];
                bool mismatch;
                const size_t before = strip_off.size();
                if (check_for(pinned + starts[k][t], size, s, at.meta.format, &strip_off, &mismatch) != BT_OK) {
                    const std::string why = bt_last_error();
                    set_error("tile file %s: %s", packed_path(directory, coords[firsts[k] + t]).c_str(), why.c_str());
                    return BT_ERR_IO;
                }
                for (size_t i = before; i < strip_off.size(); i++) strip_off[i] += starts[k][t];
            }
            return decode_chunk(a, ai, s, k, index[k], starts[k], strip_off, extents[k], scratch);
        };
        for (uint32_t c = 0; c < chunks && rc == BT_OK; c++) {
            const uint32_t k = c % kBuffers, first = c * chunk, n = std::min(chunk, count - first);
            rc = ring.wait(k);  // the buffer's previous upload must have left it
            std::vector<FileWriters::Job> jobs;
            index[k].clear(), starts[k].clear(), extents[k] = 0, firsts[k] = first;
            for (uint32_t t = 0; t < n && rc == BT_OK; t++) {
                const std::string path = packed_path(directory, coords[first + t]);
                struct stat st;
                if (stat(path.c_str(), &st) != 0) {
                    set_error("tile file not found: %s", path.c_str());
                    rc = BT_ERR_IO;
                    break;
                }
                const uint64_t size = uint64_t(st.st_size);
                if (size < 16u || size > bound || size % 8u != 0) {
                    set_error("tile file %s: %llu bytes cannot be a packed tile of this attachment", path.c_str(), (unsigned long long)size);
                    rc = BT_ERR_IO;
                    break;
                }
                bt_atlas_tile tile;
                rc = bt_atlas_get_or_allocate_tile(a, coords[first + t], &tile);
                if (rc) break;
                index[k].push_back(tile.atlas_index);
                layers.push_back(tile.atlas_index);
                starts[k].push_back(extents[k]);
                FileWriters::Job job{path, static_cast<const uint8_t*>(ring.buffer(k)) + extents[k], size_t(size), k};
                job.read = true;
                jobs.push_back(std::move(job));
                extents[k] += size;
            }
            if (rc == BT_OK) readers.push(std::move(jobs));
            if (rc == BT_OK && c > 0) rc = decode(c - 1);
        }
        if (rc == BT_OK) rc = decode(chunks - 1);
        for (uint32_t k = 0; k < kBuffers; k++) readers.wait_buffer(k);  // (error paths: nobody may still write into the buffers)
        const bt_status drained = ring.drain();
        if (rc == BT_OK) rc = drained;
    }
    return rc ? rc : mip_filled_layers(a, ai, layers);
}

bt_status bt_atlas_set_tile_files(bt_atlas* a, uint32_t tile_files) {
    if (!a || (tile_files != BT_TILE_FILES_BIN && tile_files != BT_TILE_FILES_PACKED)) {
        set_error("bt_atlas_set_tile_files: %s", !a ? "NULL atlas" : "neither BT_TILE_FILES_BIN nor BT_TILE_FILES_PACKED");
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (tile_files == BT_TILE_FILES_PACKED)
        for (uint32_t ai = 0; ai < a->attachments.size(); ai++) {
            PackShape s;
            if (bt_status st = pack_attachment("bt_atlas_set_tile_files", a, ai, &s)) return st;
        }
    a->tile_files = tile_files;
    return BT_OK;
}

}  // extern "C"

// TileAtlas (tile_atlas.rs, gpu_tile_atlas.rs): the layers of every attachment in device memory, the tile states and the LRU of free
// slots, the tile config, upload / download of whole layers, the mip chain, and the queries that read layers directly (sample, tile
// bounds).  The tile files themselves are bt_tile_io.cpp's.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>

#include "bt_tile_io.hpp"

using namespace bt;

extern "C" {

bt_status bt_atlas_create(bt_ctx* ctx, const bt_terrain_config* config, bt_atlas** out) {
    if (!ctx || !config || !out) return BT_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (config->attachment_count > BT_MAX_ATTACHMENTS) {
        set_error("at most %u attachments", BT_MAX_ATTACHMENTS);
        return BT_ERR_INVALID_ARGUMENT;
    }
    BT_HIP(hipSetDevice(ctx->device));
    // everything is checked before anything is allocated, and the device memory comes before the host-side slot list: a nonsensical
    // atlas_size or mip_level_count is an error status, not gigabytes of host memory followed by one
    size_t free_bytes = 0, total_bytes = 0;
    BT_HIP(hipMemGetInfo(&free_bytes, &total_bytes));
    uint64_t wanted = 0;
    for (uint32_t i = 0; i < config->attachment_count; i++) {
        const bt_attachment_config& c = config->attachments[i];
        if (c.texture_size == 0 || c.texture_size > 65536u || c.border_size >= c.texture_size || 2 * c.border_size >= c.texture_size) {
            set_error("attachment %u: texture_size %u / border_size %u", i, c.texture_size, c.border_size);
            return BT_ERR_INVALID_ARGUMENT;
        }
        uint32_t most_mips = 1;
        while ((c.texture_size >> most_mips) != 0) most_mips++;
        if (c.mip_level_count > most_mips) {  // (wgpu refuses such a texture descriptor: gpu_tile_atlas.rs:233-252)
            set_error("attachment %u: mip_level_count %u, a %u-texel texture has at most %u", i, c.mip_level_count, c.texture_size, most_mips);
            return BT_ERR_INVALID_ARGUMENT;
        }
        const uint64_t tile_bytes = uint64_t(c.texture_size) * c.texture_size * (c.format == BT_FORMAT_R16 ? 2u : c.format == BT_FORMAT_RGB8 ? 3u : 4u);
        const bool fits = config->atlas_size <= uint64_t(total_bytes) / tile_bytes;  // (no product that could wrap)
        if (fits) wanted += tile_bytes * config->atlas_size;
        if (!fits || wanted > uint64_t(total_bytes)) {
            set_error("atlas of %u layers does not fit the device (%llu MiB)", config->atlas_size, (unsigned long long)(total_bytes >> 20));
            return BT_ERR_DEVICE;
        }
    }
    bt_atlas* a = new bt_atlas();
    static std::atomic<uint64_t> next_uid{1};
    a->uid = next_uid++;
    a->ctx = ctx;
    a->config = *config;
    for (uint32_t i = 0; i < config->attachment_count; i++) {
        const bt_attachment_config& c = config->attachments[i];
        Attachment at;
        at.cfg = c;
        // pixel sizes: terrain_data/mod.rs:77-84
        const uint32_t px = c.format == BT_FORMAT_R16 ? 2 : c.format == BT_FORMAT_RGB8 ? 3 : 4;
        at.meta = {c.format, c.texture_size, c.border_size, c.texture_size - 2 * c.border_size, config->atlas_size, px, c.texture_size};
        at.tile_bytes = uint64_t(c.texture_size) * c.texture_size * px;
        const size_t bytes = size_t(at.tile_bytes) * config->atlas_size;
        hipError_t e = hipMalloc(&at.level0, bytes ? bytes : 1);
        if (e == hipSuccess) e = hipMemsetAsync(at.level0, 0, bytes, ctx->stream);  // wgpu textures start zeroed
        if (e != hipSuccess) {
            bt_atlas_destroy(a);
            return hip_fail(e, "atlas allocation");
        }
        at.mips.assign(c.mip_level_count ? c.mip_level_count : 1, nullptr);
        at.written.assign(config->atlas_size, 0);
        a->attachments.push_back(at);
    }
    for (uint32_t i = 0; i < config->atlas_size; i++)  // tile_atlas.rs:307-309
        a->unused_tiles.push_back({{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, i, {0, 0, 0}});
    *out = a;
    return BT_OK;
}

void bt_atlas_destroy(bt_atlas* a) {
    if (!a) return;
    hipSetDevice(a->ctx->device);
    for (Attachment& at : a->attachments) {
        if (at.level0) hipFree(at.level0);
        for (void* m : at.mips)
            if (m) hipFree(m);
    }
    delete a;
}

// tile_atlas.rs:369-381.  (A tile that load_tile_config marked as existing but that was never requested has no
// TileState: the reference's `.unwrap()` panics there; here it reads as INVALID.)
bt_status bt_atlas_get_tile(bt_atlas* a, bt_tile_coordinate c, bt_atlas_tile* out) {
    if (!a || !out) return BT_ERR_INVALID_ARGUMENT;
    *out = {c, BT_INVALID_ATLAS_INDEX, {0, 0, 0}};
    if (is_invalid(c)) return BT_OK;
    if (!a->existing_tiles.count(c)) return BT_OK;
    auto it = a->tile_states.find(c);
    if (it != a->tile_states.end()) out->atlas_index = it->second.atlas_index;
    return BT_OK;
}

// allocate_tile (tile_atlas.rs:383-389): the oldest unused slot; whatever tile was cached in it is forgotten.
// DELIBERATE DEVIATION: called from request_tile the reference has already mem::take()n tile_states, so ITS
// `tile_states.remove(evicted)` is a no-op there and the evicted tile's stale TileState (an atlas_index that now belongs to
// another tile) survives until something overwrites it; get_best_tile / a re-request of the evicted tile then see it.
// Here the evicted tile's state is erased on every path — the sane behaviour the reference's own get_or_allocate path has;
// the oracle (oracle/bt_oracle_tree.c) encodes the same choice.
static bt_status allocate_tile(bt_atlas* a, uint32_t* atlas_index) {
    if (a->unused_tiles.empty()) {
        set_error("Atlas out of indices (atlas_size %u)", a->config.atlas_size);
        return BT_ERR_ATLAS_OUT_OF_INDICES;
    }
    const bt_atlas_tile unused = a->unused_tiles.front();
    a->unused_tiles.pop_front();
    a->tile_states.erase(unused.coordinate);
    a->state_version++;
    *atlas_index = unused.atlas_index;
    return BT_OK;
}

// tile_atlas.rs:391-416
bt_status bt_atlas_get_or_allocate_tile(bt_atlas* a, bt_tile_coordinate c, bt_atlas_tile* out) {
    if (!a || !out) return BT_ERR_INVALID_ARGUMENT;
    *out = {c, BT_INVALID_ATLAS_INDEX, {0, 0, 0}};
    if (is_invalid(c)) return BT_OK;
    auto it = a->tile_states.find(c);
    if (it == a->tile_states.end()) {
        uint32_t index;
        if (bt_status s = allocate_tile(a, &index)) return s;
        it = a->tile_states.emplace(c, TileState{index, 1, 0}).first;
    }
    a->existing_tiles.insert(c);
    out->atlas_index = it->second.atlas_index;
    return BT_OK;
}

// tile_atlas.rs:418-457
bt_status bt_atlas_request_tile(bt_atlas* a, bt_tile_coordinate c) {
    if (!a) return BT_ERR_INVALID_ARGUMENT;
    if (!a->existing_tiles.count(c)) return BT_OK;
    auto it = a->tile_states.find(c);
    if (it != a->tile_states.end()) {
        if (it->second.requests == 0) {  // the tile is used again: take its slot out of the LRU
            const uint32_t index = it->second.atlas_index;
            a->unused_tiles.erase(std::remove_if(a->unused_tiles.begin(), a->unused_tiles.end(),
                                                 [index](const bt_atlas_tile& t) { return t.atlas_index == index; }),
                                  a->unused_tiles.end());
        }
        it->second.requests++;
        return BT_OK;
    }
    uint32_t index;
    if (bt_status s = allocate_tile(a, &index)) return s;
    const uint32_t attachments = uint32_t(a->attachments.size());
    a->tile_states.emplace(c, TileState{index, 1, attachments});
    a->state_version++;
    for (uint32_t ai = 0; ai < attachments; ai++) a->to_load.push_back({c, index, ai});
    if (attachments == 0) a->tile_states[c].loading = 0;  // (Loading(0) never completes upstream; nothing to load here)
    return BT_OK;
}

// tile_atlas.rs:459-476
bt_status bt_atlas_release_tile(bt_atlas* a, bt_tile_coordinate c) {
    if (!a) return BT_ERR_INVALID_ARGUMENT;
    if (!a->existing_tiles.count(c)) return BT_OK;
    auto it = a->tile_states.find(c);
    if (it == a->tile_states.end() || it->second.requests == 0) {
        set_error("Tried releasing a tile, which is not present.");  // the reference panics (:467)
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (--it->second.requests == 0) a->unused_tiles.push_back({c, it->second.atlas_index, {0, 0, 0}});
    return BT_OK;
}

// tile_atlas.rs:478-503
bt_status bt_atlas_get_best_tile(const bt_atlas* a, bt_tile_coordinate c, bt_tile_tree_entry* out) {
    if (!a || !out) return BT_ERR_INVALID_ARGUMENT;
    *out = {BT_INVALID_ATLAS_INDEX, BT_INVALID_LOD};
    while (!is_invalid(c) && c.lod != BT_INVALID_LOD) {
        auto it = a->tile_states.find(c);
        if (it != a->tile_states.end() && it->second.loading == 0) {
            *out = {it->second.atlas_index, c.lod};
            return BT_OK;
        }
        c = bt_tile_parent(c);  // lod 0 -> lod - 1 wraps to INVALID_LOD, like the reference's u32 arithmetic
    }
    return BT_OK;
}

uint32_t bt_atlas_tiles(const bt_atlas* a, bt_tile_coordinate* coords, uint32_t* idx, uint32_t cap) {
    if (!a) return 0;
    std::vector<std::pair<uint32_t, bt_tile_coordinate>> v;
    v.reserve(a->existing_tiles.size());
    for (const bt_tile_coordinate& c : a->existing_tiles) {
        auto it = a->tile_states.find(c);
        v.push_back({it != a->tile_states.end() ? it->second.atlas_index : BT_INVALID_ATLAS_INDEX, c});
    }
    std::sort(v.begin(), v.end(), [](const auto& l, const auto& r) {
        if (l.first != r.first) return l.first < r.first;
        return CoordLess()(l.second, r.second);
    });
    for (uint32_t i = 0; i < v.size() && i < cap; i++) {
        if (coords) coords[i] = v[i].second;
        if (idx) idx[i] = v[i].first;
    }
    return uint32_t(v.size());
}

bt_status bt_atlas_attachment_storage(const bt_atlas* a, uint32_t ai, void** ptr, uint64_t* tile_bytes, uint32_t* layers) {
    if (!a || ai >= a->attachments.size()) return BT_ERR_INVALID_ARGUMENT;
    if (ptr) {
        *ptr = a->attachments[ai].level0;
        // the caller may write through this pointer (a host-side collective does): no layer counts as "still zero since bt_atlas_create" any more
        const Attachment& at = a->attachments[ai];
        at.mark_written(0, uint32_t(at.written.size()));
    }
    if (tile_bytes) *tile_bytes = a->attachments[ai].tile_bytes;
    if (layers) *layers = a->config.atlas_size;
    return BT_OK;
}

bt_status bt_atlas_download_tiles(bt_atlas* a, uint32_t ai, uint32_t first, uint32_t count, void* dst, uint64_t dst_bytes) {
    if (!a || ai >= a->attachments.size() || !dst) return BT_ERR_INVALID_ARGUMENT;
    const Attachment& at = a->attachments[ai];
    if (uint64_t(first) + count > a->config.atlas_size || dst_bytes < at.tile_bytes * count) {
        set_error("download range/size");
        return BT_ERR_INVALID_ARGUMENT;
    }
    BT_HIP(hipMemcpyAsync(dst, (const uint8_t*)at.level0 + at.tile_bytes * first, at.tile_bytes * count,
                          hipMemcpyDeviceToHost, a->ctx->stream));
    BT_HIP(hipStreamSynchronize(a->ctx->stream));
    return BT_OK;
}

bt_status bt_atlas_upload_tile(bt_atlas* a, uint32_t ai, uint32_t layer, const void* src, uint64_t src_bytes) {
    if (!a || ai >= a->attachments.size() || !src) return BT_ERR_INVALID_ARGUMENT;
    const Attachment& at = a->attachments[ai];
    if (layer >= a->config.atlas_size || src_bytes != at.tile_bytes) return BT_ERR_INVALID_ARGUMENT;
    a->attachments[ai].mark_written(layer, 1);
    BT_HIP(hipMemcpyAsync((uint8_t*)at.level0 + at.tile_bytes * layer, src, src_bytes, hipMemcpyHostToDevice, a->ctx->stream));
    BT_HIP(hipStreamSynchronize(a->ctx->stream));
    return BT_OK;
}

// every existing tile that holds a slot (a tile known only from load_tile_config has no data to write)
bt_status bt_atlas_save_attachment(bt_atlas* a, uint32_t ai, const char* directory) {
    if (!a || ai >= a->attachments.size() || !directory) return BT_ERR_INVALID_ARGUMENT;
    std::vector<std::pair<uint32_t, bt_tile_coordinate>> tiles;
    for (const bt_tile_coordinate& c : a->existing_tiles) {
        auto it = a->tile_states.find(c);
        if (it != a->tile_states.end() && it->second.atlas_index != BT_INVALID_ATLAS_INDEX) tiles.push_back({it->second.atlas_index, c});
    }
    return save_tiles(a, ai, directory, std::move(tiles));
}

bt_status bt_atlas_save_tile_config(const bt_atlas* a, const char* file_path) {
    if (!a || !file_path) return BT_ERR_INVALID_ARGUMENT;
    std::vector<bt_tile_coordinate> coords(a->existing_tiles.begin(), a->existing_tiles.end());
    // the reference writes HashSet iteration order (tile_atlas.rs:605-609); sorted here, compare as a set
    std::sort(coords.begin(), coords.end(), CoordLess());
    std::vector<uint8_t> buf(bt_tc_encode(coords.data(), uint32_t(coords.size()), nullptr, 0));
    bt_tc_encode(coords.data(), uint32_t(coords.size()), buf.data(), buf.size());
    return write_file(file_path, buf.data(), buf.size());
}

bt_status bt_atlas_load_tile_config(bt_atlas* a, const char* file_path) {
    if (!a || !file_path) return BT_ERR_INVALID_ARGUMENT;
    FILE* f = fopen(file_path, "rb");
    if (!f) {
        set_error("Tile config not found: %s", file_path);  // tile_atlas.rs:620
        return BT_ERR_IO;
    }
    std::vector<uint8_t> buf;
    uint8_t tmp[65536];
    size_t r;
    while ((r = fread(tmp, 1, sizeof tmp, f)) > 0) buf.insert(buf.end(), tmp, tmp + r);
    fclose(f);
    const int64_t n = bt_tc_decode(buf.data(), buf.size(), nullptr, 0);
    if (n < 0) {
        set_error("malformed tile config %s", file_path);
        return BT_ERR_IO;
    }
    std::vector<bt_tile_coordinate> coords(size_t(n) ? size_t(n) : 1);
    bt_tc_decode(buf.data(), buf.size(), coords.data(), uint32_t(n));
    // existing_tiles only: a tile gets an atlas index when it is requested or preprocessed
    for (int64_t i = 0; i < n; i++) a->existing_tiles.insert(coords[i]);
    return BT_OK;
}

// ------------------------------------------------------------------------------------- mip chain

static uint32_t mip_pixel_size(uint32_t format) { return format == BT_FORMAT_R16 ? 2 : 4; }

bt_status bt_generate_mipmaps(bt_ctx* ctx, uint32_t format, uint32_t T, uint32_t levels, const void* level0, void* out,
                              uint64_t out_bytes) {
    if (!ctx || !level0 || !out || levels == 0) return BT_ERR_INVALID_ARGUMENT;
    if (format != BT_FORMAT_R16 && format != BT_FORMAT_RGBA8) {
        set_error("generate_mipmaps: format %u is a no-op in the reference (terrain_data/mod.rs:211-213)", format);
        return BT_ERR_UNSUPPORTED;
    }
    const uint32_t px = mip_pixel_size(format);
    uint64_t total = 0;
    for (uint32_t k = 0; k < levels; k++) total += uint64_t(T >> k) * (T >> k) * px;
    if (out_bytes < total) return BT_ERR_INVALID_ARGUMENT;
    BT_HIP(hipSetDevice(ctx->device));
    uint8_t* dev = nullptr;
    BT_HIP(hipMalloc((void**)&dev, total));
    bt_status rc = BT_OK;
    hipError_t e = hipMemcpyAsync(dev, level0, uint64_t(T) * T * px, hipMemcpyHostToDevice, ctx->stream);
    uint64_t off = 0;
    uint32_t size = T;
    for (uint32_t k = 1; k < levels && e == hipSuccess && rc == BT_OK; k++) {
        const uint64_t next = off + uint64_t(size) * size * px;
        rc = launch_mip_level(ctx, format, dev + off, dev + next, size, 1);
        off = next;
        size >>= 1;
    }
    if (e == hipSuccess && rc == BT_OK) e = hipMemcpyAsync(out, dev, total, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && rc == BT_OK) e = hipStreamSynchronize(ctx->stream);
    hipFree(dev);
    if (e != hipSuccess) return hip_fail(e, "bt_generate_mipmaps");
    return rc;
}

bt_status bt_atlas_generate_mipmaps(bt_atlas* a, uint32_t ai, uint32_t first, uint32_t count) {
    if (!a || ai >= a->attachments.size()) return BT_ERR_INVALID_ARGUMENT;
    Attachment& at = a->attachments[ai];
    if (at.meta.format != BT_FORMAT_R16 && at.meta.format != BT_FORMAT_RGBA8) return BT_ERR_UNSUPPORTED;
    if (uint64_t(first) + count > a->config.atlas_size) return BT_ERR_INVALID_ARGUMENT;
    BT_HIP(hipSetDevice(a->ctx->device));
    const uint32_t px = at.meta.pixel_size;
    uint32_t size = at.meta.texture_size;
    const uint8_t* parent = (const uint8_t*)at.level0 + at.tile_bytes * first;
    for (uint32_t k = 1; k < at.mips.size(); k++) {
        const uint32_t child = size >> 1;
        const uint64_t child_tile = uint64_t(child) * child * px;
        if (!at.mips[k]) {
            BT_HIP(hipMalloc(&at.mips[k], child_tile * a->config.atlas_size ? child_tile * a->config.atlas_size : 1));
            BT_HIP(hipMemsetAsync(at.mips[k], 0, child_tile * a->config.atlas_size, a->ctx->stream));
        }
        uint8_t* dst = (uint8_t*)at.mips[k] + child_tile * first;
        if (bt_status s = launch_mip_level(a->ctx, at.meta.format, parent, dst, size, count)) return s;
        parent = dst;
        size = child;
    }
    return BT_OK;
}

bt_status bt_atlas_sample(bt_atlas* a, uint32_t ai, const bt_tile_lookup* lookups, uint32_t count, float* out) {
    if (!a || ai >= a->attachments.size() || (count && (!lookups || !out))) return BT_ERR_INVALID_ARGUMENT;
    const Attachment& at = a->attachments[ai];
    if (at.meta.format != BT_FORMAT_R16 && at.meta.format != BT_FORMAT_RGBA8) return BT_ERR_UNSUPPORTED;
    if (!count) return BT_OK;
    BT_HIP(hipSetDevice(a->ctx->device));
    void* dev = nullptr;
    const size_t in_bytes = sizeof(bt_tile_lookup) * size_t(count), out_bytes = 16 * size_t(count);
    BT_HIP(hipMalloc(&dev, in_bytes + out_bytes));
    hipError_t e = hipMemcpyAsync(dev, lookups, in_bytes, hipMemcpyHostToDevice, a->ctx->stream);
    bt_status rc = BT_OK;
    if (e == hipSuccess) rc = launch_sample(a->ctx, at.meta, at.level0, (const bt_tile_lookup*)dev, count, (float*)((uint8_t*)dev + in_bytes));
    if (e == hipSuccess && rc == BT_OK) e = hipMemcpyAsync(out, (uint8_t*)dev + in_bytes, out_bytes, hipMemcpyDeviceToHost, a->ctx->stream);
    if (e == hipSuccess && rc == BT_OK) e = hipStreamSynchronize(a->ctx->stream);
    hipFree(dev);
    if (e != hipSuccess) return hip_fail(e, "bt_atlas_sample");
    return rc;
}

bt_status bt_atlas_tile_bounds(bt_atlas* a, uint32_t ai, const uint32_t* layers, uint32_t count, uint32_t grid, uint32_t flags, uint16_t* out,
                               uint64_t out_bytes) {
    if (!a || ai >= a->attachments.size()) {
        set_error("bt_atlas_tile_bounds: %s", a ? "attachment index out of range" : "NULL atlas");
        return BT_ERR_INVALID_ARGUMENT;
    }
    const Attachment& at = a->attachments[ai];
    if (at.meta.format != BT_FORMAT_R16) {
        set_error("bt_atlas_tile_bounds: attachment %u is not R16", ai);
        return BT_ERR_UNSUPPORTED;
    }
    const uint32_t T = at.meta.texture_size;
    if (grid == 0 || (grid & (grid - 1u)) || grid > BT_BOUNDS_MAX_GRID || T % grid) {
        set_error("bt_atlas_tile_bounds: grid %u (a power of two up to %u dividing the texture size %u)", grid, unsigned(BT_BOUNDS_MAX_GRID), T);
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (flags & ~uint32_t(BT_BOUNDS_SKIP_ZERO)) {
        set_error("bt_atlas_tile_bounds: unknown flags 0x%x", flags);
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (!count) return BT_OK;
    const uint64_t cells = (4ull * grid * grid - 1u) / 3u;
    if (!out || out_bytes < uint64_t(count) * cells * 4u) {
        set_error("bt_atlas_tile_bounds: %s", out ? "out_bytes below count * (4 g^2 - 1) / 3 * 4" : "NULL out_host");
        return BT_ERR_INVALID_ARGUMENT;
    }
    for (uint32_t i = 0; layers && i < count; i++)
        if (layers[i] >= a->config.atlas_size) {
            set_error("bt_atlas_tile_bounds: layers[%u] = %u, the atlas has %u", i, layers[i], a->config.atlas_size);
            return BT_ERR_INVALID_ARGUMENT;
        }
    if (!layers && count > a->config.atlas_size) {
        set_error("bt_atlas_tile_bounds: %u layers, the atlas has %u", count, a->config.atlas_size);
        return BT_ERR_INVALID_ARGUMENT;
    }
    // chunks of layers whose list + pyramids fit 32 MiB (the 16k job's 1365 layers at grid 64 are one chunk)
    bt_ctx* ctx = a->ctx;
    const uint32_t chunk = uint32_t(std::min<uint64_t>(count, std::max<uint64_t>(1u, (32ull << 20) / (cells * 4u + 4u))));
    const uint64_t list_bytes = (uint64_t(chunk) * 4u + 255u) & ~255ull, need = list_bytes + uint64_t(chunk) * cells * 4u;
    BT_HIP(hipSetDevice(ctx->device));
    if (bt_status s = ctx->bounds.reserve(ctx, need, true)) return s;
    uint32_t* list = (uint32_t*)ctx->bounds.host;
    uint8_t* dev = (uint8_t*)ctx->bounds.dev;
    for (uint32_t first = 0; first < count; first += chunk) {
        const uint32_t n = std::min(chunk, count - first);
        for (uint32_t i = 0; i < n; i++) list[i] = layers ? layers[first + i] : first + i;
        BT_HIP(hipMemcpyAsync(dev, list, n * 4ull, hipMemcpyHostToDevice, ctx->stream));
        if (bt_status s = launch_tile_bounds(ctx->stream, at.level0, T, (const uint32_t*)dev, n, grid, flags & BT_BOUNDS_SKIP_ZERO,
                                             (uint32_t*)(dev + list_bytes)))
            return s;
        BT_HIP(hipMemcpyAsync((uint8_t*)ctx->bounds.host + list_bytes, dev + list_bytes, n * cells * 4u, hipMemcpyDeviceToHost, ctx->stream));
        BT_HIP(hipStreamSynchronize(ctx->stream));
        memcpy(out + uint64_t(first) * cells * 2u, (const uint8_t*)ctx->bounds.host + list_bytes, n * cells * 4u);
    }
    return BT_OK;  // a read: Attachment::written stays as it is
}

bt_status bt_atlas_mip_storage(const bt_atlas* a, uint32_t ai, uint32_t level, void** ptr, uint64_t* tile_bytes) {
    if (!a || ai >= a->attachments.size() || level >= a->attachments[ai].mips.size()) return BT_ERR_INVALID_ARGUMENT;
    const Attachment& at = a->attachments[ai];
    const uint32_t s = at.meta.texture_size >> level;
    if (ptr) *ptr = level == 0 ? at.level0 : at.mips[level];
    if (ptr && level == 0) at.mark_written(0, uint32_t(at.written.size()));  // level 0 is attachment_storage's pointer: the same rule
    if (tile_bytes) *tile_bytes = uint64_t(s) * s * at.meta.pixel_size;
    return BT_OK;
}

bt_status bt_synth_fbm_r16(bt_ctx* ctx, void* dst, uint32_t w, uint32_t h, uint64_t pitch, uint32_t x0, uint32_t y0,
                           uint32_t base_cell, uint32_t octaves, uint32_t seed) {
    if (!ctx || !dst || !w || !h || !base_cell || !octaves || octaves > 16) return BT_ERR_INVALID_ARGUMENT;
    BT_HIP(hipSetDevice(ctx->device));
    return launch_synth_fbm(ctx, dst, w, h, pitch ? pitch : uint64_t(w) * 2, x0, y0, base_cell, octaves, seed);
}

}  // extern "C"

// bt_height_bounds on the host: create / destroy / read / write of the table, its definition (bt_height_bounds_build, computed here from
// the grid-1 bounds of the held layers), and the plan of bt_height_bounds_update, whose result must stay byte-identical to a build's.  The
// update's kernels, and the account of what an update has to touch, are bt_bounds_update.hip's.
#include <cstring>
#include <unordered_set>

#include "bt_height_bounds.hpp"

using namespace bt;

namespace {

// what build and update (`who`) refuse first
bt_status check_table(const char* who, const bt_height_bounds* b, const bt_atlas* a, uint32_t ai) {
    if (!b || !a || ai >= a->attachments.size()) {
        set_error("%s: %s", who, !b ? "NULL table" : !a ? "NULL atlas" : "attachment index out of range");
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (a->attachments[ai].meta.format != BT_FORMAT_R16) {
        set_error("%s: attachment %u is not R16", who, ai);
        return BT_ERR_UNSUPPORTED;
    }
    if (b->ctx != a->ctx || b->sides != (a->config.spherical ? 6u : 1u)) {
        set_error("%s: %s", who, b->ctx != a->ctx ? "table and atlas belong to different contexts" : "the atlas's side count is not the table's");
        return BT_ERR_INVALID_ARGUMENT;
    }
    return BT_OK;
}

// the table index of a tile of the table's levels
uint32_t slot(const bt_height_bounds* b, const bt_tile_coordinate& c) {
    return uint32_t(height_bounds_offset(b->sides, c.lod) + ((((uint64_t(c.side) << c.lod) + c.y) << c.lod) + c.x));
}

bool held_layer(const bt_atlas* a, const bt_tile_coordinate& c, uint32_t* layer) {  // "the atlas holds the tile": existing and loaded
    if (!a->existing_tiles.count(c)) return false;
    const auto it = a->tile_states.find(c);
    if (it == a->tile_states.end() || it->second.loading != 0) return false;
    *layer = it->second.atlas_index;
    return true;
}

bt_status check_update(bt_height_bounds* b, const bt_atlas* a, uint32_t ai, const bt_tile_coordinate* tiles, uint32_t count) {
    if (bt_status s = check_table("bt_height_bounds_update", b, a, ai)) return s;
    HeightBoundsImpl* impl = bounds_impl(b);
    if (!impl->current || impl->atlas_uid != a->uid || impl->attachment != ai) {
        set_error("bt_height_bounds_update: the table is not current for this atlas and attachment (%s): build first",
                  impl->current ? "last built against another" : "never built, or written since");
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (count && !tiles) {
        set_error("bt_height_bounds_update: NULL tiles with count %u", count);
        return BT_ERR_INVALID_ARGUMENT;
    }
    for (uint32_t i = 0; i < count; i++) {
        const bt_tile_coordinate& c = tiles[i];
        if (c.side >= b->sides || (c.lod < 32u && ((c.x >> c.lod) || (c.y >> c.lod)))) {
            set_error("bt_height_bounds_update: tiles[%u] = %u_%u_%u_%u is not a tile of %u side(s)", i, c.side, c.lod, c.x, c.y, b->sides);
            return BT_ERR_INVALID_ARGUMENT;
        }
    }
    return BT_OK;
}

// the host plan: index arithmetic, no HIP call
struct UpdatePlan {
    std::vector<uint32_t> layers;  // the held tiles of U: the layers whose own range is reduced
    std::vector<Scatter> scatter;  // U
    std::vector<Window> windows;   // level by level
    uint32_t level_window[kMaxLevels + 1] = {}, level_work[kMaxLevels + 1] = {};  // BoundsUpdateArgs'
    uint64_t total = 0;            // affected entries
};

bt_status plan_update(const bt_height_bounds* b, const bt_atlas* a, const bt_tile_coordinate* tiles, uint32_t count, UpdatePlan& plan) {
    const uint32_t levels = b->levels;
    typedef std::unordered_set<bt_tile_coordinate, CoordHash, CoordEq> TileSet;
    TileSet listed, roots;
    std::vector<bt_tile_coordinate> singles;  // U and its ancestors, each once
    for (uint32_t i = 0; i < count; i++) {
        const bt_tile_coordinate& c = tiles[i];
        if (c.lod >= levels || !listed.insert(c).second) continue;
        uint32_t layer = 0;
        if (held_layer(a, c, &layer)) {
            if (layer >= a->config.atlas_size) {
                set_error("bt_height_bounds_update: tile %u_%u_%u_%u has atlas index %u, the atlas has %u layers", c.side, c.lod, c.x, c.y, layer, a->config.atlas_size);
                return BT_ERR_INVALID_ARGUMENT;
            }
            plan.scatter.push_back({slot(b, c), uint32_t(plan.layers.size())});
            plan.layers.push_back(layer);
        } else {
            plan.scatter.push_back({slot(b, c), kNoSource});
        }
    }
    if (plan.scatter.empty()) return BT_OK;
    TileSet seen = listed;
    for (const bt_tile_coordinate& u : listed) {
        singles.push_back(u);
        for (bt_tile_coordinate p = u; p.lod > 0u;) {
            p = {p.side, p.lod - 1u, p.x >> 1, p.y >> 1};
            if (!seen.insert(p).second) break;  // the rest of the chain is there already
            singles.push_back(p);
        }
        for (uint32_t k = 0; k < 4u && u.lod + 1u < levels; k++) {
            const bt_tile_coordinate child = {u.side, u.lod + 1u, 2u * u.x + (k & 1u), 2u * u.y + (k >> 1)};
            uint32_t layer;
            if (!held_layer(a, child, &layer)) roots.insert(child);
        }
    }
    // one writer per entry: whatever lies inside another fill root's subtree is left to that root's windows
    auto covered = [&](bt_tile_coordinate c, bool self) {
        if (self && roots.count(c)) return true;
        while (c.lod > 0u) {
            c = {c.side, c.lod - 1u, c.x >> 1, c.y >> 1};
            if (roots.count(c)) return true;
        }
        return false;
    };
    std::vector<std::vector<Window>> level_windows(levels);
    if (!roots.empty())
        singles.erase(std::remove_if(singles.begin(), singles.end(), [&](const bt_tile_coordinate& c) { return covered(c, true); }), singles.end());
    for (const bt_tile_coordinate& c : singles) level_windows[c.lod].push_back({c.side, c.x, c.y, 0u});
    for (const bt_tile_coordinate& c : roots) {
        if (covered(c, false)) continue;
        for (uint32_t l = c.lod; l < levels; l++) level_windows[l].push_back({c.side | ((l - c.lod) << 8), c.x << (l - c.lod), c.y << (l - c.lod), 0u});
    }
    for (uint32_t l = 0; l < levels; l++) {
        plan.level_window[l] = uint32_t(plan.windows.size());
        plan.level_work[l] = uint32_t(plan.total);
        uint64_t first = 0;
        for (Window w : level_windows[l]) {
            w.first = uint32_t(first);
            first += 1ull << (2u * (w.side_shift >> 8));
            plan.windows.push_back(w);
        }
        plan.total += first;
    }
    plan.level_window[levels] = uint32_t(plan.windows.size());
    plan.level_work[levels] = uint32_t(plan.total);  // (distinct entries: at most b->entries < 2^24)
    return BT_OK;
}

// the plan's records -> the context's ring, the reduced ranges behind them (device only); then the launches
bt_status run_update(bt_height_bounds* b, const bt_atlas* a, const Attachment& at, const UpdatePlan& plan, bt_bounds_update_stats* stats) {
    bt_ctx* ctx = a->ctx;
    HeightBoundsImpl* impl = bounds_impl(b);
    BT_HIP(hipSetDevice(ctx->device));
    PlanRing ring;
    const uint64_t layers_at = ring.add(plan.layers), scatter_at = ring.add(plan.scatter), windows_at = ring.add(plan.windows);
    const uint64_t own_at = ring.device_only(plan.layers.size() * 4u);
    uint8_t* dev = nullptr;
    impl->current = false;  // until everything below is queued
    if (bt_status s = ring.commit(ctx, &dev)) return s;
    BoundsUpdateArgs args{};
    args.table = b->table;
    args.shadow = impl->shadow;
    args.own = (const uint32_t*)(dev + own_at);
    args.scatter = (const Scatter*)(dev + scatter_at);
    args.windows = (const Window*)(dev + windows_at);
    args.scatter_count = uint32_t(plan.scatter.size());
    args.sides = b->sides;
    args.levels = b->levels;
    memcpy(args.level_window, plan.level_window, sizeof args.level_window);
    memcpy(args.level_work, plan.level_work, sizeof args.level_work);

    uint32_t launches = 0;
    if (!plan.layers.empty()) {  // a read of the atlas: Attachment::written stays as it is
        if (bt_status s = launch_tile_bounds(ctx->stream, at.level0, at.meta.texture_size, (const uint32_t*)(dev + layers_at), uint32_t(plan.layers.size()), 1u, false,
                                             (uint32_t*)(dev + own_at)))
            return s;
        launches++;
    }
    launches += launch_bounds_update(ctx->stream, args);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "bounds_update kernels");
    impl->current = true;
    if (stats) {
        stats->tiles_listed = uint32_t(plan.scatter.size());
        stats->layers_reduced = uint32_t(plan.layers.size());
        stats->launches = launches;
        stats->entries_written = plan.total;
    }
    return BT_OK;
}

}  // namespace

extern "C" {

bt_status bt_height_bounds_create(bt_ctx* ctx, uint32_t sides, uint32_t levels, bt_height_bounds** out) {
    if (!ctx || !out || (sides != 1u && sides != 6u) || levels < 1u || levels > BT_HEIGHT_BOUNDS_MAX_LEVELS) {
        set_error("bt_height_bounds_create: %s", !ctx ? "NULL context" : !out ? "NULL out" : "sides is 1 or 6, levels 1..11");
        return BT_ERR_INVALID_ARGUMENT;
    }
    BT_HIP(hipSetDevice(ctx->device));
    HeightBoundsImpl* impl = new HeightBoundsImpl();  // (the public struct is its first member)
    bt_height_bounds* b = &impl->pub;
    b->ctx = ctx;
    b->sides = sides;
    b->levels = levels;
    b->entries = height_bounds_offset(sides, levels);
    hipError_t e = hipMalloc((void**)&b->table, b->entries * 4u);
    if (e == hipSuccess) e = hipMemsetD32Async((hipDeviceptr_t)b->table, int(0xFFFF0000u), b->entries, ctx->stream);  // (0, 65535)
    // the shadow of an empty atlas: nothing held (the table above is what a build of one gives)
    if (e == hipSuccess) e = hipMalloc((void**)&impl->shadow, b->entries * 4u);
    if (e == hipSuccess) e = hipMemsetD32Async((hipDeviceptr_t)impl->shadow, int(kBoundsNotHeld), b->entries, ctx->stream);
    if (e != hipSuccess) {
        bt_height_bounds_destroy(b);
        return hip_fail(e, "height bounds table");
    }
    *out = b;
    return BT_OK;
}

void bt_height_bounds_destroy(bt_height_bounds* b) {
    if (!b) return;
    hipSetDevice(b->ctx->device);
    if (b->table) {
        hipStreamSynchronize(b->ctx->stream);  // a prepass that borrowed the table may still be running
        hipFree(b->table);
    }
    if (bounds_impl(b)->shadow) hipFree(bounds_impl(b)->shadow);
    delete bounds_impl(b);
}

bt_status bt_height_bounds_read(const bt_height_bounds* b, uint16_t* out, uint64_t out_bytes) {
    if (!b || !out || out_bytes < b->entries * 4u) {
        set_error("bt_height_bounds_read: %s", !b ? "NULL table" : !out ? "NULL out_host" : "out_bytes below entries * 4");
        return BT_ERR_INVALID_ARGUMENT;
    }
    BT_HIP(hipSetDevice(b->ctx->device));
    BT_HIP(hipMemcpyAsync(out, b->table, b->entries * 4u, hipMemcpyDeviceToHost, b->ctx->stream));
    BT_HIP(hipStreamSynchronize(b->ctx->stream));
    return BT_OK;
}

bt_status bt_height_bounds_write(bt_height_bounds* b, const uint16_t* src, uint64_t bytes) {
    if (!b || !src || bytes != b->entries * 4u) {
        set_error("bt_height_bounds_write: %s", !b ? "NULL table" : !src ? "NULL src_host" : "bytes is not entries * 4");
        return BT_ERR_INVALID_ARGUMENT;
    }
    BT_HIP(hipSetDevice(b->ctx->device));
    bounds_impl(b)->current = false;  // own(tile) of these entries is unknown: bt_height_bounds_update asks for a build first
    BT_HIP(hipMemcpyAsync(b->table, src, bytes, hipMemcpyHostToDevice, b->ctx->stream));
    BT_HIP(hipStreamSynchronize(b->ctx->stream));  // (src is the caller's, pageable)
    return BT_OK;
}

bt_status bt_height_bounds_build(bt_height_bounds* b, bt_atlas* a, uint32_t ai) {
    if (bt_status s = check_table("bt_height_bounds_build", b, a, ai)) return s;
    // 1. own(tile) of every held tile: the grid-1 bounds of its layer (the existing kernel)
    std::vector<uint32_t> own(b->entries, kBoundsNotHeld), layers, slots;
    for (const bt_tile_coordinate& c : a->existing_tiles) {
        uint32_t layer;
        if (!held_layer(a, c, &layer) || c.lod >= b->levels || c.side >= b->sides || (c.x >> c.lod) || (c.y >> c.lod)) continue;
        layers.push_back(layer);
        slots.push_back(slot(b, c));
    }
    std::vector<uint16_t> pairs(2 * layers.size());
    if (bt_status s = bt_atlas_tile_bounds(a, ai, layers.data(), uint32_t(layers.size()), 1u, 0u, pairs.data(), pairs.size() * 2u)) return s;
    for (size_t i = 0; i < layers.size(); i++) own[slots[i]] = uint32_t(pairs[2 * i]) | (uint32_t(pairs[2 * i + 1]) << 16);
    const std::vector<uint32_t> shadow = own;  // before the fill: what bt_height_bounds_update starts from
    // 2. top down: a tile that is not held takes own of its parent (a root: the whole range); 3. bottom up: the union with the children
    std::vector<uint32_t> entry(b->entries);
    for (uint32_t l = 0; l < b->levels; l++) {
        const uint64_t n = 1ull << l, base = height_bounds_offset(b->sides, l), parent = l ? height_bounds_offset(b->sides, l - 1u) : 0;
        for (uint64_t side = 0; side < b->sides; side++)
            for (uint64_t y = 0; y < n; y++)
                for (uint64_t x = 0; x < n; x++) {
                    uint32_t& o = own[base + (side * n + y) * n + x];
                    if (o == kBoundsNotHeld) o = l ? own[parent + (side * (n >> 1) + (y >> 1)) * (n >> 1) + (x >> 1)] : 0xFFFF0000u;
                }
    }
    for (uint32_t l = b->levels; l-- > 0;) {
        const uint64_t n = 1ull << l, base = height_bounds_offset(b->sides, l), child = height_bounds_offset(b->sides, l + 1u);
        for (uint64_t side = 0; side < b->sides; side++)
            for (uint64_t y = 0; y < n; y++)
                for (uint64_t x = 0; x < n; x++) {
                    uint32_t mn = own[base + (side * n + y) * n + x] & 0xFFFFu, mx = own[base + (side * n + y) * n + x] >> 16;
                    for (uint64_t k = 0; l + 1u < b->levels && k < 4; k++) {
                        const uint32_t e = entry[child + (side * 2 * n + 2 * y + (k >> 1)) * 2 * n + 2 * x + (k & 1)];
                        mn = std::min(mn, e & 0xFFFFu);
                        mx = std::max(mx, e >> 16);
                    }
                    entry[base + (side * n + y) * n + x] = mn | (mx << 16);
                }
    }
    BT_HIP(hipSetDevice(b->ctx->device));
    HeightBoundsImpl* impl = bounds_impl(b);
    impl->current = false;
    BT_HIP(hipMemcpyAsync(b->table, entry.data(), b->entries * 4u, hipMemcpyHostToDevice, b->ctx->stream));
    BT_HIP(hipMemcpyAsync(impl->shadow, shadow.data(), b->entries * 4u, hipMemcpyHostToDevice, b->ctx->stream));
    BT_HIP(hipStreamSynchronize(b->ctx->stream));
    impl->atlas_uid = a->uid;
    impl->attachment = ai;
    impl->current = true;
    return BT_OK;
}

bt_status bt_height_bounds_update(bt_height_bounds* b, bt_atlas* a, uint32_t ai, const bt_tile_coordinate* tiles, uint32_t count,
                                  bt_bounds_update_stats* stats) {
    if (stats) *stats = bt_bounds_update_stats{};
    if (bt_status s = check_update(b, a, ai, tiles, count)) return s;
    if (!count) return BT_OK;
    UpdatePlan plan;
    if (bt_status s = plan_update(b, a, tiles, count, plan)) return s;
    if (plan.scatter.empty()) return BT_OK;  // every listed tile lies below the table
    return run_update(b, a, a->attachments[ai], plan, stats);
}

}  // extern "C"

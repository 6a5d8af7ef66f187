// bt_height_bounds_update: the height-bounds table of the culling test brought up to date from a list of changed tiles.
//
// An entry is own(tile) united with the four children's entries, and own of a tile the atlas does not hold is own of its nearest held
// ancestor.  The table alone cannot be updated (own is gone once united), so the library keeps a shadow beside it (HeightBoundsImpl):
// own of every held tile, kBoundsNotHeld elsewhere.  With U the distinct listed tiles of the table's levels:
//   - own changes for U only: the grid-1 reduction of a held tile's layer (launch_tile_bounds, into device scratch), not-held otherwise;
//   - the filled own (own after the walk up to the nearest held tile) changes for U and for everything that looks up through a tile of U:
//     the subtrees below the children of U the atlas does not hold ("fill roots"), taken whole, down to the last level;
//   - the entry changes for those and for the ancestors of U.
// The host plan (index arithmetic, O(count * levels)) turns that set into windows per level: a single entry, or the 2^s x 2^s square a fill
// root covers s levels below it.  Windows nested in a fill root's are dropped, so every entry has one writer.  The kernels:
//   scatter   shadow[slot] = the new own or not-held, for U;
//   fill      for every affected entry, of all levels at once: walk up the shadow to the nearest held tile (a root that is not held
//             gives (0, 65535)) and store the filled own in the table entry itself;
//   unite     per level from levels - 2 up to 0: entry = entry (its filled own) united with the four children's entries as they stand.
// At or below kBoundsUpdateSmall affected entries one workgroup runs all three with workgroup barriers in between (one launch); above it
// scatter, fill and every level's unite are launches of their own: kernel boundaries are the only order between workgroups.
#include <cstring>
#include <unordered_set>

#include "bt_internal.hpp"

namespace bt {

namespace {

constexpr uint32_t kMaxLevels = BT_HEIGHT_BOUNDS_MAX_LEVELS;
constexpr uint32_t kSmallThreads = 1024;  // the one workgroup of the small form
constexpr uint32_t kWideThreads = 256;
// Affected entries up to which one workgroup does the table work: the largest set whose windows (one per entry at worst, 16 bytes) fit the
// 64 KB of LDS a launch gets by default.  Measured (profiles/bounds_update.txt): one workgroup 17 / 23 / 67 us per call at 1365 / 5461 /
// 21845 entries, the wide form 33 / 37 / 40 us; they cross near 11 000.
constexpr uint32_t kBoundsUpdateSmall = 4096;
constexpr uint32_t kNoSource = 0xFFFFFFFFu;

struct Scatter {
    uint32_t slot;    // table index of a tile of U
    uint32_t source;  // index into the reduced own ranges, kNoSource: the atlas does not hold the tile
};
struct Window {  // a square of affected entries of one level
    uint32_t side_shift;  // side | shift << 8: 2^shift x 2^shift entries
    uint32_t x0, y0;
    uint32_t first;       // entries of the level's windows before this one
};
struct UpdateArgs {
    uint32_t* table;
    uint32_t* shadow;
    const uint32_t* own;  // one word per reduced layer (min | max << 16)
    const Scatter* scatter;
    const Window* windows;  // level by level
    uint32_t scatter_count, sides, levels, _pad;
    uint32_t level_window[kMaxLevels + 1];  // the first window of a level; [levels]: the number of windows
    uint32_t level_work[kMaxLevels + 1];    // affected entries of the levels before; [levels]: all of them
};

__device__ __forceinline__ uint32_t level_offset(uint32_t sides, uint32_t level) { return sides * (((1u << (2u * level)) - 1u) / 3u); }

// entry `w` of the affected entries of `level` -> its table index and coordinate (windows: a.windows, or the small form's copy in LDS)
__device__ __forceinline__ uint32_t locate(const UpdateArgs& a, const Window* windows, uint32_t level, uint32_t w, uint32_t& side, uint32_t& x, uint32_t& y) {
    uint32_t lo = a.level_window[level], hi = a.level_window[level + 1u];  // the last window with first <= w
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) / 2u;
        if (windows[mid].first <= w) lo = mid;
        else hi = mid;
    }
    const Window win = windows[lo];
    const uint32_t shift = win.side_shift >> 8, local = w - win.first;
    side = win.side_shift & 0xFFu;
    x = win.x0 + (local & ((1u << shift) - 1u));
    y = win.y0 + (local >> shift);
    return level_offset(a.sides, level) + ((((side << level) + y) << level) + x);
}

__device__ void scatter_one(const UpdateArgs& a, uint32_t i) {
    const Scatter s = a.scatter[i];
    a.shadow[s.slot] = s.source == kNoSource ? kBoundsNotHeld : a.own[s.source];
}

// w: an index into the affected entries of all levels
__device__ __forceinline__ void fill_one(const UpdateArgs& a, const Window* windows, uint32_t w) {
    uint32_t level = 0;
    while (level + 1u < a.levels && a.level_work[level + 1u] <= w) level++;
    uint32_t side, x, y;
    const uint32_t slot = locate(a, windows, level, w - a.level_work[level], side, x, y);
    uint32_t v = a.shadow[slot];
    for (uint32_t l = level; v == kBoundsNotHeld && l > 0u;) {  // the nearest held ancestor's own
        l--;
        x >>= 1, y >>= 1;
        v = a.shadow[level_offset(a.sides, l) + ((((side << l) + y) << l) + x)];
    }
    a.table[slot] = v == kBoundsNotHeld ? 0xFFFF0000u : v;
}

// w: an index into the affected entries of `level` < levels - 1
__device__ __forceinline__ void unite_one(const UpdateArgs& a, const Window* windows, uint32_t level, uint32_t w) {
    uint32_t side, x, y;
    const uint32_t slot = locate(a, windows, level, w, side, x, y);
    const uint32_t v = a.table[slot], cl = level + 1u;
    const uint32_t c0 = level_offset(a.sides, cl) + ((((side << cl) + 2u * y) << cl) + 2u * x);
    uint32_t mn = v & 0xFFFFu, mx = v >> 16;
    for (uint32_t c : {c0, c0 + 1u, c0 + (1u << cl), c0 + (1u << cl) + 1u}) {
        const uint32_t e = a.table[c];
        mn = min(mn, e & 0xFFFFu);
        mx = max(mx, e >> 16);
    }
    a.table[slot] = mn | (mx << 16);
}

// the whole update in one workgroup: the barriers order the steps (and the levels) among its waves.  The windows (at most one per
// affected entry: kBoundsUpdateSmall * 16 bytes) are copied to LDS once, so the searches of every step stay out of global memory.
__global__ __launch_bounds__(kSmallThreads) void bounds_update_small(UpdateArgs a) {
    extern __shared__ uint32_t lds[];
    Window* windows = reinterpret_cast<Window*>(lds);
    for (uint32_t i = threadIdx.x; i < a.level_window[a.levels]; i += kSmallThreads) windows[i] = a.windows[i];
    for (uint32_t i = threadIdx.x; i < a.scatter_count; i += kSmallThreads) scatter_one(a, i);
    __syncthreads();
    for (uint32_t w = threadIdx.x; w < a.level_work[a.levels]; w += kSmallThreads) fill_one(a, windows, w);
    __syncthreads();
    for (uint32_t level = a.levels - 1u; level-- > 0u;) {
        const uint32_t work = a.level_work[level + 1u] - a.level_work[level];
        if (!work) continue;  // (uniform)
        for (uint32_t w = threadIdx.x; w < work; w += kSmallThreads) unite_one(a, windows, level, w);
        __syncthreads();
    }
}

__global__ __launch_bounds__(kWideThreads) void bounds_update_scatter(UpdateArgs a) {
    const uint32_t i = blockIdx.x * kWideThreads + threadIdx.x;
    if (i < a.scatter_count) scatter_one(a, i);
}

__global__ __launch_bounds__(kWideThreads) void bounds_update_fill(UpdateArgs a) {
    const uint32_t w = blockIdx.x * kWideThreads + threadIdx.x;
    if (w < a.level_work[a.levels]) fill_one(a, a.windows, w);
}

__global__ __launch_bounds__(kWideThreads) void bounds_update_unite(UpdateArgs a, uint32_t level) {
    const uint32_t w = blockIdx.x * kWideThreads + threadIdx.x;
    if (w < a.level_work[level + 1u] - a.level_work[level]) unite_one(a, a.windows, level, w);
}

bool held_layer(const bt_atlas* a, const bt_tile_coordinate& c, uint32_t* layer) {  // what bt_height_bounds_build tests
    if (!a->existing_tiles.count(c)) return false;
    const auto it = a->tile_states.find(c);
    if (it == a->tile_states.end() || it->second.loading != 0) return false;
    *layer = it->second.atlas_index;
    return true;
}

bt_status check_update(bt_height_bounds* b, const bt_atlas* a, uint32_t ai, const bt_tile_coordinate* tiles, uint32_t count) {
    if (!b || !a || ai >= a->attachments.size()) {
        set_error("bt_height_bounds_update: %s", !b ? "NULL table" : !a ? "NULL atlas" : "attachment index out of range");
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (a->attachments[ai].meta.format != BT_FORMAT_R16) {
        set_error("bt_height_bounds_update: attachment %u is not R16", ai);
        return BT_ERR_UNSUPPORTED;
    }
    if (b->ctx != a->ctx || b->sides != (a->config.spherical ? 6u : 1u)) {
        set_error("bt_height_bounds_update: %s", b->ctx != a->ctx ? "table and atlas belong to different contexts" : "the atlas's side count is not the table's");
        return BT_ERR_INVALID_ARGUMENT;
    }
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
    uint32_t level_window[kMaxLevels + 1] = {}, level_work[kMaxLevels + 1] = {};  // UpdateArgs'
    uint64_t total = 0;            // affected entries
};

bt_status plan_update(const bt_height_bounds* b, const bt_atlas* a, const bt_tile_coordinate* tiles, uint32_t count, UpdatePlan& plan) {
    const uint32_t levels = b->levels, sides = b->sides;
    typedef std::unordered_set<bt_tile_coordinate, CoordHash, CoordEq> TileSet;
    auto slot = [&](const bt_tile_coordinate& c) { return uint32_t(height_bounds_offset(sides, c.lod) + ((((uint64_t(c.side) << c.lod) + c.y) << c.lod) + c.x)); };
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
            plan.scatter.push_back({slot(c), uint32_t(plan.layers.size())});
            plan.layers.push_back(layer);
        } else {
            plan.scatter.push_back({slot(c), kNoSource});
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
    UpdateArgs args{};
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
    auto blocks = [](uint32_t n) { return (n + kWideThreads - 1u) / kWideThreads; };
    if (plan.total <= kBoundsUpdateSmall) {
        bounds_update_small<<<1, kSmallThreads, plan.windows.size() * sizeof(Window), ctx->stream>>>(args);
        launches++;
    } else {
        bounds_update_scatter<<<blocks(args.scatter_count), kWideThreads, 0, ctx->stream>>>(args);
        bounds_update_fill<<<blocks(uint32_t(plan.total)), kWideThreads, 0, ctx->stream>>>(args);
        launches += 2;
        for (uint32_t l = b->levels - 1u; l-- > 0u;) {
            const uint32_t work = args.level_work[l + 1u] - args.level_work[l];
            if (!work) continue;
            bounds_update_unite<<<blocks(work), kWideThreads, 0, ctx->stream>>>(args, l);
            launches++;
        }
    }
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

}  // namespace bt

using namespace bt;

extern "C" bt_status bt_height_bounds_update(bt_height_bounds* b, bt_atlas* a, uint32_t ai, const bt_tile_coordinate* tiles, uint32_t count,
                                             bt_bounds_update_stats* stats) {
    if (stats) *stats = bt_bounds_update_stats{};
    if (bt_status s = check_update(b, a, ai, tiles, count)) return s;
    if (!count) return BT_OK;
    UpdatePlan plan;
    if (bt_status s = plan_update(b, a, tiles, count, plan)) return s;
    if (plan.scatter.empty()) return BT_OK;  // every listed tile lies below the table
    return run_update(b, a, a->attachments[ai], plan, stats);
}

// bt_atlas_edit_height / bt_atlas_smooth_height / bt_atlas_paint / bt_atlas_splat_from_height / bt_atlas_scatter_instances (its checks) / bt_atlas_write_region / bt_atlas_read_region /
// bt_atlas_erode_height (the simulation's kernels: bt_erode.hip) / bt_atlas_save_tiles: the host half of in-place editing.
//
// An edit changes centre texels of existing tiles of one LOD and then restores what the atlas state derives from them (the invariant F of
// include/bevy_terrain_amd.h): the ancestors' centres, the aprons of every written tile and of its existing neighbours, the mips.  The plan
// is index arithmetic on the host: per LOD from `lod` down to 0 the dirty rectangle of every tile (the parent's mosaic rectangle is
// [x0 >> 1, x1 >> 1], cut at tile boundaries; the centre size need not be a power of two), the items of each launch, the stitch tasks.  It
// travels through pinned memory into scratch of the context in ONE copy; the kernels (bt_edit.hip, launch_stitch, the mip kernels) follow
// on the context's stream and the call returns.
#include <cmath>
#include <cstring>
#include <map>

#include "bt_model.hpp"
#include "bt_tile_io.hpp"

using namespace bt;

namespace {

struct Rect {
    uint32_t x0, y0, x1, y1;  // inclusive
};
struct Box {  // a rectangle of mosaic texels of one side
    uint32_t side;
    Rect r;
};
struct Dirty {
    uint32_t layer;
    Rect r;  // in centre texels of the tile
};
typedef std::map<bt_tile_coordinate, Dirty, CoordLess> DirtyTiles;

// the layer of a tile the atlas holds, or BT_INVALID_ATLAS_INDEX (bt_atlas_get_tile)
uint32_t layer_of(const bt_atlas* a, const bt_tile_coordinate& c) {
    if (is_invalid(c) || !a->existing_tiles.count(c)) return BT_INVALID_ATLAS_INDEX;
    const auto it = a->tile_states.find(c);
    return it != a->tile_states.end() && it->second.atlas_index < a->config.atlas_size ? it->second.atlas_index : BT_INVALID_ATLAS_INDEX;
}

void unite(DirtyTiles& tiles, const bt_tile_coordinate& c, uint32_t layer, const Rect& r) {
    auto [it, fresh] = tiles.emplace(c, Dirty{layer, r});
    if (fresh) return;
    Rect& u = it->second.r;
    u = {std::min(u.x0, r.x0), std::min(u.y0, r.y0), std::max(u.x1, r.x1), std::max(u.y1, r.y1)};
}

// tiles covered by at least one of the (inclusive) tile rectangles: strips between the distinct x bounds, merged y intervals in each
uint64_t union_area(const std::vector<Rect>& rects) {
    std::vector<uint64_t> xs;
    for (const Rect& r : rects) {
        xs.push_back(r.x0);
        xs.push_back(uint64_t(r.x1) + 1u);
    }
    std::sort(xs.begin(), xs.end());
    xs.erase(std::unique(xs.begin(), xs.end()), xs.end());
    uint64_t area = 0;
    std::vector<std::pair<uint64_t, uint64_t>> spans;
    for (size_t i = 0; i + 1 < xs.size(); i++) {
        spans.clear();
        for (const Rect& r : rects)
            if (r.x0 <= xs[i] && xs[i] <= r.x1) spans.push_back({r.y0, uint64_t(r.y1) + 1u});
        std::sort(spans.begin(), spans.end());
        uint64_t covered = 0, end = 0;
        for (const auto& [lo, hi] : spans) {
            if (hi <= end) continue;
            covered += hi - std::max(lo, end);
            end = hi;
        }
        area += covered * (xs[i + 1] - xs[i]);
    }
    return area;
}

struct Plan {
    std::vector<std::vector<EditItem>> levels;  // [0]: the edited tiles of `lod`; [k]: the downsample items of lod - k
    std::vector<uint32_t> max_rows;             // the tallest rectangle of each level
    std::vector<TaskDev> stitches;
    std::vector<std::pair<bt_tile_coordinate, uint32_t>> changed;  // (tile, layer): LOD descending, then layer
    bt_edit_stats stats{};
};

EditItem make_item(const bt_tile_coordinate& c, const Dirty& d, uint32_t centre) {
    EditItem it{};
    it.layer = d.layer;
    it.x0 = d.r.x0, it.y0 = d.r.y0, it.x1 = d.r.x1, it.y1 = d.r.y1;
    it.gx0 = c.x * centre, it.gy0 = c.y * centre;
    it.side = c.side;
    for (uint32_t& ch : it.child) ch = BT_INVALID_ATLAS_INDEX;
    return it;
}

// the tiles of `lod` each box meets: existing ones get the box's part of their centre (`cur`), and all of them are counted (returned)
uint64_t meet_tiles(const bt_atlas* a, uint32_t c, uint32_t lod, const std::vector<Box>& boxes, DirtyTiles& cur) {
    uint64_t met = 0;
    for (uint32_t side = 0; side < 6; side++) {
        std::vector<Rect> tile_rects;
        for (const Box& bx : boxes)
            if (bx.side == side) tile_rects.push_back({bx.r.x0 / c, bx.r.y0 / c, bx.r.x1 / c, bx.r.y1 / c});
        if (!tile_rects.empty()) met += union_area(tile_rects);
    }
    for (const Box& bx : boxes) {
        const Rect t = {bx.r.x0 / c, bx.r.y0 / c, bx.r.x1 / c, bx.r.y1 / c};
        auto visit = [&](const bt_tile_coordinate& tile, uint32_t layer) {
            const uint64_t ox = uint64_t(tile.x) * c, oy = uint64_t(tile.y) * c;
            const Rect r = {uint32_t(std::max<uint64_t>(bx.r.x0, ox) - ox), uint32_t(std::max<uint64_t>(bx.r.y0, oy) - oy),
                            uint32_t(std::min<uint64_t>(bx.r.x1, ox + c - 1u) - ox), uint32_t(std::min<uint64_t>(bx.r.y1, oy + c - 1u) - oy)};
            unite(cur, tile, layer, r);
        };
        const uint64_t count = (uint64_t(t.x1) - t.x0 + 1u) * (uint64_t(t.y1) - t.y0 + 1u);
        if (count <= a->existing_tiles.size()) {
            for (uint32_t y = t.y0; y <= t.y1; y++)
                for (uint32_t x = t.x0; x <= t.x1; x++) {
                    const bt_tile_coordinate tile = {bx.side, lod, x, y};
                    const uint32_t layer = layer_of(a, tile);
                    if (layer != BT_INVALID_ATLAS_INDEX) visit(tile, layer);
                }
        } else {  // a box over more tiles than the atlas holds: walk the atlas's instead
            for (const bt_tile_coordinate& tile : a->existing_tiles) {
                if (tile.side != bx.side || tile.lod != lod || tile.x < t.x0 || tile.x > t.x1 || tile.y < t.y0 || tile.y > t.y1) continue;
                const uint32_t layer = layer_of(a, tile);
                if (layer != BT_INVALID_ATLAS_INDEX) visit(tile, layer);
            }
        }
    }
    return met;
}

// boxes of mosaic texels of `lod` -> the whole plan.  Host index arithmetic only.
void build_plan(const bt_atlas* a, const Attachment& at, uint32_t lod, const std::vector<Box>& boxes, Plan& plan) {
    const uint32_t c = at.meta.center_size;
    const bool spherical = a->config.spherical != 0;
    DirtyTiles cur;
    const uint64_t met = meet_tiles(a, c, lod, boxes, cur);
    plan.stats.tiles_edited = uint32_t(cur.size());
    plan.stats.tiles_missing = uint32_t(std::min<uint64_t>(met - std::min<uint64_t>(met, cur.size()), 0xFFFFFFFFull));
    if (cur.empty()) return;

    DirtyTiles written = cur;  // every tile of every LOD whose centre the call writes
    auto level_items = [&](const DirtyTiles& tiles, bool with_children) {
        std::vector<EditItem> items;
        uint32_t rows = 0;
        for (const auto& [coord, d] : tiles) {
            EditItem it = make_item(coord, d, c);
            if (with_children) {
                bt_tile_coordinate ch[4];
                tile_children(coord, ch);
                for (int k = 0; k < 4; k++) it.child[k] = layer_of(a, ch[k]);
            }
            rows = std::max(rows, d.r.y1 - d.r.y0 + 1u);
            items.push_back(it);
        }
        plan.levels.push_back(std::move(items));
        plan.max_rows.push_back(rows);
    };
    level_items(cur, false);
    for (const auto& [coord, d] : cur) {
        bt_tile_coordinate ch[4];
        tile_children(coord, ch);
        for (int k = 0; k < 4; k++)
            if (layer_of(a, ch[k]) != BT_INVALID_ATLAS_INDEX) {
                plan.stats.tiles_with_children++;
                break;
            }
    }
    for (uint32_t l = lod; l > 0 && !cur.empty(); l--) {
        DirtyTiles next;
        for (const auto& [coord, d] : cur) {
            const bt_tile_coordinate parent = {coord.side, l - 1u, coord.x >> 1, coord.y >> 1};
            const uint32_t layer = layer_of(a, parent);
            if (layer == BT_INVALID_ATLAS_INDEX) continue;  // the chain of ancestors ends where a parent does not exist
            const uint32_t ox = (coord.x & 1u) * (c / 2u), oy = (coord.y & 1u) * (c / 2u);
            unite(next, parent, layer, {ox + (d.r.x0 >> 1), oy + (d.r.y0 >> 1), ox + (d.r.x1 >> 1), oy + (d.r.y1 >> 1)});
        }
        if (next.empty()) break;
        level_items(next, true);
        plan.stats.tiles_downsampled += uint32_t(next.size());
        written.insert(next.begin(), next.end());
        cur.swap(next);
    }

    // aprons: every written tile and every existing neighbour of one, all eight regions
    std::map<bt_tile_coordinate, uint32_t, CoordLess> touched;
    for (const auto& [coord, d] : written) touched.emplace(coord, d.layer);
    if (at.meta.border_size > 0) {
        for (const auto& [coord, d] : written) {
            bt_tile_coordinate nb[8];
            tile_neighbours(coord, spherical, nb);
            for (const bt_tile_coordinate& n : nb) {
                const uint32_t layer = layer_of(a, n);
                if (layer != BT_INVALID_ATLAS_INDEX) touched.emplace(n, layer);
            }
        }
    }
    for (const auto& [coord, layer] : touched) plan.changed.push_back({coord, layer});
    std::sort(plan.changed.begin(), plan.changed.end(), [](const auto& l, const auto& r) {
        if (l.first.lod != r.first.lod) return l.first.lod > r.first.lod;
        return l.second < r.second;
    });
    if (at.meta.border_size > 0) {
        for (const auto& [coord, layer] : plan.changed) {
            TaskDev t{};
            t.atlas_index = layer;
            t.side = coord.side, t.lod = coord.lod, t.x = coord.x, t.y = coord.y;
            bt_tile_coordinate nb[8];
            tile_neighbours(coord, spherical, nb);
            for (int k = 0; k < 8; k++) {
                t.rel_index[k] = layer_of(a, nb[k]);
                t.rel_side[k] = nb[k].side;
            }
            plan.stitches.push_back(t);
        }
        plan.stats.tiles_stitched = uint32_t(plan.stitches.size());
    }
    plan.stats.changed_count = uint32_t(plan.changed.size());
}

// (bt_ctx::edit_region is the device buffer a first step reads its texels from: the staged rectangle of write_region, the new texels of smooth_height)

// The first step of a plan, the one that writes the rectangles of the edited tiles (the steps after it are the same for every call): the
// brush or the paint brush on its stamps, the copy from a rectangle of host texels, the smoothing pair on its stamps, the rules of
// bt_atlas_splat_from_height on the heights of another attachment.  prepare() runs once the plan is known
// to write something: it adds what the step wants in the ring and readies its device buffer; launch() follows the ring's commit.
struct FirstStep {
    enum Kind { kBrush, kRegion, kSmooth, kPaint, kSplat } kind;
    // brush: bt_edit_stamp[count]; paint: bt_paint_stamp[count]; smooth: bt_smooth_stamp[count] and the box's kernel_radius; splat:
    // bt_splat_rule[count] (== splat.count)
    const void* stamps = nullptr;
    uint32_t count = 0, kernel_radius = 0;
    // region: width x height texels whose (0, 0) is mosaic texel (x0, y0), rows row_pitch bytes apart; nullptr: the rectangle is already in
    // ctx->edit_region, put there on the stream by the caller (bt_atlas_erode_height)
    const void* texels = nullptr;
    uint64_t row_pitch = 0;
    uint32_t x0 = 0, y0 = 0, width = 0, height = 0;
    // splat: the heights the rules read (their attachment's meta and level 0, the model, the LOD), the mode and the fallback texel
    SplatSource splat{};
    // prepare() -> launch()
    std::vector<uint64_t> offsets;  // smooth: where each item's rectangle starts in the scratch, in dwords
    uint64_t stamps_at = 0, offsets_at = 0;

    uint32_t launches() const { return kind == kSmooth ? 2u : 1u; }
    bt_status prepare(bt_ctx* ctx, const AttachmentMeta& m, const std::vector<EditItem>& items, PlanRing& ring);
    bt_status stage_region(bt_ctx* ctx, uint64_t row_bytes);
    bt_status launch(bt_ctx* ctx, const Attachment& at, const uint8_t* ring, const EditItem* items, uint32_t n, uint32_t max_rows) const;
};

bt_status FirstStep::prepare(bt_ctx* ctx, const AttachmentMeta& m, const std::vector<EditItem>& items, PlanRing& ring) {
    switch (kind) {
        case kBrush: stamps_at = ring.add(stamps, uint64_t(count) * sizeof(bt_edit_stamp)); return BT_OK;
        case kPaint: stamps_at = ring.add(stamps, uint64_t(count) * sizeof(bt_paint_stamp)); return BT_OK;
        case kSplat: stamps_at = ring.add(stamps, uint64_t(count) * sizeof(bt_splat_rule)); return BT_OK;
        case kRegion: return texels ? stage_region(ctx, uint64_t(width) * m.pixel_size) : BT_OK;
        case kSmooth: {
            uint64_t scratch_dwords = 0;
            for (const EditItem& it : items) {
                offsets.push_back(scratch_dwords);
                scratch_dwords += smooth_item_dwords(it, m.border_size);
            }
            if (bt_status s = ctx->edit_region.reserve(ctx, scratch_dwords * sizeof(uint32_t))) return s;
            stamps_at = ring.add(stamps, uint64_t(count) * sizeof(bt_smooth_stamp));
            offsets_at = ring.add(offsets);
            return BT_OK;
        }
    }
    return BT_OK;
}

// the rectangle, tightly packed: host rows -> pinned staging -> device scratch, in chunks of whole rows
bt_status FirstStep::stage_region(bt_ctx* ctx, uint64_t row_bytes) {
    if (bt_status s = ctx->edit_region.reserve(ctx, row_bytes * height)) return s;
    return region_stage_in(ctx, ctx->edit_region.dev, texels, row_bytes, row_pitch, height);
}

bt_status FirstStep::launch(bt_ctx* ctx, const Attachment& at, const uint8_t* ring, const EditItem* items, uint32_t n, uint32_t max_rows) const {
    switch (kind) {
        case kBrush: return launch_edit_brush(ctx->stream, at.meta, at.level0, items, n, max_rows, (const bt_edit_stamp*)(ring + stamps_at), count);
        case kPaint: return launch_edit_paint(ctx->stream, at.meta, at.level0, items, n, max_rows, (const bt_paint_stamp*)(ring + stamps_at), count);
        case kSplat: return launch_edit_splat(ctx->stream, at.meta, at.level0, items, n, max_rows, splat, (const bt_splat_rule*)(ring + stamps_at));
        case kRegion: return launch_edit_region(ctx->stream, at.meta, at.level0, items, n, max_rows, ctx->edit_region.dev, x0, y0, width);
        case kSmooth:
            return launch_edit_smooth(ctx->stream, at.meta, at.level0, items, (const uint64_t*)(ring + offsets_at), n, max_rows, (const bt_smooth_stamp*)(ring + stamps_at), count,
                                      kernel_radius, ctx->edit_region.dev);
    }
    return BT_OK;
}

// uploads the plan and enqueues its launches
bt_status run_plan(bt_atlas* a, uint32_t ai, Plan& plan, FirstStep& first) {
    Attachment& at = a->attachments[ai];
    bt_ctx* ctx = a->ctx;
    if (plan.levels.empty()) return BT_OK;
    PlanRing ring;
    if (bt_status s = first.prepare(ctx, at.meta, plan.levels[0], ring)) return s;
    std::vector<uint64_t> items_at;
    for (const auto& items : plan.levels) items_at.push_back(ring.add(items));
    const uint64_t stitches_at = ring.add(plan.stitches);
    uint8_t* dev = nullptr;
    if (bt_status s = ring.commit(ctx, &dev)) return s;

    for (const auto& [coord, layer] : plan.changed) at.mark_written(layer, 1);
    if (bt_status s = first.launch(ctx, at, dev, (const EditItem*)(dev + items_at[0]), uint32_t(plan.levels[0].size()), plan.max_rows[0])) return s;
    plan.stats.launches = first.launches();
    for (size_t k = 1; k < plan.levels.size(); k++) {
        if (bt_status s = launch_edit_downsample(ctx->stream, at.meta, at.level0, (const EditItem*)(dev + items_at[k]), uint32_t(plan.levels[k].size()), plan.max_rows[k])) return s;
        plan.stats.launches++;
    }
    if (!plan.stitches.empty()) {
        if (bt_status s = launch_stitch(ctx, at.meta, at.level0, (const TaskDev*)(dev + stitches_at), uint32_t(plan.stitches.size()))) return s;
        plan.stats.launches++;
    }
    if (at.mips.size() > 1) {  // the existing mip kernels, one pass per run of consecutive layers
        std::vector<uint32_t> layers;
        for (const auto& [coord, layer] : plan.changed) layers.push_back(layer);
        std::sort(layers.begin(), layers.end());
        layers.erase(std::unique(layers.begin(), layers.end()), layers.end());
        const bt_status mips = for_each_layer_run(0, layers.size(), [&](size_t i) { return layers[i]; }, false, [&](size_t i, size_t run) -> bt_status {
            if (bt_status s = bt_atlas_generate_mipmaps(a, ai, layers[i], uint32_t(run))) return s;
            plan.stats.launches += uint32_t(at.mips.size() - 1);
            return BT_OK;
        });
        if (mips) return mips;
        plan.stats.layers_mipped = uint32_t(layers.size());
    }
    return BT_OK;
}

// what the three entry points do once their arguments have passed: boxes of mosaic texels of `lod` -> the plan -> its launches -> the report
bt_status edit_boxes(bt_atlas* a, uint32_t ai, uint32_t lod, const std::vector<Box>& boxes, FirstStep& first, bt_tile_coordinate* changed, uint32_t changed_cap,
                     bt_edit_stats* stats) {
    const hipError_t e = hipSetDevice(a->ctx->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    Plan plan;
    build_plan(a, a->attachments[ai], lod, boxes, plan);
    const bt_status rc = run_plan(a, ai, plan, first);
    for (uint32_t i = 0; i < plan.changed.size() && i < changed_cap; i++) changed[i] = plan.changed[i].first;
    if (stats) *stats = plan.stats;
    return rc;
}

// what the edit calls check of the atlas: attachment, LOD, format (the formats the call takes) and centre size
enum Target { kHeights, kColours, kTexels };  // R16 (the height brushes), Rgba8 (the paint brush), both (the regions)
bt_status check_target(const bt_atlas* a, uint32_t ai, uint32_t lod, Target target, const char* what) {
    if (ai >= a->attachments.size()) {
        set_error("%s: attachment %u of %zu", what, ai, a->attachments.size());
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (lod >= a->config.lod_count || lod > 30u) {
        set_error("%s: lod %u of lod_count %u", what, lod, a->config.lod_count);
        return BT_ERR_INVALID_ARGUMENT;
    }
    const AttachmentMeta& m = a->attachments[ai].meta;
    if (!((m.format == BT_FORMAT_R16 && target != kColours) || (m.format == BT_FORMAT_RGBA8 && target != kHeights))) {
        set_error("%s: attachment format %u (%s)", what, m.format,
                  target == kHeights ? "the brush edits R16 heights" : target == kColours ? "the paint brush edits Rgba8" : "R16 and Rgba8 only");
        return BT_ERR_UNSUPPORTED;
    }
    if (m.center_size % 2u) {
        set_error("%s: odd centre size %u (texture_size %u, border_size %u): a parent texel would straddle two children", what, m.center_size, m.texture_size, m.border_size);
        return BT_ERR_UNSUPPORTED;
    }
    if ((uint64_t(m.center_size) << lod) > 0xFFFFFFFFull) {
        set_error("%s: a mosaic of %u x 2^%u texels", what, m.center_size, lod);
        return BT_ERR_UNSUPPORTED;
    }
    return BT_OK;
}

// what bt_atlas_write_region, bt_atlas_read_region and bt_atlas_splat_from_height (`what`) check of their rectangle of mosaic texels: the
// target, the side, the rectangle inside the mosaic of `lod`
bt_status check_region(const bt_atlas* a, uint32_t ai, uint32_t side, uint32_t lod, uint32_t x0, uint32_t y0, uint32_t width, uint32_t height, Target target, const char* what) {
    if (bt_status s = check_target(a, ai, lod, target, what)) return s;
    if (side >= (a->config.spherical ? 6u : 1u)) {
        set_error("%s: side %u", what, side);
        return BT_ERR_INVALID_ARGUMENT;
    }
    const uint64_t size = uint64_t(a->attachments[ai].meta.center_size) << lod;
    if (uint64_t(x0) + width > size || uint64_t(y0) + height > size) {
        set_error("%s: [%u, %u) x [%u, %u) outside the mosaic of %llu texels", what, x0, x0 + width, y0, y0 + height, (unsigned long long)size);
        return BT_ERR_INVALID_ARGUMENT;
    }
    return BT_OK;
}

// the fields of a stamp that only its own call has, in the place the call reports them: before_falloff or after the radius
const char* bad_own(const bt_edit_stamp& s, bool before_falloff) {
    if (before_falloff) return s.mode != BT_EDIT_ADD && s.mode != BT_EDIT_FLATTEN ? "mode" : nullptr;
    return !std::isfinite(s.amount) ? "amount (not finite)" : nullptr;
}
const char* bad_own(const bt_paint_stamp& s, bool before_falloff) {
    if (before_falloff) return s.mode != BT_PAINT_BLEND && s.mode != BT_PAINT_ADD ? "mode" : nullptr;
    if (s.channel_mask == 0u || s.channel_mask > 15u) return "channel_mask (1 .. 15)";
    if (!std::isfinite(s.opacity) || !(s.opacity > 0.0f) || !(s.opacity <= 1.0f)) return "opacity (finite, in (0, 1])";
    for (float v : s.color)
        if (!std::isfinite(v)) return "color (not finite)";
    return nullptr;
}
const char* bad_own(const bt_smooth_stamp& s, bool before_falloff) {
    if (before_falloff) return nullptr;
    return !std::isfinite(s.strength) || !(s.strength > 0.0f) || !(s.strength <= 1.0f) ? "strength (finite, in (0, 1])" : nullptr;
}

// the first defect of a stamp that can be told without the atlas, in the order the calls report them
template <typename Stamp>
const char* bad_stamp(const Stamp& s) {
    if (s.side >= 6u) return "side";
    if (const char* bad = bad_own(s, true)) return bad;
    if (s.falloff != BT_EDIT_FALLOFF_SMOOTH && s.falloff != BT_EDIT_FALLOFF_HARD) return "falloff";
    if (!std::isfinite(s.center[0]) || !std::isfinite(s.center[1])) return "center (not finite)";
    if (!std::isfinite(s.radius) || !(s.radius > 0.0f)) return "radius (finite and > 0)";
    return bad_own(s, false);
}

// What bt_atlas_edit_height, bt_atlas_smooth_height and bt_atlas_paint (`what`) check alike, in the order they report it.  The stamps first: what can be
// refused without the atlas is refused without it.  own(false) / own(true): the caller's checks of its other arguments that go before the
// stamps are looked at / once the target has passed.
template <typename Stamp, typename Own>
bt_status check_stamps(const char* what, Target target, const bt_atlas* a, uint32_t ai, uint32_t lod, const Stamp* stamps, uint32_t count, const bt_tile_coordinate* changed,
                       uint32_t changed_cap, Own own) {
    if (count > BT_EDIT_MAX_STAMPS) {
        set_error("%s: %u stamps, at most %u per call", what, count, BT_EDIT_MAX_STAMPS);
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (bt_status s = own(false)) return s;
    if ((count && !stamps) || (changed_cap && !changed)) {
        set_error("%s: NULL %s", what, count && !stamps ? "stamps" : "changed with changed_cap > 0");
        return BT_ERR_INVALID_ARGUMENT;
    }
    for (uint32_t i = 0; i < count; i++)
        if (const char* bad = bad_stamp(stamps[i])) {
            set_error("%s: stamp %u: %s", what, i, bad);
            return BT_ERR_INVALID_ARGUMENT;
        }
    if (!a) {
        set_error("%s: NULL atlas", what);
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (bt_status s = check_target(a, ai, lod, target, what)) return s;
    if (bt_status s = own(true)) return s;
    const uint32_t sides = a->config.spherical ? 6u : 1u;
    for (uint32_t i = 0; i < count; i++)
        if (stamps[i].side >= sides) {
            set_error("%s: stamp %u: side %u of %u", what, i, stamps[i].side, sides);
            return BT_ERR_INVALID_ARGUMENT;
        }
    return BT_OK;
}

// The stamps' boxes.  A stamp's box is [floor(center - radius), ceil(center + radius)], clipped to the face (nothing is added where it
// misses the face): a texel outside it is at least radius + 1 away on one axis, and rounding is monotonic, so its d2 is not below r2 in
// binary32 either.
template <typename Stamp>
std::vector<Box> stamp_boxes(const bt_atlas* a, uint32_t ai, uint32_t lod, const Stamp* stamps, uint32_t count) {
    const double size = double(uint64_t(a->attachments[ai].meta.center_size) << lod);
    std::vector<Box> boxes;
    for (uint32_t i = 0; i < count; i++) {
        const Stamp& s = stamps[i];
        double lo[2], hi[2];
        for (int k = 0; k < 2; k++) {
            lo[k] = std::max(0.0, std::floor(double(s.center[k]) - double(s.radius)));
            hi[k] = std::min(size - 1.0, std::ceil(double(s.center[k]) + double(s.radius)));
        }
        if (lo[0] <= hi[0] && lo[1] <= hi[1]) boxes.push_back({s.side, {uint32_t(lo[0]), uint32_t(lo[1]), uint32_t(hi[0]), uint32_t(hi[1])}});
    }
    return boxes;
}

// the first defect of the height and slope bands of a rule (bt_splat_rule and bt_scatter_rule begin with the same six bounds), or NULL
template <typename Rule>
const char* bad_bands(const Rule& r) {
    const float bounds[2][3] = {{r.height_lo, r.height_hi, r.height_fade}, {r.steep_lo, r.steep_hi, r.steep_fade}};
    for (const float* v : {bounds[0], bounds[1]}) {
        if (std::isnan(v[0]) || std::isnan(v[1])) return "a NaN bound";
        if (v[0] > v[1]) return "lo > hi";
        if (!std::isfinite(v[2]) || v[2] < 0.0f) return "fade (finite and >= 0)";
    }
    return nullptr;
}

// the first defect of a rule of bt_atlas_splat_from_height, or NULL
const char* bad_rule(const bt_splat_rule& r, uint32_t mode) {
    if (const char* bad = bad_bands(r)) return bad;
    if (!std::isfinite(r.weight) || r.weight < 0.0f) return "weight (finite and >= 0)";
    for (float v : r.colour)
        if (mode == BT_SPLAT_COLOUR ? !std::isfinite(v) : std::isnan(v)) return "colour (not finite)";
    return nullptr;
}

// the first defect of a rule of bt_atlas_scatter_instances, or NULL; masked: the call has a mask attachment
const char* bad_scatter_rule(const bt_scatter_rule& r, bool masked) {
    if (const char* bad = bad_bands(r)) return bad;
    if (!(r.density >= 0.0f && r.density <= 1.0f)) return "density (in [0, 1])";
    if (!std::isfinite(r.scale_lo) || !std::isfinite(r.scale_hi) || r.scale_lo > r.scale_hi) return "scale (finite, scale_lo <= scale_hi)";
    if (r.mask_channel != BT_SCATTER_NO_MASK && r.mask_channel > 3u) return "mask_channel (0 .. 3 or BT_SCATTER_NO_MASK)";
    if (r.mask_channel != BT_SCATTER_NO_MASK && !masked) return "a mask_channel without a mask attachment";
    return nullptr;
}

}  // namespace

extern "C" {

bt_status bt_atlas_scatter_instances(bt_atlas* a, uint32_t hi, uint32_t mi, const bt_terrain_model* model, const bt_tile_coordinate* coords, uint32_t count,
                                     const bt_scatter_rule* rules, uint32_t rule_count, uint32_t seed, float jitter, bt_scatter_instance* out, uint64_t cap,
                                     uint64_t* out_first, bt_scatter_stats* stats) {
    const char* who = "bt_atlas_scatter_instances";
    if (stats) *stats = bt_scatter_stats{};
    // what can be refused without the atlas is refused without it (as SPLAT's rules are)
    if (!model || !rules || !stats || (count && !coords) || (cap && !out)) {
        set_error("%s: NULL %s", who, !model ? "model" : !rules ? "rules" : !stats ? "stats" : count && !coords ? "coords with count > 0" : "out_host with cap > 0");
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (rule_count == 0u || rule_count > BT_SCATTER_MAX_RULES) {
        set_error("%s: %u rules (1 .. %u)", who, rule_count, unsigned(BT_SCATTER_MAX_RULES));
        return BT_ERR_INVALID_ARGUMENT;
    }
    const bool masked = mi != BT_SCATTER_NO_MASK;
    for (uint32_t i = 0; i < rule_count; i++)
        if (const char* bad = bad_scatter_rule(rules[i], masked)) {
            set_error("%s: rule %u: %s", who, i, bad);
            return BT_ERR_INVALID_ARGUMENT;
        }
    if (!(jitter >= 0.0f && jitter <= 1.0f)) {
        set_error("%s: jitter %g (in [0, 1])", who, double(jitter));
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (bt_status s = check_model(model, who)) return s;
    if (!a) {
        set_error("%s: NULL atlas", who);
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (hi >= a->attachments.size() || (masked && (mi == hi || mi >= a->attachments.size()))) {
        set_error("%s: height attachment %u and mask attachment %u of %zu", who, hi, mi, a->attachments.size());
        return BT_ERR_INVALID_ARGUMENT;
    }
    const Attachment& heights = a->attachments[hi];
    const AttachmentMeta& hm = heights.meta;
    if (hm.format != BT_FORMAT_R16) {
        set_error("%s: height attachment format %u (the rules read R16 heights)", who, hm.format);
        return BT_ERR_UNSUPPORTED;
    }
    if (masked) {
        const AttachmentMeta& mm = a->attachments[mi].meta;
        if (mm.format != BT_FORMAT_RGBA8) {
            set_error("%s: mask attachment format %u (a mask channel is a byte of an Rgba8 texel)", who, mm.format);
            return BT_ERR_UNSUPPORTED;
        }
        if (hm.texture_size != mm.texture_size || hm.border_size != mm.border_size) {
            set_error("%s: heights of texture_size %u, border_size %u and a mask of %u, %u: a cell reads the mask texel in its place", who, hm.texture_size,
                      hm.border_size, mm.texture_size, mm.border_size);
            return BT_ERR_UNSUPPORTED;
        }
    }
    if (hm.border_size == 0) {
        set_error("%s: attachment %u has no border (the taps of an edge cell need the neighbour's texels)", who, hi);
        return BT_ERR_UNSUPPORTED;
    }
    if (hm.center_size % 2u) {
        set_error("%s: odd centre size %u (texture_size %u, border_size %u)", who, hm.center_size, hm.texture_size, hm.border_size);
        return BT_ERR_UNSUPPORTED;
    }
    const model::Model md = model::make_model(*model);
    const uint32_t layers = masked ? std::min(hm.atlas_size, a->attachments[mi].meta.atlas_size) : hm.atlas_size;
    std::vector<ScatterTile> tiles(count);
    for (uint32_t i = 0; i < count; i++) {
        const bt_tile_coordinate& co = coords[i];
        if (co.side >= model::side_count(md) || co.lod >= a->config.lod_count || co.lod > 31u || (uint64_t(co.x) >> co.lod) || (uint64_t(co.y) >> co.lod)) {
            set_error("%s: coords[%u] = (%u, %u, %u, %u): side / lod / x / y out of range", who, i, co.side, co.lod, co.x, co.y);
            return BT_ERR_INVALID_ARGUMENT;
        }
        if ((uint64_t(hm.center_size) << co.lod) > 0xFFFFFFFFull) {
            set_error("%s: coords[%u]: a mosaic of %u x 2^%u texels", who, i, hm.center_size, co.lod);
            return BT_ERR_UNSUPPORTED;
        }
        const auto it = a->tile_states.find(co);
        if (it == a->tile_states.end() || it->second.atlas_index >= layers) {
            set_error("%s: the atlas holds no layer for coords[%u] = (%u, %u, %u, %u)", who, i, co.side, co.lod, co.x, co.y);
            return BT_ERR_INVALID_ARGUMENT;
        }
        tiles[i] = {it->second.atlas_index, co.lod, co.side, co.x, co.y};
    }
    if (!count) return BT_OK;
    ScatterJob job{};
    job.meta = hm, job.heights = heights.level0, job.mask = masked ? a->attachments[mi].level0 : nullptr;  // reads: no layer is marked written
    job.model = model, job.rules = rules, job.rule_count = rule_count, job.seed = seed, job.jitter = jitter;
    return scatter_run(a->ctx, job, tiles, out, cap, out_first, stats);
}

bt_status bt_atlas_splat_from_height(bt_atlas* a, uint32_t hi, uint32_t gi, const bt_terrain_model* model, uint32_t side, uint32_t lod, uint32_t x0, uint32_t y0,
                                     uint32_t width, uint32_t height, uint32_t mode, const bt_splat_rule* rules, uint32_t count, const uint8_t fallback[4],
                                     bt_tile_coordinate* changed, uint32_t changed_cap, bt_edit_stats* stats) {
    const char* who = "bt_atlas_splat_from_height";
    if (stats) *stats = bt_edit_stats{};
    // what can be refused without the atlas is refused without it (as the stamps of the brushes are)
    if (!model || !rules || !fallback || (changed_cap && !changed)) {
        set_error("%s: NULL %s", who, !model ? "model" : !rules ? "rules" : !fallback ? "fallback" : "changed with changed_cap > 0");
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (mode != BT_SPLAT_WEIGHTS && mode != BT_SPLAT_COLOUR) {
        set_error("%s: mode %u", who, mode);
        return BT_ERR_INVALID_ARGUMENT;
    }
    const uint32_t most = mode == BT_SPLAT_WEIGHTS ? BT_SPLAT_MAX_WEIGHT_RULES : BT_SPLAT_MAX_RULES;
    if (count == 0u || count > most) {
        set_error("%s: %u rules (1 .. %u in this mode)", who, count, most);
        return BT_ERR_INVALID_ARGUMENT;
    }
    for (uint32_t i = 0; i < count; i++)
        if (const char* bad = bad_rule(rules[i], mode)) {
            set_error("%s: rule %u: %s", who, i, bad);
            return BT_ERR_INVALID_ARGUMENT;
        }
    if (bt_status s = check_model(model, who)) return s;
    if (!a) {
        set_error("%s: NULL atlas", who);
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (hi == gi || hi >= a->attachments.size() || gi >= a->attachments.size()) {
        set_error("%s: height attachment %u and target attachment %u of %zu", who, hi, gi, a->attachments.size());
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (bt_status s = check_region(a, gi, side, lod, x0, y0, width, height, kColours, who)) return s;
    const Attachment& heights = a->attachments[hi];
    const AttachmentMeta& hm = heights.meta;
    const AttachmentMeta& gm = a->attachments[gi].meta;
    if (hm.format != BT_FORMAT_R16) {
        set_error("%s: height attachment format %u (the rules read R16 heights)", who, hm.format);
        return BT_ERR_UNSUPPORTED;
    }
    if (hm.texture_size != gm.texture_size || hm.border_size != gm.border_size) {
        set_error("%s: heights of texture_size %u, border_size %u and a target of %u, %u: a target texel is derived from the height texel in its place", who,
                  hm.texture_size, hm.border_size, gm.texture_size, gm.border_size);
        return BT_ERR_UNSUPPORTED;
    }
    if (hm.border_size == 0) {
        set_error("%s: attachment %u has no border (the taps of an edge texel need the neighbour's texels)", who, hi);
        return BT_ERR_UNSUPPORTED;
    }
    if (!width || !height) return BT_OK;
    FirstStep first{FirstStep::kSplat};
    first.stamps = rules, first.count = count;
    first.splat.meta = hm, first.splat.level0 = heights.level0, first.splat.model = model;  // a read of the heights: no layer of theirs is marked written
    first.splat.lod = lod, first.splat.mode = mode, first.splat.count = count;
    memcpy(&first.splat.fallback, fallback, 4);
    return edit_boxes(a, gi, lod, {Box{side, {x0, y0, x0 + width - 1u, y0 + height - 1u}}}, first, changed, changed_cap, stats);
}

bt_status bt_atlas_edit_height(bt_atlas* a, uint32_t ai, uint32_t lod, const bt_edit_stamp* stamps, uint32_t count, bt_tile_coordinate* changed,
                               uint32_t changed_cap, bt_edit_stats* stats) {
    if (stats) *stats = bt_edit_stats{};
    if (bt_status s = check_stamps("bt_atlas_edit_height", kHeights, a, ai, lod, stamps, count, changed, changed_cap, [](bool) { return BT_OK; })) return s;
    if (!count) return BT_OK;
    FirstStep first{FirstStep::kBrush};
    first.stamps = stamps, first.count = count;
    return edit_boxes(a, ai, lod, stamp_boxes(a, ai, lod, stamps, count), first, changed, changed_cap, stats);
}

bt_status bt_atlas_smooth_height(bt_atlas* a, uint32_t ai, uint32_t lod, uint32_t kernel_radius, const bt_smooth_stamp* stamps, uint32_t count,
                                 bt_tile_coordinate* changed, uint32_t changed_cap, bt_edit_stats* stats) {
    if (stats) *stats = bt_edit_stats{};
    auto check_kernel = [&](bool with_target) {
        if (!with_target && (kernel_radius == 0u || kernel_radius > BT_SMOOTH_MAX_KERNEL)) {
            set_error("bt_atlas_smooth_height: kernel_radius %u (1 .. %u)", kernel_radius, BT_SMOOTH_MAX_KERNEL);
            return BT_ERR_INVALID_ARGUMENT;
        }
        if (with_target && kernel_radius > a->attachments[ai].meta.border_size) {
            set_error("bt_atlas_smooth_height: kernel_radius %u beyond border_size %u: the box would leave the tile's layer", kernel_radius, a->attachments[ai].meta.border_size);
            return BT_ERR_UNSUPPORTED;
        }
        return BT_OK;
    };
    if (bt_status s = check_stamps("bt_atlas_smooth_height", kHeights, a, ai, lod, stamps, count, changed, changed_cap, check_kernel)) return s;
    if (!count) return BT_OK;
    FirstStep first{FirstStep::kSmooth};
    first.stamps = stamps, first.count = count, first.kernel_radius = kernel_radius;
    return edit_boxes(a, ai, lod, stamp_boxes(a, ai, lod, stamps, count), first, changed, changed_cap, stats);
}

bt_status bt_atlas_paint(bt_atlas* a, uint32_t ai, uint32_t lod, const bt_paint_stamp* stamps, uint32_t count, bt_tile_coordinate* changed, uint32_t changed_cap,
                         bt_edit_stats* stats) {
    if (stats) *stats = bt_edit_stats{};
    if (bt_status s = check_stamps("bt_atlas_paint", kColours, a, ai, lod, stamps, count, changed, changed_cap, [](bool) { return BT_OK; })) return s;
    if (!count) return BT_OK;
    FirstStep first{FirstStep::kPaint};
    first.stamps = stamps, first.count = count;
    return edit_boxes(a, ai, lod, stamp_boxes(a, ai, lod, stamps, count), first, changed, changed_cap, stats);
}

bt_status bt_atlas_write_region(bt_atlas* a, uint32_t ai, uint32_t side, uint32_t lod, uint32_t x0, uint32_t y0, uint32_t width, uint32_t height,
                                const void* texels, uint64_t row_pitch, bt_tile_coordinate* changed, uint32_t changed_cap, bt_edit_stats* stats) {
    if (stats) *stats = bt_edit_stats{};
    if (!a) {
        set_error("bt_atlas_write_region: NULL atlas");
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (changed_cap && !changed) {
        set_error("bt_atlas_write_region: NULL changed with changed_cap > 0");
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (bt_status s = check_region(a, ai, side, lod, x0, y0, width, height, kTexels, "bt_atlas_write_region")) return s;
    const Attachment& at = a->attachments[ai];
    if (!width || !height) return BT_OK;
    const uint64_t row_bytes = uint64_t(width) * at.meta.pixel_size;
    if (!row_pitch) row_pitch = row_bytes;
    if (!texels || row_pitch < row_bytes) {
        set_error("bt_atlas_write_region: %s", !texels ? "NULL texels_host" : "row_pitch smaller than a row");
        return BT_ERR_INVALID_ARGUMENT;
    }
    FirstStep first{FirstStep::kRegion};
    first.texels = texels, first.row_pitch = row_pitch;
    first.x0 = x0, first.y0 = y0, first.width = width, first.height = height;
    bt_status rc = edit_boxes(a, ai, lod, {Box{side, {x0, y0, x0 + width - 1u, y0 + height - 1u}}}, first, changed, changed_cap, stats);
    // the one wait of this call, for its staging copies (the ring's rule no longer needs it: whether it can go is a later question)
    const bt_status drained = a->ctx->staging.drain();
    return rc ? rc : drained;
}

}  // extern "C"

bt_status bt::region_check(const bt_atlas* a, uint32_t ai, uint32_t side, uint32_t lod, uint32_t x0, uint32_t y0, uint32_t width, uint32_t height, const char* what) {
    return check_region(a, ai, side, lod, x0, y0, width, height, kTexels, what);
}

bt_status bt::region_gather(const bt_atlas* a, uint32_t ai, uint32_t side, uint32_t lod, uint32_t x0, uint32_t y0, uint32_t width, uint32_t height, void* dst, uint32_t* tiles_missing) {
    const Attachment& at = a->attachments[ai];
    bt_ctx* ctx = a->ctx;
    // the items: the rectangle's part of every tile the atlas holds, as a write's first level
    DirtyTiles tiles;
    const uint64_t met = meet_tiles(a, at.meta.center_size, lod, {Box{side, {x0, y0, x0 + width - 1u, y0 + height - 1u}}}, tiles);
    const uint64_t missing = met - std::min<uint64_t>(met, tiles.size());
    if (tiles_missing) *tiles_missing = uint32_t(std::min<uint64_t>(missing, 0xFFFFFFFFull));
    std::vector<EditItem> items;
    uint32_t max_rows = 0;
    for (const auto& [coord, d] : tiles) {
        items.push_back(make_item(coord, d, at.meta.center_size));
        max_rows = std::max(max_rows, d.r.y1 - d.r.y0 + 1u);
    }
    // layers -> the rectangle on the device (what no tile covers: zeros, from a memset queued before the launch)
    if (missing) BT_HIP(hipMemsetAsync(dst, 0, uint64_t(width) * height * at.meta.pixel_size, ctx->stream));
    if (items.empty()) return BT_OK;
    PlanRing ring;
    const uint64_t items_at = ring.add(items);
    uint8_t* dev = nullptr;
    if (bt_status s = ring.commit(ctx, &dev)) return s;
    return launch_edit_gather(ctx->stream, at.meta, at.level0, (const EditItem*)(dev + items_at), uint32_t(items.size()), max_rows, dst, x0, y0, width);
}

bt_status bt::region_stage_in(bt_ctx* ctx, void* dst, const void* texels, uint64_t row_bytes, uint64_t row_pitch, uint32_t height) {
    const uint64_t total = row_bytes * height;
    StagingRing& ring = ctx->staging;
    if (bt_status s = ring.reserve(size_t(row_bytes), size_t(std::min<uint64_t>(total, 32ull << 20)))) return s;
    const uint32_t chunk_rows = uint32_t(std::min<uint64_t>(height, ring.bytes() / row_bytes));
    uint32_t chunk = 0;
    for (uint32_t row = 0; row < height; row += chunk_rows, chunk++) {
        const uint32_t k = chunk % StagingRing::kBuffers, rows = std::min(chunk_rows, height - row);
        if (bt_status s = ring.wait(k)) return s;
        for (uint32_t r = 0; r < rows; r++) memcpy((uint8_t*)ring.buffer(k) + r * row_bytes, (const uint8_t*)texels + (uint64_t(row) + r) * row_pitch, row_bytes);
        BT_HIP(hipMemcpyAsync((uint8_t*)dst + row * row_bytes, ring.buffer(k), rows * row_bytes, hipMemcpyHostToDevice, ctx->stream));
        if (bt_status s = ring.record(k, ctx->stream)) return s;
    }
    return BT_OK;
}

bt_status bt::region_stage_out(bt_ctx* ctx, const void* src, void* texels, uint64_t row_bytes, uint64_t row_pitch, uint32_t height, const char* what) {
    // the rectangle -> pinned staging -> host rows, in chunks of whole rows: a buffer is emptied before the chunk after next lands
    const uint64_t total = row_bytes * height;
    StagingRing& ring = ctx->staging;
    if (bt_status s = ring.reserve(size_t(row_bytes), size_t(std::min<uint64_t>(total, 32ull << 20)))) return s;
    const uint32_t chunk_rows = uint32_t(std::min<uint64_t>(height, ring.bytes() / row_bytes));
    auto rows_of = [&](uint32_t chunk) { return std::min(chunk_rows, height - chunk * chunk_rows); };
    auto enqueue = [&](uint32_t chunk, uint32_t k) {
        return hipMemcpyAsync(ring.buffer(k), (const uint8_t*)src + uint64_t(chunk) * chunk_rows * row_bytes, rows_of(chunk) * row_bytes, hipMemcpyDeviceToHost, ctx->stream);
    };
    auto landed = [&](uint32_t chunk, uint32_t k) {
        for (uint32_t r = 0; r < rows_of(chunk); r++) memcpy((uint8_t*)texels + (uint64_t(chunk) * chunk_rows + r) * row_pitch, (const uint8_t*)ring.buffer(k) + r * row_bytes, row_bytes);
    };
    return stage_out_chunks(ring, ctx->stream, (height + chunk_rows - 1u) / chunk_rows, what, enqueue, landed);
}

extern "C" {

bt_status bt_atlas_read_region(bt_atlas* a, uint32_t ai, uint32_t side, uint32_t lod, uint32_t x0, uint32_t y0, uint32_t width, uint32_t height, void* texels,
                               uint64_t row_pitch, uint32_t* tiles_missing) {
    if (tiles_missing) *tiles_missing = 0;
    if (!a) {
        set_error("bt_atlas_read_region: NULL atlas");
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (bt_status s = check_region(a, ai, side, lod, x0, y0, width, height, kTexels, "bt_atlas_read_region")) return s;
    const Attachment& at = a->attachments[ai];
    if (!width || !height) return BT_OK;
    const uint64_t row_bytes = uint64_t(width) * at.meta.pixel_size;
    if (!row_pitch) row_pitch = row_bytes;
    if (!texels || row_pitch < row_bytes) {
        set_error("bt_atlas_read_region: %s", !texels ? "NULL texels_host" : "row_pitch smaller than a row");
        return BT_ERR_INVALID_ARGUMENT;
    }
    bt_ctx* ctx = a->ctx;
    BT_HIP(hipSetDevice(ctx->device));
    const uint64_t total = row_bytes * height;
    if (bt_status s = ctx->edit_region.reserve(ctx, total)) return s;
    if (bt_status s = region_gather(a, ai, side, lod, x0, y0, width, height, ctx->edit_region.dev, tiles_missing)) return s;
    return region_stage_out(ctx, ctx->edit_region.dev, texels, row_bytes, row_pitch, height, "bt_atlas_read_region staging");
}

}  // extern "C"

namespace {

// the first defect of the erosion parameters, or nullptr
const char* bad_erosion(const bt_erosion_params& p) {
    auto finite_from = [](float v, float lo, bool open) { return std::isfinite(v) && (open ? v > lo : v >= lo); };
    if (!std::isfinite(p.min_height) || !std::isfinite(p.max_height)) return "min_height / max_height (not finite)";
    if (!finite_from(p.max_height - p.min_height, 0.0f, true)) return "max_height - min_height (finite and > 0)";
    if (!finite_from(p.cell_size, 0.0f, true)) return "cell_size (finite and > 0)";
    if (!finite_from(p.dt, 0.0f, true)) return "dt (finite and > 0)";
    if (!finite_from(p.rain, 0.0f, false)) return "rain (finite and >= 0)";
    if (!finite_from(p.evaporation, 0.0f, false)) return "evaporation (finite and >= 0)";
    if (!finite_from(p.gravity, 0.0f, true)) return "gravity (finite and > 0)";
    if (!finite_from(p.capacity, 0.0f, false)) return "capacity (finite and >= 0)";
    if (!(p.erode >= 0.0f && p.erode <= 1.0f) || !(p.deposit >= 0.0f && p.deposit <= 1.0f)) return "erode / deposit (in [0, 1])";
    if (!(p.min_tilt >= 0.0f && p.min_tilt <= 1.0f)) return "min_tilt (in [0, 1])";
    if (!finite_from(p.min_depth, 0.0f, true)) return "min_depth (finite and > 0)";
    if (p.steps == 0u || p.steps > BT_ERODE_MAX_STEPS) return "steps (1 .. BT_ERODE_MAX_STEPS)";
    return nullptr;
}

// the index of the first entry of a host plane that is negative or not finite, or `cells`
uint64_t first_bad_entry(const float* plane, uint64_t cells) {
    for (uint64_t i = 0; i < cells; i++)
        if (!(plane[i] >= 0.0f) || !std::isfinite(plane[i])) return i;
    return cells;
}

}  // namespace

extern "C" {

bt_status bt_atlas_erode_height(bt_atlas* a, uint32_t ai, uint32_t side, uint32_t lod, uint32_t x0, uint32_t y0, uint32_t width, uint32_t height,
                                const bt_erosion_params* params, const uint8_t* weight_host, float* water_host, float* sediment_host, bt_tile_coordinate* changed,
                                uint32_t changed_cap, bt_erosion_stats* stats) {
    const char* who = "bt_atlas_erode_height";
    if (stats) *stats = bt_erosion_stats{};
    if (!a || (changed_cap && !changed)) {
        set_error("%s: NULL %s", who, !a ? "atlas" : "changed with changed_cap > 0");
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (bt_status s = check_region(a, ai, side, lod, x0, y0, width, height, kTexels, who)) return s;
    const Attachment& at = a->attachments[ai];
    if (at.meta.format != BT_FORMAT_R16) {
        set_error("%s: attachment format %u (heights are R16)", who, at.meta.format);
        return BT_ERR_UNSUPPORTED;
    }
    if (!params) {
        set_error("%s: NULL params", who);
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (const char* bad = bad_erosion(*params)) {
        set_error("%s: %s", who, bad);
        return BT_ERR_INVALID_ARGUMENT;
    }
    const uint64_t cells = uint64_t(width) * height;
    if (cells > BT_ERODE_MAX_CELLS) {
        set_error("%s: %u x %u cells, at most %u", who, width, height, BT_ERODE_MAX_CELLS);
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (!cells) return BT_OK;
    for (const float* plane : {(const float*)water_host, (const float*)sediment_host}) {
        if (!plane) continue;
        const uint64_t bad = first_bad_entry(plane, cells);
        if (bad < cells) {
            set_error("%s: %s[%llu] = %g (finite and >= 0)", who, plane == water_host ? "water_host" : "sediment_host", (unsigned long long)bad, double(plane[bad]));
            return BT_ERR_INVALID_ARGUMENT;
        }
    }

    const bt_erosion_params& p = *params;
    ErodeConsts c{};
    c.min_height = p.min_height, c.range = p.max_height - p.min_height, c.cell_size = p.cell_size, c.dt = p.dt;
    c.capacity = p.capacity, c.erode = p.erode, c.deposit = p.deposit, c.min_tilt = p.min_tilt, c.min_depth = p.min_depth;
    c.rain_dt = p.dt * p.rain;
    c.cf = (p.dt * p.gravity) * p.cell_size;
    c.l2 = p.cell_size * p.cell_size;
    c.two_l = 2.0f * p.cell_size;
    const float e = p.evaporation * p.dt;
    c.keep = 1.0f - (e < 1.0f ? e : 1.0f);

    bt_ctx* ctx = a->ctx;
    BT_HIP(hipSetDevice(ctx->device));
    hipStream_t stream = ctx->stream;
    // the planes of the call, carved from one buffer: the gathered texels, the activity and weight bytes, 2 x 7 float planes
    const uint64_t plane = align256(cells * 4u);
    const uint64_t at_raw = 0, at_act = at_raw + align256(cells * 2u), at_weight = at_act + align256(cells), at_state = at_weight + (weight_host ? align256(cells) : 0u);
    if (bt_status s = ctx->erode.reserve(ctx, at_state + 14u * plane)) return s;
    if (bt_status s = ctx->edit_region.reserve(ctx, cells * 2u)) return s;
    uint8_t* base = (uint8_t*)ctx->erode.dev;
    uint16_t* raw = (uint16_t*)(base + at_raw);
    uint8_t* act = base + at_act;
    uint8_t* weight = weight_host ? base + at_weight : nullptr;
    ErodePlanes planes[2];
    for (uint32_t i = 0; i < 2u; i++) {
        float* first = (float*)(base + at_state + i * 7u * plane);
        const uint64_t stride = plane / 4u;
        planes[i].b = first, planes[i].d = first + stride, planes[i].s = first + 2u * stride;
        for (uint32_t k = 0; k < 4u; k++) planes[i].f[k] = first + (3u + k) * stride;
    }

    uint32_t tiles_missing = 0;
    if (bt_status s = region_gather(a, ai, side, lod, x0, y0, width, height, raw, &tiles_missing)) return s;
    if (weight)
        if (bt_status s = region_stage_in(ctx, weight, weight_host, width, width, height)) return s;
    if (water_host)
        if (bt_status s = region_stage_in(ctx, planes[0].d, water_host, uint64_t(width) * 4u, uint64_t(width) * 4u, height)) return s;
    if (sediment_host)
        if (bt_status s = region_stage_in(ctx, planes[0].s, sediment_host, uint64_t(width) * 4u, uint64_t(width) * 4u, height)) return s;
    if (bt_status s = launch_erode_init(stream, raw, water_host != nullptr, sediment_host != nullptr, planes[0], act, uint32_t(cells), c)) return s;
    for (uint32_t step = 0; step < p.steps; step++)
        if (bt_status s = launch_erode_step(stream, planes[step & 1u], planes[(step + 1u) & 1u], act, width, height, c)) return s;
    const ErodePlanes& last = planes[p.steps & 1u];
    if (bt_status s = launch_erode_finish(stream, raw, last.b, weight, (uint16_t*)ctx->edit_region.dev, uint32_t(cells), c)) return s;
    if (water_host)
        if (bt_status s = region_stage_out(ctx, last.d, water_host, uint64_t(width) * 4u, uint64_t(width) * 4u, height, "bt_atlas_erode_height staging")) return s;
    if (sediment_host)
        if (bt_status s = region_stage_out(ctx, last.s, sediment_host, uint64_t(width) * 4u, uint64_t(width) * 4u, height, "bt_atlas_erode_height staging")) return s;

    FirstStep first{FirstStep::kRegion};  // texels nullptr: the rectangle is on the device
    first.x0 = x0, first.y0 = y0, first.width = width, first.height = height;
    bt_edit_stats edit{};
    bt_status rc = edit_boxes(a, ai, lod, {Box{side, {x0, y0, x0 + width - 1u, y0 + height - 1u}}}, first, changed, changed_cap, &edit);
    const bt_status drained = ctx->staging.drain();  // the staging copies of the weight plane (the only wait of a call without water and sediment)
    if (stats) {
        stats->cells = uint32_t(cells), stats->tiles_missing = tiles_missing, stats->steps = p.steps, stats->sim_launches = p.steps + 2u;
        stats->edit = edit;
    }
    return rc ? rc : drained;
}

// The host half of the DISTANCE section of the header (the kernels: bt_distance.hip).  It lives here for the bake, which is the device-side
// write-back of bt_atlas_erode_height: the merged rectangle in ctx->edit_region and a region first step without host texels.
bt_status bt_atlas_distance_field(bt_atlas* a, uint32_t ai, uint32_t side, uint32_t lod, uint32_t x0, uint32_t y0, uint32_t width, uint32_t height,
                                  const bt_distance_seeds* seeds, const uint8_t* seed_host, uint32_t* dist2_out, uint32_t* nearest_out, const bt_distance_bake* bake,
                                  bt_tile_coordinate* changed, uint32_t changed_cap, bt_distance_stats* stats) {
    const char* who = "bt_atlas_distance_field";
    if (stats) *stats = bt_distance_stats{};
    if (!a || (changed_cap && !changed)) {
        set_error("%s: NULL %s", who, !a ? "atlas" : "changed with changed_cap > 0");
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (bt_status s = check_region(a, ai, side, lod, x0, y0, width, height, kTexels, who)) return s;
    const Attachment& at = a->attachments[ai];
    const bool wide = at.meta.format == BT_FORMAT_RGBA8;
    if (!seeds) {
        set_error("%s: NULL seeds", who);
        return BT_ERR_INVALID_ARGUMENT;
    }
    const bool from_texels = (seeds->flags & BT_DISTANCE_FROM_TEXELS) != 0u;
    const uint32_t top = wide ? 255u : 65535u;
    const char* bad = (seeds->flags & ~uint32_t(BT_DISTANCE_FROM_TEXELS | BT_DISTANCE_INVERT)) ? "unknown flag bits"
                      : !from_texels && !seed_host                                            ? "neither BT_DISTANCE_FROM_TEXELS nor seed_host"
                      : seeds->channel > (wide ? 3u : 0u)                                     ? "channel (0..3 on Rgba8, 0 on R16)"
                      : seeds->hi > top                                                       ? "hi above the largest texel value"
                      : from_texels && seeds->lo > seeds->hi                                  ? "lo > hi"
                                                                                              : nullptr;
    if (bad) {
        set_error("%s: seeds: %s (channel %u, lo %u, hi %u, flags %#x)", who, bad, seeds->channel, seeds->lo, seeds->hi, seeds->flags);
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (width > BT_DISTANCE_MAX_SIDE || height > BT_DISTANCE_MAX_SIDE) {
        set_error("%s: a side of %u x %u above %u", who, width, height, BT_DISTANCE_MAX_SIDE);
        return BT_ERR_INVALID_ARGUMENT;
    }
    const uint64_t cells = uint64_t(width) * height;
    if (cells > BT_DISTANCE_MAX_CELLS) {
        set_error("%s: %u x %u cells, at most %u", who, width, height, BT_DISTANCE_MAX_CELLS);
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (bake) {
        const char* bad_bake = bake->attachment >= a->attachments.size()               ? "attachment out of range"
                               : bake->channel > 3u                                    ? "channel (0..3)"
                               : bake->reach == 0u || bake->reach > 65535u             ? "reach (1..65535)"
                               : (bake->flags & ~uint32_t(BT_DISTANCE_BAKE_NEAR)) != 0u ? "unknown flag bits"
                                                                                       : nullptr;
        if (bad_bake) {
            set_error("%s: bake: %s (attachment %u, channel %u, reach %u, flags %#x)", who, bad_bake, bake->attachment, bake->channel, bake->reach, bake->flags);
            return BT_ERR_INVALID_ARGUMENT;
        }
        const AttachmentMeta& dm = a->attachments[bake->attachment].meta;
        if (dm.format != BT_FORMAT_RGBA8 || dm.texture_size != at.meta.texture_size || dm.border_size != at.meta.border_size) {
            set_error("%s: bake: attachment %u (format %u, texture_size %u, border_size %u): an Rgba8 attachment of the source's texture_size %u and border_size %u", who,
                      bake->attachment, dm.format, dm.texture_size, dm.border_size, at.meta.texture_size, at.meta.border_size);
            return BT_ERR_UNSUPPORTED;
        }
    }
    if (!cells) return BT_OK;  // an empty window: nothing to do

    bt_ctx* ctx = a->ctx;
    BT_HIP(hipSetDevice(ctx->device));
    hipStream_t stream = ctx->stream;
    DistancePlanes p{};
    p.width = width, p.height = height, p.bands = (height + kDistanceBand - 1u) / kDistanceBand;
    // the planes of the call, carved from one buffer
    const uint64_t summary = align256(uint64_t(p.bands) * width * 2u);
    const uint64_t at_raw = 0, at_host = at_raw + align256(cells * at.meta.pixel_size), at_first = at_host + (seed_host ? align256(cells) : 0u), at_last = at_first + summary,
                   at_r = at_last + summary, at_dist2 = at_r + align256(cells * 2u), at_nearest = at_dist2 + align256(cells * 4u), total = at_nearest + align256(cells * 4u);
    if (bt_status s = ctx->distance.reserve(ctx, total)) return s;
    if (bt_status s = ctx->distance_words.reserve(ctx, 256, true)) return s;
    if (bake)
        if (bt_status s = ctx->edit_region.reserve(ctx, cells * 4u)) return s;
    uint8_t* base = (uint8_t*)ctx->distance.dev;
    p.raw = base + at_raw;
    p.host = seed_host ? base + at_host : nullptr;
    p.wide = wide, p.shift = 8u * seeds->channel, p.value_mask = top;
    p.lo = from_texels ? seeds->lo : 1u, p.hi = from_texels ? seeds->hi : 0u;
    p.invert = (seeds->flags & BT_DISTANCE_INVERT) != 0u;
    p.first = (uint16_t*)(base + at_first), p.last = (uint16_t*)(base + at_last), p.r = (uint16_t*)(base + at_r);
    p.dist2 = (uint32_t*)(base + at_dist2), p.nearest = (uint32_t*)(base + at_nearest);
    DistanceBake merge{};
    if (bake) merge.texels = (uint32_t*)ctx->edit_region.dev, merge.shift = 8u * bake->channel, merge.near = bake->flags & BT_DISTANCE_BAKE_NEAR, merge.reach2 = uint64_t(bake->reach) * bake->reach;
    DistanceCounts* counts = (DistanceCounts*)ctx->distance_words.dev;
    const DistanceCounts* counts_host = (const DistanceCounts*)ctx->distance_words.host;

    uint32_t tiles_missing = 0;
    if (bt_status s = region_gather(a, ai, side, lod, x0, y0, width, height, base + at_raw, &tiles_missing)) return s;
    if (seed_host)
        if (bt_status s = region_stage_in(ctx, base + at_host, seed_host, width, width, height)) return s;
    if (bake)
        if (bt_status s = region_gather(a, bake->attachment, side, lod, x0, y0, width, height, ctx->edit_region.dev, nullptr)) return s;
    BT_HIP(hipMemsetAsync(counts, 0, sizeof(DistanceCounts), stream));
    if (bt_status s = launch_distance_columns(stream, p)) return s;
    if (bt_status s = launch_distance_rows(stream, p)) return s;
    if (bt_status s = launch_distance_finish(stream, p, merge, counts)) return s;
    BT_HIP(hipMemcpyAsync((void*)counts_host, counts, sizeof(DistanceCounts), hipMemcpyDeviceToHost, stream));
    const char* what = "bt_atlas_distance_field staging";
    if (dist2_out)
        if (bt_status s = region_stage_out(ctx, p.dist2, dist2_out, uint64_t(width) * 4u, uint64_t(width) * 4u, height, what)) return s;
    if (nearest_out)
        if (bt_status s = region_stage_out(ctx, p.nearest, nearest_out, uint64_t(width) * 4u, uint64_t(width) * 4u, height, what)) return s;
    bt_edit_stats edit{};
    bt_status rc = BT_OK;
    if (bake) {
        FirstStep first{FirstStep::kRegion};  // texels nullptr: the rectangle is on the device
        first.x0 = x0, first.y0 = y0, first.width = width, first.height = height;
        rc = edit_boxes(a, bake->attachment, lod, {Box{side, {x0, y0, x0 + width - 1u, y0 + height - 1u}}}, first, changed, changed_cap, &edit);
    }
    const bt_status drained = ctx->staging.drain();  // the staging copies of the seed plane
    BT_HIP(hipStreamSynchronize(stream));
    if (stats) {
        stats->cells = uint32_t(cells), stats->seeds = counts_host->seeds, stats->tiles_missing = tiles_missing;
        stats->max_dist2 = counts_host->max_dist2, stats->sum_dist2 = counts_host->sum_dist2;
        stats->launches = bake ? 7u : 6u;  // the gather, the three of the column phase, the row phase, the finish; a bake's gather
        stats->edit = edit;
    }
    return rc ? rc : drained;
}

// The host half of the REGIONS section of the header (the kernels: bt_regions.hip).  It lives here for the bake, as
// bt_atlas_distance_field does.
bt_status bt_atlas_label_regions(bt_atlas* a, uint32_t ai, uint32_t side, uint32_t lod, uint32_t x0, uint32_t y0, uint32_t width, uint32_t height,
                                 const bt_regions_rule* rule, const uint8_t* member_host, uint32_t* label_out, uint32_t* id_out, bt_region* regions_out, uint32_t region_cap,
                                 const bt_regions_bake* bake, bt_tile_coordinate* changed, uint32_t changed_cap, bt_regions_stats* stats) {
    const char* who = "bt_atlas_label_regions";
    if (stats) *stats = bt_regions_stats{};
    if (!a || (changed_cap && !changed) || (region_cap && !regions_out)) {
        set_error("%s: NULL %s", who, !a ? "atlas" : (changed_cap && !changed) ? "changed with changed_cap > 0" : "regions_out with region_cap > 0");
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (bt_status s = check_region(a, ai, side, lod, x0, y0, width, height, kTexels, who)) return s;
    const Attachment& at = a->attachments[ai];
    const bool wide = at.meta.format == BT_FORMAT_RGBA8;
    if (!rule) {
        set_error("%s: NULL rule", who);
        return BT_ERR_INVALID_ARGUMENT;
    }
    const bool from_texels = (rule->flags & BT_REGIONS_FROM_TEXELS) != 0u;
    const uint32_t top = wide ? 255u : 65535u;
    const char* bad = (rule->flags & ~uint32_t(BT_REGIONS_FROM_TEXELS | BT_REGIONS_INVERT | BT_REGIONS_EIGHT)) ? "unknown flag bits"
                      : !from_texels && !member_host                                                         ? "neither BT_REGIONS_FROM_TEXELS nor member_host"
                      : rule->channel > (wide ? 3u : 0u)                                                     ? "channel (0..3 on Rgba8, 0 on R16)"
                      : rule->hi > top                                                                       ? "hi above the largest texel value"
                      : from_texels && rule->lo > rule->hi                                                   ? "lo > hi"
                      : rule->max_step > 65535u                                                              ? "max_step (0..65535)"
                                                                                                             : nullptr;
    if (bad) {
        set_error("%s: rule: %s (channel %u, lo %u, hi %u, max_step %u, flags %#x)", who, bad, rule->channel, rule->lo, rule->hi, rule->max_step, rule->flags);
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (width > BT_REGIONS_MAX_SIDE || height > BT_REGIONS_MAX_SIDE) {
        set_error("%s: a side of %u x %u above %u", who, width, height, BT_REGIONS_MAX_SIDE);
        return BT_ERR_INVALID_ARGUMENT;
    }
    const uint64_t cells = uint64_t(width) * height;
    if (cells > BT_REGIONS_MAX_CELLS) {
        set_error("%s: %u x %u cells, at most %u", who, width, height, BT_REGIONS_MAX_CELLS);
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (bake) {
        const char* bad_bake = bake->attachment >= a->attachments.size() ? "attachment out of range"
                               : bake->channel > 3u                      ? "channel (0..3)"
                               : bake->min_area > bake->max_area         ? "min_area > max_area"
                               : bake->value > 255u                      ? "value (0..255)"
                               : bake->flags != 0u                       ? "unknown flag bits"
                                                                         : nullptr;
        if (bad_bake) {
            set_error("%s: bake: %s (attachment %u, channel %u, min_area %u, max_area %u, value %u, flags %#x)", who, bad_bake, bake->attachment, bake->channel, bake->min_area,
                      bake->max_area, bake->value, bake->flags);
            return BT_ERR_INVALID_ARGUMENT;
        }
        const AttachmentMeta& dm = a->attachments[bake->attachment].meta;
        if (dm.format != BT_FORMAT_RGBA8 || dm.texture_size != at.meta.texture_size || dm.border_size != at.meta.border_size) {
            set_error("%s: bake: attachment %u (format %u, texture_size %u, border_size %u): an Rgba8 attachment of the source's texture_size %u and border_size %u", who,
                      bake->attachment, dm.format, dm.texture_size, dm.border_size, at.meta.texture_size, at.meta.border_size);
            return BT_ERR_UNSUPPORTED;
        }
    }
    if (!cells) return BT_OK;  // an empty window: nothing to do

    bt_ctx* ctx = a->ctx;
    BT_HIP(hipSetDevice(ctx->device));
    hipStream_t stream = ctx->stream;
    RegionsPlanes p{};
    p.width = width, p.height = height;
    p.region_cap = uint32_t(std::min<uint64_t>(region_cap, cells));  // there are no more regions than cells
    // the planes of the call, carved from one buffer
    const uint64_t chunks = (cells + kRegionsChunk - 1u) / kRegionsChunk, plane = align256(cells * 4u);
    const uint64_t at_raw = 0, at_host = at_raw + align256(cells * at.meta.pixel_size), at_P = at_host + (member_host ? align256(cells) : 0u), at_id = at_P + plane,
                   at_area = at_id + plane, at_rank = at_area + plane, at_chunks = at_rank + plane, at_accum = at_chunks + align256(chunks * 4u),
                   at_table = at_accum + align256(p.region_cap * sizeof(RegionAccum)), total = at_table + align256(p.region_cap * sizeof(bt_region));
    if (bt_status s = ctx->regions.reserve(ctx, total)) return s;
    if (bt_status s = ctx->regions_words.reserve(ctx, 256, true)) return s;
    if (bake)
        if (bt_status s = ctx->edit_region.reserve(ctx, cells * 4u)) return s;
    uint8_t* base = (uint8_t*)ctx->regions.dev;
    p.raw = base + at_raw;
    p.host = member_host ? base + at_host : nullptr;
    p.wide = wide, p.shift = 8u * rule->channel, p.value_mask = top;
    p.lo = from_texels ? rule->lo : 1u, p.hi = from_texels ? rule->hi : 0u;
    p.invert = (rule->flags & BT_REGIONS_INVERT) != 0u, p.eight = (rule->flags & BT_REGIONS_EIGHT) != 0u;
    p.max_step = rule->max_step;
    p.P = (uint32_t*)(base + at_P), p.id = (uint32_t*)(base + at_id), p.area = (uint32_t*)(base + at_area), p.rank = (uint32_t*)(base + at_rank);
    p.chunk_roots = (uint32_t*)(base + at_chunks), p.accum = (RegionAccum*)(base + at_accum);
    bt_region* table = (bt_region*)(base + at_table);
    RegionsBake merge{};
    if (bake) merge.texels = (uint32_t*)ctx->edit_region.dev, merge.shift = 8u * bake->channel, merge.min_area = bake->min_area, merge.max_area = bake->max_area, merge.value = bake->value;
    RegionsCounts* counts = (RegionsCounts*)ctx->regions_words.dev;
    const RegionsCounts* counts_host = (const RegionsCounts*)ctx->regions_words.host;

    uint32_t tiles_missing = 0;
    if (bt_status s = region_gather(a, ai, side, lod, x0, y0, width, height, base + at_raw, &tiles_missing)) return s;
    if (member_host)
        if (bt_status s = region_stage_in(ctx, base + at_host, member_host, width, width, height)) return s;
    if (bake)
        if (bt_status s = region_gather(a, bake->attachment, side, lod, x0, y0, width, height, ctx->edit_region.dev, nullptr)) return s;
    BT_HIP(hipMemsetAsync(counts, 0, sizeof(RegionsCounts), stream));
    if (p.region_cap) BT_HIP(hipMemsetAsync(p.accum, 0, p.region_cap * sizeof(RegionAccum), stream));
    if (bt_status s = launch_regions_label(stream, p, counts)) return s;
    if (bt_status s = launch_regions_emit(stream, p)) return s;
    if (bt_status s = launch_regions_finish(stream, p, merge, counts, table)) return s;
    BT_HIP(hipMemcpyAsync((void*)counts_host, counts, sizeof(RegionsCounts), hipMemcpyDeviceToHost, stream));
    const char* what = "bt_atlas_label_regions staging";
    if (label_out)
        if (bt_status s = region_stage_out(ctx, p.P, label_out, uint64_t(width) * 4u, uint64_t(width) * 4u, height, what)) return s;
    if (id_out)
        if (bt_status s = region_stage_out(ctx, p.id, id_out, uint64_t(width) * 4u, uint64_t(width) * 4u, height, what)) return s;
    bt_edit_stats edit{};
    bt_status rc = BT_OK;
    if (bake) {
        FirstStep first{FirstStep::kRegion};  // texels nullptr: the rectangle is on the device
        first.x0 = x0, first.y0 = y0, first.width = width, first.height = height;
        rc = edit_boxes(a, bake->attachment, lod, {Box{side, {x0, y0, x0 + width - 1u, y0 + height - 1u}}}, first, changed, changed_cap, &edit);
    }
    const bt_status drained = ctx->staging.drain();  // the staging copies of the member plane
    BT_HIP(hipStreamSynchronize(stream));
    // the records: how many there are is known only now; rows of 1024 records and one of the rest
    const uint32_t written = std::min(counts_host->regions, region_cap);
    if (written) {
        constexpr uint32_t kRow = 1024;
        const uint32_t rows = written / kRow, rest = written % kRow;
        if (rows)
            if (bt_status s = region_stage_out(ctx, table, regions_out, kRow * sizeof(bt_region), kRow * sizeof(bt_region), rows, what)) return s;
        if (rest)
            if (bt_status s = region_stage_out(ctx, table + uint64_t(rows) * kRow, regions_out + uint64_t(rows) * kRow, rest * sizeof(bt_region), rest * sizeof(bt_region), 1, what)) return s;
    }
    if (stats) {
        stats->cells = uint32_t(cells), stats->members = counts_host->members, stats->regions = counts_host->regions, stats->regions_written = written;
        stats->largest_area = uint32_t(counts_host->largest >> 32), stats->largest_label = BT_REGIONS_NONE - uint32_t(counts_host->largest);
        stats->tiles_missing = tiles_missing, stats->baked = counts_host->baked;
        stats->launches = bake ? 8u : 7u;  // the gather, local, seams, flatten, scan, emit, finish; a bake's gather
        stats->edit = edit;
    }
    return rc ? rc : drained;
}

// The call of the SKYLINE section of the header (the kernels: bt_skyline.hip; the line geometry and the plan: bt_skyline.cpp).  It lives
// here for the bake, as bt_atlas_distance_field does.
bt_status bt_atlas_skyline(bt_atlas* a, uint32_t ai, uint32_t side, uint32_t lod, uint32_t x0, uint32_t y0, uint32_t width, uint32_t height,
                           const bt_skyline_direction* directions, uint32_t direction_count, uint16_t* steps_out, int32_t* rise_out, uint64_t* mask_out, uint8_t* count_out,
                           const bt_skyline_bake* bake, bt_tile_coordinate* changed, uint32_t changed_cap, bt_skyline_stats* stats) {
    const char* who = "bt_atlas_skyline";
    if (stats) *stats = bt_skyline_stats{};
    if (!a || (changed_cap && !changed)) {
        set_error("%s: NULL %s", who, !a ? "atlas" : "changed with changed_cap > 0");
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (bt_status s = check_region(a, ai, side, lod, x0, y0, width, height, kTexels, who)) return s;
    const Attachment& at = a->attachments[ai];
    if (at.meta.format != BT_FORMAT_R16) {
        set_error("%s: attachment format %u (heights are R16)", who, at.meta.format);
        return BT_ERR_UNSUPPORTED;
    }
    if (!directions) {
        set_error("%s: NULL directions", who);
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (direction_count == 0u || direction_count > BT_SKYLINE_MAX_DIRECTIONS) {
        set_error("%s: %u directions, 1 to %u", who, direction_count, BT_SKYLINE_MAX_DIRECTIONS);
        return BT_ERR_INVALID_ARGUMENT;
    }
    uint32_t which = 0;
    if (const char* bad = skyline_bad_direction(directions, direction_count, &which)) {
        const bt_skyline_direction& d = directions[which];
        set_error("%s: direction %u: %s (dx %d, dy %d, sun_num %u, sun_den %u)", who, which, bad, d.dx, d.dy, d.sun_num, d.sun_den);
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (width > BT_SKYLINE_MAX_SIDE || height > BT_SKYLINE_MAX_SIDE) {
        set_error("%s: a side of %u x %u above %u", who, width, height, BT_SKYLINE_MAX_SIDE);
        return BT_ERR_INVALID_ARGUMENT;
    }
    const uint64_t cells = uint64_t(width) * height;
    if (cells > BT_SKYLINE_MAX_CELLS) {
        set_error("%s: %u x %u cells, at most %u", who, width, height, BT_SKYLINE_MAX_CELLS);
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (bake) {
        const char* bad_bake = bake->attachment >= a->attachments.size()                 ? "attachment out of range"
                               : bake->channel > 3u                                      ? "channel (0..3)"
                               : (bake->flags & ~uint32_t(BT_SKYLINE_BAKE_SHADE)) != 0u ? "unknown flag bits"
                                                                                         : nullptr;
        if (bad_bake) {
            set_error("%s: bake: %s (attachment %u, channel %u, flags %#x)", who, bad_bake, bake->attachment, bake->channel, bake->flags);
            return BT_ERR_INVALID_ARGUMENT;
        }
        const AttachmentMeta& dm = a->attachments[bake->attachment].meta;
        if (dm.format != BT_FORMAT_RGBA8 || dm.texture_size != at.meta.texture_size || dm.border_size != at.meta.border_size) {
            set_error("%s: bake: attachment %u (format %u, texture_size %u, border_size %u): an Rgba8 attachment of the source's texture_size %u and border_size %u", who,
                      bake->attachment, dm.format, dm.texture_size, dm.border_size, at.meta.texture_size, at.meta.border_size);
            return BT_ERR_UNSUPPORTED;
        }
    }
    if (!cells) return BT_OK;  // an empty window: nothing to do

    bt_ctx* ctx = a->ctx;
    BT_HIP(hipSetDevice(ctx->device));
    hipStream_t stream = ctx->stream;
    const SkylinePlan plan = skyline_plan(width, height, directions, direction_count, bake != nullptr);
    // the planes of the call, carved from one buffer; the per-direction ones lie plane after plane, so a batch stages out as one rectangle
    const uint64_t at_raw = 0, at_transposed = at_raw + align256(cells * 2u), at_mask = at_transposed + align256(cells * 2u), at_count = at_mask + align256(cells * 8u),
                   at_stack = at_count + align256(cells), at_rise = at_stack + align256(plan.batch * cells * 4u), at_steps = at_rise + align256(plan.batch * cells * 4u),
                   total = at_steps + align256(plan.batch * cells * 2u);
    if (bt_status s = ctx->skyline.reserve(ctx, total)) return s;
    if (bt_status s = ctx->skyline_words.reserve(ctx, 256, true)) return s;
    if (bake)
        if (bt_status s = ctx->edit_region.reserve(ctx, cells * 4u)) return s;
    uint8_t* base = (uint8_t*)ctx->skyline.dev;
    SkylinePlanes p{};
    p.width = width, p.height = height;
    p.raw = (const uint16_t*)(base + at_raw), p.transposed = (uint16_t*)(base + at_transposed);
    p.stack = (uint32_t*)(base + at_stack), p.steps = (uint16_t*)(base + at_steps), p.rise = (int32_t*)(base + at_rise);
    p.mask = (uint64_t*)(base + at_mask), p.count = base + at_count;
    p.direction_count = direction_count;
    memcpy(p.directions, directions, sizeof(bt_skyline_direction) * direction_count);
    SkylineBake merge{};
    if (bake) merge.texels = (uint32_t*)ctx->edit_region.dev, merge.shift = 8u * bake->channel, merge.shade = bake->flags & BT_SKYLINE_BAKE_SHADE;
    SkylineCounts* counts = (SkylineCounts*)ctx->skyline_words.dev;
    const SkylineCounts* counts_host = (const SkylineCounts*)ctx->skyline_words.host;

    uint32_t tiles_missing = 0;
    if (bt_status s = region_gather(a, ai, side, lod, x0, y0, width, height, base + at_raw, &tiles_missing)) return s;
    if (bake)
        if (bt_status s = region_gather(a, bake->attachment, side, lod, x0, y0, width, height, ctx->edit_region.dev, nullptr)) return s;
    BT_HIP(hipMemsetAsync(counts, 0, sizeof(SkylineCounts), stream));
    if (bt_status s = launch_skyline_transpose(stream, p)) return s;
    const char* what = "bt_atlas_skyline staging";
    for (uint32_t first = 0; first < direction_count; first += plan.batch) {
        p.first = first, p.batch = std::min(plan.batch, direction_count - first);
        const bool last = first + p.batch == direction_count;
        if (bt_status s = launch_skyline_walk(stream, p)) return s;
        if (bt_status s = launch_skyline_finish(stream, p, last ? merge : SkylineBake{}, last, counts)) return s;
        // the batch's planes leave before the next batch overwrites them: the staging waits for its copies
        if (steps_out)
            if (bt_status s = region_stage_out(ctx, p.steps, steps_out + first * cells, uint64_t(width) * 2u, uint64_t(width) * 2u, p.batch * height, what)) return s;
        if (rise_out)
            if (bt_status s = region_stage_out(ctx, p.rise, rise_out + first * cells, uint64_t(width) * 4u, uint64_t(width) * 4u, p.batch * height, what)) return s;
    }
    BT_HIP(hipMemcpyAsync((void*)counts_host, counts, sizeof(SkylineCounts), hipMemcpyDeviceToHost, stream));
    if (mask_out)
        if (bt_status s = region_stage_out(ctx, p.mask, mask_out, uint64_t(width) * 8u, uint64_t(width) * 8u, height, what)) return s;
    if (count_out)
        if (bt_status s = region_stage_out(ctx, p.count, count_out, width, width, height, what)) return s;
    bt_edit_stats edit{};
    bt_status rc = BT_OK;
    if (bake) {
        FirstStep first{FirstStep::kRegion};  // texels nullptr: the rectangle is on the device
        first.x0 = x0, first.y0 = y0, first.width = width, first.height = height;
        rc = edit_boxes(a, bake->attachment, lod, {Box{side, {x0, y0, x0 + width - 1u, y0 + height - 1u}}}, first, changed, changed_cap, &edit);
    }
    BT_HIP(hipStreamSynchronize(stream));
    if (stats) {
        stats->cells = uint32_t(cells), stats->voids = counts_host->voids, stats->tiles_missing = tiles_missing, stats->directions = direction_count;
        stats->lines = plan.lines, stats->longest_line = plan.longest_line, stats->max_steps = counts_host->max_steps, stats->launches = plan.launches;
        stats->lit = counts_host->lit, stats->sum_steps = counts_host->sum_steps;
        stats->edit = edit;
    }
    return rc;
}

// The call of the SHAPES section of the header (the kernel: bt_shapes.hip; the rules, the boxes and the records: bt_shapes.cpp).  It lives
// here for the write-back, as bt_atlas_distance_field does.
bt_status bt_atlas_rasterize_shapes(bt_atlas* a, uint32_t ai, uint32_t side, uint32_t lod, uint32_t x0, uint32_t y0, uint32_t width, uint32_t height, uint32_t channel,
                                    const bt_shape_vertex* vertices, uint32_t vertex_count, const bt_shape* shapes, uint32_t entry_count, uint32_t flags, uint8_t* count_out,
                                    uint16_t* last_out, bt_tile_coordinate* changed, uint32_t changed_cap, bt_shapes_stats* stats) {
    const char* who = "bt_atlas_rasterize_shapes";
    if (stats) *stats = bt_shapes_stats{};
    if (!a || (changed_cap && !changed)) {
        set_error("%s: NULL %s", who, !a ? "atlas" : "changed with changed_cap > 0");
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (bt_status s = check_region(a, ai, side, lod, x0, y0, width, height, kTexels, who)) return s;
    const Attachment& at = a->attachments[ai];
    const bool wide = at.meta.format == BT_FORMAT_RGBA8;
    const char* bad = (flags & ~uint32_t(BT_SHAPES_DRY_RUN)) != 0u                      ? "unknown flag bits"
                      : channel > (wide ? 3u : 0u)                                      ? "channel (0..3 on Rgba8, 0 on R16)"
                      : (!vertices && vertex_count) || (!shapes && entry_count)         ? "NULL vertices or shapes with a non-zero count"
                                                                                        : nullptr;
    if (bad) {
        set_error("%s: %s (channel %u, flags %#x)", who, bad, channel, flags);
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (width > BT_SHAPES_MAX_SIDE || height > BT_SHAPES_MAX_SIDE) {
        set_error("%s: a side of %u x %u above %u", who, width, height, BT_SHAPES_MAX_SIDE);
        return BT_ERR_INVALID_ARGUMENT;
    }
    const uint64_t cells = uint64_t(width) * height;
    if (cells > BT_SHAPES_MAX_CELLS) {
        set_error("%s: %u x %u cells, at most %u", who, width, height, BT_SHAPES_MAX_CELLS);
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (!cells || !entry_count) return BT_OK;  // an empty window or an empty list: nothing to do
    std::vector<ShapeRecord> records;
    uint32_t shape_count = 0, bad_entry = BT_SHAPES_NO_ENTRY;
    const char* defect = shapes_check(vertices, vertex_count, shapes, entry_count, width, height, nullptr, &records, &shape_count, &bad_entry);
    if (!defect && wide)
        for (uint32_t i = 0; i < entry_count && !defect; i++)
            if (shapes[i].value > 255u) defect = "value above 255 on Rgba8", bad_entry = i;
    if (defect) {
        if (bad_entry != BT_SHAPES_NO_ENTRY)
            set_error("%s: entry %u: %s", who, bad_entry, defect);
        else
            set_error("%s: %s", who, defect);
        return BT_ERR_INVALID_ARGUMENT;
    }

    // the planes outside U; U's part is staged over them
    if (count_out) memset(count_out, 0, cells);
    if (last_out) memset(last_out, 0xFF, cells * 2u);
    bt_shape_box u{1, 1, 0, 0};
    for (const ShapeRecord& r : records) {
        if (u.x_lo > u.x_hi) u = r.box;
        u.x_lo = std::min(u.x_lo, r.box.x_lo), u.y_lo = std::min(u.y_lo, r.box.y_lo), u.x_hi = std::max(u.x_hi, r.box.x_hi), u.y_hi = std::max(u.y_hi, r.box.y_hi);
    }
    if (stats) stats->cells = uint32_t(cells), stats->shapes = shape_count, stats->shapes_culled = shape_count - uint32_t(records.size()), stats->box = u;
    if (records.empty()) return BT_OK;  // U is empty: nothing is written

    bt_ctx* ctx = a->ctx;
    BT_HIP(hipSetDevice(ctx->device));
    hipStream_t stream = ctx->stream;
    const uint32_t uw = uint32_t(u.x_hi) - u.x_lo + 1u, uh = uint32_t(u.y_hi) - u.y_lo + 1u, ux0 = x0 + u.x_lo, uy0 = y0 + u.y_lo;
    const uint64_t ucells = uint64_t(uw) * uh;
    const uint64_t vertex_bytes = uint64_t(vertex_count) * sizeof(bt_shape_vertex), entry_bytes = uint64_t(entry_count) * sizeof(bt_shape),
                   record_bytes = records.size() * sizeof(ShapeRecord);
    const uint64_t at_vertices = 0, at_entries = at_vertices + align256(vertex_bytes), at_records = at_entries + align256(entry_bytes), at_count = at_records + align256(record_bytes),
                   at_last = at_count + align256(ucells), total = at_last + align256(ucells * 2u);
    if (bt_status s = ctx->shapes.reserve(ctx, total)) return s;
    if (bt_status s = ctx->shapes_words.reserve(ctx, 256, true)) return s;
    if (bt_status s = ctx->edit_region.reserve(ctx, ucells * at.meta.pixel_size)) return s;
    uint8_t* base = (uint8_t*)ctx->shapes.dev;
    ShapesJob job{};
    job.vertices = (const bt_shape_vertex*)(base + at_vertices), job.entries = (const bt_shape*)(base + at_entries), job.records = (const ShapeRecord*)(base + at_records);
    job.record_count = uint32_t(records.size()), job.wide = wide, job.shift = 8u * channel, job.u = u;
    job.texels = ctx->edit_region.dev, job.count = base + at_count, job.last = (uint16_t*)(base + at_last);
    job.counts = (ShapesCounts*)ctx->shapes_words.dev;
    const ShapesCounts* counts_host = (const ShapesCounts*)ctx->shapes_words.host;

    uint32_t tiles_missing = 0;
    if (bt_status s = region_gather(a, ai, side, lod, ux0, uy0, uw, uh, job.texels, &tiles_missing)) return s;
    // the three arrays, each as one row
    if (bt_status s = region_stage_in(ctx, base + at_vertices, vertices, vertex_bytes, vertex_bytes, 1)) return s;
    if (bt_status s = region_stage_in(ctx, base + at_entries, shapes, entry_bytes, entry_bytes, 1)) return s;
    if (bt_status s = region_stage_in(ctx, base + at_records, records.data(), record_bytes, record_bytes, 1)) return s;
    BT_HIP(hipMemsetAsync(job.counts, 0, sizeof(ShapesCounts), stream));
    if (bt_status s = launch_shapes_raster(stream, job)) return s;
    BT_HIP(hipMemcpyAsync((void*)counts_host, job.counts, sizeof(ShapesCounts), hipMemcpyDeviceToHost, stream));
    const char* what = "bt_atlas_rasterize_shapes staging";
    const uint64_t origin = uint64_t(u.y_lo) * width + u.x_lo;
    if (count_out)
        if (bt_status s = region_stage_out(ctx, job.count, count_out + origin, uw, width, uh, what)) return s;
    if (last_out)
        if (bt_status s = region_stage_out(ctx, job.last, last_out + origin, uint64_t(uw) * 2u, uint64_t(width) * 2u, uh, what)) return s;
    bt_edit_stats edit{};
    bt_status rc = BT_OK;
    if (!(flags & BT_SHAPES_DRY_RUN)) {
        FirstStep first{FirstStep::kRegion};  // texels nullptr: the rectangle is on the device
        first.x0 = ux0, first.y0 = uy0, first.width = uw, first.height = uh;
        rc = edit_boxes(a, ai, lod, {Box{side, {ux0, uy0, ux0 + uw - 1u, uy0 + uh - 1u}}}, first, changed, changed_cap, &edit);
    }
    const bt_status drained = ctx->staging.drain();  // the staging copies of the list
    BT_HIP(hipStreamSynchronize(stream));
    if (stats) {
        stats->tiles_missing = tiles_missing, stats->covered = counts_host->covered, stats->written = counts_host->written;
        stats->launches = 2u;  // the gather and the raster
        stats->edit = edit;
    }
    return rc ? rc : drained;
}

bt_status bt_atlas_save_tiles(bt_atlas* a, uint32_t ai, const char* directory, const bt_tile_coordinate* coords, uint32_t count) {
    if (!a || !directory || (count && !coords)) {
        set_error("bt_atlas_save_tiles: NULL %s", !a ? "atlas" : !directory ? "directory" : "coords");
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (ai >= a->attachments.size()) {
        set_error("bt_atlas_save_tiles: attachment %u of %zu", ai, a->attachments.size());
        return BT_ERR_INVALID_ARGUMENT;
    }
    TileSaver::Tiles tiles;
    for (uint32_t i = 0; i < count; i++) {
        const uint32_t layer = layer_of(a, coords[i]);
        if (layer == BT_INVALID_ATLAS_INDEX) {
            set_error("bt_atlas_save_tiles: tile %u_%u_%u_%u is not in the atlas", coords[i].side, coords[i].lod, coords[i].x, coords[i].y);
            return BT_ERR_INVALID_ARGUMENT;
        }
        tiles.push_back({layer, coords[i]});
    }
    return save_tiles(a, ai, directory, std::move(tiles));
}

}  // extern "C"

// bt_atlas_viewshed: the host half (the kernels: bt_viewshed.hip; the definition: the VIEWSHED section of include/bevy_terrain_amd.h).
//
// The call checks its arguments, gathers the rectangle's texels on the device by the plan of bt_atlas_read_region, transposes them, walks
// the lines, counts, and stages the planes that were asked for out.  The observers travel in the kernel arguments.
#include <cstring>

#include "bt_internal.hpp"

using namespace bt;

extern "C" {

bt_status bt_atlas_viewshed(bt_atlas* a, uint32_t ai, uint32_t side, uint32_t lod, uint32_t x0, uint32_t y0, uint32_t width, uint32_t height, const bt_viewshed_observer* observers,
                            uint32_t observer_count, uint32_t target_height, uint32_t* clearance_out, uint8_t* count_out, uint64_t* mask_out, bt_viewshed_stats* stats) {
    if (stats) *stats = bt_viewshed_stats{};
    if (!a) {
        set_error("bt_atlas_viewshed: NULL %s", "atlas");
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (bt_status s = region_check(a, ai, side, lod, x0, y0, width, height, "bt_atlas_viewshed")) return s;
    const Attachment& at = a->attachments[ai];
    if (at.meta.format != BT_FORMAT_R16) {
        set_error("bt_atlas_viewshed: attachment format %u (heights are R16)", at.meta.format);
        return BT_ERR_UNSUPPORTED;
    }
    if (!observers) {
        set_error("bt_atlas_viewshed: NULL %s", "observers");
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (observer_count == 0u || observer_count > BT_VIEWSHED_MAX_OBSERVERS) {
        set_error("bt_atlas_viewshed: %u observers, 1 to %u", observer_count, BT_VIEWSHED_MAX_OBSERVERS);
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (target_height > 65535u) {
        set_error("bt_atlas_viewshed: target_height %u, at most 65535", target_height);
        return BT_ERR_INVALID_ARGUMENT;
    }
    for (uint32_t o = 0; o < observer_count; o++)
        if (observers[o].eye_height > 65535u) {
            set_error("bt_atlas_viewshed: eye_height %u of observer %u, at most 65535", observers[o].eye_height, o);
            return BT_ERR_INVALID_ARGUMENT;
        }
    if (width > BT_VIEWSHED_MAX_SIDE || height > BT_VIEWSHED_MAX_SIDE) {
        set_error("bt_atlas_viewshed: a side of %u x %u above %u", width, height, BT_VIEWSHED_MAX_SIDE);
        return BT_ERR_INVALID_ARGUMENT;
    }
    const uint64_t cells = uint64_t(width) * height;
    if (cells > BT_VIEWSHED_MAX_CELLS) {
        set_error("bt_atlas_viewshed: %u x %u cells, at most %u", width, height, BT_VIEWSHED_MAX_CELLS);
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (!cells) return BT_OK;  // an empty window: nothing to do
    for (uint32_t o = 0; o < observer_count; o++)
        if (observers[o].x >= width || observers[o].y >= height) {
            set_error("bt_atlas_viewshed: observer %u at (%u, %u) outside the %u x %u window", o, observers[o].x, observers[o].y, width, height);
            return BT_ERR_INVALID_ARGUMENT;
        }

    bt_ctx* ctx = a->ctx;
    BT_HIP(hipSetDevice(ctx->device));
    hipStream_t stream = ctx->stream;
    // the planes of the call, carved from one buffer
    const uint64_t at_raw = 0, at_transposed = at_raw + align256(cells * 2u), at_clearance = at_transposed + align256(cells * 2u), at_count = at_clearance + align256(cells * 4u),
                   at_mask = at_count + align256(cells), total = at_mask + (mask_out ? align256(cells * 8u) : 0u);
    if (bt_status s = ctx->viewshed.reserve(ctx, total)) return s;
    if (bt_status s = ctx->viewshed_words.reserve(ctx, 256, true)) return s;
    uint8_t* base = (uint8_t*)ctx->viewshed.dev;
    ViewshedPlanes p{};
    p.width = width, p.height = height;
    p.raw = (const uint16_t*)(base + at_raw);
    p.transposed = (uint16_t*)(base + at_transposed);
    p.clearance = (uint32_t*)(base + at_clearance);
    p.count = base + at_count;
    p.mask = mask_out ? (uint64_t*)(base + at_mask) : nullptr;
    p.target_height = target_height;
    p.observer_count = observer_count;
    memcpy(p.observers, observers, sizeof(bt_viewshed_observer) * observer_count);
    ViewshedCounts* counts = (ViewshedCounts*)ctx->viewshed_words.dev;
    const ViewshedCounts* counts_host = (const ViewshedCounts*)ctx->viewshed_words.host;

    uint32_t tiles_missing = 0;
    if (bt_status s = region_gather(a, ai, side, lod, x0, y0, width, height, base + at_raw, &tiles_missing)) return s;
    BT_HIP(hipMemsetAsync(counts, 0, sizeof(ViewshedCounts), stream));
    if (bt_status s = launch_viewshed_transpose(stream, p)) return s;
    if (bt_status s = launch_viewshed_walk(stream, p)) return s;
    if (bt_status s = launch_viewshed_finish(stream, p, counts)) return s;
    BT_HIP(hipMemcpyAsync((void*)counts_host, counts, sizeof(ViewshedCounts), hipMemcpyDeviceToHost, stream));
    const char* what = "bt_atlas_viewshed staging";
    if (clearance_out)
        if (bt_status s = region_stage_out(ctx, p.clearance, clearance_out, uint64_t(width) * 4u, uint64_t(width) * 4u, height, what)) return s;
    if (count_out)
        if (bt_status s = region_stage_out(ctx, p.count, count_out, width, width, height, what)) return s;
    if (mask_out)
        if (bt_status s = region_stage_out(ctx, p.mask, mask_out, uint64_t(width) * 8u, uint64_t(width) * 8u, height, what)) return s;
    BT_HIP(hipStreamSynchronize(stream));
    if (stats) {
        stats->cells = uint32_t(cells);
        stats->voids = counts_host->voids;
        stats->tiles_missing = tiles_missing;
        stats->observers_used = counts_host->observers_used;
        stats->observers_skipped = counts_host->observers_skipped;
        stats->covered = counts_host->covered;
        stats->visible = counts_host->visible;
        stats->max_clearance = counts_host->max_clearance;
        stats->samples = counts_host->samples;
        stats->launches = 5;  // the gather counted as one, the transpose, the two walks, the finish
    }
    return BT_OK;
}

}  // extern "C"

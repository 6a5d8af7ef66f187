// bt_atlas_drainage: the host half (the kernels: bt_drain.hip; the definition: the DRAINAGE section of include/bevy_terrain_amd.h).
//
// The call checks its arguments, gathers the rectangle's texels on the device by the plan of bt_atlas_read_region, prepares the planes, and
// then brings three relaxations to their fixed points one after the other: the filled level, the flat distance (which reads the final
// level), and, behind the direction plane, the accumulation (which reads the final directions).  Each starts with every block flagged and
// runs the sweeps of the block relaxation (relax_sweeps, bt_relax.hpp).  No result depends on the schedule (the header says why).
#include <cstring>

#include "bt_relax.hpp"

using namespace bt;

extern "C" {

bt_status bt_atlas_drainage(bt_atlas* a, uint32_t ai, uint32_t side, uint32_t lod, uint32_t x0, uint32_t y0, uint32_t width, uint32_t height, const uint8_t* void_host,
                            const uint8_t* weight_host, uint16_t* filled_out, uint32_t* flat_out, uint8_t* direction_out, uint32_t* accumulation_out, bt_drainage_stats* stats) {
    if (stats) *stats = bt_drainage_stats{};
    if (!a) {
        set_error("bt_atlas_drainage: NULL %s", "atlas");
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (bt_status s = region_check(a, ai, side, lod, x0, y0, width, height, "bt_atlas_drainage")) return s;
    const Attachment& at = a->attachments[ai];
    if (at.meta.format != BT_FORMAT_R16) {
        set_error("bt_atlas_drainage: attachment format %u (heights are R16)", at.meta.format);
        return BT_ERR_UNSUPPORTED;
    }
    const uint64_t cells = uint64_t(width) * height;
    if (cells > BT_DRAIN_MAX_CELLS) {
        set_error("bt_atlas_drainage: %u x %u cells, at most %u", width, height, BT_DRAIN_MAX_CELLS);
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (!cells) return BT_OK;  // an empty window: nothing to do

    bt_ctx* ctx = a->ctx;
    BT_HIP(hipSetDevice(ctx->device));
    hipStream_t stream = ctx->stream;
    // the planes of the call, carved from one buffer
    DrainPlanes p{RelaxGrid::of(width, height)};
    const uint64_t blocks = uint64_t(p.blocks_x) * p.blocks_y;
    const uint64_t at_raw = 0, at_mask = at_raw + align256(cells * 2u), at_weight = at_mask + (void_host ? align256(cells) : 0u),
                   at_z = at_weight + (weight_host ? align256(cells) : 0u), at_w = at_z + align256(cells * 2u), at_f = at_w + align256(cells * 2u),
                   at_dir = at_f + align256(cells * 4u), at_a = at_dir + align256(cells), at_flags = at_a + align256(cells * 4u),
                   total = at_flags + align256(2u * blocks * 4u);
    if (bt_status s = ctx->drain.reserve(ctx, total)) return s;
    constexpr uint64_t kWordsBytes = 256;  // kBatchMax sweep counters, then the DrainCounts
    if (bt_status s = ctx->drain_words.reserve(ctx, kWordsBytes, true)) return s;
    uint8_t* base = (uint8_t*)ctx->drain.dev;
    uint16_t* raw = (uint16_t*)(base + at_raw);
    uint8_t* mask = void_host ? base + at_mask : nullptr;
    uint8_t* weight = weight_host ? base + at_weight : nullptr;
    p.raw = raw, p.mask = mask, p.weight = weight, p.z = (uint16_t*)(base + at_z), p.W = (uint16_t*)(base + at_w), p.F = (uint32_t*)(base + at_f), p.dir = base + at_dir,
    p.A = (uint32_t*)(base + at_a);
    uint32_t* sweep_marked = (uint32_t*)ctx->drain_words.dev;
    DrainCounts* counts = (DrainCounts*)(sweep_marked + kBatchMax);
    const uint32_t* sweep_marked_host = (const uint32_t*)ctx->drain_words.host;
    const DrainCounts* counts_host = (const DrainCounts*)(sweep_marked_host + kBatchMax);

    uint32_t tiles_missing = 0, launches = 0;
    if (bt_status s = region_gather(a, ai, side, lod, x0, y0, width, height, raw, &tiles_missing)) return s;
    launches++;  // the gather, counted as one
    if (mask) BT_HIP(hipMemcpyAsync(mask, void_host, cells, hipMemcpyHostToDevice, stream));
    if (weight) BT_HIP(hipMemcpyAsync(weight, weight_host, cells, hipMemcpyHostToDevice, stream));
    BT_HIP(hipMemsetAsync(counts, 0, sizeof(DrainCounts), stream));
    if (bt_status s = launch_drain_prepare(stream, p, counts)) return s;
    launches++;

    uint32_t* flags[2] = {(uint32_t*)(base + at_flags), (uint32_t*)(base + at_flags) + blocks};
    const uint32_t rounds = relax_rounds("BT_DRAIN_ROUNDS");
    // one relaxation: every block flagged, then sweeps until one flags nothing; *sweeps: how many were launched
    auto relax = [&](DrainRule rule, const char* name, uint32_t* sweeps) -> bt_status {
        BT_HIP(hipMemsetD32Async(hipDeviceptr_t(flags[0]), 1, blocks, stream));
        BT_HIP(hipMemsetAsync(flags[1], 0, blocks * 4u, stream));
        bool converged = false;
        auto sweep = [&](uint32_t* active, uint32_t* activate, uint32_t* marked) { return launch_drain_relax(stream, rule, p, rounds, active, activate, marked); };
        if (bt_status s = relax_sweeps(stream, cells, flags, sweep_marked, sweep_marked_host, sweep, sweeps, &converged)) return s;
        if (!converged) {
            set_error("bt_atlas_drainage: no fixed point of the %s after %u sweeps of %llu cells", name, *sweeps, (unsigned long long)cells);
            return BT_ERR_INTERNAL;
        }
        return BT_OK;
    };
    uint32_t sweeps_fill = 0, sweeps_flat = 0, sweeps_accumulate = 0;
    if (bt_status s = relax(kDrainFill, "filled level", &sweeps_fill)) return s;
    if (bt_status s = launch_drain_flat_seed(stream, p)) return s;
    if (bt_status s = relax(kDrainFlat, "flat distance", &sweeps_flat)) return s;
    if (bt_status s = launch_drain_direction(stream, p)) return s;
    if (bt_status s = relax(kDrainAccumulate, "accumulation", &sweeps_accumulate)) return s;
    if (bt_status s = launch_drain_finish(stream, p, counts)) return s;
    launches += 3u + sweeps_fill + sweeps_flat + sweeps_accumulate;
    BT_HIP(hipMemcpyAsync((void*)counts_host, counts, sizeof(DrainCounts), hipMemcpyDeviceToHost, stream));
    const char* what = "bt_atlas_drainage staging";
    if (filled_out)
        if (bt_status s = region_stage_out(ctx, p.W, filled_out, uint64_t(width) * 2u, uint64_t(width) * 2u, height, what)) return s;
    if (flat_out)
        if (bt_status s = region_stage_out(ctx, p.F, flat_out, uint64_t(width) * 4u, uint64_t(width) * 4u, height, what)) return s;
    if (direction_out)
        if (bt_status s = region_stage_out(ctx, p.dir, direction_out, width, width, height, what)) return s;
    if (accumulation_out)
        if (bt_status s = region_stage_out(ctx, p.A, accumulation_out, uint64_t(width) * 4u, uint64_t(width) * 4u, height, what)) return s;
    BT_HIP(hipStreamSynchronize(stream));
    if (stats) {
        stats->cells = uint32_t(cells);
        stats->voids = counts_host->voids;
        stats->outlets = counts_host->outlets;
        stats->tiles_missing = tiles_missing;
        stats->filled = counts_host->filled;
        stats->flats = counts_host->flats;
        stats->max_flat_distance = counts_host->max_flat_distance;
        stats->max_accumulation = counts_host->max_accumulation;
        stats->outflow = counts_host->outflow;
        stats->sweeps_fill = sweeps_fill;
        stats->sweeps_flat = sweeps_flat;
        stats->sweeps_accumulate = sweeps_accumulate;
        stats->launches = launches;
    }
    return BT_OK;
}

}  // extern "C"

// bt_atlas_path_field / bt_path_trace: the host half of path-finding (the kernels: bt_path.hip; the definition: the PATH FIELD section of
// include/bevy_terrain_amd.h).
//
// The field call checks its arguments, gathers the rectangle's texels on the device by the plan of bt_atlas_read_region, prepares the
// planes, flags the 3 x 3 blocks around every goal, and then runs the sweeps of the block relaxation to its fixed point (relax_sweeps,
// bt_relax.hpp).  The result does not depend on the schedule (the header says why).
#include <cmath>
#include <cstring>

#include "bt_relax.hpp"

using namespace bt;

namespace {

bt_status refuse(const char* fmt, const char* what) {
    set_error(fmt, what);
    return BT_ERR_INVALID_ARGUMENT;
}

// the first defect of the cost record, or nullptr
const char* bad_cost(const bt_path_cost& c) {
    if (!std::isfinite(c.min_height) || !std::isfinite(c.max_height)) return "min_height / max_height (not finite)";
    if (!std::isfinite(c.max_height - c.min_height)) return "max_height - min_height (not finite)";
    if (!std::isfinite(c.cell_size) || !(c.cell_size > 0.0f)) return "cell_size (finite and > 0)";
    if (!(c.max_grade >= 0.0f)) return "max_grade (>= 0; +inf allowed)";
    for (float w : {c.grade_weight, c.climb_weight, c.descend_weight})
        if (!std::isfinite(w) || !(w >= 0.0f)) return "a weight (finite and >= 0)";
    return nullptr;
}

}  // namespace

extern "C" {

bt_status bt_atlas_path_field(bt_atlas* a, uint32_t ai, uint32_t side, uint32_t lod, uint32_t x0, uint32_t y0, uint32_t width, uint32_t height, const bt_path_cost* cost,
                              const bt_path_goal* goals, uint32_t goal_count, const uint8_t* blocked_host, float* cost_out, uint8_t* next_out, bt_path_stats* stats) {
    if (stats) *stats = bt_path_stats{};
    if (!a) return refuse("bt_atlas_path_field: NULL %s", "atlas");
    if (bt_status s = region_check(a, ai, side, lod, x0, y0, width, height, "bt_atlas_path_field")) return s;
    const Attachment& at = a->attachments[ai];
    if (at.meta.format != BT_FORMAT_R16) {
        set_error("bt_atlas_path_field: attachment format %u (heights are R16)", at.meta.format);
        return BT_ERR_UNSUPPORTED;
    }
    if (!cost || !goals) return refuse("bt_atlas_path_field: NULL %s", !cost ? "cost" : "goals");
    if (const char* bad = bad_cost(*cost)) return refuse("bt_atlas_path_field: %s", bad);
    if (goal_count == 0u || goal_count > BT_PATH_MAX_GOALS) {
        set_error("bt_atlas_path_field: %u goals, 1 .. %u per call", goal_count, BT_PATH_MAX_GOALS);
        return BT_ERR_INVALID_ARGUMENT;
    }
    const uint64_t cells = uint64_t(width) * height;
    if (cells > BT_PATH_MAX_CELLS) {
        set_error("bt_atlas_path_field: %u x %u cells, at most %u", width, height, BT_PATH_MAX_CELLS);
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (!cells) return BT_OK;  // an empty window: nothing to do, the goals are not looked at
    std::vector<bt_path_goal> goal_list(goals, goals + goal_count);
    for (uint32_t i = 0; i < goal_count; i++) {
        bt_path_goal& g = goal_list[i];
        if (g.x >= width || g.y >= height || !std::isfinite(g.cost0) || !(g.cost0 >= 0.0f)) {
            set_error("bt_atlas_path_field: goal %u: %s", i, g.x >= width || g.y >= height ? "outside the window" : "cost0 (finite and >= 0)");
            return BT_ERR_INVALID_ARGUMENT;
        }
        g.cost0 = g.cost0 + 0.0f;  // -0 becomes +0, nothing else moves: the device orders costs by their bits
    }

    bt_ctx* ctx = a->ctx;
    BT_HIP(hipSetDevice(ctx->device));
    hipStream_t stream = ctx->stream;
    // the planes of the call, carved from one buffer
    PathPlanes p{RelaxGrid::of(width, height)};
    const uint64_t blocks = uint64_t(p.blocks_x) * p.blocks_y;
    uint64_t at_raw = 0, at_mask = at_raw + align256(cells * 2u), at_h = at_mask + (blocked_host ? align256(cells) : 0u), at_d = at_h + align256(cells * 4u),
             at_next = at_d + align256(cells * 4u), at_flags = at_next + align256(cells), total = at_flags + align256(2u * blocks * 4u);
    if (bt_status s = ctx->path.reserve(ctx, total)) return s;
    constexpr uint64_t kWordsBytes = 256;  // kBatchMax sweep counters, then the PathCounts
    if (bt_status s = ctx->path_words.reserve(ctx, kWordsBytes, true)) return s;
    uint8_t* base = (uint8_t*)ctx->path.dev;
    uint16_t* raw = (uint16_t*)(base + at_raw);
    uint8_t* mask = blocked_host ? base + at_mask : nullptr;
    p.raw = raw, p.mask = mask, p.h = (float*)(base + at_h), p.D = (uint32_t*)(base + at_d), p.next = base + at_next;
    uint32_t* flags[2] = {(uint32_t*)(base + at_flags), (uint32_t*)(base + at_flags) + blocks};
    uint32_t* sweep_marked = (uint32_t*)ctx->path_words.dev;
    PathCounts* counts = (PathCounts*)(sweep_marked + kBatchMax);
    const uint32_t* sweep_marked_host = (const uint32_t*)ctx->path_words.host;
    const PathCounts* counts_host = (const PathCounts*)(sweep_marked_host + kBatchMax);

    uint32_t tiles_missing = 0, launches = 0;
    if (bt_status s = region_gather(a, ai, side, lod, x0, y0, width, height, raw, &tiles_missing)) return s;
    launches++;  // the gather, counted as one
    if (mask) BT_HIP(hipMemcpyAsync(mask, blocked_host, cells, hipMemcpyHostToDevice, stream));
    PlanRing ring;
    const uint64_t goals_at = ring.add(goal_list);
    uint8_t* ring_dev = nullptr;
    if (bt_status s = ring.commit(ctx, &ring_dev)) return s;
    const bt_path_goal* goals_dev = (const bt_path_goal*)(ring_dev + goals_at);
    BT_HIP(hipMemsetD32Async(hipDeviceptr_t(p.D), 0x7F800000, cells, stream));  // +inf
    BT_HIP(hipMemsetAsync(p.next, 0, cells, stream));
    BT_HIP(hipMemsetAsync(flags[0], 0, 2u * blocks * 4u, stream));
    BT_HIP(hipMemsetAsync(counts, 0, sizeof(PathCounts), stream));
    if (bt_status s = launch_path_prepare(stream, p, *cost, goals_dev, goal_count, flags[0], counts)) return s;
    launches++;

    const float cell_diag = cost->cell_size * 1.41421356f;
    const uint32_t rounds = relax_rounds("BT_PATH_ROUNDS");
    uint32_t sweeps = 0;
    bool converged = false;
    auto sweep = [&](uint32_t* active, uint32_t* activate, uint32_t* marked) { return launch_path_relax(stream, p, *cost, cell_diag, rounds, active, activate, marked); };
    if (bt_status s = relax_sweeps(stream, cells, flags, sweep_marked, sweep_marked_host, sweep, &sweeps, &converged)) return s;
    launches += sweeps;
    if (!converged) {
        set_error("bt_atlas_path_field: no fixed point after %u sweeps of %llu cells", sweeps, (unsigned long long)cells);
        return BT_ERR_INTERNAL;
    }
    if (bt_status s = launch_path_next(stream, p, *cost, cell_diag, goals_dev, goal_count, counts)) return s;
    launches++;
    BT_HIP(hipMemcpyAsync((void*)counts_host, counts, sizeof(PathCounts), hipMemcpyDeviceToHost, stream));
    if (cost_out)
        if (bt_status s = region_stage_out(ctx, p.D, cost_out, uint64_t(width) * 4u, uint64_t(width) * 4u, height, "bt_atlas_path_field staging")) return s;
    if (next_out)
        if (bt_status s = region_stage_out(ctx, p.next, next_out, width, width, height, "bt_atlas_path_field staging")) return s;
    BT_HIP(hipStreamSynchronize(stream));
    if (stats) {
        stats->cells = uint32_t(cells);
        stats->blocked = counts_host->blocked;
        stats->reachable = counts_host->reachable;
        stats->goals_blocked = counts_host->goals_blocked;
        stats->goals_used = goal_count - counts_host->goals_blocked;
        stats->tiles_missing = tiles_missing;
        stats->sweeps = sweeps;
        stats->launches = launches;
    }
    return BT_OK;
}

bt_status bt_path_trace(const uint8_t* next, uint32_t width, uint32_t height, uint32_t start_x, uint32_t start_y, uint32_t* out_xy, uint32_t cap, uint32_t* count_out,
                        uint32_t* status_out) {
    if (count_out) *count_out = 0;
    if (!next || !status_out || (cap && !out_xy) || !width || !height || start_x >= width || start_y >= height) {
        set_error("bt_path_trace: %s", !next ? "NULL next" : !status_out ? "NULL status_out" : cap && !out_xy ? "NULL out_xy with cap > 0" : "an empty window or a start outside it");
        return BT_ERR_INVALID_ARGUMENT;
    }
    const uint64_t cells = uint64_t(width) * height;
    uint32_t x = start_x, y = start_y, status = BT_PATH_TRACE_LOOP;
    uint64_t count = 0;
    for (uint64_t step = 0; step <= cells; step++) {
        if (count < cap) out_xy[2u * count] = x, out_xy[2u * count + 1u] = y;
        count++;
        const uint8_t n = next[uint64_t(y) * width + x];
        if (n == BT_PATH_GOAL) {
            status = BT_PATH_TRACE_OK;
            break;
        }
        if (step == 0 && (n == BT_PATH_BLOCKED || n == BT_PATH_UNREACHABLE)) {
            status = n == BT_PATH_BLOCKED ? BT_PATH_TRACE_BLOCKED : BT_PATH_TRACE_UNREACHABLE;
            break;
        }
        if (n > 7u || step == cells) break;  // a byte that is no direction; or width * height steps without a goal
        const int64_t nx = int64_t(x) + neighbour_dx(n), ny = int64_t(y) + neighbour_dy(n);
        if (nx < 0 || ny < 0 || nx >= int64_t(width) || ny >= int64_t(height)) break;  // points outside the window
        x = uint32_t(nx), y = uint32_t(ny);
    }
    if (count_out) *count_out = uint32_t(std::min<uint64_t>(count, 0xFFFFFFFFull));
    *status_out = status;
    return BT_OK;
}

}  // extern "C"

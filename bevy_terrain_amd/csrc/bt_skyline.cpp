// bt_atlas_skyline: the device-free part of the host half (the kernels: bt_skyline.hip; the call itself: bt_edit.cpp, beside the other
// bakes; the definition: the SKYLINE section of include/bevy_terrain_amd.h).  The geometry of the digital lines, the check of the
// directions, and the plan: how many directions run in one batch and how many launches the call takes, from its arguments alone.
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "bt_internal.hpp"

namespace bt {

namespace {

// floor(a / b) for b > 0, towards minus infinity
int64_t floor_div(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// The lines of one direction over a window whose major axis has `major` cells and whose minor axis `minor`: n, m of the header.  The
// lines present at major coordinate u are the `minor` consecutive j from -off(u): a difference array over the lines gives every length.
void line_geometry(uint32_t major, uint32_t minor, int64_t n, int64_t m, uint32_t* lines, uint32_t* longest) {
    const int64_t last = floor_div(2 * int64_t(major - 1u) * m + n, 2 * n);  // off(major - 1); off(0) = 0 and off is monotone
    const int64_t j_min = -std::max<int64_t>(last, 0);
    const uint32_t count = minor + uint32_t(std::llabs(last));
    std::vector<int32_t> edge(count + 1u, 0);
    for (uint32_t u = 0; u < major; u++) {
        const int64_t first = -floor_div(2 * int64_t(u) * m + n, 2 * n) - j_min;  // of the lines at u, as an index
        edge[size_t(first)]++, edge[size_t(first) + minor]--;
    }
    int32_t length = 0, best = 0;
    for (uint32_t j = 0; j < count; j++) length += edge[j], best = std::max(best, length);
    *lines = count, *longest = uint32_t(best);
}

bool bad_vector(int32_t dx, int32_t dy) {
    return (dx == 0 && dy == 0) || std::abs(int64_t(dx)) > BT_SKYLINE_MAX_COMPONENT || std::abs(int64_t(dy)) > BT_SKYLINE_MAX_COMPONENT;
}

void count_lines(uint32_t width, uint32_t height, int32_t dx, int32_t dy, uint32_t* lines, uint32_t* longest) {
    const bool x_major = std::abs(dx) >= std::abs(dy);
    const int32_t major_d = x_major ? dx : dy, minor_d = x_major ? dy : dx;
    line_geometry(x_major ? width : height, x_major ? height : width, std::abs(major_d), major_d < 0 ? -minor_d : minor_d, lines, longest);
}

}  // namespace

const char* skyline_bad_direction(const bt_skyline_direction* directions, uint32_t direction_count, uint32_t* which) {
    for (uint32_t k = 0; k < direction_count; k++) {
        const bt_skyline_direction& d = directions[k];
        *which = k;
        if (d.dx == 0 && d.dy == 0) return "a zero vector";
        if (bad_vector(d.dx, d.dy)) return "a component above BT_SKYLINE_MAX_COMPONENT";
        if (d.sun_den == 0u || d.sun_den > 65535u) return "sun_den (1..65535)";
        if (d.sun_num > 0x7FFFFFFFu) return "sun_num (at most 2^31 - 1)";
    }
    return nullptr;
}

SkylinePlan skyline_plan(uint32_t width, uint32_t height, const bt_skyline_direction* directions, uint32_t direction_count, bool bake) {
    SkylinePlan plan{};
    const uint64_t cells = uint64_t(width) * height;
    if (!cells || !direction_count) return plan;
    plan.batch = uint32_t(std::min<uint64_t>(direction_count, std::max<uint64_t>(1u, BT_SKYLINE_STACK_BUDGET / (4u * cells))));
    plan.batches = (direction_count + plan.batch - 1u) / plan.batch;
    plan.launches = 2u + 2u * plan.batches + (bake ? 1u : 0u);  // the gather, the transpose; a walk and a finish per batch; a bake's gather
    for (uint32_t k = 0; k < direction_count; k++) {
        uint32_t lines = 0, longest = 0;
        count_lines(width, height, directions[k].dx, directions[k].dy, &lines, &longest);
        plan.lines += lines;
        plan.longest_line = std::max(plan.longest_line, longest);
    }
    return plan;
}

}  // namespace bt

using namespace bt;

extern "C" {

bt_status bt_skyline_line_count(uint32_t width, uint32_t height, int32_t dx, int32_t dy, uint32_t* lines, uint32_t* longest) {
    if (lines) *lines = 0;
    if (longest) *longest = 0;
    if (bad_vector(dx, dy)) {
        set_error("bt_skyline_line_count: (%d, %d): not both 0, components within +-%d", dx, dy, BT_SKYLINE_MAX_COMPONENT);
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (width > BT_SKYLINE_MAX_SIDE || height > BT_SKYLINE_MAX_SIDE) {
        set_error("bt_skyline_line_count: a side of %u x %u above %u", width, height, BT_SKYLINE_MAX_SIDE);
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (!width || !height) return BT_OK;
    uint32_t n = 0, l = 0;
    count_lines(width, height, dx, dy, &n, &l);
    if (lines) *lines = n;
    if (longest) *longest = l;
    return BT_OK;
}

}  // extern "C"

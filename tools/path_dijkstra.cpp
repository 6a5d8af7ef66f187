// The host side of tools/path_bench.py: the PATH FIELD definition of include/bevy_terrain_amd.h as a plain Dijkstra search with
// std::priority_queue, for timing beside bt_atlas_path_field on the same gathered heights.  Compiled by the bench tool (-O3
// -ffp-contract=off: one rounding per written operation); not part of the library.
#include <cmath>
#include <cstdint>
#include <limits>
#include <queue>
#include <utility>
#include <vector>

namespace {

struct Cost {  // bt_path_cost
    float min_height, max_height, cell_size, max_grade, grade_weight, climb_weight, descend_weight;
    uint32_t padding;
};
struct Goal {  // bt_path_goal
    uint32_t x, y;
    float cost0;
};

const int kDx[8] = {1, 1, 0, -1, -1, -1, 0, 1}, kDy[8] = {0, 1, 1, 1, 0, -1, -1, -1};
const float kInf = std::numeric_limits<float>::infinity();

}  // namespace

// raw: width x height texels (0 = no data); mask: the same size or NULL; D_out: width x height floats.  Returns the reachable cells.
extern "C" uint32_t path_dijkstra(const uint16_t* raw, const uint8_t* mask, uint32_t width, uint32_t height, const Cost* c, const Goal* goals, uint32_t goal_count, float* D) {
    const size_t cells = size_t(width) * height;
    std::vector<float> h(cells);
    std::vector<uint8_t> blocked(cells);
    for (size_t i = 0; i < cells; i++) {
        blocked[i] = raw[i] == 0 || (mask && mask[i]);
        h[i] = c->min_height + (c->max_height - c->min_height) * (float(raw[i]) / 65535.0f);
        D[i] = kInf;
    }
    const float cell_diag = c->cell_size * 1.41421356f;
    typedef std::pair<float, uint32_t> Entry;
    std::priority_queue<Entry, std::vector<Entry>, std::greater<Entry>> heap;
    for (uint32_t g = 0; g < goal_count; g++) {
        const size_t i = size_t(goals[g].y) * width + goals[g].x;
        if (blocked[i] || !(goals[g].cost0 < D[i])) continue;
        D[i] = goals[g].cost0;
        heap.push({D[i], uint32_t(i)});
    }
    auto is_free = [&](int x, int y) { return x >= 0 && y >= 0 && x < int(width) && y < int(height) && !blocked[size_t(y) * width + x]; };
    uint32_t reachable = 0;
    while (!heap.empty()) {
        const Entry top = heap.top();
        heap.pop();
        const uint32_t b = top.second;
        if (top.first > D[b]) continue;
        reachable++;
        const int bx = int(b % width), by = int(b / width);
        // every cell a whose neighbour k is b: the edge a -> b
        for (int k = 0; k < 8; k++) {
            const int ax = bx - kDx[k], ay = by - kDy[k];
            if (!is_free(ax, ay)) continue;
            if ((k & 1) && (!is_free(ax + kDx[k], ay) || !is_free(ax, ay + kDy[k]))) continue;
            const size_t a = size_t(ay) * width + ax;
            const float run = (k & 1) ? cell_diag : c->cell_size;
            const float rise = h[b] - h[a];
            const float g = std::fabs(rise) / run;
            if (!(g <= c->max_grade)) continue;
            const float up = rise > 0.0f ? rise : 0.0f;
            const float down = rise < 0.0f ? -rise : 0.0f;
            const float w = ((run * (1.0f + c->grade_weight * g)) + c->climb_weight * up) + c->descend_weight * down;
            const float cand = D[b] + w;
            if (cand < D[a]) {
                D[a] = cand;
                heap.push({cand, uint32_t(a)});
            }
        }
    }
    return reachable;
}

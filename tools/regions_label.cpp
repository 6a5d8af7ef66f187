// A sequential two-pass host labeller with the rule of the REGIONS section of include/bevy_terrain_amd.h, for tools/regions_bench.py (which
// compiles it with -O3): the baseline bt_atlas_label_regions is timed against, and a third statement of the definition.
//
// Pass one walks the cells in row-major order and unites every member with its linked neighbours already seen (left, upper, and with
// `eight` upper-left and upper-right) in a union-find over cell indices whose roots are the smallest index of their set (union by index).
// Pass two takes every cell's root as its label, ranks the labels in the order they appear (row-major, so ascending) and folds the cells
// into their records.
#include <cstdint>
#include <cstdlib>
#include <vector>

namespace {

struct Region {  // bt_region
    uint32_t label, area;
    uint16_t x_min, y_min, x_max, y_max, v_min, v_max;
    uint32_t edges;
    uint64_t v_sum;
};
static_assert(sizeof(Region) == 32, "bt_region");

constexpr uint32_t kNone = 0xFFFFFFFFu;

uint32_t find(uint32_t* parent, uint32_t c) {
    uint32_t root = c;
    while (parent[root] != root) root = parent[root];
    while (parent[c] != root) {  // path compression
        const uint32_t next = parent[c];
        parent[c] = root;
        c = next;
    }
    return root;
}

}  // namespace

// member: width * height bytes (non-zero = member); v: width * height values; label, id: width * height words out; table: room for
// `cap` records.  Returns the number of regions; the first min(regions, cap) records are written
extern "C" uint32_t regions_label(const uint8_t* member, const uint16_t* v, uint32_t width, uint32_t height, uint32_t max_step, uint32_t eight, uint32_t* label,
                                  uint32_t* id, Region* table, uint32_t cap) {
    const uint32_t cells = width * height;
    uint32_t* parent = label;  // the label plane holds the parents until pass two
    auto linked = [&](uint32_t a, uint32_t b) { return member[b] && uint32_t(std::abs(int(v[a]) - int(v[b]))) <= max_step; };
    auto unite = [&](uint32_t a, uint32_t b) {
        a = find(parent, a), b = find(parent, b);
        if (a < b) parent[b] = a;
        else parent[a] = b;
    };
    for (uint32_t y = 0, i = 0; y < height; y++)
        for (uint32_t x = 0; x < width; x++, i++) {
            if (!member[i]) {
                parent[i] = kNone;
                continue;
            }
            parent[i] = i;
            if (x > 0 && linked(i, i - 1)) unite(i, i - 1);
            if (y > 0 && linked(i, i - width)) unite(i, i - width);
            if (eight && y > 0) {
                if (x > 0 && linked(i, i - width - 1)) unite(i, i - width - 1);
                if (x + 1 < width && linked(i, i - width + 1)) unite(i, i - width + 1);
            }
        }
    uint32_t regions = 0;
    for (uint32_t i = 0; i < cells; i++) {  // a root comes before every other cell of its set: its id is there when they ask
        if (parent[i] == kNone) {
            id[i] = kNone;
            continue;
        }
        const uint32_t root = find(parent, i);
        if (root == i) id[i] = regions++;
        else id[i] = id[root];
    }
    for (uint32_t i = 0; i < cells; i++)
        if (parent[i] != kNone) label[i] = find(parent, i);
    for (uint32_t y = 0, i = 0; y < height; y++)
        for (uint32_t x = 0; x < width; x++, i++) {
            if (label[i] == kNone || id[i] >= cap) continue;
            Region& r = table[id[i]];
            if (label[i] == i) r = Region{i, 0, uint16_t(x), uint16_t(y), uint16_t(x), uint16_t(y), v[i], v[i], 0, 0};
            r.area++, r.v_sum += v[i];
            if (x < r.x_min) r.x_min = uint16_t(x);
            if (x > r.x_max) r.x_max = uint16_t(x);
            if (y > r.y_max) r.y_max = uint16_t(y);
            if (v[i] < r.v_min) r.v_min = v[i];
            if (v[i] > r.v_max) r.v_max = v[i];
            r.edges += uint32_t(x == 0 || label[i - 1] != label[i]) + uint32_t(x + 1 == width || label[i + 1] != label[i]) + uint32_t(y == 0 || label[i - width] != label[i]) +
                       uint32_t(y + 1 == height || label[i + width] != label[i]);
        }
    return regions;
}

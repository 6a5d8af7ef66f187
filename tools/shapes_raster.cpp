// A sequential host rasteriser with the rules of the SHAPES section of include/bevy_terrain_amd.h, for tools/shapes_bench.py: the planes
// and texels the device's raster must equal, and the time one host thread takes for them.  Compiled by the tool (g++ -O3), never by the
// library.  It takes a VALID list (bt_shapes_check) and works shape by shape inside the shape's box: a polygon row by row, collecting the
// edges whose y-range holds the row and evaluating the cross product of those alone; a stroke segment by segment inside the segment's own
// box grown by r, marking cells in a stamp plane so that a cell counts once per shape.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../include/bevy_terrain_amd.h"

namespace {

typedef __int128 wide_t;

inline int64_t floor256(int64_t v) { return v >> 8; }
inline int64_t ceil256(int64_t v) { return (v + 255) >> 8; }

struct Cells {  // a range of cells per axis, both ends included; empty: x_lo > x_hi
    int64_t x_lo, y_lo, x_hi, y_hi;
};

Cells clip(int64_t x_min, int64_t x_max, int64_t y_min, int64_t y_max, int64_t r, uint32_t width, uint32_t height) {
    Cells c{std::max<int64_t>(0, ceil256(x_min - r)), std::max<int64_t>(0, ceil256(y_min - r)), std::min<int64_t>(int64_t(width) - 1, floor256(x_max + r)),
            std::min<int64_t>(int64_t(height) - 1, floor256(y_max + r))};
    if (c.y_lo > c.y_hi) c.x_lo = 1, c.x_hi = 0;
    return c;
}

inline bool segment_covers(int64_t px, int64_t py, const bt_shape_vertex& a, const bt_shape_vertex& b, int64_t r2) {
    const int64_t dx = int64_t(b.x) - a.x, dy = int64_t(b.y) - a.y, ex = px - a.x, ey = py - a.y;
    const int64_t L = dx * dx + dy * dy, t = ex * dx + ey * dy;
    if (L == 0 || t <= 0) return ex * ex + ey * ey <= r2;
    if (t >= L) return (px - b.x) * (px - b.x) + (py - b.y) * (py - b.y) <= r2;
    const int64_t c = dx * ey - dy * ex;
    return wide_t(c) * c <= wide_t(r2) * L;
}

inline uint32_t fold(uint32_t v, uint32_t op, uint32_t value, bool wide) {
    if (!wide && v == 0u) return 0u;
    int64_t r = v;
    switch (op) {
        case BT_SHAPE_SET: r = value; break;
        case BT_SHAPE_MAX: r = std::max<int64_t>(r, value); break;
        case BT_SHAPE_MIN: r = std::min<int64_t>(r, value); break;
        case BT_SHAPE_ADD: r += value; break;
        default: r -= value; break;
    }
    return uint32_t(wide ? std::min<int64_t>(std::max<int64_t>(r, 0), 255) : std::min<int64_t>(std::max<int64_t>(r, 1), 65535));
}

}  // namespace

// texels: width * height of pixel_size 2 (R16) or 4 (Rgba8, byte `channel`), folded in place; count (u8) and last (u16): width * height,
// written everywhere.  Returns the number of cells with count > 0
extern "C" uint64_t shapes_raster(const bt_shape_vertex* vertices, const bt_shape* shapes, uint32_t entry_count, uint32_t width, uint32_t height, void* texels,
                                  uint32_t pixel_size, uint32_t channel, uint8_t* count, uint16_t* last) {
    const uint64_t cells = uint64_t(width) * height;
    std::fill(count, count + cells, uint8_t(0));
    std::fill(last, last + cells, uint16_t(BT_SHAPES_NONE));
    std::vector<uint32_t> stamp(cells, 0u);  // k + 1 of the last shape that covered the cell
    std::vector<int32_t> winding(width);
    std::vector<uint32_t> spanning;
    const bool wide = pixel_size == 4u;
    uint32_t k = 0;
    for (uint32_t first = 0; first < entry_count; k++) {
        uint32_t end = first;
        while (shapes[end++].flags & BT_SHAPE_MORE) {
        }
        const bt_shape& s = shapes[first];
        int64_t x_min = INT64_MAX, x_max = INT64_MIN, y_min = INT64_MAX, y_max = INT64_MIN;
        for (uint32_t e = first; e < end; e++)
            for (uint32_t i = 0; i < shapes[e].vertex_count; i++) {
                const bt_shape_vertex& v = vertices[shapes[e].first_vertex + i];
                x_min = std::min<int64_t>(x_min, v.x), x_max = std::max<int64_t>(x_max, v.x), y_min = std::min<int64_t>(y_min, v.y), y_max = std::max<int64_t>(y_max, v.y);
            }
        const Cells box = clip(x_min, x_max, y_min, y_max, s.half_width, width, height);
        if (box.x_lo <= box.x_hi) {
            if (s.kind == BT_SHAPE_POLYGON) {
                for (int64_t cy = box.y_lo; cy <= box.y_hi; cy++) {
                    const int64_t py = 256 * cy;
                    std::fill(winding.begin() + box.x_lo, winding.begin() + box.x_hi + 1, 0);
                    for (uint32_t e = first; e < end; e++) {
                        const bt_shape_vertex* v = vertices + shapes[e].first_vertex;
                        const uint32_t n = shapes[e].vertex_count;
                        for (uint32_t i = 0; i < n; i++) {
                            const bt_shape_vertex &a = v[i], &b = v[i + 1u == n ? 0u : i + 1u];
                            const bool up = a.y <= py && py < b.y, down = b.y <= py && py < a.y;
                            if (!up && !down) continue;
                            const int64_t dx = int64_t(b.x) - a.x, dy = int64_t(b.y) - a.y;
                            for (int64_t cx = box.x_lo; cx <= box.x_hi; cx++) {
                                const int64_t c = dx * (py - a.y) - dy * (256 * cx - a.x);
                                if (up && c > 0) winding[cx]++;
                                if (down && c < 0) winding[cx]--;
                            }
                        }
                    }
                    for (int64_t cx = box.x_lo; cx <= box.x_hi; cx++)
                        if (s.flags & BT_SHAPE_NONZERO ? winding[cx] != 0 : (winding[cx] & 1) != 0) stamp[cy * width + cx] = k + 1u;
                }
            } else {
                const bt_shape_vertex* v = vertices + s.first_vertex;
                const uint32_t n = s.vertex_count, segments = (s.flags & BT_SHAPE_CLOSED) ? n : std::max(n - 1u, 1u);
                const int64_t r = s.half_width, r2 = r * r;
                for (uint32_t i = 0; i < segments; i++) {
                    const bt_shape_vertex &a = v[i], &b = v[(i + 1u) % n];
                    const Cells c = clip(std::min(a.x, b.x), std::max(a.x, b.x), std::min(a.y, b.y), std::max(a.y, b.y), r, width, height);
                    for (int64_t cy = c.y_lo; cy <= c.y_hi; cy++)
                        for (int64_t cx = c.x_lo; cx <= c.x_hi; cx++)
                            if (stamp[cy * width + cx] != k + 1u && segment_covers(256 * cx, 256 * cy, a, b, r2)) stamp[cy * width + cx] = k + 1u;
                }
            }
            for (int64_t cy = box.y_lo; cy <= box.y_hi; cy++)
                for (int64_t cx = box.x_lo; cx <= box.x_hi; cx++) {
                    const uint64_t i = uint64_t(cy) * width + cx;
                    if (stamp[i] != k + 1u) continue;
                    count[i] = uint8_t(std::min<uint32_t>(count[i] + 1u, 255u));
                    last[i] = uint16_t(k);
                    if (wide) {
                        uint8_t* byte = (uint8_t*)texels + i * 4u + channel;
                        *byte = uint8_t(fold(*byte, s.op, s.value, true));
                    } else {
                        uint16_t* t = (uint16_t*)texels + i;
                        *t = uint16_t(fold(*t, s.op, s.value, false));
                    }
                }
        }
        first = end;
    }
    uint64_t covered = 0;
    for (uint64_t i = 0; i < cells; i++) covered += count[i] != 0u;
    return covered;
}

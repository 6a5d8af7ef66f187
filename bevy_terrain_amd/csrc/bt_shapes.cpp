// The device-free half of the SHAPES section of include/bevy_terrain_amd.h: the rules of a shape list, the boxes, and the records the
// raster kernel (bt_shapes.hip) walks.  bt_shapes_check is the exported form; bt_atlas_rasterize_shapes (bt_edit.cpp, for the write-back)
// plans with the same function.
#include <cstdio>

#include "bt_internal.hpp"

namespace bt {

namespace {

// floor(v / 256) and ceil(v / 256), the division mathematical (an arithmetic shift floors)
inline int64_t floor256(int64_t v) { return v >> 8; }
inline int64_t ceil256(int64_t v) { return (v + 255) >> 8; }

struct Extent {  // of the vertices of a shape, per axis
    int64_t x_min, x_max, y_min, y_max;
};

bt_shape_box box_of(const Extent& e, int64_t r, uint32_t width, uint32_t height) {
    const bt_shape_box empty{1, 1, 0, 0};
    if (!width || !height) return empty;
    const int64_t x_lo = std::max<int64_t>(0, ceil256(e.x_min - r)), x_hi = std::min<int64_t>(int64_t(width) - 1, floor256(e.x_max + r));
    const int64_t y_lo = std::max<int64_t>(0, ceil256(e.y_min - r)), y_hi = std::min<int64_t>(int64_t(height) - 1, floor256(e.y_max + r));
    if (x_lo > x_hi || y_lo > y_hi) return empty;
    return bt_shape_box{uint16_t(x_lo), uint16_t(y_lo), uint16_t(x_hi), uint16_t(y_hi)};
}

// the first defect of one entry on its own, or nullptr
const char* bad_entry(const bt_shape& s, const bt_shape_vertex* vertices, uint32_t vertex_count) {
    if (s.kind != BT_SHAPE_POLYGON && s.kind != BT_SHAPE_STROKE) return "kind";
    const uint32_t allowed = s.kind == BT_SHAPE_POLYGON ? uint32_t(BT_SHAPE_NONZERO | BT_SHAPE_MORE) : uint32_t(BT_SHAPE_CLOSED);
    if (s.flags & ~allowed) return "flags (NONZERO and MORE on a polygon, CLOSED on a stroke)";
    if (s.op > BT_SHAPE_SUB) return "op";
    if (s.value > 65535u) return "value above 65535";
    if (s._pad != 0u) return "_pad (0)";
    if (s.kind == BT_SHAPE_POLYGON && s.half_width != 0u) return "half_width on a polygon (0)";
    if (s.half_width > BT_SHAPES_MAX_HALF_WIDTH) return "half_width above BT_SHAPES_MAX_HALF_WIDTH";
    if (s.vertex_count < (s.kind == BT_SHAPE_POLYGON ? 3u : 1u)) return "vertex_count (a contour has 3 or more vertices, a stroke 1 or more)";
    if (uint64_t(s.first_vertex) + s.vertex_count > vertex_count) return "vertex range outside the array";
    for (uint32_t i = 0; i < s.vertex_count; i++) {
        const bt_shape_vertex& v = vertices[s.first_vertex + i];
        if (v.x < -BT_SHAPES_MAX_COORD || v.x > BT_SHAPES_MAX_COORD || v.y < -BT_SHAPES_MAX_COORD || v.y > BT_SHAPES_MAX_COORD) return "a vertex beyond BT_SHAPES_MAX_COORD";
    }
    return nullptr;
}

}  // namespace

const char* shapes_check(const bt_shape_vertex* vertices, uint32_t vertex_count, const bt_shape* shapes, uint32_t entry_count, uint32_t width, uint32_t height,
                         bt_shape_box* boxes, std::vector<ShapeRecord>* records, uint32_t* shape_count, uint32_t* bad) {
    *bad = BT_SHAPES_NO_ENTRY, *shape_count = 0;
    if ((!vertices && vertex_count) || (!shapes && entry_count)) return "NULL vertices or shapes with a non-zero count";
    if (width > BT_SHAPES_MAX_SIDE || height > BT_SHAPES_MAX_SIDE) return "a side of the window above BT_SHAPES_MAX_SIDE";
    if (uint64_t(width) * height > BT_SHAPES_MAX_CELLS) return "more cells than BT_SHAPES_MAX_CELLS";
    if (entry_count > BT_SHAPES_MAX_ENTRIES) return "more entries than BT_SHAPES_MAX_ENTRIES";
    if (vertex_count > BT_SHAPES_MAX_VERTICES) return "more vertices than BT_SHAPES_MAX_VERTICES";
    // the rules first, so a refusal writes no box
    uint32_t count = 0;
    for (uint32_t i = 0; i < entry_count; i++) {
        *bad = i;
        if (const char* defect = bad_entry(shapes[i], vertices, vertex_count)) return defect;
        const bool continues = i > 0u && (shapes[i - 1u].flags & BT_SHAPE_MORE) != 0u;
        if (continues) {
            const bt_shape &p = shapes[i - 1u], &s = shapes[i];
            if (s.kind != p.kind || s.op != p.op || s.value != p.value || ((s.flags ^ p.flags) & BT_SHAPE_NONZERO)) return "a contour that differs from its run in kind, op, value or NONZERO";
        } else if (++count > BT_SHAPES_MAX_SHAPES) {
            return "more shapes than BT_SHAPES_MAX_SHAPES";
        }
        if (i + 1u == entry_count && (shapes[i].flags & BT_SHAPE_MORE)) return "MORE on the last entry";
    }
    *bad = BT_SHAPES_NO_ENTRY, *shape_count = count;
    if (!boxes && !records) return nullptr;
    uint32_t k = 0;
    for (uint32_t first = 0; first < entry_count; k++) {
        uint32_t end = first;
        Extent e{INT64_MAX, INT64_MIN, INT64_MAX, INT64_MIN};
        do {
            const bt_shape& s = shapes[end];
            for (uint32_t i = 0; i < s.vertex_count; i++) {
                const bt_shape_vertex& v = vertices[s.first_vertex + i];
                e.x_min = std::min<int64_t>(e.x_min, v.x), e.x_max = std::max<int64_t>(e.x_max, v.x);
                e.y_min = std::min<int64_t>(e.y_min, v.y), e.y_max = std::max<int64_t>(e.y_max, v.y);
            }
        } while (shapes[end++].flags & BT_SHAPE_MORE);
        const bt_shape& s = shapes[first];
        const bt_shape_box box = box_of(e, s.half_width, width, height);
        if (boxes) boxes[k] = box;
        if (records && box.x_lo <= box.x_hi) records->push_back(ShapeRecord{first, end - first, box, k, s.kind, s.flags, s.op, s.value, s.half_width});
        first = end;
    }
    return nullptr;
}

}  // namespace bt

extern "C" bt_status bt_shapes_check(const bt_shape_vertex* vertices, uint32_t vertex_count, const bt_shape* shapes, uint32_t entry_count, uint32_t width,
                                     uint32_t height, bt_shape_box* boxes_out, uint32_t* shape_count_out, uint32_t* bad_entry_out) {
    uint32_t count = 0, bad = BT_SHAPES_NO_ENTRY;
    const char* defect = bt::shapes_check(vertices, vertex_count, shapes, entry_count, width, height, boxes_out, nullptr, &count, &bad);
    if (shape_count_out) *shape_count_out = defect ? 0u : count;
    if (bad_entry_out) *bad_entry_out = bad;
    if (!defect) return BT_OK;
    if (bad != BT_SHAPES_NO_ENTRY)
        bt::set_error("bt_shapes_check: entry %u: %s", bad, defect);
    else
        bt::set_error("bt_shapes_check: %s", defect);
    return BT_ERR_INVALID_ARGUMENT;
}

// bt_height_bounds, the min/max height table of the culling test (declared in the ABI header), between its host code
// (bt_height_bounds.cpp) and the update kernels (bt_bounds_update.hip): the table's layout, what the handle really points at, and the
// records the host fills for one update.
#pragma once

#include "bt_internal.hpp"

namespace bt {

// level l of the table starts at height_bounds_offset(sides, l)
inline uint64_t height_bounds_offset(uint32_t sides, uint32_t level) { return uint64_t(sides) * (((1ull << (2u * level)) - 1u) / 3u); }
constexpr uint32_t kBoundsNotHeld = 0x0000FFFFu;  // min > max: the shadow's (and bt_height_bounds_build's) word of a tile the atlas does not hold
// What bt_height_bounds_create really allocates: the public struct first (the handle points at it), then what bt_height_bounds_update
// needs.  shadow has the table's shape and holds own(tile) of every held tile, kBoundsNotHeld elsewhere: an entry is own united with the
// children, so the table alone does not say what own was.  current: table and shadow describe `atlas` / `attachment` as of the last build
// or update (bt_height_bounds_write clears it).
struct HeightBoundsImpl {
    bt_height_bounds pub{};
    uint32_t* shadow = nullptr;
    uint64_t atlas_uid = 0;  // bt_atlas::uid
    uint32_t attachment = 0;
    bool current = false;
};
inline HeightBoundsImpl* bounds_impl(bt_height_bounds* b) { return reinterpret_cast<HeightBoundsImpl*>(b); }

// ---- one update: the records of the host plan, as the kernels read them ----

constexpr uint32_t kMaxLevels = BT_HEIGHT_BOUNDS_MAX_LEVELS;
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
struct BoundsUpdateArgs {
    uint32_t* table;
    uint32_t* shadow;
    const uint32_t* own;  // one word per reduced layer (min | max << 16)
    const Scatter* scatter;
    const Window* windows;  // level by level
    uint32_t scatter_count, sides, levels, _pad;
    uint32_t level_window[kMaxLevels + 1];  // the first window of a level; [levels]: the number of windows
    uint32_t level_work[kMaxLevels + 1];    // affected entries of the levels before; [levels]: all of them
};

// (bt_bounds_update.hip wraps this record as `UpdateArgs` in its unnamed namespace, the name and scope the kernels' symbols have always
// spelt; taking the wrapper out renames the kernels, which changes the code object's symbol names and .note metadata and nothing else)
// bt_bounds_update.hip: the table work of one update on `stream` — one workgroup at or below kBoundsUpdateSmall affected entries, else
// scatter, fill and one unite per level that has entries.  Returns the number of launches; a launch error is left to hipGetLastError
uint32_t launch_bounds_update(hipStream_t stream, const BoundsUpdateArgs& args);

}  // namespace bt

// Internal declarations shared by the host (.cpp) and device (.hip) halves of libbevy_terrain_amd.so.
// Nothing here is part of the ABI; the ABI is include/bevy_terrain_amd.h.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstdint>
#include <deque>
#include <string>
#include <tuple>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "bevy_terrain_amd.h"

struct bt_preprocessor;
struct bt_ctx;

namespace bt {

void set_error(const char* fmt, ...);
bt_status hip_fail(hipError_t e, const char* what);
// kind and axes of a caller's terrain model (bt_view.cpp); `who`: the entry point the refusal names
bt_status check_model(const bt_terrain_model* m, const char* who);

#define BT_HIP(expr)                                          \
    do {                                                      \
        hipError_t _e = (expr);                               \
        if (_e != hipSuccess) return bt::hip_fail(_e, #expr); \
    } while (0)

// behind a kernel launch: what the launch left, `what` naming the kernel
inline bt_status launched(const char* what) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? BT_OK : hip_fail(e, what);
}

// offsets of the arrays carved from one device buffer: each 256-byte aligned, as an allocation of its own is
inline uint64_t align256(uint64_t v) { return (v + 255u) & ~uint64_t(255); }

inline bool operator_eq(const bt_tile_coordinate& a, const bt_tile_coordinate& b) {
    return a.side == b.side && a.lod == b.lod && a.x == b.x && a.y == b.y;
}
inline bool is_invalid(const bt_tile_coordinate& c) {
    return c.side == 0xFFFFFFFFu && c.lod == 0xFFFFFFFFu && c.x == 0xFFFFFFFFu && c.y == 0xFFFFFFFFu;
}

struct CoordHash {
    size_t operator()(const bt_tile_coordinate& c) const {
        uint64_t h = (uint64_t(c.side) << 59) ^ (uint64_t(c.lod) << 53) ^ (uint64_t(c.x) << 26) ^ uint64_t(c.y);
        h ^= h >> 31;
        h *= 0x9E3779B97F4A7C15ull;
        return size_t(h ^ (h >> 29));
    }
};
struct CoordEq {
    bool operator()(const bt_tile_coordinate& a, const bt_tile_coordinate& b) const { return operator_eq(a, b); }
};
struct CoordLess {  // the (side, lod, x, y) order of every sorted tile list
    bool operator()(const bt_tile_coordinate& l, const bt_tile_coordinate& r) const {
        return std::tie(l.side, l.lod, l.x, l.y) < std::tie(r.side, r.lod, r.x, r.y);
    }
};

// The runs of consecutive atlas layers among elements [begin, end) of a list, `layer(i)` being the layer of element i: fn(first, count) per
// run, in order, until one fails.  An element continues a run when its layer is the previous element's + 1 or, with merge_duplicates (a
// sorted list that may name a layer twice: the mip passes), the previous element's again.
template <typename Layer, typename Fn>
bt_status for_each_layer_run(size_t begin, size_t end, Layer layer, bool merge_duplicates, Fn fn) {
    for (size_t i = begin; i < end;) {
        size_t j = i + 1;
        while (j < end && (uint64_t(layer(j)) == uint64_t(layer(j - 1)) + 1u || (merge_duplicates && layer(j) == layer(j - 1)))) j++;
        if (bt_status s = fn(i, j - i)) return s;
        i = j;
    }
    return BT_OK;
}

// ---- device-visible descriptors -------------------------------------------------------------

// AttachmentMeta of the reference (gpu_tile_atlas.rs:45-56) reduced to what the kernels read.
struct AttachmentMeta {
    uint32_t format;        // BT_FORMAT_R16 / BT_FORMAT_RGBA8
    uint32_t texture_size;  // T
    uint32_t border_size;   // b
    uint32_t center_size;   // c = T - 2b
    uint32_t atlas_size;    // layers
    uint32_t pixel_size;    // bytes
    uint32_t row_limit;     // rows [0, row_limit) of a tile are written by the batched kernels: T, or (T / 8) * 8 under BT_RUN_REFERENCE_DISPATCH
};

struct RasterDev {
    const void* data;
    uint32_t width, height;
    uint64_t pitch;  // bytes per row
};

// One queued Split / Downsample / Stitch task in the form the batched kernels read.
struct TaskDev {
    uint32_t atlas_index;
    uint32_t side, lod, x, y;
    float tlx, tly, brx, bry;
    uint32_t raster;
    uint32_t regions;       // stitch: bit r set = only apron region r (0 top .. 7 bottom-left) is written; 0 = all eight
    uint32_t rel_index[8];  // children (4) or neighbours (8): atlas indices, INVALID if absent
    uint32_t rel_side[8];   // neighbour sides (stitch across cube faces)
};

// ---- host state -------------------------------------------------------------------------------

struct Attachment {
    bt_attachment_config cfg;
    AttachmentMeta meta;
    uint64_t tile_bytes = 0;
    void* level0 = nullptr;           // atlas_size x T x T texels
    std::vector<void*> mips;          // level k (k>=1): atlas_size x (T>>k)^2 texels; lazily allocated
    // written[layer] == 0: the layer still holds bt_atlas_create's zeros (a wgpu texture starts zeroed) — nothing has run on it, been
    // uploaded or loaded into it, and its device pointer has not been handed out (bt_atlas_attachment_storage marks every layer).  A split of a
    // job whose finest tiles are all unwritten takes "the previous value" of a no-data pixel (split.wgsl:34-42) as 0 without fetching it.
    mutable std::vector<uint8_t> written;  // (mutable: handing out the storage pointer of a const atlas counts as a write, bt_atlas_attachment_storage / bt_atlas_mip_storage level 0)
    void mark_written(uint32_t first, uint32_t count) const {
        for (uint64_t i = first; i < uint64_t(first) + count && i < written.size(); i++) written[i] = 1;
    }
};

// TileState of the atlas (tile_atlas.rs:260-277): `loading` = 0 is LoadingState::Loaded, n > 0 is Loading(n).
struct TileState {
    uint32_t atlas_index;
    uint32_t requests;
    uint32_t loading;
};

// AtlasTileAttachment (tile_atlas.rs:62-67)
struct AtlasTileAttachment {
    bt_tile_coordinate coordinate;
    uint32_t atlas_index;
    uint32_t attachment_index;
};

enum TaskType : uint32_t { kSplit = 0, kStitch = 1, kDownsample = 2, kSave = 3, kBarrier = 4 };

struct Task {
    TaskType type;
    bt_tile_coordinate coord;
    uint32_t atlas_index;
    uint32_t attachment_index;
    bt_atlas_tile rel[8];
    float tl[2], br[2];
    int32_t raster;  // index into bt_preprocessor::rasters
    uint32_t job;    // which preprocess_tile / preprocess_spherical call queued it
};

struct Raster {
    RasterDev dev;
    uint32_t format;
    bool owned;
    // bt_raster.on_device == BT_RASTER_HOST_DEFERRED: the device buffer exists, the caller's rows are copied when the queue runs
    // (all at once by bt_preprocessor_run, band by band next to the kernels by bt_preprocessor_run_streamed)
    const void* host = nullptr;
    uint64_t host_bytes = 0;
    uint64_t host_pitch = 0;  // the caller's row pitch (the device copy's may be padded to 16 bytes)
    bool pending = false;
    const void* dev_src = nullptr;  // a borrowed device raster that is not 16-byte aligned: copied into the padded buffer `dev` by the first run
    uint64_t dev_src_pitch = 0;
    // the rectangles {x0, y0, x1, y1} of a deferred raster that have travelled (a sharded run: this rank's window): the device holds each of
    // them completely; a window counts as present when ONE of them contains it
    std::vector<std::array<uint32_t, 4>> windows;
    bool holds(const uint32_t w[4]) const {
        for (const std::array<uint32_t, 4>& h : windows)
            if (w[0] >= h[0] && w[1] >= h[1] && w[2] <= h[2] && w[3] <= h[3]) return true;
        return false;
    }
    void add_window(const uint32_t w[4]) {
        if (holds(w)) return;
        windows.erase(std::remove_if(windows.begin(), windows.end(), [&](const std::array<uint32_t, 4>& h) { return h[0] >= w[0] && h[1] >= w[1] && h[2] <= w[2] && h[3] <= w[3]; }),
                      windows.end());
        windows.push_back({w[0], w[1], w[2], w[3]});
    }
    uint64_t alloc_bytes = 0;  // size of the owned device allocation
};

// A device buffer, optionally with a pinned twin of the same size, that only grows and is kept until bt_ctx_trim: a per-frame caller pays
// no allocation (bt_ctx.cpp)
struct Scratch {
    void* dev = nullptr;
    void* host = nullptr;
    uint64_t bytes = 0;
    // at least `need` bytes; a buffer that is too small is replaced once the context's stream has drained (work in flight may use it).
    // A failed allocation leaves the scratch empty
    bt_status reserve(bt_ctx* ctx, uint64_t need, bool with_pinned_twin = false);
    // frees both halves and returns the bytes given back (`bytes` per half that existed); *error keeps the first failure
    uint64_t release(hipError_t* error = nullptr);
};

}  // namespace bt

#include "bt_staging.hpp"  // the rings a context owns

struct bt_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipEvent_t ev_begin = nullptr, ev_end = nullptr;
    // the pinned buffers of every chunked transfer between host memory and the device (tile files, regions, normal maps)
    bt::StagingRing staging;
    // streamed runs: uploads and downloads on their own queues beside the kernels' stream (created on first use)
    hipStream_t copy_stream = nullptr, save_stream = nullptr;
    // released raster allocations are kept for the next queue (hipMalloc + hipFree of a 512 MB source cost ~1.5 ms of the
    // end-to-end span; a host that preprocesses dataset after dataset pays them once; a cube job has six): at most kSpareRasters buffers
    // and kSpareRasterBytes in all, the smallest goes first (bt_ctx_trim gives them all back)
    static constexpr size_t kSpareRasters = 8;
    static constexpr uint64_t kSpareRasterBytes = 4ull << 30;
    std::vector<std::pair<void*, uint64_t>> spare_rasters;  // (device pointer, bytes)
    void* take_spare_raster(uint64_t need, uint64_t* bytes) {  // the smallest kept buffer that holds `need` bytes, or nullptr
        size_t best = spare_rasters.size();
        for (size_t i = 0; i < spare_rasters.size(); i++)
            if (spare_rasters[i].second >= need && (best == spare_rasters.size() || spare_rasters[i].second < spare_rasters[best].second)) best = i;
        if (best == spare_rasters.size()) return nullptr;
        void* ptr = spare_rasters[best].first;
        *bytes = spare_rasters[best].second;
        spare_rasters.erase(spare_rasters.begin() + long(best));
        return ptr;
    }
    void park_raster(void* ptr, uint64_t bytes) {  // keeps it, or frees what does not fit any more (the smallest first)
        spare_rasters.push_back({ptr, bytes});
        for (;;) {
            uint64_t total = 0;
            size_t smallest = 0;
            for (size_t i = 0; i < spare_rasters.size(); i++) {
                total += spare_rasters[i].second;
                if (spare_rasters[i].second < spare_rasters[smallest].second) smallest = i;
            }
            if (spare_rasters.size() <= kSpareRasters && total <= kSpareRasterBytes) break;
            hipFree(spare_rasters[smallest].first);
            spare_rasters.erase(spare_rasters.begin() + long(smallest));
        }
    }
    uint32_t io_threads = 0;  // writer / reader threads of the save and load paths; 0 = automatic (bt_ctx_set_io_threads)
    // The scratch of the query calls: each grown on demand by its call (bt::Scratch::reserve), kept until bt_ctx_trim
    // bt_atlas_tile_bounds: the layer list and the pyramids of one chunk of layers, on the device and pinned
    bt::Scratch bounds;
    // bt_tile_tree_raycast: the rays and the hits of one call on the device; bt_tile_tree_sun_occlusion: the counters, points, directions
    // and statuses of one call; bt_tile_tree_collide_spheres / bt_tile_tree_sweep_spheres: the spheres (sweeps) and the contacts (hits) of one call
    bt::Scratch raycast;
    // bt_tile_tree_sample_normal: the positions, normals and cosines of one call; bt_atlas_tile_normals: the tile list and up to three
    // chunks of normal maps on their way to the pinned staging buffers; bt_tile_tree_tile_geometry(_hp): the tile list and the vertices of one chunk
    bt::Scratch normal;
    // bt_tile_tree_render: the pixel counters and the planes of one call on the device
    bt::Scratch render;
    // the staged rectangle of write_region and read_region / the new texels of smooth_height on the device
    bt::Scratch edit_region;
    // bt_atlas_path_field: the planes of one call on the device (raw texels, mask, heights, D, next, the block flags); and its
    // words with a pinned twin (the per-sweep counters of a batch, the counts of bt_path_stats)
    bt::Scratch path, path_words;
    // bt_atlas_scatter_instances: the totals, the tile list and the firsts of one call, the block records, block offsets and cell bytes of
    // one chunk of it, and the instance list on the device
    bt::Scratch scatter;
    // bt_atlas_erode_height: the planes of one call on the device (the gathered texels, the activity bytes, the weight bytes and the seven
    // state planes twice)
    bt::Scratch erode;
    // bt_atlas_drainage: the planes of one call on the device (raw texels, the two host masks, z, W, F, the directions, A, the block flags);
    // and its words with a pinned twin (the per-sweep counters of a batch, the counts of bt_drainage_stats)
    bt::Scratch drain, drain_words;
    // bt_atlas_viewshed: the planes of one call on the device (raw texels, their transpose, the clearance, the count, the mask); and the
    // counts of bt_viewshed_stats with a pinned twin
    bt::Scratch viewshed, viewshed_words;
    // bt_atlas_distance_field: the planes of one call on the device (raw texels, the host seed plane, the band summaries, r, dist2,
    // nearest); and the counts of bt_distance_stats with a pinned twin
    bt::Scratch distance, distance_words;
    // bt_atlas_skyline: the planes of one call on the device (raw texels, their transpose, the mask, the count, and per direction of a
    // batch the hull stack, steps and rise); and the counts of bt_skyline_stats with a pinned twin
    bt::Scratch skyline, skyline_words;
    // the packed tile calls (bt_pack.cpp): the streams, strip offsets and strip sizes of one chunk on the device; and the stream starts
    // of a packed chunk with a pinned twin
    bt::Scratch pack, pack_words;
    // bt_atlas_rasterize_shapes: the vertices, the entries, the shape records and the two planes of U on the device; and the counts of
    // bt_shapes_stats with a pinned twin
    bt::Scratch shapes, shapes_words;
    // bt_atlas_label_regions: the planes of one call on the device (raw texels, the host member plane, P, id, area, rank, the chunk
    // counts, the accumulators and the records); and the counts of bt_regions_stats with a pinned twin
    bt::Scratch regions, regions_words;
    std::array<bt::Scratch*, 23> scratch() {  // all of them: bt_ctx_trim, bt_ctx_destroy
        return {&bounds, &raycast,     &normal,   &render,         &edit_region, &path,           &path_words, &scatter,      &erode,
                &drain,  &drain_words, &viewshed, &viewshed_words, &distance,    &distance_words, &skyline,    &skyline_words,
                &pack,   &pack_words,  &shapes,   &shapes_words,   &regions,     &regions_words};
    }  // all of them: bt_ctx_trim, bt_ctx_destroy
    // the edit calls and bt_height_bounds_update: the plans of the calls in flight (bt::PlanRing::commit hands it out)
    bt::PlanRingState plan_ring;
};

namespace bt {
uint32_t usable_cpus();                 // CPUs this process may use: affinity mask capped by the cgroup CPU quota
uint32_t ctx_io_threads(const bt_ctx* ctx);  // the resolved thread count of the save / load paths
}

struct bt_atlas {
    bt_ctx* ctx = nullptr;
    bt_terrain_config config{};
    std::vector<bt::Attachment> attachments;
    // TileAtlasState (tile_atlas.rs:279-298)
    std::unordered_set<bt_tile_coordinate, bt::CoordHash, bt::CoordEq> existing_tiles;
    std::unordered_map<bt_tile_coordinate, bt::TileState, bt::CoordHash, bt::CoordEq> tile_states;
    std::deque<bt_atlas_tile> unused_tiles;        // LRU of free / released slots (:307-309, 459-476)
    std::deque<bt::AtlasTileAttachment> to_load;   // queued by request_tile (:445-451), drained by bt_atlas_update
    uint64_t uid = 0;                              // unique per bt_atlas_create of the process (an address can come back)
    uint64_t state_version = 1;                    // bumped whenever tile_states changes (device copies are rebuilt lazily)
    // the Save tasks of the preprocessor runs since the last bt_preprocessor_save (preprocessor.rs:378-380)
    std::vector<bt::AtlasTileAttachment> to_save;
    uint32_t tile_files = BT_TILE_FILES_BIN;  // what bt_atlas_update reads (bt_atlas_set_tile_files)
};

namespace bt {

// the R16 attachment a height query reads (bt_tile_tree_query.cpp): an index out of range is BT_ERR_INVALID_ARGUMENT, another format
// BT_ERR_UNSUPPORTED, each with a message that starts with `who`
bt_status height_attachment(const char* who, const bt_atlas* a, uint32_t ai, const Attachment** height);

// One launch of the compiled plan.
enum LaunchKind : uint32_t { kLaunchSplit, kLaunchDownsample, kLaunchStitch, kLaunchFusedMain, kLaunchFusedTail, kLaunchFusedDirect, kLaunchFusedTodo };
struct Launch {
    LaunchKind kind;
    uint32_t attachment;
    uint32_t first_task, task_count;  // into the device task array
    uint32_t aux0 = 0, aux1 = 0;
    uint64_t algorithmic_bytes = 0;  // inputs read once + outputs written once
    uint32_t phase = 0;              // sharded runs: 0 = BT_RUN_SHARD_LOCAL part, 2 = BT_RUN_SHARD_FINISH part
    uint32_t kernels = 1;            // kernels this plan entry launches (fused main without an LDS window: fused_corner + itself)
    uint32_t variant = 0;            // the BT_VARIANT_* bit of the kernel instance it runs, chosen at plan time (run_plan_entry reports it)
};

// the device record of a queued task (the batched kernels, fused_plan's stitch and seam records)
TaskDev to_device_task(const Task& t);

// host-side launchers implemented in bt_kernels.hip
bt_status launch_split(bt_ctx* ctx, const AttachmentMeta& m, void* atlas, const TaskDev* tasks, uint32_t n,
                       const RasterDev* rasters);
bt_status launch_downsample(bt_ctx* ctx, const AttachmentMeta& m, void* atlas, const TaskDev* tasks, uint32_t n);
// rows_only: just the top / bottom apron rows (full width, corners included) — the fused path writes the left / right
// apron columns of those tiles itself
bt_status launch_stitch(bt_ctx* ctx, const AttachmentMeta& m, void* atlas, const TaskDev* tasks, uint32_t n, bool rows_only = false, bool one_region = false);
bt_status launch_sample(bt_ctx* ctx, const AttachmentMeta& m, const void* atlas, const bt_tile_lookup* lookups, uint32_t count, float* out);
bt_status launch_mip_level(bt_ctx* ctx, uint32_t format, const void* parent, void* child, uint32_t parent_size,
                           uint32_t layers);
bt_status launch_gather_layers(hipStream_t stream, const void* atlas, const uint32_t* layers, uint32_t count, void* pinned_dst, uint64_t tile_bytes);
// bt_bounds.hip: the min/max pyramids of `count` R16 layers of size T (layers: device list) -> out (device, (4g^2 - 1) / 3 words per layer)
bt_status launch_tile_bounds(hipStream_t stream, const void* atlas, uint32_t T, const uint32_t* layers, uint32_t count, uint32_t grid,
                             bool skip_zero, uint32_t* out);
// bt_edit.hip: the in-place edit kernels.  An item is one tile's dirty rectangle (inclusive, in centre texels) of one launch
struct EditItem {
    uint32_t layer;           // the atlas layer written
    uint32_t x0, y0, x1, y1;  // the rectangle inside the tile's centre
    uint32_t gx0, gy0;        // mosaic position of the tile's centre texel (0, 0)
    uint32_t side;
    uint32_t child[4];        // downsample: the four child layers, BT_INVALID_ATLAS_INDEX where absent
};
bt_status launch_edit_brush(hipStream_t stream, const AttachmentMeta& m, void* atlas, const EditItem* items, uint32_t n, uint32_t max_rows,
                            const bt_edit_stamp* stamps, uint32_t stamp_count);
bt_status launch_edit_paint(hipStream_t stream, const AttachmentMeta& m, void* atlas, const EditItem* items, uint32_t n, uint32_t max_rows,
                            const bt_paint_stamp* stamps, uint32_t stamp_count);
// src: the staged rectangle (device, `src_width` texels per row, tightly packed) whose texel (0, 0) is mosaic texel (rx0, ry0)
bt_status launch_edit_region(hipStream_t stream, const AttachmentMeta& m, void* atlas, const EditItem* items, uint32_t n, uint32_t max_rows,
                             const void* src, uint32_t rx0, uint32_t ry0, uint32_t src_width);
// the other direction (bt_atlas_read_region): the items' rectangles of the layers -> the staged rectangle `dst`
bt_status launch_edit_gather(hipStream_t stream, const AttachmentMeta& m, const void* atlas, const EditItem* items, uint32_t n, uint32_t max_rows,
                             void* dst, uint32_t rx0, uint32_t ry0, uint32_t dst_width);
bt_status launch_edit_downsample(hipStream_t stream, const AttachmentMeta& m, void* atlas, const EditItem* items, uint32_t n, uint32_t max_rows);
// bt_atlas_smooth_height, two launches: edit_smooth_kernel<kernel_radius> reads the layers and writes the new dwords of every item's rectangle
// to `scratch` (device), the copy launch moves them into the layers.  offsets[i] (device): where item i's rectangle starts in `scratch`, in
// dwords; it holds (y1 - y0 + 1) rows of ((b + x1) >> 1) - ((b + x0) >> 1) + 1 dwords, the aligned pairs of texels the rectangle touches
// (smooth_item_dwords)
inline uint64_t smooth_item_dwords(const EditItem& it, uint32_t border_size) {
    return uint64_t(it.y1 - it.y0 + 1u) * (((border_size + it.x1) >> 1) - ((border_size + it.x0) >> 1) + 1u);
}
bt_status launch_edit_smooth(hipStream_t stream, const AttachmentMeta& m, void* atlas, const EditItem* items, const uint64_t* offsets, uint32_t n, uint32_t max_rows,
                             const bt_smooth_stamp* stamps, uint32_t stamp_count, uint32_t kernel_radius, void* scratch);
// bt_splat.hip, the first step of bt_atlas_splat_from_height: the items are rectangles of the Rgba8 attachment (`m`, `atlas`) and every texel
// of them is derived from the R16 attachment `src` of the same atlas (same texture_size and border_size; a tile has one layer index in
// both).  rules: src.count records on the device.  splat_reach: how far, in texels, the height texels a target texel reads lie from it
struct SplatSource {
    AttachmentMeta meta;  // of the heights
    const void* level0;
    const bt_terrain_model* model;
    uint32_t lod, mode, count;
    uint32_t fallback;  // the four bytes as the texel's dword
};
uint32_t splat_reach(const AttachmentMeta& m);
bt_status launch_edit_splat(hipStream_t stream, const AttachmentMeta& m, void* atlas, const EditItem* items, uint32_t n, uint32_t max_rows, const SplatSource& src,
                            const bt_splat_rule* rules);
// bt_scatter.hip, bt_atlas_scatter_instances behind its argument checks (bt_edit.cpp): the listed tiles (each with the layer that holds it)
// of the R16 attachment `meta` / `heights`, the optional Rgba8 mask attachment of the same texture_size and border_size (`mask`: its
// level 0, or nullptr), the checked rules.  Synchronous: the list, the firsts and the stats are the caller's when it returns
struct ScatterTile {
    uint32_t layer, lod, side, x, y;
};
struct ScatterJob {
    AttachmentMeta meta;  // of the heights
    const void* heights;
    const void* mask;
    const bt_terrain_model* model;
    const bt_scatter_rule* rules;
    uint32_t rule_count, seed;
    float jitter;
};
bt_status scatter_run(bt_ctx* ctx, const ScatterJob& job, const std::vector<ScatterTile>& tiles, bt_scatter_instance* out, uint64_t cap, uint64_t* out_first,
                      bt_scatter_stats* stats);
bt_status launch_synth_fbm(bt_ctx* ctx, void* dst, uint32_t w, uint32_t h, uint64_t pitch, uint32_t x0, uint32_t y0,
                           uint32_t base_cell, uint32_t octaves, uint32_t seed);

// fused-path state of a preprocessor (bt_fused_args.hpp; bt_fused_plan.cpp fills it): launch descriptors + device buffers of its compiled queue
struct FusedState;
void fused_release(struct ::bt_preprocessor* p);

bt_status release_queue(struct ::bt_preprocessor* p);  // bt_run.cpp
bt_status ensure_compiled(struct ::bt_preprocessor* p, struct ::bt_atlas* a, uint32_t mode);  // bt_run.cpp: queue -> launch plan
// bt_run.cpp: one launch of the plan; a fused main / direct launch runs the items [item_begin, item_begin + item_count) of its list (streamed runs' bands)
bt_status run_plan_entry(struct ::bt_preprocessor* p, struct ::bt_atlas* a, const Launch& l, uint32_t item_begin = 0, uint32_t item_count = 0xFFFFFFFFu);
uint32_t fused_begin_run(struct ::bt_preprocessor* p, struct ::bt_atlas* a);  // bt_fused_plan.cpp: per run, before its launches (FusedArgs::prev_zero, Attachment::written)
bt_status check_distributed_one_sided(const struct ::bt_preprocessor* p);  // bt_run.cpp: BT_RUN_SHARD_DISTRIBUTED is refused for a cube job
void record_saves(struct ::bt_preprocessor* p, struct ::bt_atlas* a);      // bt_run.cpp: the queue's Save tasks -> bt_atlas::to_save, once per queue and save
bool fused_plan(struct ::bt_preprocessor* p, struct ::bt_atlas* a, std::vector<TaskDev>& tasks, std::vector<Launch>& plan);  // bt_fused_plan.cpp: queue -> fused launch plan; false: the generic plan
bool fused_source_window(const struct ::bt_preprocessor* p, uint32_t raster, uint32_t out[4]);  // bt_fused_plan.cpp: the texels of a raster the plan's launches read; false: no window is known
// bt_stream.cpp: w = the fused source window of raster i when the caller asks for it and the plan has one, else the whole raster
void raster_window(const struct ::bt_preprocessor* p, uint32_t i, bool use_fused_window, uint32_t w[4]);
bt_status upload_pending_rasters(struct ::bt_preprocessor* p, const std::vector<uint8_t>* skip = nullptr);  // bt_stream.cpp: deferred host rasters, all at once (skip[i]: not raster i)
// bt_comm.cpp: the grouped collective of a sharded step, and whether a communicator fits the preprocessor's rank and world
bt_status shard_exchange(struct ::bt_preprocessor* p, struct ::bt_atlas* a, bt_comm* comm, hipStream_t stream, bool distributed);
bt_status shard_check_comm(const struct ::bt_preprocessor* p, const bt_comm* comm);

// streamed run (bt_stream.cpp drives it): a fused main / direct launch cut into bands of whole tile rows
struct StreamBand {
    uint32_t item_begin, item_count;  // into the job's item list ((side, tile row, x) order)
    uint32_t tile_y_begin, tile_y_end;
    uint32_t side, raster;            // the cube side of the band's tiles and the source raster they read
    uint32_t source_row_end;          // the band's kernels read rows of that raster below this one (exclusive)
};
// true when plan entry `l` is a fused main / direct launch that can run band by band (tile_rows_per_band 0: automatic)
bool fused_stream_bands(struct ::bt_preprocessor* p, const Launch& l, uint32_t tile_rows_per_band, std::vector<StreamBand>* bands);
bt_status fused_launch_range(struct ::bt_preprocessor* p, struct ::bt_atlas* a, const Launch& l, uint32_t item_begin, uint32_t item_count);
// the finest tiles [item_begin, item_begin + item_count) of a fused main / direct launch, in launch order
struct FusedTile {
    bt_tile_coordinate coordinate;
    uint32_t atlas_index;
};
void fused_launch_tiles(const struct ::bt_preprocessor* p, const Launch& l, uint32_t item_begin, uint32_t item_count, std::vector<FusedTile>* out);

// coordinate math (bt_coordinate.cpp)
// neighbour k of a tile is at (x, y) + kNeighbourOffsets[k]: N, E, S, W, NW, NE, SE, SW (coordinate.rs:209-218) == the region order of stitch.wgsl:57-66
inline constexpr int kNeighbourOffsets[8][2] = {{0, -1}, {1, 0}, {0, 1}, {-1, 0}, {-1, -1}, {1, -1}, {1, 1}, {-1, 1}};
void tile_children(bt_tile_coordinate c, bt_tile_coordinate out[4]);
void tile_neighbours(bt_tile_coordinate c, bool spherical, bt_tile_coordinate out[8]);
inline bool on_face_edge(const bt_tile_coordinate& c) {  // the tile touches an edge of its cube face
    const uint32_t n = 1u << c.lod;
    return c.x == 0 || c.y == 0 || c.x == n - 1 || c.y == n - 1;
}

}  // namespace bt

struct bt_preprocessor {
    bt_ctx* ctx = nullptr;
    std::vector<bt::Task> queue;
    std::vector<bt::Raster> rasters;
    uint32_t jobs = 0;
    uint32_t shard_rank = 0, shard_world = 1;
    bool shard_distributed = false;  // the last sharded run kept the finest LOD on its owners (BT_RUN_SHARD_DISTRIBUTED)
    std::vector<bt_shard_range> shard_ranges;
    std::vector<bt_shard_piece> shard_pieces;
    // BT_RUN_SHARD_OVERLAP: the job's collective runs on the communicator's stream between these two events
    hipEvent_t shard_local_done = nullptr, shard_exchange_done = nullptr;
    bool shard_exchange_pending = false;  // bt_preprocessor_finish_sharded has to follow
    uint64_t uploaded_source_bytes = 0;   // bytes of the last deferred host raster that actually travelled (a sharded run: its window)
    // compiled plan (rebuilt when the queue changes)
    bool compiled = false;
    bool saves_recorded = false;  // the kept queue's Save tasks are already in the atlas's to_save list
    uint32_t compiled_flags = 0;
    std::vector<bt::Launch> plan;
    bt::TaskDev* tasks_dev = nullptr;
    size_t tasks_dev_cap = 0;
    std::vector<bt::TaskDev> tasks_host;  // the same records on the host (which layers a batched launch writes: Attachment::written)
    bt::RasterDev* rasters_dev = nullptr;
    size_t rasters_dev_cap = 0;
    bt_run_stats stats{};
    bt::FusedState* fused = nullptr;  // owned; freed by fused_release
    // BT_RUN_PROFILE: events[run * (plan.size() + 1) + i]; event 0 of a run precedes its first launch
    std::vector<hipEvent_t> events;
    std::vector<hipEvent_t> event_pool;  // events read by bt_preprocessor_profile, kept for the next profiled runs (no hipEventCreate inside a timed step)
    uint32_t profiled_runs = 0;
    std::vector<uint32_t> profiled_phases;  // per profiled run: BT_RUN_SHARD_LOCAL | BT_RUN_SHARD_FINISH bits of the plan halves it executed
};

namespace bt {
// the finest LOD among the sharded pieces of an attachment (what BT_RUN_SHARD_DISTRIBUTED leaves on its owners)
inline uint32_t shard_finest_lod(const ::bt_preprocessor* p, uint32_t attachment) {
    uint32_t lod = 0;
    for (const bt_shard_piece& piece : p->shard_pieces)
        if (piece.attachment_index == attachment && piece.lod > lod) lod = piece.lod;
    return lod;
}
// the rank that holds tile `atlas_index` of `attachment` after a distributed run: the owner of its finest-LOD piece, or,
// for every other tile (all ranks hold those), atlas_index % world — one writer per file
inline uint32_t shard_holder(const ::bt_preprocessor* p, uint32_t attachment, uint32_t lod, uint32_t atlas_index) {
    if (lod == shard_finest_lod(p, attachment))
        for (const bt_shard_piece& piece : p->shard_pieces)
            if (piece.attachment_index == attachment && piece.lod == lod && atlas_index >= piece.first_layer && atlas_index < piece.first_layer + piece.layers)
                return piece.owner_rank;
    return atlas_index % p->shard_world;
}

// bt_edit.cpp, the halves of bt_atlas_read_region that bt_atlas_path_field shares.  region_check: what the read refuses of attachment,
// side, lod and rectangle (`what` names the entry point).  region_gather: the rectangle's texels of the layers -> `dst` on the device
// (tightly packed rows; tiles the atlas does not hold: zeros, counted in *tiles_missing), enqueued on the context's stream.
// region_stage_out: `height` rows of row_bytes from `src` on the device through the context's pinned staging buffers into host rows
// row_pitch apart; synchronous
bt_status region_check(const bt_atlas* a, uint32_t ai, uint32_t side, uint32_t lod, uint32_t x0, uint32_t y0, uint32_t width, uint32_t height, const char* what);
bt_status region_gather(const bt_atlas* a, uint32_t ai, uint32_t side, uint32_t lod, uint32_t x0, uint32_t y0, uint32_t width, uint32_t height, void* dst, uint32_t* tiles_missing);
bt_status region_stage_out(bt_ctx* ctx, const void* src, void* texels, uint64_t row_bytes, uint64_t row_pitch, uint32_t height, const char* what);
// the way in (bt_atlas_write_region's rectangle, the host planes of bt_atlas_erode_height): `height` host rows row_pitch apart -> pinned staging ->
// tightly packed rows at `dst` on the device, enqueued; the ring's events cover the copies (the caller drains it before it returns)
bt_status region_stage_in(bt_ctx* ctx, void* dst, const void* texels, uint64_t row_bytes, uint64_t row_pitch, uint32_t height);

// bt_erode.hip: the kernels of bt_atlas_erode_height.  Planes are width x height, row-major
struct ErodePlanes {  // one side of the ping-pong
    float *b, *d, *s, *f[4];
};
struct ErodeConsts {  // the parameters the kernels read and the host constants of the header, each formed once
    float min_height, range, cell_size, dt, capacity, erode, deposit, min_tilt, min_depth;
    float rain_dt, cf, l2, two_l, keep;
};
constexpr uint32_t kErodeBlock = BT_ERODE_BLOCK;  // a workgroup's cells are kErodeBlock x kErodeBlock
// raw texels -> b, the fluxes (0) and the activity bytes; water / sediment: p.d / p.s hold the caller's plane (kept on active cells), else set to 0
bt_status launch_erode_init(hipStream_t stream, const uint16_t* raw, bool water, bool sediment, const ErodePlanes& p, uint8_t* act, uint32_t cells, const ErodeConsts& c);
// one step: in -> out
bt_status launch_erode_step(hipStream_t stream, const ErodePlanes& in, const ErodePlanes& out, const uint8_t* act, uint32_t width, uint32_t height, const ErodeConsts& c);
// the blend (weight: bytes on the device, or nullptr) and the quantisation -> the staged rectangle of R16 texels
bt_status launch_erode_finish(hipStream_t stream, const uint16_t* raw, const float* bT, const uint8_t* weight, uint16_t* texels, uint32_t cells, const ErodeConsts& c);

// bt_relax.hpp: the window of a block relaxation and its blocks of kRelaxBlock x kRelaxBlock cells, one workgroup each
constexpr uint32_t kRelaxBlock = BT_DRAIN_BLOCK;
struct RelaxGrid {
    uint32_t width, height;
    uint32_t blocks_x, blocks_y;
    static RelaxGrid of(uint32_t width, uint32_t height) { return {width, height, (width + kRelaxBlock - 1u) / kRelaxBlock, (height + kRelaxBlock - 1u) / kRelaxBlock}; }
};

// bt_path.hip: the kernels of bt_atlas_path_field.  Planes are width x height, row-major; D holds the bits of non-negative floats
struct PathPlanes : RelaxGrid {
    const uint16_t* raw;   // the gathered texels
    const uint8_t* mask;   // the caller's mask on the device, or nullptr
    float* h;              // heights; NaN = blocked (raw 0, a missing tile or the mask)
    uint32_t* D;           // the field, as bits
    uint8_t* next;         // between prepare and next: 1 marks a cell that some goal entry names
};
struct PathCounts {  // the device words of bt_path_stats
    uint32_t blocked, reachable, goals_blocked, _padding;
};
// prepare: h and the count of blocked cells; the goals (device list) into D (memset to +inf before) by atomicMin, their cells
// marked in `next` (memset to 0 before) and the 3 x 3 blocks around each in `flags` (memset to 0 before); blocked goals counted
bt_status launch_path_prepare(hipStream_t stream, const PathPlanes& p, const bt_path_cost& cost, const bt_path_goal* goals, uint32_t goal_count, uint32_t* flags, PathCounts* counts);
// one sweep of relax_kernel (bt_relax.hpp): every block whose flag in `active` is set clears it, relaxes its cells in LDS (at most `rounds` rounds), writes back
// the cells it changed and sets the flags of the blocks that have to look again in `activate`; *marked counts the blocks that set a flag
bt_status launch_path_relax(hipStream_t stream, const PathPlanes& p, const bt_path_cost& cost, float cell_diag, uint32_t rounds, uint32_t* active, uint32_t* activate, uint32_t* marked);
// the next plane by the header's rule, and the count of reachable cells
bt_status launch_path_next(hipStream_t stream, const PathPlanes& p, const bt_path_cost& cost, float cell_diag, const bt_path_goal* goals, uint32_t goal_count, PathCounts* counts);

// bt_drain.hip: the kernels of bt_atlas_drainage.  Planes are width x height, row-major
struct DrainPlanes : RelaxGrid {
    const uint16_t* raw;    // the gathered texels
    const uint8_t* mask;    // the caller's void mask on the device, or nullptr
    const uint8_t* weight;  // the caller's weights on the device, or nullptr (every w = 1)
    uint16_t* z;            // heights; 0 = void (raw 0, a missing tile or the mask)
    uint16_t* W;            // the filled level; 0 on void cells
    uint32_t* F;            // the flat distance; 0 on void cells
    uint8_t* dir;           // the direction plane
    uint32_t* A;            // the accumulation; 0 on void cells
};
struct DrainCounts {  // the device words of bt_drainage_stats
    uint32_t voids, outlets, filled, flats, max_flat_distance, max_accumulation, outflow, _padding;
};
enum DrainRule : uint32_t { kDrainFill = 0, kDrainFlat = 1, kDrainAccumulate = 2 };
// prepare: z, the initial X of the fill (z on outlets, 65535 on other active cells, 0 on void ones) in W, the counts of void cells and outlets
bt_status launch_drain_prepare(hipStream_t stream, const DrainPlanes& p, DrainCounts* counts);
// one sweep of one rule, as launch_path_relax
bt_status launch_drain_relax(hipStream_t stream, DrainRule rule, const DrainPlanes& p, uint32_t rounds, uint32_t* active, uint32_t* activate, uint32_t* marked);
// the seed of the flat relaxation from the final W: F = 0 on drain cells and void ones, 0xFFFFFFFF elsewhere
bt_status launch_drain_flat_seed(hipStream_t stream, const DrainPlanes& p);
// the direction plane by the header's rule from the final W and F, and the seed of the accumulation: A = w (0 on void cells)
bt_status launch_drain_direction(hipStream_t stream, const DrainPlanes& p);
// the counts that need the final planes: filled, flats, the two maxima and the outflow
bt_status launch_drain_finish(hipStream_t stream, const DrainPlanes& p, DrainCounts* counts);

// bt_viewshed.hip: the kernels of bt_atlas_viewshed.  Planes are width x height, row-major
struct ViewshedPlanes {
    uint32_t width, height;
    const uint16_t* raw;      // the gathered texels: 0 = void
    uint16_t* transposed;     // raw with the axes exchanged: cell (x, y) at x * height + y
    uint32_t* clearance;      // BT_VIEWSHED_NONE on void cells and on cells no used observer covers
    uint8_t* count;
    uint64_t* mask;           // or nullptr: not asked for
    uint32_t target_height;
    uint32_t observer_count;
    bt_viewshed_observer observers[BT_VIEWSHED_MAX_OBSERVERS];  // in the kernel arguments: every wave reads them as scalars
};
struct ViewshedCounts {  // the device words of bt_viewshed_stats
    uint32_t voids, observers_used, observers_skipped, covered, visible, max_clearance;
    unsigned long long samples;
};
// raw -> transposed
bt_status launch_viewshed_transpose(hipStream_t stream, const ViewshedPlanes& p);
// the line walk: the three output planes, in two launches (the x-major lines on the transposed plane, then the y-major ones)
bt_status launch_viewshed_walk(hipStream_t stream, const ViewshedPlanes& p);
// the counts
bt_status launch_viewshed_finish(hipStream_t stream, const ViewshedPlanes& p, ViewshedCounts* counts);

// bt_distance.hip: the kernels of bt_atlas_distance_field.  Planes are width x height, row-major
constexpr uint32_t kDistanceBand = BT_DISTANCE_BAND;  // rows of a band of the column phase: a band's seeds are the bits of one word
struct DistancePlanes {
    uint32_t width, height, bands;  // bands = ceil(height / kDistanceBand)
    const void* raw;                // the gathered texels: u16 (R16) or u32 (Rgba8)
    const uint8_t* host;            // the caller's seed plane on the device, or nullptr
    uint32_t wide;                  // 1: Rgba8 texels
    uint32_t shift;                 // of the texel to its channel: 8 * channel
    uint32_t value_mask;            // 0xFFFF or 0xFF
    uint32_t lo, hi;                // from_texels: lo <= v <= hi; a band no v lies in (lo 1, hi 0) without FROM_TEXELS
    uint32_t invert;                // 0 or 1
    uint16_t* first;                // bands x width: a band's first seed row per column, 0xFFFF = none; after the carry: the first seed row below the band
    uint16_t* last;                 // its last seed row; after the carry: the last seed row above the band
    uint16_t* r;                    // the row of the column's nearest seed, the upper on a tie; 0xFFFF = none
    uint32_t* dist2;
    uint32_t* nearest;
};
struct DistanceBake {  // the byte the finish launch merges into the staged rectangle
    uint32_t* texels;  // the destination's Rgba8 texels on the device, or nullptr: no bake
    uint32_t shift;    // 8 * channel
    uint32_t near;     // 0 or 1: 255 - b
    uint64_t reach2;   // reach * reach
};
struct DistanceCounts {  // the device words of bt_distance_stats
    uint32_t seeds, max_dist2;
    unsigned long long sum_dist2;
};
// the column phase in its three launches: the band summaries, the carry across the bands, r
bt_status launch_distance_columns(hipStream_t stream, const DistancePlanes& p);
// the row phase: dist2 and nearest
bt_status launch_distance_rows(hipStream_t stream, const DistancePlanes& p);
// the counts, and the baked byte
bt_status launch_distance_finish(hipStream_t stream, const DistancePlanes& p, const DistanceBake& bake, DistanceCounts* counts);

// bt_skyline.hip: the kernels of bt_atlas_skyline.  Planes are width x height, row-major; the per-direction ones hold a batch
struct SkylinePlanes {
    uint32_t width, height;
    const uint16_t* raw;      // the gathered texels
    uint16_t* transposed;     // raw with the axes exchanged: cell (x, y) at x * height + y
    uint32_t* stack;          // batch x cells hull entries below the two in registers: major coordinate << 16 | z
    uint16_t* steps;          // batch x cells
    int32_t* rise;            // batch x cells
    uint64_t* mask;
    uint8_t* count;
    uint32_t direction_count;  // of the call
    uint32_t first, batch;     // the directions of this batch: first .. first + batch - 1
    bt_skyline_direction directions[BT_SKYLINE_MAX_DIRECTIONS];  // in the kernel arguments: every wave reads them as scalars
};
struct SkylineBake {   // the byte the last finish launch merges into the staged rectangle
    uint32_t* texels;  // the destination's Rgba8 texels on the device, or nullptr: no bake
    uint32_t shift;    // 8 * channel
    uint32_t shade;    // 0 or 1: 255 - b
};
struct SkylineCounts {  // the device words of bt_skyline_stats
    uint32_t voids, max_steps;
    unsigned long long lit, sum_steps;
};
struct SkylinePlan {  // bt_skyline.cpp: what the call does, from its arguments alone
    uint32_t batch;     // directions in flight: B of the header
    uint32_t batches;   // ceil(direction_count / batch)
    uint32_t launches;  // of bt_skyline_stats
    uint32_t lines, longest_line;
};
SkylinePlan skyline_plan(uint32_t width, uint32_t height, const bt_skyline_direction* directions, uint32_t direction_count, bool bake);
// the first defect of the directions as text, or nullptr; *which: the index of the direction
const char* skyline_bad_direction(const bt_skyline_direction* directions, uint32_t direction_count, uint32_t* which);
// raw -> transposed
bt_status launch_skyline_transpose(hipStream_t stream, const SkylinePlanes& p);
// the hull walk of the batch: steps and rise
bt_status launch_skyline_walk(hipStream_t stream, const SkylinePlanes& p);
// the batch's bits into the mask and the running counts; last: count, the void count and the baked byte
bt_status launch_skyline_finish(hipStream_t stream, const SkylinePlanes& p, const SkylineBake& bake, bool last, SkylineCounts* counts);

// bt_shapes.cpp / bt_shapes.hip: bt_shapes_check's rules and the raster kernel of bt_atlas_rasterize_shapes (SHAPES in the header)
struct ShapeRecord {  // one shape with a box inside the window, as the kernel reads it (uniformly)
    uint32_t first_entry, entry_count;  // of the entry array
    bt_shape_box box;                   // in cells of the window
    uint32_t k;                         // the shape's number in the list
    uint32_t kind, flags, op, value;    // of its entries (they agree)
    uint32_t half_width;
};
static_assert(sizeof(ShapeRecord) == 40, "ten words");
struct ShapesCounts {  // the device words of bt_shapes_stats
    unsigned long long covered, written;
};
struct ShapesJob {
    const bt_shape_vertex* vertices;
    const bt_shape* entries;
    const ShapeRecord* records;
    uint32_t record_count;
    uint32_t wide;           // 1: Rgba8 texels
    uint32_t shift;          // of the texel to its channel: 8 * channel
    bt_shape_box u;          // the written rectangle, in cells of the window
    void* texels;            // U's texels, (u.x_hi - u.x_lo + 1) a row: u16 (R16) or u32 (Rgba8); folded in place
    uint8_t* count;          // U's planes, rows as the texels'
    uint16_t* last;
    ShapesCounts* counts;
};
// The first defect of a list as text (nullptr: none) and *bad_entry, the entry it names (BT_SHAPES_NO_ENTRY: not one entry's).  boxes
// (may be nullptr): one per shape; records (may be nullptr): the shapes whose box is not empty, in list order; *shape_count: all shapes
const char* shapes_check(const bt_shape_vertex* vertices, uint32_t vertex_count, const bt_shape* shapes, uint32_t entry_count, uint32_t width, uint32_t height,
                         bt_shape_box* boxes, std::vector<ShapeRecord>* records, uint32_t* shape_count, uint32_t* bad_entry);
bt_status launch_shapes_raster(hipStream_t stream, const ShapesJob& job);

// bt_regions.hip: the kernels of bt_atlas_label_regions (REGIONS in the header).  Planes are width x height, row-major
constexpr uint32_t kRegionsBlock = BT_REGIONS_BLOCK;  // cells across a block of the local launch
constexpr uint32_t kRegionsChunk = BT_REGIONS_CHUNK;  // consecutive cells of a workgroup of the linear launches
struct RegionAccum {  // what the emit launch folds a region's cells into: all zeros at first, so the minima are kept as maxima of complements
    uint32_t label, area;
    uint32_t not_x_min, not_y_min, x_max, y_max, not_v_min, v_max;
    uint32_t edges, _padding;
    unsigned long long v_sum;
};
static_assert(sizeof(RegionAccum) == 48, "twelve words");
struct RegionsPlanes {
    uint32_t width, height;
    const void* raw;         // the gathered texels: u16 (R16) or u32 (Rgba8)
    const uint8_t* host;     // the caller's member plane on the device, or nullptr
    uint32_t wide;           // 1: Rgba8 texels
    uint32_t shift;          // of the texel to its channel: 8 * channel
    uint32_t value_mask;     // 0xFFFF or 0xFF
    uint32_t lo, hi;         // from_texels: lo <= v <= hi; a band no v lies in (lo 1, hi 0) without FROM_TEXELS
    uint32_t invert, eight;  // 0 or 1 each
    uint32_t max_step;
    uint32_t region_cap;     // records of `accum`: min(the caller's region_cap, cells)
    uint32_t* P;             // the parent plane; after the flatten launch: label
    uint32_t* id;
    uint32_t* area;          // at a label: the cells of its region
    uint32_t* rank;          // at a label: its rank among the labels of its chunk
    uint32_t* chunk_roots;   // per chunk: its labels; after the scan launch: the labels of the chunks before it
    RegionAccum* accum;
};
struct RegionsBake {   // the byte the finish launch merges into the staged rectangle
    uint32_t* texels;  // the destination's Rgba8 texels on the device, or nullptr: no bake
    uint32_t shift;    // 8 * channel
    uint32_t min_area, max_area, value;
};
struct RegionsCounts {  // the device words of bt_regions_stats
    uint32_t members, regions, baked, _padding;
    unsigned long long largest;  // area << 32 | ~label of the largest region, the smallest label among equals; 0 without a region
};
// the local, seam, flatten and scan launches: P becomes label, area, rank and chunk_roots are filled, counts->members and ->regions
bt_status launch_regions_label(hipStream_t stream, const RegionsPlanes& p, RegionsCounts* counts);
// id, and the accumulators of the regions with an id below region_cap
bt_status launch_regions_emit(hipStream_t stream, const RegionsPlanes& p);
// the largest region, the baked byte, the records
bt_status launch_regions_finish(hipStream_t stream, const RegionsPlanes& p, const RegionsBake& bake, RegionsCounts* counts, bt_region* table);

// bt_pack.hip: the kernels of the packed tile calls (the format: PACKED TILES in the header).  One wave per strip of a tile; a chunk holds
// at most kPackChunk tiles, whose layers and stream starts travel in the kernel arguments
constexpr uint32_t kPackChunk = 64;
struct PackShape {  // of one attachment's tiles
    uint32_t T, planes, bits, gpr, strips;
    uint32_t W;     // groups = width bytes of a tile
    uint32_t head;  // 16 + pad8(W): a stream's bytes before its payload
    uint64_t tile_bytes;
    uint64_t bound() const { return head + 8ull * bits * W; }  // the largest stream: a group takes 64 lanes' bits, the dead ones included
    static PackShape of(uint32_t format, uint32_t T) {
        PackShape s{};
        s.T = T, s.planes = format == BT_FORMAT_R16 ? 1u : 4u, s.bits = format == BT_FORMAT_R16 ? 16u : 8u;
        s.gpr = (T + 63u) / 64u, s.strips = (T + BT_PACK_STRIP_ROWS - 1u) / BT_PACK_STRIP_ROWS;
        s.W = s.planes * T * s.gpr, s.head = 16u + ((s.W + 7u) & ~7u);
        s.tile_bytes = uint64_t(T) * T * (format == BT_FORMAT_R16 ? 2u : 4u);
        return s;
    }
};
struct PackTiles {
    uint32_t count;
    uint32_t layers[kPackChunk];
};
// measure: strip_bytes[q * strips + s] = the payload bytes of strip s of tile q; scan: starts[q] (count + 1 of them) = where tile q's stream begins
// in the chunk's output, strip_off[q * strips + s] = where that strip's payload begins; emit: the streams into `out`
bt_status launch_pack_measure(hipStream_t stream, uint32_t format, const PackShape& s, const void* level0, const PackTiles& tiles, uint32_t* strip_bytes);
bt_status launch_pack_scan(hipStream_t stream, const PackShape& s, uint32_t count, const uint32_t* strip_bytes, uint64_t* starts, uint64_t* strip_off);
bt_status launch_pack_emit(hipStream_t stream, uint32_t format, const PackShape& s, const void* level0, const PackTiles& tiles, const uint64_t* starts,
                           const uint64_t* strip_off, uint8_t* out);
// decode: validated streams in `packed` (stream q at starts[q], its strips' payloads at strip_off[q * strips + s], both device tables) -> the layers
bt_status launch_pack_decode(hipStream_t stream, uint32_t format, const PackShape& s, void* level0, const PackTiles& tiles, const uint8_t* packed,
                             const uint64_t* starts, const uint64_t* strip_off);

// the three forms of the tiling prepass with the view's approximate_height optionally taken from device memory (bt_frame_update);
// form: 0 = bt_tiling_prepass_run, 1 = _run_unordered, 2 = _run_plain
bt_status tiling_prepass_enqueue(bt_tiling_prepass* t, const bt_view_state* view, const float* device_height, uint32_t form);
bt_ctx* tiling_prepass_ctx(const bt_tiling_prepass* t);  // the context (stream) its kernels run on
// the final tile list on the device, the word that holds its length (as the last run left it) and the buffer's capacity in tiles
void tiling_prepass_final(const bt_tiling_prepass* t, const bt_tile_coordinate** final_tiles, const uint32_t** final_count, uint32_t* capacity);
}  // namespace bt

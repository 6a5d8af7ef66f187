// What the fused path's planner (bt_fused_plan.cpp) and its kernels and launcher (bt_fused.hip) share: the constants both use, the kernels'
// argument block, fused_main's LDS layout (the planner sizes the window behind it) and the per-queue state the planner fills and the
// launcher reads.  Read by host and device.
// The kernel arguments stay in the anonymous namespace: a kernel's symbol carries its argument type's, so they name the kernels.  Both
// translation units read this one text, and nothing of these types crosses between them except inside FusedState.
// A known wart: FusedJobDev and FusedState, in namespace bt, embed those types, so formally each unit defines bt::FusedState with a member type
// of its own (an ODR violation) and the linker merges the two units' std::vector<FusedJobDev> instantiations.  It is harmless only because both
// see the same layout and the same code: keep these two structs plain data, with no inline member function that is not trivial.
#pragma once

#include <vector>

#include "bt_internal.hpp"

namespace bt {

namespace {

constexpr uint32_t kInvalid = 0xFFFFFFFFu;
constexpr uint32_t kMainRows = 8;                // centre rows per fused_main workgroup (multiple of 4)
constexpr uint32_t kMaxBorder = 8;
constexpr uint32_t kApronPairsPerThread = 4;  // fused_tail's R16 apron rows (a workgroup = 1024 pixel pairs: a T = 512, b = 2 tile's four apron rows — a quarter of the extra workgroups of one pair per thread)
constexpr uint32_t kDirectRows = 4, kDirectMaxBlocks = 16;  // fused_direct: centre rows per block, and the most blocks one workgroup runs

struct MainItem {  // one finest-LOD tile
    uint32_t side, x, y, atlas_index, raster;
};

struct FusedArgs {
    AttachmentMeta m;
    uint16_t* atlas;
    const RasterDev* rasters;
    const MainItem* items;
    const uint32_t* grids;         // per (side, lod): n x n atlas indices, x-major (x * n + y), INVALID = absent
    uint32_t grid_lod_lo, grid_lod_hi, grid_sides;  // the grids of (side, lod), lod_lo <= lod <= lod_hi, follow each other side-major, LODs ascending
    // A job queued onto a fresh atlas holds its tiles in the reference's allocation order (preprocessor.rs:234-343: per side the finest
    // LOD first, x-major, then each coarser LOD), i.e. atlas index = arithmetic on the coordinate.  regular != 0: the host checked every
    // grid entry against that closed form, and a lookup is a handful of scalar operations instead of a dependent load from the grids
    // (fused_tail was a chain of five dependent round trips, three of them lookups).
    uint32_t regular, reg_first;
    // fused_tail on a cube (round 5): the cross-face apron regions of the LODs fused_main produced — their sources, the neighbour faces'
    // centres, are complete when the tail starts — ride in the tail launch as extra workgroups, one region each (stitch.wgsl:12-51, 79-118),
    // instead of waiting for a launch of their own behind it.  seam_skip: the tail's own apron-row workgroups leave those regions alone.
    const TaskDev* seam_tasks;
    uint32_t seam_count, seam_skip;
    // round 6: the cross-face regions of the LODs the tail ITSELF produces ride in it too — not as copies of the neighbour face's centre (another
    // workgroup of this launch is still writing it) but PULLED: evaluated from the tail's input LOD on the neighbour face with the tail's own
    // reduction (TaskDev::raster = LODs below the input, rel_index[region] = the neighbour tile's x << 16 | y).  seam_pull: the tail's pushes then
    // leave a region beyond exactly one face edge alone instead of clamping into it (a pull workgroup writes it) — and no stitch launch follows.
    uint32_t seam_pull;
    uint32_t tail_extras;  // fused_tail: apron blocks per side (the top / bottom apron rows — Rgba8: and columns — of the LODs above)
    float tlx, tly, brx, bry;
    uint32_t lod;         // finest LOD of this launch (fused_main) / input LOD (fused_tail)
    uint32_t levels;      // LODs produced by this launch: main 1..3 (lod, lod-1, lod-2); tail 1..3 below lod
    uint32_t item_count;  // fused_main: tiles
    uint32_t groups;      // fused_main: row groups per tile
    uint32_t sides;       // fused_tail: 1 or 6
    uint32_t lds_pitch;   // fused_main: texels per staged source row (multiple of 8)
    uint32_t lds_rows;    // fused_main: staged source rows that fit
    uint32_t apron_lods;  // fused_tail: LODs lod, lod+1, ... (this many) get their top / bottom apron rows from extra workgroups
    uint32_t rotate_priority;  // fused_main: wave priority rotates with the chunk index (see fused_main_chunks)
    uint32_t apron_cols;  // fused_tail (Rgba8 after fused_direct, which writes centres only): ... and their left / right apron columns
    // fused_main / fused_direct: every finest tile of the job still holds bt_atlas_create's zeros (Attachment::written, decided by the host per
    // run): "the previous value" of a pixel without data (split.wgsl:34-42) IS 0 — taken as a constant instead of fetched from the atlas.  Both
    // reference examples are this case (clear_attachment, then one dataset per attachment: preprocess_planar.rs:16-60).
    uint32_t prev_zero;
    // fused_main: the tile's 2b apron rows (first / last chunk only) read their source rows from global memory instead of the staged window, which
    // then holds the centre rows alone — set by the host when that is what lets four workgroups share a CU's LDS (source-to-tile ratios from ~1.25)
    uint32_t apron_global;
    // fused_main, run-time-pitch DMA variant: ONE staging buffer — the next chunk's rows are requested when every wave has read this chunk's (no overlap inside the
    // workgroup; the CU's other workgroups cover) — set by the host when two buffers would keep a fourth workgroup off the CU's LDS (ratios from ~1.36 at T = 512)
    uint32_t single_buffer;
    uint32_t ablate;      // debug only (env BT_FUSED_ABLATE): 1 no pyramid, 2 no finest stores, 4 no parent stores, 64 no grand-parent stores (static path), 8 no staging loads, 16 prologue only, 256 / 512 finest / parent stores without arithmetic (use with 16); skeleton shapes: 65536 parent rows in bursts of four chunks, 262144 parent rows as 16-byte stores, 1048576 finest rows as 16-byte stores
};

struct Axis {
    int i0, i1;
    float fr;
};

// split.wgsl:25-32 for centre coordinate r (0..c-1) of tile index `tile` (see bt_kernels.hip split_axis)
// (also evaluated on the host by the planner, bit for bit the same IEEE operations, to size the LDS window and the source windows exactly: hence
// its home here, the one device helper of this header)
__host__ __device__ __forceinline__ Axis split_axis(uint32_t r, uint32_t c, uint32_t tile, float scale, float lo, float hi, uint32_t dim) {
    const float tc = float(r) / float(c);
    const float s = (float(tile) + tc) / scale;
    const float u = (s - lo) / (hi - lo);
    const float q = u * float(dim) - 0.5f;
    const float fl = floorf(q);
    Axis a;
    a.fr = q - fl;
    const int i = int(fl);
    const int last = int(dim) - 1;
    const int j = i + 1;
    a.i0 = i < 0 ? 0 : (i > last ? last : i);
    a.i1 = j < 0 ? 0 : (j > last ? last : j);
    return a;
}

struct RowParam {  // one centre row of the workgroup: LDS slots of its two source rows + the y weight
    int y0, y1;
    float fy;
    uint32_t pad;
};

constexpr uint32_t kMaxChunks = 64;  // chunks one workgroup may run through (T <= 512: a whole tile)
struct MainShared {  // fixed part of the dynamic LDS block (size is a multiple of 16 bytes)
    // row tables of ALL chunks of the workgroup's run, written once in the prologue; index = (k - k_begin) * kMainRows + row
    int row_y0[kMaxChunks * kMainRows];    // first source row; bit 31: the second source row is the same one (clamped)
    float2 row_fy[kMaxChunks * kMainRows];  // y weights (fy, 1 - fy): read by every lane at one address (a broadcast), used as they arrive
    int win_ymin[kMaxChunks];              // source window of a chunk: first row ...
    uint32_t win_slots[kMaxChunks];        // ... and row count; bit 31: the chunk's rows use source rows y, y+1, ..., y+kMainRows
    RowParam apron[2 * kMaxBorder];  // [0, b): top apron rows, [b, 2b): bottom apron rows (pad = mosaic row ry)
    int xmin, xmax;
    uint32_t pad_[2];  // (the dynamic LDS block behind this struct stays 16-byte aligned)
};
static_assert(sizeof(MainShared) % 16 == 0, "LDS carve must stay 16-byte aligned");

}  // namespace

struct FusedJobDev {  // one fused launch of a compiled queue
    FusedArgs args;
    uint32_t attachment;
    uint32_t queue_job = 0;  // the preprocess job whose item list and grids args.items / args.grids point to (fused_upload)
    uint32_t lds_pad = 0;    // profiling build only (BT_FUSED_LDS_PAD at plan time): extra dynamic LDS per workgroup
    std::vector<MainItem> host_items;  // fused_main's / fused_direct's items as uploaded (tile-row order): streamed runs cut fused_main's into bands, fused_source_window reads both
    uint32_t seam_first = 0;  // fused_tail with seam workgroups: its tasks are p->tasks_dev[seam_first ...] (args.seam_count of them)
    // fused_main / fused_direct: the atlas layers of the job's finest tiles (a no-data pixel's "previous value" is read from one of them) and of
    // all its tiles (written by this job's launches); fused_begin_run decides args.prev_zero from Attachment::written before every run
    std::vector<uint32_t> finest_layers, all_layers;
};

// the fused path's per-queue state, owned by the bt_preprocessor that compiled it (bt_preprocessor::fused)
struct FusedState {
    std::vector<FusedJobDev> jobs;
    void* arrays = nullptr;  // device copy of every job's item list and grids (one allocation per queue: fused_upload)
    std::vector<uint8_t> whole_raster;  // [raster]: a launch without an item list (the hybrid plan's batched split) reads it: no window is known
};

}  // namespace bt

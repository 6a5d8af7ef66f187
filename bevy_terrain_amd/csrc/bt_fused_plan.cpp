// The fused path's planner: a compiled queue -> the fused launches of its jobs (fused_plan and its stages), their arrays on the device, and
// what a run asks of the plan afterwards (fused_begin_run, fused_source_window, fused_stream_bands, fused_launch_tiles).  Host code only: the
// kernels and the one function that names their instances, fused_launch_range, are in bt_fused.hip.
#include <algorithm>
#include <cstdlib>

#include "bt_fused_args.hpp"

namespace bt {

static FusedState& state_of(bt_preprocessor* p) {
    if (!p->fused) p->fused = new FusedState();
    return *p->fused;
}

void fused_release(bt_preprocessor* p) {
    if (!p->fused) return;
    hipFree(p->fused->arrays);
    delete p->fused;
    p->fused = nullptr;
}

// The dense grids of atlas indices of a job, one per (side, LOD): sides [0, sides) x LODs [lod_lo, lod_hi], kInvalid where no tile is queued
struct JobGrid {
    uint32_t sides = 1, lod_lo = 0, lod_hi = 0;
    std::vector<uint32_t> offsets, cells;  // offsets[side * 32 + lod]: where that grid starts in cells (x-major: x * n + y)
    JobGrid() = default;
    JobGrid(uint32_t sides_, uint32_t lo, uint32_t hi) : sides(sides_), lod_lo(lo), lod_hi(hi), offsets(6 * 32, kInvalid) {
        for (uint32_t side = 0; side < sides; side++)
            for (uint32_t lod = lod_lo; lod <= lod_hi; lod++) {
                offsets[side * 32 + lod] = uint32_t(cells.size());
                cells.resize(cells.size() + (size_t(1) << (2 * lod)), kInvalid);
            }
    }
    bool holds(const bt_tile_coordinate& c) const { return c.side < sides && c.lod >= lod_lo && c.lod <= lod_hi && c.x < (1u << c.lod) && c.y < (1u << c.lod); }
    uint32_t& cell(const bt_tile_coordinate& c) { return cells[offsets[c.side * 32 + c.lod] + (size_t(c.x) << c.lod) + c.y]; }
    uint32_t cell(const bt_tile_coordinate& c) const { return cells[offsets[c.side * 32 + c.lod] + (size_t(c.x) << c.lod) + c.y]; }
    // f(side, lod, x, y, atlas index) for every cell of the LODs [lo, end) of every side (side, LOD, x, y ascending); false from f stops the
    // walk, and for_each returns false then
    template <typename F>
    bool for_each(uint32_t lo, uint32_t end, F&& f) const {
        for (uint32_t side = 0; side < sides; side++)
            for (uint32_t lod = lo; lod < end; lod++) {
                const uint32_t* g = cells.data() + offsets[side * 32 + lod];
                for (uint32_t x = 0; x < (1u << lod); x++)
                    for (uint32_t y = 0; y < (1u << lod); y++)
                        if (!f(side, lod, x, y, g[(size_t(x) << lod) + y])) return false;
            }
        return true;
    }
    uint64_t tiles_at(uint32_t lod) const {
        uint64_t n = 0;
        for_each(lod, lod + 1, [&](uint32_t, uint32_t, uint32_t, uint32_t, uint32_t v) {
            n += v != kInvalid;
            return true;
        });
        return n;
    }
};

// One job (one preprocess_tile / preprocess_spherical call) while fused_plan plans it
struct JobPlan {
    uint32_t job = 0;
    std::vector<const Task*> splits, downs, stitches;
    uint32_t ai = 0;  // attachment
    AttachmentMeta m{};
    bool direct = false, hybrid = false;  // the plan of the finest LOD: fused_direct, the batched kernels, or (neither) fused_main
    bool spherical = false;
    uint32_t main_levels = 1;  // LODs the main / direct launch produces (the hybrid plan: 1, the batched kernels')
    JobGrid grid;
    bool shard = false;  // sharded: this rank's column strips (plan_shards)
    uint32_t strip_shift = 0, strips = 0, units_per_rank = 0;
    std::vector<MainItem> items;  // this rank's finest tiles in launch order
    FusedArgs args{};  // what the job's fused launches share
    uint64_t source_bytes = 0;
    std::vector<uint32_t> finest_layers, all_layers;  // (Attachment::written bookkeeping: fused_begin_run)

    uint32_t main_lo() const { return grid.lod_hi - (main_levels - 1); }  // LODs main_lo .. lod_hi come out of the main launch
    // the first tail launch also fills the top / bottom apron rows of the LODs fused_main produced (no stitch launch for them)
    // (after fused_direct, which writes centres only, the tail's extra workgroups do all four sides: no stitch launch)
    bool rows_in_tail() const { return !shard && main_lo() > grid.lod_lo && main_levels > 1 && (direct || m.border_size % 2u == 0); }
    uint64_t tile_bytes() const { return uint64_t(m.texture_size) * m.texture_size * m.pixel_size; }
    uint64_t apron_bytes() const { return 2 * (2 * uint64_t(m.border_size) * (m.texture_size + m.center_size)) * m.pixel_size; }  // a whole stitch: read + written
    FusedJobDev fused_job() const {
        FusedJobDev d{args, ai};
        d.queue_job = job;
        return d;
    }
};

// What the stages append to: the queue's task records and launches, and the fused jobs the launches point to (Launch::aux0)
struct PlanOut {
    std::vector<TaskDev>& tasks;
    std::vector<Launch>& plan;
    FusedState& state;
};

static Launch job_launch(const JobPlan& j, LaunchKind kind, uint32_t variant) {
    Launch l{};
    l.kind = kind;
    l.variant = variant;
    l.attachment = j.ai;
    return l;
}

// A job qualifies for the fused path when
//  - the attachment is R16 with T <= 512, even b, c % 4 == 0, c >= 2b;
//  - at every LOD but the finest, each queued tile has all four children queued (full quadtree below it).
// Otherwise the whole queue runs on the generic kernels.  collect_job, fill_grid and qualifies return false where it does not.
static bool collect_job(const bt_preprocessor* p, const bt_atlas* a, uint32_t job, JobPlan& j) {
    j.job = job;
    for (const Task& t : p->queue) {
        if (t.job != job) continue;
        if (t.type == kSplit) j.splits.push_back(&t);
        else if (t.type == kDownsample) j.downs.push_back(&t);
        else if (t.type == kStitch) j.stitches.push_back(&t);
    }
    if (j.splits.empty()) return false;
    j.ai = j.splits[0]->attachment_index;
    const AttachmentMeta& m = j.m = a->attachments[j.ai].meta;
    // fused_main: R16, T <= 512, even b <= 8.  Otherwise (Rgba8, large tiles, odd borders) the HYBRID plan: the batched
    // split + stitch kernels produce the finest LOD, fused_tail (format-generic) everything below it, three LODs per
    // launch, aprons pushed — instead of one downsample launch per LOD and a stitch over every tile.
    const bool tail_ok = (m.format == BT_FORMAT_R16 || m.format == BT_FORMAT_RGBA8) && (m.center_size & 3u) == 0 &&
                         m.center_size >= 2 * m.border_size && m.border_size != 0 && (m.format != BT_FORMAT_R16 || (m.border_size & 1u) == 0);
    const bool main_ok = tail_ok && m.format == BT_FORMAT_R16 && m.texture_size <= 512 && m.border_size <= 8;
    if (!tail_ok) return false;
    // Rgba8: fused_direct (no LDS staging) produces the finest LOD with its aprons and the two parent LODs
    j.direct = !main_ok && m.format == BT_FORMAT_RGBA8;
    j.hybrid = !main_ok && !j.direct;
    // (layer x tile texels is formed in 64 bits everywhere: an attachment of 2^32 texels or more — 16384 tiles of 512^2 — takes the fused plans
    // like any other; rounds 2 - 6 sent such atlases to the batched kernels, found with a GEBCO-sized job at the end of round 6)
    const uint32_t lod_hi = j.splits[0]->coord.lod;
    uint32_t lod_lo = lod_hi;
    for (const Task* t : j.downs) lod_lo = std::min(lod_lo, t->coord.lod);
    if (lod_hi > 13) return false;  // dense per-LOD grids (4^lod entries) and 32-bit grid offsets
    j.spherical = a->config.spherical != 0;
    j.grid = JobGrid(j.spherical ? 6u : 1u, lod_lo, lod_hi);
    // main launch: finest LOD + up to two more
    j.main_levels = j.hybrid ? 1u : std::min(3u, lod_hi - lod_lo + 1);
    return true;
}

static bool fill_grid(JobPlan& j) {
    JobGrid& g = j.grid;
    for (const Task* t : j.splits) {
        if (!g.holds(t->coord) || t->coord.lod != g.lod_hi) return false;
        g.cell(t->coord) = t->atlas_index;
    }
    for (const Task* t : j.downs) {
        if (!g.holds(t->coord)) return false;
        g.cell(t->coord) = t->atlas_index;
    }
    return true;
}

static bool qualifies(const JobPlan& j) {
    const JobGrid& g = j.grid;
    // completeness: every downsample tile has its four children in the grids
    for (const Task* t : j.downs) {
        bt_tile_coordinate ch[4];
        tile_children(t->coord, ch);
        for (int k = 0; k < 4; k++)
            if (g.cell(ch[k]) == kInvalid) return false;
    }
    // every tile that is stitched must be in the grids and vice versa (same tile set)
    size_t present = 0;
    for (uint32_t v : g.cells) present += v != kInvalid;
    if (present != j.stitches.size()) return false;
    // The fused kernels take a tile's apron from the job's own grid; the queue recorded the neighbours the ATLAS holds
    // (stitch_and_save_layer -> get_tile).  They differ when tiles of an earlier job or dataset border this one: then
    // only the generic path stitches across that seam, so the job does not qualify.
    for (const Task* t : j.stitches) {
        const bt_tile_coordinate& c = t->coord;
        if (!g.holds(c) || g.cell(c) != t->atlas_index) return false;
        bt_tile_coordinate nb[8];
        tile_neighbours(c, false, nb);  // same-face neighbours (cube seams are re-stitched by the generic kernel)
        for (int i = 0; i < 8; i++) {
            const bool same_face = !is_invalid(nb[i]);
            const uint32_t in_grid = same_face ? g.cell(nb[i]) : kInvalid;
            const bool recorded_same_face = t->rel[i].atlas_index != BT_INVALID_ATLAS_INDEX && t->rel[i].coordinate.side == c.side && same_face;
            if (same_face && in_grid != (recorded_same_face ? t->rel[i].atlas_index : kInvalid)) return false;
        }
    }
    // all split tasks share the dataset rectangle
    const Task* s0 = j.splits[0];
    for (const Task* t : j.splits)
        if (t->tl[0] != s0->tl[0] || t->tl[1] != s0->tl[1] || t->br[0] != s0->br[0] || t->br[1] != s0->br[1]) return false;
    return true;
}

// ---- sharding (multi-GPU).  Unit = one column strip of one side at the granularity of the coarsest LOD the main
// kernel produces (a strip = 2^(levels-1) finest columns = one column of that LOD), units numbered side-major;
// rank r owns the units [r * U / world, (r + 1) * U / world).  A unit's tiles of a LOD are contiguous atlas layers
// (x-major allocation order), so the exchange is a list of contiguous layer runs, each with its owning rank.
static void plan_shards(bt_preprocessor* p, JobPlan& j) {
    const JobGrid& g = j.grid;
    const uint32_t world = p->shard_world, levels = std::min(3u, g.lod_hi - g.lod_lo + 1);
    j.strip_shift = levels - 1;
    j.strips = 1u << (g.lod_hi - j.strip_shift);
    const uint32_t units = g.sides * j.strips;
    // (fused_direct shards like fused_main: finest tiles complete from the source, parent centres inside a strip, everything else after the exchange)
    j.shard = world > 1 && units % world == 0 && !j.hybrid;
    if (!j.shard) return;
    j.units_per_rank = units / world;
    auto base_of = [&](uint32_t side, uint32_t lod) { return g.cells[g.offsets[side * 32 + lod]]; };
    j.shard = g.for_each(g.lod_hi + 1 - levels, g.lod_hi + 1, [&](uint32_t side, uint32_t lod, uint32_t x, uint32_t y, uint32_t v) {
        const uint32_t base = base_of(side, lod);
        return base != kInvalid && v == base + ((x << lod) + y);  // the fresh x-major layout
    });
    if (!j.shard) return;
    for (uint32_t side = 0; side < g.sides; side++)
        for (uint32_t k = 0; k < levels; k++) {
            const uint32_t lod = g.lod_hi - k, n = 1u << lod, base = base_of(side, lod), cols_per_strip = n / j.strips;
            // maximal runs of strips with one owner
            for (uint32_t strip = 0; strip < j.strips;) {
                const uint32_t owner = (side * j.strips + strip) / j.units_per_rank;
                uint32_t end = strip + 1;
                while (end < j.strips && (side * j.strips + end) / j.units_per_rank == owner) end++;
                p->shard_pieces.push_back({j.ai, side, lod, base + strip * cols_per_strip * n, (end - strip) * cols_per_strip * n, owner});
                strip = end;
            }
            // the regular case (one side, every rank an equal run): also expressible as ONE in-place all-gather
            if (g.sides == 1) p->shard_ranges.push_back({j.ai, side, lod, base, n / world * n});
        }
}

static void order_items(const bt_preprocessor* p, JobPlan& j) {
    for (const Task* t : j.splits) {
        if (j.shard && (t->coord.side * j.strips + (t->coord.x >> j.strip_shift)) / j.units_per_rank != p->shard_rank) continue;
        j.items.push_back({t->coord.side, t->coord.x, t->coord.y, t->atlas_index, uint32_t(t->raster)});
    }
    // Workgroup order = tile rows (y outer, x inner) instead of the queue's x-major order: an XCD then streams whole
    // source rows (its 128 concurrent workgroups cover 4 tile rows x all columns), and x neighbours run on the same XCD
    // at the same time, so the apron bytes one pushes into the other's parent rows merge in one L2.  16k job: 333 -> 285 us.
    std::stable_sort(j.items.begin(), j.items.end(), [](const MainItem& a, const MainItem& b2) {
        return a.side != b2.side ? a.side < b2.side : (a.y != b2.y ? a.y < b2.y : a.x < b2.x);
    });
}

// the closed form of grid_lookup: does every entry follow it?  (*first: FusedArgs::reg_first)
static bool regular_layout(const JobGrid& g, uint32_t* first) {
    const uint32_t hi4 = 4u << (2u * g.lod_hi), per_side = (hi4 - (1u << (2u * g.lod_lo))) / 3u, f = g.cells.empty() ? 0u : g.cells[g.offsets[g.lod_hi]];
    *first = f;
    return f != kInvalid && g.for_each(g.lod_lo, g.lod_hi + 1, [&](uint32_t side, uint32_t lod, uint32_t x, uint32_t y, uint32_t v) {
        return v == f + side * per_side + (hi4 - (4u << (2u * lod))) / 3u + ((x << lod) + y);
    });
}

// what the job's fused launches share, the source bytes it reads and the atlas layers it writes
static void describe_job(const bt_preprocessor* p, const bt_atlas* a, JobPlan& j) {
    FusedArgs& args = j.args;
    args.m = j.m;
#ifdef BT_DEBUG_HOOKS
    if (const char* e = getenv("BT_FUSED_ABLATE")) args.ablate = uint32_t(strtoul(e, nullptr, 0));
#endif
    args.atlas = (uint16_t*)a->attachments[j.ai].level0;
    args.rasters = p->rasters_dev;  // (re)allocated by bt_preprocessor_run before the first launch
    args.tlx = j.splits[0]->tl[0];
    args.tly = j.splits[0]->tl[1];
    args.brx = j.splits[0]->br[0];
    args.bry = j.splits[0]->br[1];
    args.sides = j.grid.sides;
    args.grid_lod_lo = j.grid.lod_lo;
    args.grid_lod_hi = j.grid.lod_hi;
    args.grid_sides = j.grid.sides;
    args.regular = regular_layout(j.grid, &args.reg_first) ? 1u : 0u;
    std::vector<bool> seen(p->rasters.size(), false);
    for (const Task* t : j.splits)
        if (!seen[t->raster]) {
            seen[t->raster] = true;
            j.source_bytes += uint64_t(p->rasters[t->raster].dev.width) * p->rasters[t->raster].dev.height * j.m.pixel_size;
        }
    j.grid.for_each(j.grid.lod_lo, j.grid.lod_hi + 1, [&](uint32_t, uint32_t lod, uint32_t, uint32_t, uint32_t v) {
        if (v != kInvalid) {
            j.all_layers.push_back(v);
            if (lod == j.grid.lod_hi) j.finest_layers.push_back(v);
        }
        return true;
    });
}

// the source once + every tile of the LODs the main / direct launch produces
static uint64_t main_bytes(const JobPlan& j) {
    uint64_t bytes = j.source_bytes;
    for (uint32_t k = 0; k < j.main_levels; k++) bytes += j.grid.tiles_at(j.grid.lod_hi - k) * j.tile_bytes();
    return bytes;
}

static FusedJobDev main_job(const JobPlan& j) {  // a fused_main / fused_direct launch over the job's items
    FusedJobDev job = j.fused_job();
    job.args.lod = j.grid.lod_hi;
    job.args.levels = j.main_levels;
    job.args.item_count = uint32_t(j.items.size());
    job.host_items = j.items;
    job.finest_layers = j.finest_layers;
    job.all_layers = j.all_layers;
    return job;
}

static void plan_hybrid(const JobPlan& j, PlanOut& out) {
    Launch ls = job_launch(j, kLaunchSplit, BT_VARIANT_HYBRID);
    ls.first_task = uint32_t(out.tasks.size());
    for (const Task* t : j.splits) {
        out.tasks.push_back(to_device_task(*t));
        if (t->raster >= 0 && size_t(t->raster) < out.state.whole_raster.size()) out.state.whole_raster[size_t(t->raster)] = 1;  // (every rank splits every tile)
    }
    ls.task_count = uint32_t(j.splits.size());
    ls.algorithmic_bytes = j.source_bytes + uint64_t(j.splits.size()) * j.tile_bytes();
    out.plan.push_back(ls);
    Launch lt = job_launch(j, kLaunchStitch, BT_VARIANT_HYBRID);
    lt.first_task = uint32_t(out.tasks.size());
    for (const Task* t : j.stitches)
        if (t->coord.lod == j.grid.lod_hi) out.tasks.push_back(to_device_task(*t));
    lt.task_count = uint32_t(out.tasks.size()) - lt.first_task;
    lt.algorithmic_bytes = uint64_t(lt.task_count) * j.apron_bytes();
    if (lt.task_count) out.plan.push_back(lt);
}

static void plan_direct(const bt_preprocessor* p, const JobPlan& j, PlanOut& out) {
    FusedJobDev job = main_job(j);
    bool rep = false, skips = false;
    {   // source rows per tile row: below 1 output rows repeat source-row pairs
        const double mosaic = double(j.m.center_size) * double(1u << j.grid.lod_hi);
        for (const Task* t : j.splits) {
            const RasterDev& r = p->rasters[t->raster].dev;
            const double ratio = double(r.height) / (double(j.args.bry - j.args.tly) * mosaic);
            if (ratio < 0.9999) rep = true;
            if (ratio > 1.02) skips = true;  // (the BASELINE shapes, 1.008, pass over a row in one block of 32: they stay on the plain kernel)
        }
    }
    {   // row blocks per workgroup: as many as keep at least one resident generation (1024 workgroups) busy
        const uint64_t blocks = uint64_t(j.items.size()) * ((j.m.center_size + kDirectRows - 1) / kDirectRows);
        job.args.groups = uint32_t(std::min<uint64_t>(kDirectMaxBlocks, std::max<uint64_t>(1, (blocks + 1023) / 1024)));
#ifdef BT_DEBUG_HOOKS
        if (const char* e = getenv("BT_FUSED_PARTS")) job.args.groups = std::max(1u, std::min(kDirectMaxBlocks, uint32_t(atoi(e))));
#endif
    }
    Launch ld = job_launch(j, kLaunchFusedDirect, rep ? BT_VARIANT_DIRECT_REP : skips ? BT_VARIANT_DIRECT_SKIPS : BT_VARIANT_DIRECT);
    ld.task_count = uint32_t(j.items.size());
    ld.aux0 = uint32_t(out.state.jobs.size());
    ld.algorithmic_bytes = main_bytes(j);
    out.state.jobs.push_back(job);
    out.plan.push_back(ld);
}

// fused_main's LDS window (FusedArgs::lds_pitch, lds_rows, apron_global, single_buffer) and the instance that runs it: its BT_VARIANT_* bit
static uint32_t size_main_window(const bt_preprocessor* p, const JobPlan& j, FusedArgs& A) {
    const AttachmentMeta& m = j.m;
    const uint32_t lod_hi = j.grid.lod_hi;
    // LDS window of a workgroup: T consecutive mosaic columns x (kMainRows + 2b) mosaic rows of the source
    double ratio_x = 0.0, ratio_y = 0.0;
    uint64_t max_pitch = 0;
    // every raster of the job 16-byte aligned in base and pitch, as LDS-DMA needs: add_raster (bt_preprocess.cpp) gives every R16 raster such a
    // base and pitch, so this only checks that invariant; a job that breaks it takes the run-time-pitch register staging
    bool aligned = true;
    const double mosaic = double(1u << lod_hi) * double(m.center_size);
    for (const Task* t : j.splits) {
        const RasterDev& r = p->rasters[t->raster].dev;
        max_pitch = std::max<uint64_t>(max_pitch, r.pitch);
        ratio_x = std::max(ratio_x, double(r.width) / (double(A.brx - A.tlx) * mosaic));
        ratio_y = std::max(ratio_y, double(r.height) / (double(A.bry - A.tly) * mosaic));
        if (((reinterpret_cast<uintptr_t>(r.data) | r.pitch) & 15u) != 0) aligned = false;
    }
    const uint32_t rows = std::min(kMainRows, m.center_size) + 2 * m.border_size;
    const uint64_t cols_needed = uint64_t(double(m.texture_size - 1) * ratio_x) + 4 + 7;
    uint64_t rows_needed = uint64_t(double(rows - 1) * ratio_y) + 4;  // contiguous source-row range (safe bound)
    uint64_t exact_core = rows_needed;  // ... of the centre rows alone (without the first / last chunk's apron rows)
    {   // exact: replay the kernel's own window computation for every tile row and chunk (same f32 operations)
        const uint32_t c = m.center_size, b = m.border_size, chunks = (c + kMainRows - 1) / kMainRows;
        const float scale = float(1u << lod_hi);
        uint64_t exact = 1;
        exact_core = 1;
        std::vector<std::pair<uint32_t, int>> seen;  // (tile row, raster)
        for (const Task* t : j.splits) {
            const std::pair<uint32_t, int> key(t->coord.y, t->raster);
            if (std::find(seen.begin(), seen.end(), key) != seen.end()) continue;
            seen.push_back(key);
            const uint32_t H = p->rasters[t->raster].dev.height, n = 1u << lod_hi, ty = t->coord.y;
            auto axis = [&](uint32_t tile, uint32_t r) { return split_axis(r, c, tile, scale, A.tly, A.bry, H); };
            for (uint32_t k = 0; k < chunks; k++) {
                const uint32_t r0 = k * kMainRows, r1 = std::min(c, r0 + kMainRows) - 1;
                int lo = axis(ty, r0).i0, hi = axis(ty, r1).i1;
                exact_core = std::max<uint64_t>(exact_core, uint64_t(hi - lo + 1));
                if (k == 0) lo = std::min(lo, ty > 0 ? axis(ty - 1, c - b).i0 : axis(ty, 0).i0);
                if (k == chunks - 1) hi = std::max(hi, ty + 1 < n ? axis(ty + 1, b - 1).i1 : axis(ty, c - 1).i1);
                exact = std::max<uint64_t>(exact, uint64_t(hi - lo + 1));
            }
        }
        rows_needed = std::min(rows_needed, exact);
    }
    const uint64_t pitch = (cols_needed + 7) / 8 * 8;
    const uint64_t budget = 65536 - sizeof(MainShared);
    A.lds_pitch = uint32_t(std::min<uint64_t>(pitch, 1u << 20));
    // the whole window must fit (the bounds above are conservative); otherwise lds_rows = 0 selects the
    // kernel variant that reads the source directly
    // the staging loop holds one batch of 8 x 16-byte loads per thread: the window must fit that too
    // and its byte offsets from the first row are kept in 32 bits
    // (the register staging holds one batch of 4 x 16-byte loads per thread: a window of more pieces than that — ratios from ~1.2 up at
    // T = 512 — is staged by LDS-DMA alone, when every raster of the job is 16-byte aligned; rounds 2 - 6 sent such jobs to the unstaged kernel)
    // Four workgroups per CU need <= 40 KB each (160 KB of LDS).  When the window with the apron rows is past that and the centre rows alone are
    // not (ratios ~1.25 - 1.35 at T = 512; at 1.41 the same step takes the job from two workgroups to three), the apron rows — 2b of a tile's T —
    // read global memory and the window shrinks: ratio 1.3, 553 -> 3xx us (round 6, profiles/r06_gebco_size.txt)
    const uint64_t kQuarter = (160u << 10) / 4, kThird = (160u << 10) / 3, fixed = sizeof(MainShared);
    const uint64_t core_rows = std::min(rows_needed, exact_core);
    // (only the run-time-pitch DMA variant knows the mode: aligned rasters, T = 512 or a window past the register batch, not the 528 pitch)
    const bool dma_variant = aligned && pitch <= 4096 && pitch != 528 && (m.texture_size == 512 || core_rows * (pitch / 8) > 256 * 4);
    {
        const uint64_t with_aprons = fixed + 2 * rows_needed * pitch * 2, core = fixed + 2 * core_rows * pitch * 2;
        auto groups = [&](uint64_t bytes) { return bytes <= kQuarter ? 4 : bytes <= kThird ? 3 : bytes <= (80u << 10) ? 2 : 1; };
        if (dma_variant && groups(core) > groups(with_aprons)) {
            A.apron_global = 1;
            rows_needed = core_rows;
        }
    }
    uint64_t buffers = 2;
    // ... and where even the centre rows alone, twice, leave room for three workgroups or fewer, ONE buffer of them may leave room for four (FusedArgs::single_buffer)
    if (dma_variant && fixed + 2 * rows_needed * pitch * 2 > kQuarter && fixed + core_rows * pitch * 2 <= kQuarter) {
        A.single_buffer = 1;
        A.apron_global = 1;
        rows_needed = core_rows;
        buffers = 1;
    }
    const bool fits_lds = buffers * rows_needed * pitch * 2 <= budget && (rows_needed + 1) * max_pitch < (1ull << 31);
    const bool fits_batch = rows_needed * (pitch / 8) <= 256 * 4;
    // (and by choice at T = 512, where it measured 2 % faster than the register staging on a 86400 x 43200 job; at T = 256 — half-empty
    // 1 KB pieces — the register staging is 6 % faster and stays)
    const bool dma_only = fits_lds && aligned && pitch <= 4096 && (!fits_batch || m.texture_size == 512);
    A.lds_rows = fits_lds && (fits_batch || dma_only) ? uint32_t(rows_needed) : 0u;
    if ((A.apron_global || A.single_buffer) && A.lds_rows && !dma_only) {  // (cannot happen by the conditions above; a window without apron rows in a variant that stages them would overrun)
        A.apron_global = 0;
        A.single_buffer = 0;
        A.lds_rows = 0;
    }
    if (!A.lds_rows) return BT_VARIANT_MAIN_UNSTAGED;
    if (aligned && m.texture_size == 512 && A.lds_pitch == 528) return BT_VARIANT_MAIN_DMA_528;
    // a window the register staging cannot batch (a source-to-tile ratio away from 1), or T = 512 at any other pitch: LDS-DMA with a run-time pitch (round 6)
    if (dma_only) return A.single_buffer ? BT_VARIANT_MAIN_SINGLE_BUFFER : A.apron_global ? BT_VARIANT_MAIN_APRON_GLOBAL : BT_VARIANT_MAIN_DMA_PITCH;
    return BT_VARIANT_MAIN_REG_PITCH;
}

static void plan_main(const bt_preprocessor* p, const JobPlan& j, PlanOut& out) {
    FusedJobDev job = main_job(j);
#ifdef BT_DEBUG_HOOKS
    if (const char* e = getenv("BT_FUSED_LDS_PAD")) job.lds_pad = uint32_t(atoi(e));
#endif
    {
        const uint32_t chunks = (j.m.center_size + kMainRows - 1) / kMainRows;
        // 4 workgroups of 4 waves per CU (128 VGPRs each) = 1024 resident: pick the number of parts per tile so
        // that the grid is a whole number of 1024-workgroup rounds where possible
        uint32_t parts = 1;
#ifdef BT_DEBUG_HOOKS
        if (const char* e = getenv("BT_FUSED_PARTS")) parts = uint32_t(atoi(e));
        else
#endif
        {
            while (parts < chunks && uint64_t(j.items.size()) * parts < 1024) parts++;
            for (uint32_t cand = parts; cand <= std::min(chunks, parts + 8); cand++)
                if ((uint64_t(j.items.size()) * cand) % 1024 == 0) { parts = cand; break; }
        }
        parts = std::max(parts, (chunks + kMaxChunks - 1) / kMaxChunks);  // row tables of a workgroup hold kMaxChunks chunks
        job.args.groups = std::max(1u, std::min(parts, chunks));
    }
    Launch lm = job_launch(j, kLaunchFusedMain, size_main_window(p, j, job.args));
    job.args.rotate_priority = 1;
    lm.kernels = lm.variant == BT_VARIANT_MAIN_UNSTAGED ? 2u : 1u;  // (without the LDS window: fused_corner + fused_main in one entry)
    lm.task_count = uint32_t(j.items.size());
    lm.aux0 = uint32_t(out.state.jobs.size());
    lm.algorithmic_bytes = main_bytes(j);
    out.state.jobs.push_back(job);
    out.plan.push_back(lm);
}

static void plan_apron_stitch(const JobPlan& j, PlanOut& out) {
    if (j.main_levels <= 1 || j.rows_in_tail()) return;
    // fused_main writes the centres and the left / right apron columns of the parent / grand-parent tiles; their
    // top / bottom apron rows (whole 1 KB rows) come from the batched stitch kernel — sharded: everything, after
    // the all-gather, from the then complete centres
    Launch ls = job_launch(j, kLaunchStitch, BT_VARIANT_STITCH_LAUNCH);
    ls.first_task = uint32_t(out.tasks.size());
    for (const Task* t : j.stitches)
        if (t->coord.lod != j.grid.lod_hi && t->coord.lod + j.main_levels > j.grid.lod_hi) out.tasks.push_back(to_device_task(*t));
    ls.task_count = uint32_t(out.tasks.size()) - ls.first_task;
    ls.algorithmic_bytes = uint64_t(ls.task_count) * j.apron_bytes();
    ls.phase = j.shard ? 2u : 0u;
    // fused_main also writes the left / right apron columns of these tiles (from registers); sharded runs lose
    // the ones that crossed a strip boundary in the all-gather and re-stitch everything
    ls.aux0 = (j.shard || j.direct) ? 0u : 1u;  // (fused_direct writes centres only: all four sides)
    if (!j.shard && !j.direct) ls.algorithmic_bytes = uint64_t(ls.task_count) * 2 * (2 * j.m.border_size * uint64_t(j.m.texture_size)) * j.m.pixel_size;
    if (ls.task_count) out.plan.push_back(ls);
}

struct TailPlan {
    int job = -1, plan = -1;  // the first tail launch: its fused job and plan entry (-1: none)
    uint32_t launches = 0;
};

// tail launches: three LODs at a time below the last fused one
static TailPlan plan_tails(const JobPlan& j, PlanOut& out) {
    const uint64_t Tt = j.m.texture_size, cc = j.m.center_size, bpp = j.m.pixel_size;
    TailPlan tails;
    for (uint32_t in_lod = j.main_lo(); in_lod > j.grid.lod_lo;) {
        tails.launches++;
        const uint32_t levels = std::min(3u, in_lod - j.grid.lod_lo);
        FusedJobDev tail = j.fused_job();
        tail.all_layers = j.all_layers;
        tail.args.lod = in_lod;
        tail.args.levels = levels;
        tail.args.apron_lods = (j.rows_in_tail() && in_lod == j.main_lo()) ? j.main_levels - 1 : 0u;
        tail.args.apron_cols = j.direct ? 1u : 0u;
        Launch lt = job_launch(j, kLaunchFusedTail, j.args.regular ? BT_VARIANT_TAIL_REGULAR : BT_VARIANT_TAIL_IRREGULAR);
        lt.aux0 = uint32_t(out.state.jobs.size());
        lt.phase = j.shard ? 2u : 0u;
        lt.algorithmic_bytes = j.grid.tiles_at(in_lod) * cc * cc * bpp;
        for (uint32_t k = 0; k < tail.args.apron_lods; k++) lt.algorithmic_bytes += j.grid.tiles_at(in_lod + k) * 2 * (2 * j.m.border_size * (Tt + (j.direct ? cc : 0))) * bpp;
        for (uint32_t k = 1; k <= levels; k++) {
            lt.algorithmic_bytes += j.grid.tiles_at(in_lod - k) * j.tile_bytes();
            lt.task_count += uint32_t(j.grid.tiles_at(in_lod - k));
        }
        if (tails.job < 0) {
            tails.job = int(out.state.jobs.size());
            tails.plan = int(out.plan.size());
        }
        out.state.jobs.push_back(tail);
        out.plan.push_back(lt);
        in_lod -= levels;
    }
    return tails;
}

// Every region beyond exactly one face edge of the face-edge stitch tasks of the LODs [lo, end) has its neighbour on the other face (pulled:
// of the same LOD, with 16-bit coordinates), and every face-edge tile of those LODs that the grids hold has a stitch task (seam_skip / seam_pull
// make the tail leave the cross-face regions of every such grid tile alone: one without a task would keep stale apron texels there)
static bool seams_covered(const JobPlan& j, uint32_t lo, uint32_t end, bool pulled) {
    std::unordered_set<uint32_t> stitched;
    for (const Task* t : j.stitches) {
        if (!on_face_edge(t->coord) || t->coord.lod < lo || t->coord.lod >= end) continue;
        stitched.insert(t->atlas_index);
        const int n = int(1u << t->coord.lod);
        for (int i = 0; i < 8; i++) {
            const int nx = int(t->coord.x) + kNeighbourOffsets[i][0], ny = int(t->coord.y) + kNeighbourOffsets[i][1];
            const bool out_x = nx < 0 || nx >= n, out_y = ny < 0 || ny >= n;
            const bt_atlas_tile& r = t->rel[i];
            const bool across = r.atlas_index != BT_INVALID_ATLAS_INDEX && r.coordinate.side != t->coord.side;
            if (out_x != out_y && !(across && (!pulled || (r.coordinate.lod == t->coord.lod && r.coordinate.x < 65536u && r.coordinate.y < 65536u))))
                return false;
        }
    }
    return j.grid.for_each(lo, end, [&](uint32_t, uint32_t lod, uint32_t x, uint32_t y, uint32_t v) {
        return !(on_face_edge({0, lod, x, y}) && v != kInvalid && !stitched.count(v));
    });
}

// cube: aprons that cross a face edge (stitch.wgsl:12-51, 79-118), one task — one workgroup — per region: only the apron regions whose
// neighbour lives on another face (the fused kernels wrote the rest).  The regions of the LODs fused_main produced read centres that are
// complete when the tail launch starts: they ride in that launch as extra workgroups (round 5: the 16k-texel-wide job's seam launch was
// 33 of 500 us), and the tail's own apron-row workgroups leave those regions alone (FusedArgs::seam_skip).  What the tail itself
// produces (the few tiles of the top LODs) is stitched by the generic kernel behind it, as before.
static void plan_cube_seams(const JobPlan& j, const TailPlan& tails, PlanOut& out) {
    const AttachmentMeta& m = j.m;
    const uint32_t main_lo = j.main_lo(), lod_hi = j.grid.lod_hi;
    // in the tail launch: R16 main plan, unsharded, a tail launch with apron-row workgroups exists, and EVERY region beyond exactly one
    // face edge of the tiles whose apron rows the tail writes has its neighbour (then "skip" and "a seam workgroup writes it" coincide)
    const bool in_tail = !j.shard && !j.hybrid && tails.job >= 0 && out.state.jobs[size_t(tails.job)].args.apron_lods != 0 &&  // (round 6: Rgba8 after fused_direct too)
                         seams_covered(j, main_lo, lod_hi, false);
    // Round 6: the cross-face regions of the LODs the tail ITSELF produces ride in it as well, PULLED from the tail's input (FusedArgs::seam_pull) —
    // when ONE tail launch produces every lower LOD (its input then lies at most three LODs above any of them), every region beyond exactly
    // one face edge of those tiles has its cross-face neighbour, and every face-edge grid tile of those LODs has a stitch task (the tail's
    // pushes leave those regions alone).  No stitch launch follows the tail then: the cube job is two launches.
    const bool pull = in_tail && tails.launches == 1 && seams_covered(j, j.grid.lod_lo, main_lo, true);
    uint64_t tail_pixels = 0, late_pixels = 0;
    const uint32_t tail_first = uint32_t(out.tasks.size());
    for (int pass = 0; pass < 2; pass++) {  // the tail launch's regions first, then the later launch's
        if (pass == 1 && in_tail) {
            FusedJobDev& tj = out.state.jobs[size_t(tails.job)];
            tj.seam_first = tail_first;
            tj.args.seam_count = uint32_t(out.tasks.size()) - tail_first;
            tj.args.seam_skip = 1;
            tj.args.seam_pull = pull ? 1u : 0u;
            out.plan[size_t(tails.plan)].algorithmic_bytes += 2 * tail_pixels * m.pixel_size;
        }
        const uint32_t first = uint32_t(out.tasks.size());
        // (pass 0 in two sweeps: the pulled regions FIRST — they are the launch's longest workgroups and the seam list's head is dispatched first)
        for (int sweep = (pass == 0 && pull) ? 0 : 1; sweep < 2; sweep++)
            for (const Task* t : j.stitches) {
                if (!on_face_edge(t->coord)) continue;
                if (j.hybrid && t->coord.lod == lod_hi) continue;  // stitched completely by the batched kernel above
                const bool pulled = pull && t->coord.lod < main_lo;
                const bool rides = in_tail && (t->coord.lod >= main_lo || pulled);
                if (rides != (pass == 0)) continue;
                if (pass == 0 && pull && pulled != (sweep == 0)) continue;
                const TaskDev d = to_device_task(*t);
                for (int i = 0; i < 8; i++)
                    if (d.rel_index[i] != BT_INVALID_ATLAS_INDEX && d.rel_side[i] != d.side) {
                        TaskDev e = d;
                        e.regions = 1u << i;
                        uint32_t parts = 1;
                        if (pulled) {  // evaluated from the tail's input LOD (main_lo) on the neighbour face: how many LODs up, and where the neighbour tile lies
                            // an edge region is shared out so that a thread evaluates one pixel pair (256 per workgroup); a corner region is one workgroup
                            const uint32_t pixels = m.border_size * (i < 4 ? m.center_size : m.border_size);
                            const uint32_t pairs = (m.format != BT_FORMAT_R16 || ((m.border_size | m.texture_size) & 1u)) ? pixels : pixels / 2u;  // what one thread stores
                            parts = std::max(1u, std::min(255u, (pairs + 255u) / 256u));
                            e.rel_index[i] = (t->rel[i].coordinate.x << 16) | t->rel[i].coordinate.y;
                        }
                        for (uint32_t part = 0; part < parts; part++) {
                            if (pulled) e.raster = (main_lo - t->coord.lod) | (part << 8) | (parts << 16);
                            out.tasks.push_back(e);
                        }
                        (pass == 0 ? tail_pixels : late_pixels) += uint64_t(m.border_size) * (i < 4 ? m.center_size : m.border_size);
                    }
            }
        if (pass == 0) continue;
        Launch ls = job_launch(j, kLaunchStitch, BT_VARIANT_STITCH_LAUNCH);
        ls.aux0 = 2u;  // one region per task
        ls.first_task = first;
        ls.task_count = uint32_t(out.tasks.size()) - first;
        ls.algorithmic_bytes = 2 * late_pixels * m.pixel_size;
        ls.phase = j.shard ? 2u : 0u;
        if (ls.task_count) out.plan.push_back(ls);
    }
}

// Every job's item list and grids in ONE device allocation, each array 256-byte aligned (as an allocation of its own is): at[2k] is where
// job k's items start, at[2k + 1] its grids.  The fused jobs' args.items / args.grids point into it
static bt_status fused_upload(FusedState& state, const std::vector<std::vector<MainItem>>& items, const std::vector<std::vector<uint32_t>>& grids) {
    std::vector<size_t> at(2 * items.size());
    size_t bytes = 0;
    for (size_t k = 0; k < at.size(); k++) {
        at[k] = (bytes + 255) & ~size_t(255);
        bytes = at[k] + (k % 2 ? grids[k / 2].size() * sizeof(uint32_t) : items[k / 2].size() * sizeof(MainItem));
    }
    BT_HIP(hipMalloc(&state.arrays, bytes ? bytes : 1));
    uint8_t* base = (uint8_t*)state.arrays;
    for (size_t k = 0; k < items.size(); k++) {
        if (!items[k].empty()) BT_HIP(hipMemcpy(base + at[2 * k], items[k].data(), items[k].size() * sizeof(MainItem), hipMemcpyHostToDevice));
        if (!grids[k].empty()) BT_HIP(hipMemcpy(base + at[2 * k + 1], grids[k].data(), grids[k].size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    for (FusedJobDev& job : state.jobs) {
        job.args.items = (const MainItem*)(base + at[2 * job.queue_job]);
        job.args.grids = (const uint32_t*)(base + at[2 * job.queue_job + 1]);
    }
    return BT_OK;
}

bool fused_plan(bt_preprocessor* p, bt_atlas* a, std::vector<TaskDev>& tasks, std::vector<Launch>& plan) {
    FusedState& state = state_of(p);
    hipFree(state.arrays);
    state.arrays = nullptr;
    state.jobs.clear();
    state.whole_raster.assign(p->rasters.size(), 0);
    if (p->queue.empty()) return false;

    PlanOut out{tasks, plan, state};
    std::vector<std::vector<MainItem>> items;
    std::vector<std::vector<uint32_t>> grids;
    for (uint32_t job = 0; job < p->jobs; job++) {
        JobPlan j;
        if (!collect_job(p, a, job, j) || !fill_grid(j) || !qualifies(j)) return false;
        plan_shards(p, j);
        order_items(p, j);
        describe_job(p, a, j);
        if (j.hybrid) plan_hybrid(j, out);
        else if (j.direct) plan_direct(p, j, out);
        else plan_main(p, j, out);
        plan_apron_stitch(j, out);
        const TailPlan tails = plan_tails(j, out);
        if (j.spherical) plan_cube_seams(j, tails, out);
        items.push_back(std::move(j.items));
        grids.push_back(std::move(j.grid.cells));
    }
    return fused_upload(state, items, grids) == BT_OK;
}

// Before the launches of a run, in plan order: a fused main / direct launch whose finest tiles are all still unwritten since bt_atlas_create
// (Attachment::written) runs with FusedArgs::prev_zero — bit-identical by construction, the fetch would return the memset's 0 — and every
// launch marks the layers it writes, so a later job of the same queue that overlays these tiles takes the fetching path.  Returns how many
// launches got the flag (bt_run_stats::prev_zero_launches).
uint32_t fused_begin_run(bt_preprocessor* p, bt_atlas* a) {
    uint32_t flagged = 0;
    for (const Launch& l : p->plan) {
        Attachment& at = a->attachments[l.attachment];
        if (l.kind == kLaunchSplit || l.kind == kLaunchDownsample || l.kind == kLaunchStitch) {
            for (uint32_t i = l.first_task; i < l.first_task + l.task_count && i < p->tasks_host.size(); i++) at.mark_written(p->tasks_host[i].atlas_index, 1);
            continue;
        }
        if (!p->fused || l.aux0 >= p->fused->jobs.size()) continue;
        FusedJobDev& job = p->fused->jobs[l.aux0];
        if (l.kind == kLaunchFusedMain || l.kind == kLaunchFusedDirect) {
            bool fresh = !job.finest_layers.empty();
            for (uint32_t layer : job.finest_layers) fresh = fresh && layer < at.written.size() && !at.written[layer];
            job.args.prev_zero = fresh ? 1u : 0u;
            flagged += fresh;
        }
        for (uint32_t layer : job.all_layers) at.mark_written(layer, 1);
    }
    return flagged;
}

// The source texels [x0, x1) x [y0, y1) of raster `raster` that the launches of the compiled plan read — for a sharded
// preprocessor: this rank's column strips + their halo (finest aprons are evaluated from the source; fused_main's staged windows
// start on an 8-texel boundary and are lds_pitch wide; fused_direct reads texel by texel).  Conservative (a missing neighbour tile
// only shrinks what the kernel reads).  Decided PER RASTER: false — the caller assumes the whole raster — unless every launch that
// reads it is a fused_main / fused_direct launch with an item list (a height raster read by fused_main and an albedo raster read by
// fused_direct in one queue get a window each; a raster the hybrid plan's batched split reads has none).
bool fused_source_window(const bt_preprocessor* p, uint32_t raster, uint32_t out[4]) {
    if (!p->fused || raster >= p->rasters.size()) return false;
    if (raster < p->fused->whole_raster.size() && p->fused->whole_raster[raster]) return false;
    const RasterDev& r = p->rasters[raster].dev;
    uint32_t x0 = r.width, y0 = r.height, x1 = 0, y1 = 0;
    bool any = false, known = false;
    for (const Launch& l : p->plan) {
        if ((l.kind != kLaunchFusedMain && l.kind != kLaunchFusedDirect) || l.aux0 >= p->fused->jobs.size()) continue;
        const FusedJobDev& job = p->fused->jobs[l.aux0];
        if (job.host_items.empty()) continue;
        known = true;
        const bool direct = l.variant == BT_VARIANT_DIRECT || l.variant == BT_VARIANT_DIRECT_REP || l.variant == BT_VARIANT_DIRECT_SKIPS;
        const FusedArgs& A = job.args;
        const uint32_t c = A.m.center_size, b = A.m.border_size, n = 1u << A.lod;
        const float scale = float(n);
        auto ax = [&](uint32_t tile, uint32_t col) { return split_axis(col, c, tile, scale, A.tlx, A.brx, r.width); };
        auto ay = [&](uint32_t tile, uint32_t row) { return split_axis(row, c, tile, scale, A.tly, A.bry, r.height); };
        for (const MainItem& it : job.host_items) {
            if (it.raster != raster) continue;
            any = true;
            const int lo_x = std::min(it.x > 0 ? ax(it.x - 1, c - b).i0 : ax(it.x, 0).i0, ax(it.x, 0).i0);
            const int hi_x = std::max(it.x + 1 < n ? ax(it.x + 1, b - 1).i1 : ax(it.x, c - 1).i1, ax(it.x, c - 1).i1);
            const int lo_y = std::min(it.y > 0 ? ay(it.y - 1, c - b).i0 : ay(it.y, 0).i0, ay(it.y, 0).i0);
            const int hi_y = std::max(it.y + 1 < n ? ay(it.y + 1, b - 1).i1 : ay(it.y, c - 1).i1, ay(it.y, c - 1).i1);
            uint32_t xa = uint32_t(std::max(lo_x, 0)), xe = uint32_t(hi_x) + 1u;
            if (!direct) {
                xa &= ~7u;
                if (l.variant != BT_VARIANT_MAIN_UNSTAGED) xe = std::max(xe, xa + A.lds_pitch);  // the staged window: lds_pitch texels from the aligned start
                if (xe + 8u > r.width) xe = r.width;                   // (pieces past the row's end re-read its last 16 bytes)
            }
            x0 = std::min(x0, xa);
            x1 = std::max(x1, std::min(xe, r.width));
            y0 = std::min(y0, uint32_t(std::max(lo_y, 0)));
            y1 = std::max(y1, std::min(uint32_t(hi_y) + 1u, r.height));
        }
    }
    if (!known) return false;
    if (!any) x0 = y0 = x1 = y1 = 0;  // a cube face none of this rank's units lie on
    out[0] = x0;
    out[1] = y0;
    out[2] = x1;
    out[3] = y1;
    return true;
}

// Bands of whole tile rows of a fused main / direct launch (streamed runs), with the raster each band reads and the last source row its
// kernels touch (the bottom apron rows of its last tile row are evaluated with the next tile row's formula: same f32 operations as the
// kernels' row tables).  The items are in (side, tile row, x) order; a band never crosses a side (a cube job: six rasters, one after the
// other).  tile_rows_per_band == 0: a quarter of the face's tile rows, at most 4 (the 16k job: 8 bands of 4 rows; a 4k job: 4 bands of 2).
bool fused_stream_bands(bt_preprocessor* p, const Launch& l, uint32_t tile_rows_per_band, std::vector<StreamBand>* bands) {
    if ((l.kind != kLaunchFusedMain && l.kind != kLaunchFusedDirect) || !p->fused || l.aux0 >= p->fused->jobs.size()) return false;
    const FusedJobDev& job = p->fused->jobs[l.aux0];
    const std::vector<MainItem>& items = job.host_items;
    if (items.empty() || l.variant == BT_VARIANT_MAIN_UNSTAGED) return false;  // (the unstaged fused_main is two kernels over the whole item list)
    const uint32_t c = job.args.m.center_size, b = job.args.m.border_size, n = 1u << job.args.lod;
    if (tile_rows_per_band == 0) tile_rows_per_band = std::max(1u, std::min(4u, n / 4u));
    const float scale = float(n);
    bands->clear();
    size_t i = 0;
    while (i < items.size()) {
        const uint32_t side = items[i].side, raster = items[i].raster;
        if (raster >= p->rasters.size()) return false;
        const RasterDev& r = p->rasters[raster].dev;
        auto axis = [&](uint32_t tile, uint32_t row) { return split_axis(row, c, tile, scale, job.args.tly, job.args.bry, r.height); };
        StreamBand band{};
        band.item_begin = uint32_t(i);
        band.tile_y_begin = items[i].y;
        band.side = side;
        band.raster = raster;
        uint32_t rows = 0, y = items[i].y;
        while (i < items.size() && items[i].side == side && (items[i].y == y || rows + 1 < tile_rows_per_band)) {
            if (items[i].raster != raster) return false;  // one source per side
            if (items[i].y != y) {
                if (items[i].y < y) return false;  // not in tile-row order
                y = items[i].y;
                rows++;
            }
            i++;
        }
        band.item_count = uint32_t(i) - band.item_begin;
        band.tile_y_end = y + 1;
        const int hi = y + 1 < n ? axis(y + 1, b - 1).i1 : axis(y, c - 1).i1;
        band.source_row_end = uint32_t(std::min<int64_t>(int64_t(r.height), int64_t(hi) + 1));
        // a raster's bands follow each other and its source rows never decrease from band to band (they do not for a dataset rectangle with
        // top < bottom); a raster that comes back after another one's bands cannot be streamed
        if (!bands->empty() && bands->back().raster == raster) {
            if (bands->back().source_row_end > band.source_row_end) return false;
        } else {
            for (const StreamBand& earlier : *bands)
                if (earlier.raster == raster) return false;
        }
        bands->push_back(band);
    }
    return true;
}

void fused_launch_tiles(const bt_preprocessor* p, const Launch& l, uint32_t item_begin, uint32_t item_count, std::vector<FusedTile>* out) {
    out->clear();
    if ((l.kind != kLaunchFusedMain && l.kind != kLaunchFusedDirect) || !p->fused || l.aux0 >= p->fused->jobs.size()) return;
    const FusedJobDev& job = p->fused->jobs[l.aux0];
    for (uint64_t i = item_begin; i < uint64_t(item_begin) + item_count && i < job.host_items.size(); i++) {
        const MainItem& it = job.host_items[size_t(i)];
        out->push_back({{it.side, job.args.lod, it.x, it.y}, it.atlas_index});
    }
}

}  // namespace bt

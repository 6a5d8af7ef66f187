// The streamed run (bt_preprocessor_run_streamed / _sharded) and the upload of deferred host rasters: the source travels in bands of tile
// rows on a copy queue, each band's kernels run when its rows have landed, and a saver thread downloads and writes finished tiles on a
// third queue meanwhile.  run_streamed_impl at the end is the driver over the stages above it.
#include <cstdio>
#include <cstdlib>

#include "bt_tile_io.hpp"

using namespace bt;

namespace bt {

void raster_window(const bt_preprocessor* p, uint32_t i, bool use_fused_window, uint32_t w[4]) {
    if (use_fused_window && fused_source_window(p, i, w)) return;
    w[0] = w[1] = 0;
    w[2] = p->rasters[i].dev.width;
    w[3] = p->rasters[i].dev.height;
}

// Rows [row_begin, row_end) of the window w = {x0, y0, x1, y1} of deferred raster r, host to device on `stream`: one contiguous copy when the
// pitches agree and the window is full width (it ends with the last texel of the caller's buffer, not with a whole pitch), a pitched one for
// a column window (a sharded rank's strips) or a padded device copy (the caller's rows are not 16-byte aligned).  band: the rows are a band
// of the window; without it only the whole raster travels contiguously.  *bytes: what travels.
static hipError_t copy_raster_rows(const Raster& r, const uint32_t w[4], uint32_t row_begin, uint32_t row_end, bool band, hipStream_t stream, uint64_t* bytes) {
    const uint64_t px = r.format == BT_FORMAT_R16 ? 2 : 4;
    const uint8_t* host = (const uint8_t*)r.host;
    uint8_t* dev = (uint8_t*)r.dev.data;
    if (r.host_pitch == r.dev.pitch && w[0] == 0 && w[2] == r.dev.width && (band || (row_begin == 0 && row_end == r.dev.height))) {
        const uint64_t off = uint64_t(row_begin) * r.dev.pitch, end = std::min<uint64_t>(r.host_bytes, uint64_t(row_end) * r.dev.pitch);
        *bytes = end - off;
        return hipMemcpyAsync(dev + off, host + off, end - off, hipMemcpyHostToDevice, stream);
    }
    *bytes = uint64_t(w[2] - w[0]) * px * (row_end - row_begin);
    return hipMemcpy2DAsync(dev + uint64_t(row_begin) * r.dev.pitch + w[0] * px, r.dev.pitch, host + uint64_t(row_begin) * r.host_pitch + w[0] * px, r.host_pitch,
                            uint64_t(w[2] - w[0]) * px, row_end - row_begin, hipMemcpyHostToDevice, stream);
}

// Deferred host rasters travel when the queue runs.  A SHARDED preprocessor (compiled plan known) uploads only the texels its
// own launches read — its column strips + halo (a rank never touches the rest of the source).  What has travelled is
// remembered per raster (Raster::windows, every rectangle the device holds): when a kept queue is compiled again — another rank / world
// (bt_preprocessor_set_shard), BT_RUN_GENERIC or BT_RUN_REFERENCE_DISPATCH, whose launches read the whole raster — and its launches read
// texels outside every such rectangle, the missing window travels before the run (the caller keeps the rows of a deferred raster alive
// until the queue is RELEASED: the ABI-6 lifetime rule of bt_raster).  A borrowed device raster that is not 16-byte aligned is copied into
// its padded buffer by EVERY run ("borrowed" means "read at run time", whatever the width).  skip[i] != 0: raster i is handled by the
// caller (the streamed run uploads it band by band).
bt_status upload_pending_rasters(bt_preprocessor* p, const std::vector<uint8_t>* skip) {
    for (size_t i = 0; i < p->rasters.size(); i++) {
        Raster& r = p->rasters[i];
        if (skip && i < skip->size() && (*skip)[i]) continue;
        if (r.dev_src) {
            const uint64_t px2 = r.format == BT_FORMAT_R16 ? 2 : 4;
            BT_HIP(hipMemcpy2DAsync((void*)r.dev.data, r.dev.pitch, r.dev_src, r.dev_src_pitch, uint64_t(r.dev.width) * px2, r.dev.height, hipMemcpyDeviceToDevice, p->ctx->stream));
            r.pending = false;
            continue;
        }
        if (!r.host) continue;  // not a deferred raster
        uint32_t w[4];
        raster_window(p, uint32_t(i), p->shard_world > 1 && p->compiled, w);
        const bool empty = !(w[2] > w[0] && w[3] > w[1]);
        const bool covered = empty || r.holds(w);
        if (!r.pending && covered) continue;
        p->uploaded_source_bytes = 0;  // (the last deferred raster that was looked at: an empty window travels as 0 bytes)
        if (covered) {
            r.pending = false;
            continue;
        }
        uint64_t bytes = 0;
        BT_HIP(copy_raster_rows(r, w, w[1], w[3], false, p->ctx->stream, &bytes));
        p->uploaded_source_bytes = bytes;
        BT_HIP(hipStreamSynchronize(p->ctx->stream));
        r.add_window(w);
        r.pending = false;
    }
    return BT_OK;
}
}  // namespace bt

namespace {
// The upload and download queues of the streamed run.  They get NON-DEFAULT PRIORITIES — not for the priority's sake: the runtime maps HIP
// streams onto a handful of hardware queues round-robin PER PRIORITY CLASS, and a process that owns a few other default-priority streams
// (a host application does; bench.py's second lane does) can land the download stream on the kernels' own hardware queue, where every copy
// then waits behind the next bands' kernels: config 2 end to end 6.6 -> 8.9 ms with exactly one extra stream in the process (round 6
// probe).  A class of their own keeps the three queues apart whatever else the process has created.
bt_status ctx_side_streams(bt_ctx* ctx) {
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) least = greatest = 0;
    if (!ctx->copy_stream) BT_HIP(hipStreamCreateWithPriority(&ctx->copy_stream, hipStreamNonBlocking, greatest));
    if (!ctx->save_stream) BT_HIP(hipStreamCreateWithPriority(&ctx->save_stream, hipStreamNonBlocking, least));
    return BT_OK;
}

// The arguments of a streamed call and what check_streamed_call reads off them.
struct StreamCall {
    bt_preprocessor* p;
    bt_atlas* a;
    bt_comm* comm;
    const char* assets_root;
    uint32_t flags;
    bool sharded = false, local = true, finish = true;  // which halves of a sharded step this call runs (an unsharded one: both)
    uint32_t mode = 0;                                  // the BT_RUN_GENERIC / BT_RUN_REFERENCE_DISPATCH bits of `flags`
};

// One step of a streamed run: an upload (optional), a launch — a whole plan entry or a band of a fused main / direct launch — and the
// tiles that are complete, and may leave, once that launch has run.
struct StreamStep {
    size_t plan_index = 0;
    bool band = false;
    uint32_t item_begin = 0, item_count = 0;
    int32_t raster = -1;        // band: rows below `row_end` of this deferred raster travel first (those that have not yet)
    uint32_t row_end = 0;
    uint32_t attachment = 0;
    TileSaver::Tiles early;     // the band's finished finest tiles
    TileSaver::Tiles rest;      // behind the attachment's last launch: every tile of it that has not left yet
    bool exchange_before = false;  // a sharded run with a communicator: the grouped collective precedes this step's launch
};

struct StreamPlan {
    std::vector<StreamStep> steps;
    std::vector<uint8_t> banded_raster;             // per raster: it travels band by band
    std::vector<std::array<uint32_t, 4>> window;    // per banded raster: the column window that travels (a sharded rank: its strips + halo)
    bool exchange_at_end = false;
};

// Which tiles leave after which step (assign_saves fills this and the steps' `early` and `rest` lists).
struct SavePlan {
    std::vector<uint8_t> in_plan;                   // per attachment: the plan has a launch of it
    std::vector<std::unordered_map<uint32_t, bt_tile_coordinate>> waiting;  // to_save entries of those attachments that no step takes, by atlas index
    size_t last_saving = 0;
};

bt_status check_streamed_call(StreamCall& c) {
    bt_preprocessor* p = c.p;
    if (!p || !c.a || !c.assets_root) return BT_ERR_INVALID_ARGUMENT;
    if (p->ctx != c.a->ctx) {
        set_error("preprocessor and atlas belong to different contexts");
        return BT_ERR_INVALID_ARGUMENT;
    }
    c.sharded = p->shard_world > 1;
    uint32_t halves = c.flags & (BT_RUN_SHARD_LOCAL | BT_RUN_SHARD_FINISH);
    if (!c.sharded || !halves) halves = BT_RUN_SHARD_LOCAL | BT_RUN_SHARD_FINISH;
    c.local = (halves & BT_RUN_SHARD_LOCAL) != 0;
    c.finish = (halves & BT_RUN_SHARD_FINISH) != 0;
    if (c.sharded && c.local && c.finish && !c.comm) {
        set_error("bt_preprocessor_run_streamed_sharded: both halves in one call need a communicator (or call BT_RUN_SHARD_LOCAL, exchange, BT_RUN_SHARD_FINISH)");
        return BT_ERR_INVALID_ARGUMENT;
    }
    BT_HIP(hipSetDevice(p->ctx->device));
    c.mode = c.flags & (BT_RUN_GENERIC | BT_RUN_REFERENCE_DISPATCH);
    if (bt_status s = ensure_compiled(p, c.a, c.mode)) return s;
    if (c.sharded) {
        // only the distributed result makes sense here (a replicated atlas has no "share" to write): the finest LOD stays where it was computed
        if (p->shard_pieces.empty()) {
            set_error("bt_preprocessor_run_streamed_sharded: the queue does not shard (world %u must divide its units; fused plans only)", p->shard_world);
            return BT_ERR_UNSUPPORTED;
        }
        if (bt_status s = check_distributed_one_sided(p)) return s;
        p->shard_distributed = true;
    }
    return BT_OK;
}

// The steps: the plan's entries in launch order (a sharded step: the local half, the exchange, the finishing half), bandable launches cut
// into bands.
StreamPlan plan_steps(const StreamCall& c, bt_stream_stats* st) {
    bt_preprocessor* p = c.p;
    uint32_t rows_per_band = 0;  // automatic
#ifdef BT_DEBUG_HOOKS
    if (const char* e = getenv("BT_STREAM_BAND_ROWS")) rows_per_band = uint32_t(std::max(1, atoi(e)));
#endif
    StreamPlan sp;
    sp.banded_raster.assign(p->rasters.size(), 0);
    for (int half = 0; half < 2; half++) {
        if (half == 0 ? !c.local : !c.finish) continue;
        bool first_of_half = true;
        for (size_t i = 0; i < p->plan.size(); i++) {
            const Launch& l = p->plan[i];
            if (c.sharded ? (l.phase == 2) != (half == 1) : half == 1) continue;
            std::vector<StreamBand> bands;
            bool bandable = fused_stream_bands(p, l, rows_per_band, &bands) && !bands.empty();
            for (const StreamBand& b : bands) {
                const Raster& r = p->rasters[b.raster];
                bandable = bandable && r.host != nullptr && r.pending && !r.dev_src;  // a deferred host raster that has not travelled
            }
            StreamStep proto;
            proto.plan_index = i;
            proto.attachment = l.attachment;
            proto.exchange_before = c.sharded && c.comm && half == 1 && first_of_half && c.local;
            first_of_half = false;
            if (!bandable) {
                sp.steps.push_back(proto);
                continue;
            }
            for (size_t k = 0; k < bands.size(); k++) {
                StreamStep sb = proto;
                sb.exchange_before = proto.exchange_before && k == 0;
                sb.band = true;
                sb.item_begin = bands[k].item_begin;
                sb.item_count = bands[k].item_count;
                sb.raster = int32_t(bands[k].raster);
                // (the last band of a raster takes the rest of it: rows below the last tile row's apron that no kernel reads still count as uploaded)
                const bool last_of_raster = k + 1 == bands.size() || bands[k + 1].raster != bands[k].raster;
                sb.row_end = last_of_raster ? p->rasters[bands[k].raster].dev.height : bands[k].source_row_end;
                sp.banded_raster[bands[k].raster] = 1;
                sp.steps.push_back(sb);
            }
            st->banded_launches++;
            st->bands += uint32_t(bands.size());
        }
    }
    // (a sharded one-call run whose plan has no finishing launch — a single-LOD job — still owes the step its collective)
    bool exchange_scheduled = false;
    for (const StreamStep& s : sp.steps) exchange_scheduled = exchange_scheduled || s.exchange_before;
    sp.exchange_at_end = c.sharded && c.comm && c.local && c.finish && !exchange_scheduled;
    // (the windows depend on the compiled plan alone: the same before the up-front uploads as after them)
    sp.window.resize(p->rasters.size());
    for (size_t i = 0; i < p->rasters.size(); i++)
        if (sp.banded_raster[i]) raster_window(p, uint32_t(i), c.sharded, sp.window[i].data());
    return sp;
}

// Nothing to stream (at most one band): the same result, one leg after the other.
bt_status run_unstreamed(const StreamCall& c, bt_stream_stats* out) {
    bt_preprocessor* p = c.p;
    bt_atlas* a = c.a;
    const uint32_t keep = c.mode | BT_RUN_KEEP_QUEUE;
    if (!c.sharded) {
        if (bt_status s = bt_preprocessor_run(p, a, keep)) return s;
    } else {
        if (c.local)
            if (bt_status s = bt_preprocessor_run(p, a, keep | BT_RUN_SHARD_LOCAL | BT_RUN_SHARD_DISTRIBUTED)) return s;
        if (c.local && c.finish)
            if (bt_status s = shard_exchange(p, a, c.comm, p->ctx->stream, true)) return s;
        if (c.finish)
            if (bt_status s = bt_preprocessor_run(p, a, keep | BT_RUN_SHARD_FINISH | BT_RUN_SHARD_DISTRIBUTED)) return s;
    }
    bt_stream_stats none{};
    if (c.finish) {
        for (const AtlasTileAttachment& t : a->to_save)  // what bt_preprocessor_save is about to write (a sharded rank: its share)
            if (t.atlas_index != BT_INVALID_ATLAS_INDEX && (!c.sharded || shard_holder(p, t.attachment_index, t.coordinate.lod, t.atlas_index) == p->shard_rank))
                none.saved_bytes += a->attachments[t.attachment_index].tile_bytes;
        if (bt_status s = bt_preprocessor_save(p, a, c.assets_root)) return s;
    }
    if (out) *out = none;
    return ((c.flags & BT_RUN_KEEP_QUEUE) || !c.finish) ? BT_OK : release_queue(p);
}

// Which tiles leave after which step.  A finest tile of a banded launch leaves with its band when nothing later writes it: the
// attachment has ONE job in the queue (an overlay or an adjacent dataset would write or stitch it again), and on a cube it does not
// touch a face edge (its cross-face aprons are stitched after the last face).  Everything else of an attachment leaves behind the
// attachment's last launch.  A sharded rank writes its share only (shard_holder).
SavePlan assign_saves(const StreamCall& c, std::vector<StreamStep>& steps, bt_stream_stats* st) {
    const bt_preprocessor* p = c.p;
    const bt_atlas* a = c.a;
    SavePlan sp;
    std::vector<uint32_t> jobs_of(a->attachments.size(), 0);
    {
        std::vector<std::vector<uint32_t>> seen(a->attachments.size());
        for (const Task& t : p->queue)
            if (t.type == kSplit && std::find(seen[t.attachment_index].begin(), seen[t.attachment_index].end(), t.job) == seen[t.attachment_index].end()) {
                seen[t.attachment_index].push_back(t.job);
                jobs_of[t.attachment_index]++;
            }
    }
    sp.in_plan.assign(a->attachments.size(), 0);
    for (const StreamStep& s : steps) sp.in_plan[s.attachment] = 1;
    // to_save entries of the attachments this run handles, by (attachment, atlas index)
    sp.waiting.resize(a->attachments.size());
    for (const AtlasTileAttachment& t : a->to_save) {
        if (t.atlas_index == BT_INVALID_ATLAS_INDEX || !sp.in_plan[t.attachment_index]) continue;
        if (c.sharded && shard_holder(p, t.attachment_index, t.coordinate.lod, t.atlas_index) != p->shard_rank) continue;
        sp.waiting[t.attachment_index][t.atlas_index] = t.coordinate;
    }
    const bool spherical = a->config.spherical != 0;
    for (StreamStep& s : steps) {
        if (!s.band || jobs_of[s.attachment] != 1) continue;
        std::vector<FusedTile> tiles;
        fused_launch_tiles(p, p->plan[s.plan_index], s.item_begin, s.item_count, &tiles);
        for (const FusedTile& t : tiles) {
            if (spherical && on_face_edge(t.coordinate)) continue;
            auto w = sp.waiting[s.attachment].find(t.atlas_index);
            if (w == sp.waiting[s.attachment].end() || !operator_eq(w->second, t.coordinate)) continue;
            s.early.push_back({t.atlas_index, t.coordinate});
            sp.waiting[s.attachment].erase(w);
        }
        st->early_tiles += uint32_t(s.early.size());
    }
    if (c.finish)
        for (uint32_t ai = 0; ai < a->attachments.size(); ai++) {
            if (!sp.in_plan[ai] || sp.waiting[ai].empty()) continue;
            size_t last = steps.size();
            for (size_t k = 0; k < steps.size(); k++)
                if (steps[k].attachment == ai) last = k;
            for (const auto& [index, coord] : sp.waiting[ai]) steps[last].rest.push_back({index, coord});
        }
    for (size_t k = 0; k < steps.size(); k++)
        if (!steps[k].early.empty() || !steps[k].rest.empty()) sp.last_saving = k;
    return sp;
}

// The events of a streamed run: computed[k] follows step k's launch on the kernels' stream, `uploaded` a band's copy on the copy stream.
struct StreamEvents {
    std::vector<hipEvent_t> computed;
    hipEvent_t uploaded = nullptr;
    bt_status create(size_t steps) {
        computed.assign(steps, nullptr);
        for (hipEvent_t& e : computed) BT_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        BT_HIP(hipEventCreateWithFlags(&uploaded, hipEventDisableTiming));
        return BT_OK;
    }
    ~StreamEvents() {
        for (hipEvent_t e : computed)
            if (e) hipEventDestroy(e);
        if (uploaded) hipEventDestroy(uploaded);
    }
};

// The saver thread: step after step as their kernels are enqueued (host handshake: publish), ordered on the GPU by events.  Its status, its
// copy of the error text (set_error is per thread) and saved_bytes are read after join().
class StepSaver {
  public:
    StepSaver(const StreamCall& c, const std::vector<StreamStep>& steps, size_t last_saving, const StreamEvents& events) : c_(c), steps_(steps), last_saving_(last_saving), events_(events), thread_([this] { run(); }) {}
    void publish(size_t n) {  // the `computed` events of the steps below n have been recorded
        { std::lock_guard<std::mutex> lock(m_); launched_ = n; }
        cv_.notify_all();
    }
    void abort() {
        { std::lock_guard<std::mutex> lock(m_); abort_ = true; }
        cv_.notify_all();
    }
    void join() { thread_.join(); }
    bt_status status = BT_OK;
    char error[512] = "";
    uint64_t saved_bytes = 0;

  private:
    void run() {
        bt_atlas* a = c_.a;
        hipStream_t stream = a->ctx->save_stream;
        const std::vector<StreamStep>& steps = steps_;
        const size_t ns = steps.size();
        const std::string terrain = std::string(c_.assets_root) + "/" + a->config.path;
        hipSetDevice(a->ctx->device);
        TileSaver ts(a, stream);
        bt_status s = ts.begin();
        for (size_t k = 0; k < ns && s == BT_OK;) {
            if (steps[k].early.empty() && steps[k].rest.empty()) {
                k++;
                continue;
            }
            // The saver takes what is ready: step k and every following step of the same attachment that the launcher has enqueued by
            // now travel as ONE hand-over (sorted by layer, cut into 32 MB chunks).  When the download + write side is the slower one — it
            // is, on PCIe — the bands it falls behind on merge into full-size chunks instead of paying the per-chunk latencies band by band
            // (config 2's 8 MB and 16 MB bands: 0.6 / 0.9 ms each, i.e. 13 - 17 GB/s; merged 32 MB chunks move at 45).
            size_t last = k;
            {
                std::unique_lock<std::mutex> lock(m_);
                cv_.wait(lock, [&] { return launched_ > k || abort_; });
                if (abort_) break;
                while (last + 1 < ns && launched_ > last + 1 && steps[last + 1].attachment == steps[k].attachment) last++;
            }
            if (hipStreamWaitEvent(stream, events_.computed[last], 0) != hipSuccess) s = BT_ERR_DEVICE;
            trace_stamp("saver: steps taken up to", last);
            TileSaver::Tiles tiles;
            for (size_t q = k; q <= last; q++) {
                tiles.insert(tiles.end(), steps[q].early.begin(), steps[q].early.end());
                tiles.insert(tiles.end(), steps[q].rest.begin(), steps[q].rest.end());
            }
            const uint32_t ai = steps[k].attachment;
            if (s == BT_OK && !tiles.empty()) s = ts.add(ai, terrain + "/data/" + a->attachments[ai].cfg.name, std::move(tiles), last >= last_saving_);
            trace_stamp("saver: copies issued, previous chunks handed to the writers", last);
            k = last + 1;
        }
        if (s == BT_OK) s = ts.finish();
        saved_bytes = ts.saved_bytes();
        if (s != BT_OK) {
            snprintf(error, sizeof error, "%s", bt_last_error());
            status = s;
        }
    }
    const StreamCall& c_;
    const std::vector<StreamStep>& steps_;
    const size_t last_saving_;
    const StreamEvents& events_;
    std::mutex m_;
    std::condition_variable cv_;
    size_t launched_ = 0;  // steps whose `computed` event has been recorded
    bool abort_ = false;
    std::thread thread_;  // (the last member: it starts in the constructor and reads the others)
};

// The rows of band step k's raster that have not travelled yet, on the copy stream; the kernels' stream waits for them.
bt_status upload_band(const StreamCall& c, const StreamPlan& sp, size_t k, hipEvent_t uploaded, uint32_t* done, uint64_t* uploaded_bytes) {
    const StreamStep& step = sp.steps[k];
    const uint32_t* w = sp.window[size_t(step.raster)].data();
    const uint32_t end_row = std::min(step.row_end, w[3]);
    if (!(end_row > *done && w[2] > w[0])) return BT_OK;
    trace_stamp("upload begin", k);
    uint64_t bytes = 0;
    const hipError_t e = copy_raster_rows(c.p->rasters[size_t(step.raster)], w, *done, end_row, true, c.p->ctx->copy_stream, &bytes);
    *uploaded_bytes += bytes;
    trace_stamp("upload call returned", k);
    *done = end_row;
    if (e != hipSuccess || hipEventRecord(uploaded, c.p->ctx->copy_stream) != hipSuccess) return BT_ERR_DEVICE;
    return hipStreamWaitEvent(c.p->ctx->stream, uploaded, 0) == hipSuccess ? BT_OK : BT_ERR_DEVICE;
}

// The launcher, on the calling thread: upload what a step needs (a pageable copy holds the host until it is done; the GPU meanwhile runs the
// step before), launch it, tell the saver.
bt_status launch_steps(const StreamCall& c, const StreamPlan& sp, const StreamEvents& events, StepSaver& saver, uint64_t* uploaded_bytes) {
    bt_preprocessor* p = c.p;
    if (c.local) {
        // rasters no band covers (a launch that cannot be banded reads them): whole, up front, on the kernels' stream
        if (bt_status s = upload_pending_rasters(p, &sp.banded_raster)) return s;
        p->stats.variants = 0;
        p->stats.prev_zero_launches = fused_begin_run(p, c.a);
    }
    std::vector<uint32_t> done_rows(p->rasters.size(), 0);  // per banded raster: the rows of its window that have travelled
    for (size_t i = 0; i < p->rasters.size(); i++)
        if (sp.banded_raster[i]) done_rows[i] = sp.window[i][1];
    for (size_t k = 0; k < sp.steps.size(); k++) {
        const StreamStep& step = sp.steps[k];
        const Launch& l = p->plan[step.plan_index];
        if (step.exchange_before)
            if (bt_status s = shard_exchange(p, c.a, c.comm, p->ctx->stream, true)) return s;
        if (step.band)
            if (bt_status s = upload_band(c, sp, k, events.uploaded, &done_rows[size_t(step.raster)], uploaded_bytes)) return s;
        if (bt_status s = step.band ? run_plan_entry(p, c.a, l, step.item_begin, step.item_count) : run_plan_entry(p, c.a, l)) return s;
        if (hipEventRecord(events.computed[k], p->ctx->stream) != hipSuccess) return BT_ERR_DEVICE;
        saver.publish(k + 1);
    }
    return sp.exchange_at_end ? shard_exchange(p, c.a, c.comm, p->ctx->stream, true) : BT_OK;
}

// Launcher and saver are done: wait for the device, book what travelled and what was written, save the rest, release the queue.
bt_status settle(const StreamCall& c, const StreamPlan& sp, const SavePlan& saves, bt_status rc, const StepSaver& saver, bt_stream_stats st, bt_stream_stats* out) {
    bt_preprocessor* p = c.p;
    bt_atlas* a = c.a;
    hipStreamSynchronize(p->ctx->stream);
    if (rc != BT_OK || saver.status != BT_OK) {  // nothing of this call may still read the caller's raster or write the pinned buffers
        hipStreamSynchronize(p->ctx->copy_stream);
        hipStreamSynchronize(p->ctx->save_stream);
    }
    // a raster counts as uploaded only when every band of it went out; after a failure a later run of the kept queue uploads it whole
    if (rc == BT_OK)
        for (size_t i = 0; i < p->rasters.size(); i++)
            if (sp.banded_raster[i]) {
                const uint32_t* w = sp.window[i].data();
                p->rasters[i].pending = false;
                if (w[2] > w[0] && w[3] > w[1]) p->rasters[i].add_window(w);
            }
    p->uploaded_source_bytes = st.uploaded_bytes;
    if (rc == BT_ERR_DEVICE) set_error("bt_preprocessor_run_streamed: HIP call failed (%s)", hipGetErrorString(hipGetLastError()));
    if (rc != BT_OK) return rc;
    if (saver.status != BT_OK) {
        set_error("%s", saver.error);
        return saver.status;
    }
    st.saved_bytes = saver.saved_bytes;
    // What the saver wrote leaves the atlas's list.  A finishing call wrote every entry of the plan's attachments (a sharded rank: its
    // share — the others' entries go too, their holders write them); a local-only call only the early tiles.  Whatever else waits (Save
    // tasks of another attachment from an earlier run that was not saved yet) goes through bt_preprocessor_save, which also writes config.tc.
    a->to_save.erase(std::remove_if(a->to_save.begin(), a->to_save.end(),
                                    [&](const AtlasTileAttachment& t) {
                                        if (!saves.in_plan[t.attachment_index]) return false;
                                        if (c.finish) return true;
                                        const auto& w = saves.waiting[t.attachment_index];
                                        const bool mine = !c.sharded || shard_holder(p, t.attachment_index, t.coordinate.lod, t.atlas_index) == p->shard_rank;
                                        return mine && w.find(t.atlas_index) == w.end();  // (held by this rank and no longer waiting: it left with a band)
                                    }),
                     a->to_save.end());
    if (c.finish)
        if (bt_status s = bt_preprocessor_save(p, a, c.assets_root)) return s;
    st.streamed = 1;
    if (out) *out = st;
    return ((c.flags & BT_RUN_KEEP_QUEUE) || !c.finish) ? BT_OK : release_queue(p);
}

bt_status run_streamed_impl(bt_preprocessor* p, bt_atlas* a, bt_comm* comm, const char* assets_root, uint32_t flags, bt_stream_stats* out) {
    StreamCall c{p, a, comm, assets_root, flags};
    if (bt_status s = check_streamed_call(c)) return s;
    record_saves(p, a);
    bt_stream_stats st{};
    StreamPlan sp = plan_steps(c, &st);
    if (st.bands <= 1) return run_unstreamed(c, out);
    if (bt_status s = ctx_side_streams(p->ctx)) return s;
    const SavePlan saves = assign_saves(c, sp.steps, &st);
    StreamEvents events;
    if (bt_status s = events.create(sp.steps.size())) return s;
    trace_start();
    StepSaver saver(c, sp.steps, saves.last_saving, events);
    const bt_status rc = launch_steps(c, sp, events, saver, &st.uploaded_bytes);
    if (rc != BT_OK) saver.abort();
    trace_stamp("all launched", sp.steps.size());
    saver.join();
    trace_stamp("saver done", sp.steps.size());
    return settle(c, sp, saves, rc, saver, st, out);
}
}  // namespace

extern "C" {

// The reference's own span (preprocessor.rs:363,419: sources loaded -> all saves done) as ONE overlapped pipeline: the source
// rasters travel to the GPU in bands of tile rows on a copy queue, each band's kernels start when its rows (and the few
// apron rows below it) have landed, and a second thread downloads and writes a band's finished tiles on a third queue while
// the next bands upload and run: H2D, kernels, D2H and the file system work at the same time (PCIe is full duplex).  Round 6: every
// fused main / direct launch of the plan is banded — several attachments (examples/preprocess_planar.rs:16-60), the six faces of a
// cube job (examples/preprocess_spherical.rs:20-48) — and a sharded rank streams its own window and share.
bt_status bt_preprocessor_run_streamed(bt_preprocessor* p, bt_atlas* a, const char* assets_root, uint32_t flags, bt_stream_stats* out) {
    if (p && p->shard_world > 1) {
        set_error("bt_preprocessor_run_streamed: a sharded preprocessor runs through bt_preprocessor_run_streamed_sharded");
        return BT_ERR_UNSUPPORTED;
    }
    return run_streamed_impl(p, a, nullptr, assets_root, flags, out);
}

bt_status bt_preprocessor_run_streamed_sharded(bt_preprocessor* p, bt_atlas* a, bt_comm* comm, const char* assets_root, uint32_t flags, bt_stream_stats* out) {
    if (!p) return BT_ERR_INVALID_ARGUMENT;
    if (comm && p->shard_world > 1)
        if (bt_status s = shard_check_comm(p, comm)) return s;
    return run_streamed_impl(p, a, comm, assets_root, flags, out);
}

}  // extern "C"

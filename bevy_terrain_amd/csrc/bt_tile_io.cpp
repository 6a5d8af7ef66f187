// Tile files: the writer / reader threads, the download-and-write pipeline of the save path, the two load paths (bt_atlas_load_tiles,
// bt_atlas_update), the small file-system helpers, and the time stamps of the profiling build.
#include <dirent.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cstdio>
#include <cstring>

#include "bt_tile_io.hpp"

namespace bt {

#ifdef BT_DEBUG_HOOKS
static std::chrono::steady_clock::time_point g_trace_start;
static bool g_trace = false;
void trace_start() {
    g_trace = getenv("BT_STREAM_TRACE") != nullptr;
    g_trace_start = std::chrono::steady_clock::now();
}
void trace_stamp(const char* what, size_t k) {
    if (g_trace) fprintf(stderr, "[stream] %7.3f ms %s %zu\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - g_trace_start).count(), what, k);
}
#endif

bt_status write_file(const std::string& path, const void* data, size_t bytes) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) {
        set_error("cannot open %s: %s", path.c_str(), strerror(errno));
        return BT_ERR_IO;
    }
    const size_t wr = fwrite(data, 1, bytes, f);
    fclose(f);
    if (wr != bytes) {
        set_error("short write to %s", path.c_str());
        return BT_ERR_IO;
    }
    return BT_OK;
}

void remove_tree(const std::string& dir) {
    DIR* d = opendir(dir.c_str());
    if (!d) return;
    while (dirent* e = readdir(d)) {
        if (!strcmp(e->d_name, ".") || !strcmp(e->d_name, "..")) continue;
        const std::string p = dir + "/" + e->d_name;
        struct stat st;
        if (lstat(p.c_str(), &st) == 0 && S_ISDIR(st.st_mode))
            remove_tree(p);
        else
            unlink(p.c_str());
    }
    closedir(d);
    rmdir(dir.c_str());
}

bt_status make_dirs(const std::string& dir) {
    std::string cur;
    for (size_t i = 0; i <= dir.size(); i++) {
        if (i == dir.size() || dir[i] == '/') {
            if (!cur.empty() && mkdir(cur.c_str(), 0777) != 0 && errno != EEXIST) {
                set_error("mkdir %s: %s", cur.c_str(), strerror(errno));
                return BT_ERR_IO;
            }
        }
        if (i < dir.size()) cur.push_back(dir[i]);
    }
    return BT_OK;
}

void FileWriters::run() {
    for (;;) {
        Job j;
        {
            std::unique_lock<std::mutex> lock(m_);
            cv_.wait(lock, [&] { return stop_ || !queue_.empty(); });
            if (queue_.empty()) return;
            j = std::move(queue_.front());
            queue_.pop_front();
        }
        bool ok = false;
        std::string why;
        if (j.read) {
            const int fd = open(j.path.c_str(), O_RDONLY);
            if (fd >= 0) {
                uint8_t* dst = const_cast<uint8_t*>(j.data);
                size_t done = 0;
                while (done < j.bytes) {
                    const ssize_t r = ::read(fd, dst + done, j.bytes - done);
                    if (r <= 0) break;
                    done += size_t(r);
                }
                uint8_t extra;
                ok = done == j.bytes && ::read(fd, &extra, 1) == 0;
                close(fd);
                if (!ok) why = "tile file " + j.path + " does not hold " + std::to_string(j.bytes) + " bytes";
            } else {
                why = "tile file not found: " + j.path;
            }
            {
                std::lock_guard<std::mutex> lock(m_);
                if (!ok && !failed_) {
                    failed_ = true;
                    error_ = why;
                }
                pending_[j.buffer]--;
            }
            done_.notify_all();
            continue;
        }
        const int fd = open(j.path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
        if (fd >= 0) {
            size_t done = 0;
            while (done < j.bytes) {
                const ssize_t w = write(fd, j.data + done, j.bytes - done);
                if (w <= 0) break;
                done += size_t(w);
            }
            ok = done == j.bytes;
            ok = (close(fd) == 0) && ok;
            if (!ok) why = "short write to " + j.path;
        } else {
            why = "cannot open " + j.path + ": " + strerror(errno);
        }
        {
            std::lock_guard<std::mutex> lock(m_);
            if (!ok && !failed_) {
                failed_ = true;
                error_ = why;
            }
            pending_[j.buffer]--;
        }
        done_.notify_all();
    }
}

TileSaver::~TileSaver() {
    if (writers_)
        for (uint32_t k = 0; k < kBuffers; k++) writers_->wait_buffer(k);
}

bt_status TileSaver::begin() {
    BT_HIP(hipSetDevice(a_->ctx->device));
    size_t largest = 32ull << 20;
    for (const Attachment& at : a_->attachments) largest = std::max<size_t>(largest, at.tile_bytes);
    if (bt_status s = a_->ctx->staging.reserve(largest)) return s;
    // 16 writers: measured on tmpfs and the overlay disk, 6 / 8 / 12 / 16 / 24 / 32 / 64 / 128 threads write at 29 / 34 / 42 /
    // 46-49 / 46 / 35 / 4 / 5 GB/s — beyond ~24 the page-cache allocation lock dominates
    // (the count follows the CPUs the process may use, not the machine's hardware threads: bt_ctx_set_io_threads)
    uint32_t threads = ctx_io_threads(a_->ctx);
#ifdef BT_DEBUG_HOOKS
    if (const char* e = getenv("BT_SAVE_THREADS")) threads = std::max(1, atoi(e));  // tools build only: writer-count experiments
#endif
    writers_.reset(new FileWriters(threads, kBuffers));
    return BT_OK;
}

bt_status TileSaver::add(uint32_t ai, const std::string& dir, Tiles tiles, bool taper) {
    const Attachment& at = a_->attachments[ai];
    StagingRing& ring = a_->ctx->staging;
    if (std::find(dirs_.begin(), dirs_.end(), dir) == dirs_.end()) {
        if (bt_status s = make_dirs(dir)) return s;
        dirs_.push_back(dir);
    }
    const uint32_t chunk = uint32_t(std::max<uint64_t>(1, std::min<uint64_t>(64, (32ull << 20) / at.tile_bytes)));
    std::sort(tiles.begin(), tiles.end(), [](const auto& l, const auto& r) { return l.first < r.first; });
    tiles.erase(std::unique(tiles.begin(), tiles.end(), [](const auto& l, const auto& r) { return l.first == r.first && operator_eq(l.second, r.second); }),
                tiles.end());
    const size_t n = tiles.size();
    for (size_t lo = 0, step = 0; lo < n; lo += step) {
        step = chunk;
        if (taper && n - lo <= 2 * size_t(chunk)) step = std::max<size_t>(std::min<size_t>(8, chunk), (n - lo) / 2);
        const size_t hi = std::min(n, lo + step);
        const uint32_t k = uint32_t(chunks_++ % kBuffers);
        trace_stamp("  saver chunk: tiles", hi - lo);
        writers_->wait_buffer(k);
        if (bt_status s = ring.wait(k)) return s;  // no wait unless an earlier call failed: hand_over has waited for the chunk that was here
        void* pinned = ring.buffer(k);
        trace_stamp("  saver chunk: buffer free", k);
        // runs of consecutive layers; equally long runs at a constant layer stride (a band of tile rows in the x-major
        // atlas order: 4 layers every 32) travel as ONE pitched copy instead of one call per run
        std::vector<std::pair<size_t, size_t>> runs;  // (first tile of the chunk, length)
        for_each_layer_run(lo, hi, [&](size_t i) { return tiles[i].first; }, false, [&](size_t i, size_t run) -> bt_status {
            runs.push_back({i, run});
            return BT_OK;
        });
        bool regular = runs.size() >= 2;
        const uint64_t stride = regular ? uint64_t(tiles[runs[1].first].first) - tiles[runs[0].first].first : 0;
        for (size_t q = 1; regular && q < runs.size(); q++)
            regular = runs[q].second == runs[0].second && uint64_t(tiles[runs[q].first].first) - tiles[runs[q - 1].first].first == stride;
        hipError_t e = hipSuccess;
        bt_status gathered = BT_OK;
        if (regular) {
            e = hipMemcpy2DAsync(pinned, at.tile_bytes * runs[0].second, (const uint8_t*)at.level0 + at.tile_bytes * tiles[lo].first,
                                 at.tile_bytes * stride, at.tile_bytes * runs[0].second, runs.size(), hipMemcpyDeviceToHost, stream_);
        } else if (runs.size() > 2 && hi - lo <= 64 && at.tile_bytes % 16u == 0) {
            // an irregular chunk (the lower LODs behind a band's tiles, a cube's face-edge tiles, merged hand-overs): ONE gather kernel that
            // writes the pinned buffer over PCIe instead of one copy-engine call per run — a burst of small copy calls stalled the issuing
            // thread for 15 - 20 ms now and then (config 2's 37-tile chunk: 2.2 -> 21.0 ms between two stamps, round 6 traces), the kernel never
            uint32_t layers[64];
            for (size_t i = lo; i < hi; i++) layers[i - lo] = tiles[i].first;
            gathered = launch_gather_layers(stream_, at.level0, layers, uint32_t(hi - lo), pinned, at.tile_bytes);
        } else {
            for (const auto& [i, run] : runs)
                if (e == hipSuccess)
                    e = hipMemcpyAsync((uint8_t*)pinned + at.tile_bytes * (i - lo), (const uint8_t*)at.level0 + at.tile_bytes * tiles[i].first, at.tile_bytes * run, hipMemcpyDeviceToHost, stream_);
        }
        const bt_status recorded = ring.record(k, stream_);  // (behind a failed copy too: the ones before it are on their way)
        if (e != hipSuccess) return hip_fail(e, "tile download");
        if (gathered || recorded) return gathered ? gathered : recorded;
        trace_stamp("  saver chunk: copy issued", k);
        if (bt_status s = hand_over()) return s;  // the chunk enqueued BEFORE this one: wait for its copies, queue its files
        trace_stamp("  saver chunk: previous chunk handed over", k);
        in_flight_.assign(tiles.begin() + lo, tiles.begin() + hi);
        in_flight_buffer_ = k;
        in_flight_ai_ = ai;
        in_flight_dir_ = dir;
        have_in_flight_ = true;
        saved_bytes_ += uint64_t(hi - lo) * at.tile_bytes;
    }
    return BT_OK;
}

bt_status TileSaver::finish() {
    if (bt_status s = hand_over()) return s;
    for (uint32_t k = 0; k < kBuffers; k++) writers_->wait_buffer(k);
    return writers_->status();
}

bt_status TileSaver::hand_over() {
    if (!have_in_flight_) return BT_OK;
    have_in_flight_ = false;
    const Attachment& at = a_->attachments[in_flight_ai_];
    if (bt_status s = a_->ctx->staging.wait(in_flight_buffer_)) return s;
    std::vector<FileWriters::Job> jobs;
    for (size_t i = 0; i < in_flight_.size(); i++) {
        char name[64];
        bt_tile_name(in_flight_[i].second, name, sizeof name);
        jobs.push_back({in_flight_dir_ + "/" + name + ".bin", (const uint8_t*)a_->ctx->staging.buffer(in_flight_buffer_) + at.tile_bytes * i, size_t(at.tile_bytes), in_flight_buffer_});
    }
    writers_->push(std::move(jobs));
    return BT_OK;
}

bt_status save_tiles(bt_atlas* a, uint32_t ai, const char* directory, std::vector<std::pair<uint32_t, bt_tile_coordinate>> tiles) {
    if (tiles.empty()) return make_dirs(directory);
    TileSaver saver(a, a->ctx->stream);
    if (bt_status s = saver.begin()) return s;
    if (bt_status s = saver.add(ai, directory, std::move(tiles))) return s;
    return saver.finish();
}

}  // namespace bt

using namespace bt;

// The tail of every load path: these layers of attachment `ai` have been filled, in any order and possibly one of them twice; ONE batched
// mip-chain pass per run of consecutive layers
bt_status bt::mip_filled_layers(bt_atlas* a, uint32_t ai, std::vector<uint32_t>& layers) {
    if (a->attachments[ai].mips.size() <= 1) return BT_OK;
    std::sort(layers.begin(), layers.end());
    return for_each_layer_run(0, layers.size(), [&](size_t i) { return layers[i]; }, true, [&](size_t i, size_t n) {
        return bt_atlas_generate_mipmaps(a, ai, layers[i], layers[i + n - 1] - layers[i] + 1);
    });
}

extern "C" {

// AtlasTileAttachmentWithData::start_loading (tile_atlas.rs:118-149) + GpuAtlasAttachment::upload_tiles
// (gpu_tile_atlas.rs:309-336) for a batch of tiles: "{directory}/{coord}.bin" -> atlas layer of the tile (allocated
// on demand, like request_tile does), then ONE batched mip-chain pass per run of consecutive layers instead of the
// reference's per-tile CPU loop.  coords == NULL: every existing tile (load_tile_config) of the atlas.
bt_status bt_atlas_load_tiles(bt_atlas* a, uint32_t ai, const char* directory, const bt_tile_coordinate* coords, uint32_t count) {
    if (!a || ai >= a->attachments.size() || !directory || (count && !coords)) return BT_ERR_INVALID_ARGUMENT;
    Attachment& at = a->attachments[ai];
    std::vector<bt_tile_coordinate> all;
    if (!coords) {
        for (const bt_tile_coordinate& c : a->existing_tiles) all.push_back(c);
        std::sort(all.begin(), all.end(), CoordLess());
        coords = all.data();
        count = uint32_t(all.size());
    }
    if (!count) return BT_OK;
    BT_HIP(hipSetDevice(a->ctx->device));
    // files -> three pinned buffers (reader threads) -> H2D on the context's stream: chunk c + 1 is read while chunk c uploads
    constexpr uint32_t kBuffers = StagingRing::kBuffers;
    const uint32_t chunk = uint32_t(std::max<uint64_t>(1, std::min<uint64_t>(64, (32ull << 20) / at.tile_bytes)));
    StagingRing& ring = a->ctx->staging;
    if (bt_status s = ring.reserve(std::max<size_t>(32ull << 20, at.tile_bytes))) return s;
    std::vector<uint32_t> layers;
    bt_status rc = BT_OK;
    {
        FileWriters readers(ctx_io_threads(a->ctx), kBuffers);
        const uint32_t chunks = (count + chunk - 1) / chunk;
        std::vector<std::vector<uint32_t>> index(kBuffers);
        auto upload = [&](uint32_t c) -> bt_status {  // chunk c has been queued for reading: wait for its files, enqueue its copies
            const uint32_t k = c % kBuffers;
            readers.wait_buffer(k);
            if (bt_status s = readers.status()) return s;
            const bt_status copies = for_each_layer_run(0, index[k].size(), [&](size_t t) { return index[k][t]; }, false, [&](size_t t, size_t run) -> bt_status {
                a->attachments[ai].mark_written(index[k][t], uint32_t(run));  // runs of consecutive layers are one copy
                hipError_t e = hipMemcpyAsync((uint8_t*)at.level0 + at.tile_bytes * index[k][t], (const uint8_t*)ring.buffer(k) + at.tile_bytes * t,
                                              at.tile_bytes * run, hipMemcpyHostToDevice, a->ctx->stream);
                return e != hipSuccess ? hip_fail(e, "tile upload") : BT_OK;
            });
            const bt_status recorded = ring.record(k, a->ctx->stream);  // (behind a failed copy too: the ones before it are on their way)
            return copies ? copies : recorded;
        };
        for (uint32_t c = 0; c < chunks && rc == BT_OK; c++) {
            const uint32_t k = c % kBuffers, first = c * chunk, n = std::min(chunk, count - first);
            rc = ring.wait(k);  // the buffer's previous upload must have left it
            std::vector<FileWriters::Job> jobs;
            index[k].clear();
            for (uint32_t t = 0; t < n && rc == BT_OK; t++) {
                bt_atlas_tile tile;
                rc = bt_atlas_get_or_allocate_tile(a, coords[first + t], &tile);
                if (rc) break;
                index[k].push_back(tile.atlas_index);
                layers.push_back(tile.atlas_index);
                char name[64];
                bt_tile_name(coords[first + t], name, sizeof name);
                FileWriters::Job job{std::string(directory) + "/" + name + ".bin", (const uint8_t*)ring.buffer(k) + at.tile_bytes * t, size_t(at.tile_bytes), k};
                job.read = true;
                jobs.push_back(std::move(job));
            }
            if (rc == BT_OK) readers.push(std::move(jobs));
            if (rc == BT_OK && c > 0) rc = upload(c - 1);
        }
        if (rc == BT_OK) rc = upload(chunks - 1);
        for (uint32_t k = 0; k < kBuffers; k++) readers.wait_buffer(k);  // (error paths: nobody may still write into the buffers)
        const bt_status drained = ring.drain();  // every chunk's copies are recorded: the call stays synchronous with respect to its uploads
        if (rc == BT_OK) rc = drained;
    }
    return rc ? rc : mip_filled_layers(a, ai, layers);
}

uint32_t bt_atlas_pending_loads(const bt_atlas* a) { return a ? uint32_t(a->to_load.size()) : 0u; }

// TileAtlasState::update (tile_atlas.rs:327-345: start up to load_slots loads) + AtlasAttachment::update (:195-224:
// finished loads -> loaded_tile_attachment, data into the atlas) + GpuAtlasAttachment::upload_tiles
// (gpu_tile_atlas.rs:309-336), done synchronously for up to `max_loads` queued entries.
bt_status bt_atlas_update(bt_atlas* a, const char* assets_root, uint32_t max_loads, uint32_t* loaded, uint32_t* failed) {
    if (!a || !assets_root) return BT_ERR_INVALID_ARGUMENT;
    if (loaded) *loaded = 0;
    if (failed) *failed = 0;
    if (a->to_load.empty()) return BT_OK;
    if (a->tile_files == BT_TILE_FILES_PACKED) return update_packed(a, assets_root, max_loads, loaded, failed);  // "{coord}.btp", decoded on the device
    BT_HIP(hipSetDevice(a->ctx->device));
    uint64_t largest = 0;
    for (const Attachment& at : a->attachments) largest = std::max(largest, at.tile_bytes);
    const uint32_t chunk = uint32_t(std::max<uint64_t>(1, std::min<uint64_t>(64, (32ull << 20) / std::max<uint64_t>(largest, 1))));
    StagingRing& ring = a->ctx->staging;
    if (bt_status s = ring.reserve(std::max<size_t>(32ull << 20, largest))) return s;
    if (bt_status s = ring.wait(0)) return s;
    void* pinned = ring.buffer(0);  // the one buffer this call uses, synchronously
    std::vector<std::vector<uint32_t>> mip_layers(a->attachments.size());
    uint32_t budget = max_loads ? max_loads : 0xFFFFFFFFu, done = 0, bad = 0;
    bt_status rc = BT_OK;
    while (!a->to_load.empty() && budget && rc == BT_OK) {
        std::vector<AtlasTileAttachment> batch;
        while (!a->to_load.empty() && budget && batch.size() < chunk) {
            batch.push_back(a->to_load.front());
            a->to_load.pop_front();
            budget--;
        }
        std::vector<bool> ok(batch.size(), false);
        for (size_t k = 0; k < batch.size(); k++) {
            const AtlasTileAttachment& t = batch[k];
            const Attachment& at = a->attachments[t.attachment_index];
            char name[64];
            bt_tile_name(t.coordinate, name, sizeof name);
            const std::string path = std::string(assets_root) + "/" + a->config.path + "/data/" + at.cfg.name + "/" + name + ".bin";
            FILE* f = fopen(path.c_str(), "rb");
            if (!f) continue;  // the reference returns the load slot and leaves the tile Loading (:202-204)
            const size_t got = fread((uint8_t*)pinned + largest * k, 1, at.tile_bytes, f);
            const bool longer = got == at.tile_bytes && fgetc(f) != EOF;
            fclose(f);
            ok[k] = got == at.tile_bytes && !longer;
        }
        for (size_t k = 0; k < batch.size() && rc == BT_OK; k++) {
            if (!ok[k]) {
                bad++;
                continue;
            }
            const AtlasTileAttachment& t = batch[k];
            Attachment& at = a->attachments[t.attachment_index];
            at.mark_written(t.atlas_index, 1);
            hipError_t e = hipMemcpyAsync((uint8_t*)at.level0 + at.tile_bytes * t.atlas_index, (const uint8_t*)pinned + largest * k, at.tile_bytes,
                                          hipMemcpyHostToDevice, a->ctx->stream);
            if (e != hipSuccess) rc = hip_fail(e, "tile upload");
        }
        if (rc != BT_OK) ring.record(0, a->ctx->stream);  // (the copies before the failed one are on their way)
        if (rc == BT_OK) {
            hipError_t e = hipStreamSynchronize(a->ctx->stream);  // the pinned buffer is refilled next
            if (e != hipSuccess) rc = hip_fail(e, "tile upload");
        }
        for (size_t k = 0; k < batch.size() && rc == BT_OK; k++) {
            if (!ok[k]) continue;
            const AtlasTileAttachment& t = batch[k];
            // loaded_tile_attachment (:347-359); a slot that was reused for another tile meanwhile is ignored
            auto it = a->tile_states.find(t.coordinate);
            if (it == a->tile_states.end() || it->second.atlas_index != t.atlas_index || it->second.loading == 0) continue;
            if (--it->second.loading == 0) a->state_version++;
            mip_layers[t.attachment_index].push_back(t.atlas_index);
            done++;
        }
    }
    for (uint32_t ai = 0; ai < a->attachments.size() && rc == BT_OK; ai++) rc = mip_filled_layers(a, ai, mip_layers[ai]);
    if (loaded) *loaded = done;
    if (failed) *failed = bad;
    return rc;
}

}  // extern "C"

// Tile files: the writer / reader threads, the download-and-write pipeline of the save path, and the time stamps of the profiling build.
#include <fcntl.h>
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
    for (uint32_t k = 0; k < kBuffers; k++)
        if (copied_[k]) hipEventDestroy(copied_[k]);
}

bt_status TileSaver::begin() {
    BT_HIP(hipSetDevice(a_->ctx->device));
    size_t largest = 32ull << 20;
    for (const Attachment& at : a_->attachments) largest = std::max<size_t>(largest, at.tile_bytes);
    if (bt_status s = ctx_staging(a_->ctx, largest)) return s;
    for (uint32_t k = 0; k < kBuffers; k++) {
        hipError_t e = hipEventCreateWithFlags(&copied_[k], hipEventDisableTiming);
        if (e != hipSuccess) return hip_fail(e, "save events");
    }
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
    void** pinned = a_->ctx->staging;
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
        trace_stamp("  saver chunk: buffer free", k);
        // runs of consecutive layers; equally long runs at a constant layer stride (a band of tile rows in the x-major
        // atlas order: 4 layers every 32) travel as ONE pitched copy instead of one call per run
        std::vector<std::pair<size_t, size_t>> runs;  // (first tile of the chunk, length)
        for (size_t i = lo; i < hi;) {
            size_t run = 1;
            while (i + run < hi && tiles[i + run].first == tiles[i].first + run) run++;
            runs.push_back({i, run});
            i += run;
        }
        bool regular = runs.size() >= 2;
        const uint64_t stride = regular ? uint64_t(tiles[runs[1].first].first) - tiles[runs[0].first].first : 0;
        for (size_t q = 1; regular && q < runs.size(); q++)
            regular = runs[q].second == runs[0].second && uint64_t(tiles[runs[q].first].first) - tiles[runs[q - 1].first].first == stride;
        if (regular) {
            hipError_t e = hipMemcpy2DAsync(pinned[k], at.tile_bytes * runs[0].second, (const uint8_t*)at.level0 + at.tile_bytes * tiles[lo].first,
                                            at.tile_bytes * stride, at.tile_bytes * runs[0].second, runs.size(), hipMemcpyDeviceToHost, stream_);
            if (e != hipSuccess) return hip_fail(e, "tile download");
        } else if (runs.size() > 2 && hi - lo <= 64 && at.tile_bytes % 16u == 0) {
            // an irregular chunk (the lower LODs behind a band's tiles, a cube's face-edge tiles, merged hand-overs): ONE gather kernel that
            // writes the pinned buffer over PCIe instead of one copy-engine call per run — a burst of small copy calls stalled the issuing
            // thread for 15 - 20 ms now and then (config 2's 37-tile chunk: 2.2 -> 21.0 ms between two stamps, round 6 traces), the kernel never
            uint32_t layers[64];
            for (size_t i = lo; i < hi; i++) layers[i - lo] = tiles[i].first;
            if (bt_status s = launch_gather_layers(stream_, at.level0, layers, uint32_t(hi - lo), pinned[k], at.tile_bytes)) return s;
        } else {
            for (const auto& [i, run] : runs) {
                hipError_t e = hipMemcpyAsync((uint8_t*)pinned[k] + at.tile_bytes * (i - lo), (const uint8_t*)at.level0 + at.tile_bytes * tiles[i].first,
                                              at.tile_bytes * run, hipMemcpyDeviceToHost, stream_);
                if (e != hipSuccess) return hip_fail(e, "tile download");
            }
        }
        hipError_t e = hipEventRecord(copied_[k], stream_);
        if (e != hipSuccess) return hip_fail(e, "tile download");
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
    hipError_t e = hipEventSynchronize(copied_[in_flight_buffer_]);
    if (e != hipSuccess) return hip_fail(e, "tile download");
    std::vector<FileWriters::Job> jobs;
    for (size_t i = 0; i < in_flight_.size(); i++) {
        char name[64];
        bt_tile_name(in_flight_[i].second, name, sizeof name);
        jobs.push_back({in_flight_dir_ + "/" + name + ".bin", (const uint8_t*)a_->ctx->staging[in_flight_buffer_] + at.tile_bytes * i, size_t(at.tile_bytes), in_flight_buffer_});
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

// Tile files (bt_tile_io.cpp, which also holds the load paths): the writer / reader threads and the saver, shared by the save path, the
// load paths and the streamed run (bt_stream.cpp), and the file-system helpers of whoever writes beside the tiles.
#pragma once

#include <condition_variable>
#include <memory>
#include <mutex>
#include <thread>

#include "bt_internal.hpp"

namespace bt {

#ifdef BT_DEBUG_HOOKS
// tools build: BT_STREAM_TRACE=1 prints host time stamps of the streamed run's launcher, its saver thread and the TileSaver underneath
void trace_start();  // reads the switch and restarts the clock: once per streamed run
void trace_stamp(const char* what, size_t k);
#else
inline void trace_start() {}
inline void trace_stamp(const char*, size_t) {}
#endif

// fs::write for a batch of files on a few threads (the reference spawns one AsyncComputeTaskPool task per tile,
// tile_atlas.rs:77-116): jobs are (path, bytes) pairs; a chunk's pinned buffer is reused once its jobs are done.
class FileWriters {
  public:
    struct Job {
        std::string path;
        const uint8_t* data;
        size_t bytes;
        uint32_t buffer;
        bool read = false;  // fill `data` from the file, which must hold exactly `bytes` (tile load path)
    };
    FileWriters(uint32_t threads, uint32_t buffers) : pending_(buffers, 0) {
        for (uint32_t i = 0; i < threads; i++) workers_.emplace_back([this] { run(); });
    }
    ~FileWriters() {
        {
            std::lock_guard<std::mutex> lock(m_);
            stop_ = true;
        }
        cv_.notify_all();
        for (std::thread& t : workers_) t.join();
    }
    void push(std::vector<Job>&& jobs) {
        {
            std::lock_guard<std::mutex> lock(m_);
            for (Job& j : jobs) {
                pending_[j.buffer]++;
                queue_.push_back(std::move(j));
            }
        }
        cv_.notify_all();
    }
    void wait_buffer(uint32_t buffer) {
        std::unique_lock<std::mutex> lock(m_);
        done_.wait(lock, [&] { return pending_[buffer] == 0; });
    }
    bt_status status() {
        std::lock_guard<std::mutex> lock(m_);
        if (failed_) set_error("%s", error_.c_str());
        return failed_ ? BT_ERR_IO : BT_OK;
    }

  private:
    void run();
    std::mutex m_;
    std::condition_variable cv_, done_;
    std::deque<Job> queue_;
    std::vector<uint32_t> pending_;
    std::vector<std::thread> workers_;
    bool stop_ = false, failed_ = false;
    std::string error_;
};

// Download + write tiles: D2H through the context's staging ring on `stream` (runs of consecutive layers are one copy), files written by
// the writer threads while the next chunk downloads.  add() may be called many times (the streamed run hands over band after band,
// attachment after attachment); the tiles of one add() are written in atlas-index order.
class TileSaver {
  public:
    typedef std::vector<std::pair<uint32_t, bt_tile_coordinate>> Tiles;
    TileSaver(bt_atlas* a, hipStream_t stream) : a_(a), stream_(stream) {}
    ~TileSaver();
    bt_status begin();
    // taper: the call's last tiles travel in shrinking chunks (half of what is left, down to 8 tiles) — full-size chunks keep the
    // copy engine at its rate, the small ones at the very end shorten the writers' tail behind the last copy
    bt_status add(uint32_t ai, const std::string& dir, Tiles tiles, bool taper = false);
    bt_status finish();
    uint64_t saved_bytes() const { return saved_bytes_; }

  private:
    static constexpr uint32_t kBuffers = StagingRing::kBuffers;
    bt_status hand_over();
    bt_atlas* a_;
    hipStream_t stream_;
    size_t chunks_ = 0;
    std::unique_ptr<FileWriters> writers_;
    std::vector<std::string> dirs_;  // directories that exist by now
    Tiles in_flight_;
    uint32_t in_flight_buffer_ = 0, in_flight_ai_ = 0;
    std::string in_flight_dir_;
    bool have_in_flight_ = false;
    uint64_t saved_bytes_ = 0;
};

bt_status save_tiles(bt_atlas* a, uint32_t ai, const char* directory, TileSaver::Tiles tiles);

// the tail of every load path (bt_tile_io.cpp): these layers of attachment `ai` have been filled; one mip-chain pass per run of consecutive layers (sorts the list)
bt_status mip_filled_layers(bt_atlas* a, uint32_t ai, std::vector<uint32_t>& layers);
// bt_atlas_update while the atlas reads packed tile files (bt_pack.cpp)
bt_status update_packed(bt_atlas* a, const char* assets_root, uint32_t max_loads, uint32_t* loaded, uint32_t* failed);

bt_status make_dirs(const std::string& dir);  // mkdir -p
bt_status write_file(const std::string& path, const void* data, size_t bytes);
void remove_tree(const std::string& dir);  // rm -r; a directory that does not exist is fine

}  // namespace bt

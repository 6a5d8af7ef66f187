// The two rings of pinned memory a context owns (bt_staging.cpp): the staging ring of every chunked transfer between host memory and the device, and the
// plan ring of the edit calls' records.  A part of bt_internal.hpp, which includes it between bt::Scratch and bt_ctx: include that.
#pragma once

namespace bt {

// Three pinned buffers of one size and one event each, allocated on first use (pinning 100 MB costs tens of milliseconds) and kept until bt_ctx_trim; the
// events live until bt_ctx_destroy.  ONE RULE for every user: wait(k) before the host or a copy touches buffer k, record(k, stream) after enqueuing the copies
// that use it; only reserve() replaces the buffers, after waiting for all three.  wait() is an event wait on the host, so it does not matter which stream
// recorded.  A copy that an error path leaves in flight is therefore harmless: it is recorded, and the next wait(k) or reserve(), of this call or of any later
// one, covers it.  One thread at a time uses the ring (a streamed run's saver thread is its only user while the run lasts): there is no lock.
class StagingRing {
  public:
    static constexpr uint32_t kBuffers = 3;
    // Nothing happens while each buffer holds at_least bytes.  Smaller ones are replaced by buffers of max(at_least, grow_to) bytes
    bt_status reserve(size_t at_least, size_t grow_to = 0);
    void* buffer(uint32_t k) const { return buffers_[k]; }
    size_t bytes() const { return bytes_; }  // per buffer
    bt_status wait(uint32_t k) {  // what was last recorded on buffer k has run; nothing recorded since the last wait: returns at once
        if (recorded_[k]) BT_HIP(hipEventSynchronize(events_[k]));
        recorded_[k] = false;
        return BT_OK;
    }
    bt_status record(uint32_t k, hipStream_t stream) {
        BT_HIP(hipEventRecord(events_[k], stream));
        recorded_[k] = true;
        return BT_OK;
    }
    bt_status drain() {  // every buffer is waited for, the first failure is returned
        const bt_status a = wait(0), b = wait(1), c = wait(2);
        return a ? a : b ? b : c;
    }
    // waits for the events, frees the buffers and, with destroy_events, the events; returns the bytes given back (bytes() per buffer that existed); *error keeps the first failure
    uint64_t release(bool destroy_events, hipError_t* error = nullptr);

  private:
    void* buffers_[kBuffers] = {};
    size_t bytes_ = 0;
    hipEvent_t events_[kBuffers] = {};
    bool recorded_[kBuffers] = {};
};

// `chunks` chunks from the device through the ring to the host, three in flight.  enqueue(i, k): enqueue chunk i's way into buffer(k) on `stream` (a kernel
// first, if the chunk has to be made), a hipError_t that a failure reports under `what`; landed(i, k): chunk i is in buffer(k), hand it over.  Chunk i uses
// buffer i % 3 once chunk i - 3 has been handed over; what is left at the end is handed over oldest first.  A failure drains the ring
template <typename Enqueue, typename Landed>
bt_status stage_out_chunks(StagingRing& ring, hipStream_t stream, uint32_t chunks, const char* what, Enqueue enqueue, Landed landed) {
    bt_status rc = BT_OK;
    for (uint64_t i = 0; i < uint64_t(chunks) + StagingRing::kBuffers && rc == BT_OK; i++) {
        const uint32_t k = uint32_t(i % StagingRing::kBuffers);
        if ((rc = ring.wait(k)) != BT_OK) break;
        if (i >= StagingRing::kBuffers) landed(uint32_t(i - StagingRing::kBuffers), k);
        if (i >= chunks) continue;
        const hipError_t e = enqueue(uint32_t(i), k);
        rc = ring.record(k, stream);  // (behind a failed enqueue too: part of it may be on its way)
        if (e != hipSuccess) rc = hip_fail(e, what);
    }
    if (rc != BT_OK) ring.drain();
    return rc;
}

// The plans (items, stamps, stitch tasks; scatter records, windows) of the edit calls and bounds updates in flight: a scratch with its pinned twin, handed
// out front to back as a ring (kept until bt_ctx_trim: release() gives back 2 * bytes).  A call's records must stay in the pinned half until its copy has
// run: `copied` is recorded behind each call's copy and waited for when the ring wraps.  Only PlanRing::commit hands it out
struct PlanRingState : Scratch {
    uint64_t used = 0;  // of each half
    hipEvent_t copied = nullptr;
};

// The records of one call (an edit's plan, a bounds update's) on their way through the context's plan ring (bt_ctx::plan_ring).
// add() the host records, each 16-byte aligned; then, optionally, device_only() bytes behind them; every offset returned is relative to the device base
// commit() hands back.  commit(), once: reserves pinned and device bytes of the ring, copies the records (they must still be where
// add() saw them) into the pinned half, enqueues the ONE copy to the device half on the context's stream and records the ring's event
// behind it, which the ring waits for before it wraps onto pinned records.
class PlanRing {
  public:
    uint64_t add(const void* src, uint64_t bytes);
    template <typename T>
    uint64_t add(const std::vector<T>& v) { return add(v.data(), v.size() * sizeof(T)); }
    uint64_t device_only(uint64_t bytes) { return add(nullptr, bytes); }  // after the last add() of a host record
    bt_status commit(bt_ctx* ctx, uint8_t** dev);

  private:
    struct Record {
        const void* src;  // NULL: device only
        uint64_t bytes, at;
    };
    std::vector<Record> records;
    uint64_t size = 0, upload = 0;  // of all records; of those up to the last host record: what the copy moves
};

}  // namespace bt

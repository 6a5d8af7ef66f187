// The context's staging ring and plan ring (bt_staging.hpp).
#include <cstring>

#include "bt_internal.hpp"

namespace bt {

bt_status StagingRing::reserve(size_t at_least, size_t grow_to) {
    for (hipEvent_t& ev : events_)
        if (!ev) BT_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    if (buffers_[0] && bytes_ >= at_least) return BT_OK;
    hipError_t e = hipSuccess;
    release(false, &e);  // (waits for all three events first)
    for (void*& p : buffers_)
        if (e == hipSuccess) e = hipHostMalloc(&p, std::max(at_least, grow_to), hipHostMallocDefault);
    if (e != hipSuccess) return hip_fail(e, "pinned staging buffers");  // (bytes_ is 0: the next reserve starts over)
    bytes_ = std::max(at_least, grow_to);
    return BT_OK;
}

uint64_t StagingRing::release(bool destroy_events, hipError_t* error) {
    hipError_t e = hipSuccess;
    uint64_t freed = 0;
    for (uint32_t k = 0; k < kBuffers; k++) {
        if (recorded_[k] && e == hipSuccess) e = hipEventSynchronize(events_[k]);  // no copy may be in flight when the buffer goes away
        if (buffers_[k] && e == hipSuccess) e = hipHostFree(buffers_[k]);
        if (buffers_[k]) freed += bytes_;
        if (destroy_events && events_[k]) hipEventDestroy(events_[k]), events_[k] = nullptr;
        buffers_[k] = nullptr, recorded_[k] = false;
    }
    bytes_ = 0;
    if (error && *error == hipSuccess) *error = e;
    return freed;
}

uint64_t PlanRing::add(const void* src, uint64_t bytes) {
    records.push_back({src, bytes, size});
    size += (bytes + 15u) & ~uint64_t(15);
    if (src) upload = size;
    return records.back().at;
}

bt_status PlanRing::commit(bt_ctx* ctx, uint8_t** dev) {
    PlanRingState& ring = ctx->plan_ring;
    const uint64_t need = (size + 255u) & ~uint64_t(255);
    if (!ring.copied) BT_HIP(hipEventCreateWithFlags(&ring.copied, hipEventDisableTiming));
    if (need > ring.bytes) {  // (the reserve waits for the stream: launches in flight read the buffers that go away)
        if (bt_status s = ring.reserve(ctx, std::max<uint64_t>(1ull << 20, 2u * need), true)) return s;
        ring.used = 0;
    }
    if (ring.used + need > ring.bytes) {
        // the ring wraps: the pinned records of earlier calls must have been copied (their device halves are safe: this call's copy and
        // kernels are ordered behind theirs on the stream)
        BT_HIP(hipEventSynchronize(ring.copied));
        ring.used = 0;
    }
    uint8_t* host = (uint8_t*)ring.host + ring.used;
    *dev = (uint8_t*)ring.dev + ring.used;
    ring.used += need;
    for (const Record& r : records)
        if (r.src && r.bytes) memcpy(host + r.at, r.src, r.bytes);
    BT_HIP(hipMemcpyAsync(*dev, host, upload, hipMemcpyHostToDevice, ctx->stream));
    BT_HIP(hipEventRecord(ring.copied, ctx->stream));  // what the wrap of a later call waits for
    return BT_OK;
}

}  // namespace bt

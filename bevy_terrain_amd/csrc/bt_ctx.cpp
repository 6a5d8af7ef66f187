// The context: the calling thread's error text, bt_ctx and what it owns (stream, timer events, pinned staging buffers, the scratch of the
// query calls), the thread count of the file paths, and the device-memory helpers of the ABI.
#include <sched.h>

#include <algorithm>
#include <cerrno>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <thread>

#include "bt_internal.hpp"

namespace bt {

static thread_local char g_error[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
}

bt_status hip_fail(hipError_t e, const char* what) {
    set_error("HIP error %d (%s) in %s", int(e), hipGetErrorString(e), what);
    return BT_ERR_DEVICE;
}

// CPUs this process may use: the scheduler's affinity mask, capped by the cgroup's CPU quota (cgroup v2 cpu.max, v1 cfs quota) — a
// container on a 256-thread host may own 16 of them, and std::thread::hardware_concurrency() reports the host's
uint32_t usable_cpus() {
    uint32_t n = 0;
    // (a dynamically sized mask: the fixed cpu_set_t holds 1024 CPUs and sched_getaffinity fails with EINVAL on a larger host)
    for (size_t cpus = 1024; cpus <= (1u << 20) && n == 0; cpus *= 4) {
        cpu_set_t* set = CPU_ALLOC(cpus);
        if (!set) break;
        const size_t bytes = CPU_ALLOC_SIZE(cpus);
        CPU_ZERO_S(bytes, set);
        const int rc = sched_getaffinity(0, bytes, set);
        if (rc == 0) n = uint32_t(CPU_COUNT_S(bytes, set));
        CPU_FREE(set);
        if (rc != 0 && errno != EINVAL) break;
    }
    if (n == 0) n = std::max(1u, std::thread::hardware_concurrency());
    auto quota_from = [](const std::string& path, const std::string& period_path) -> double {
        FILE* f = fopen(path.c_str(), "r");
        if (!f) return 0.0;
        char a[64] = "", b2[64] = "";
        const int got = fscanf(f, "%63s %63s", a, b2);
        fclose(f);
        if (got < 1 || !strcmp(a, "max")) return 0.0;
        double quota = atof(a), period = got >= 2 ? atof(b2) : 0.0;
        if (!period_path.empty()) {
            FILE* g = fopen(period_path.c_str(), "r");
            if (g) {
                if (fscanf(g, "%63s", b2) == 1) period = atof(b2);
                fclose(g);
            }
        }
        return quota > 0.0 && period > 0.0 ? quota / period : 0.0;
    };
    // The process's OWN cgroup (/proc/self/cgroup): without a cgroup namespace — a systemd slice, some Kubernetes set-ups — the quota sits in
    // a nested directory, not at the mount's root; every ancestor's quota applies, the smallest wins.  v2: "0::/path"; v1: "N:cpu,cpuacct:/path".
    std::string v2_path, v1_path;
    if (FILE* f = fopen("/proc/self/cgroup", "r")) {
        char line[1024];
        while (fgets(line, sizeof line, f)) {
            std::string l(line);
            while (!l.empty() && (l.back() == '\n' || l.back() == '\r')) l.pop_back();
            const size_t c1 = l.find(':'), c2 = c1 == std::string::npos ? c1 : l.find(':', c1 + 1);
            if (c2 == std::string::npos) continue;
            const std::string controllers = l.substr(c1 + 1, c2 - c1 - 1), path = l.substr(c2 + 1);
            if (controllers.empty()) v2_path = path;
            else if (("," + controllers + ",").find(",cpu,") != std::string::npos) v1_path = path;
        }
        fclose(f);
    }
    double q = 0.0;
    auto walk = [&](const std::string& root, std::string path, const char* file, const char* period_file) {
        for (;;) {  // the cgroup itself, then every ancestor up to the mount's root
            const std::string dir = root + (path == "/" ? "" : path);
            const double v = quota_from(dir + "/" + file, period_file ? dir + "/" + period_file : std::string());
            if (v > 0.0 && (q <= 0.0 || v < q)) q = v;
            if (path.empty() || path == "/") break;
            const size_t cut = path.find_last_of('/');
            path = cut == 0 || cut == std::string::npos ? "/" : path.substr(0, cut);
        }
    };
    walk("/sys/fs/cgroup", v2_path.empty() ? "/" : v2_path, "cpu.max", nullptr);
    if (q <= 0.0) walk("/sys/fs/cgroup/cpu", v1_path.empty() ? "/" : v1_path, "cpu.cfs_quota_us", "cpu.cfs_period_us");
    if (q > 0.0) n = std::min(n, std::max(1u, uint32_t(q + 0.999)));
    return n;
}

// Writer / reader threads of the save and load paths.  Automatic: min(16, usable CPUs) — on tmpfs and the overlay disk 6 / 8 / 12 / 16 /
// 24 / 32 / 64 threads write at 29 / 34 / 42 / 46-49 / 46 / 35 / 4 GB/s on a 16-CPU quota (beyond ~24 the page-cache allocation lock
// dominates): the threads mostly sleep in the kernel's copy, so the quota itself, not quota - 2, is the optimum there.
uint32_t ctx_io_threads(const bt_ctx* ctx) {
    if (ctx->io_threads) return ctx->io_threads;
    return std::max(1u, std::min(16u, usable_cpus()));
}

bt_status Scratch::reserve(bt_ctx* ctx, uint64_t need, bool with_pinned_twin) {
    if (bytes >= need) return BT_OK;
    if (dev) BT_HIP(hipStreamSynchronize(ctx->stream));  // work in flight may use the buffer that goes away
    hipError_t e = hipSuccess;
    release(&e);
    if (e == hipSuccess) e = hipMalloc(&dev, need);
    if (e == hipSuccess && with_pinned_twin) e = hipHostMalloc(&host, need, hipHostMallocDefault);
    if (e != hipSuccess) {
        release();
        return hip_fail(e, "scratch buffer");
    }
    bytes = need;
    return BT_OK;
}

uint64_t Scratch::release(hipError_t* error) {
    const hipError_t d = dev ? hipFree(dev) : hipSuccess, h = host ? hipHostFree(host) : hipSuccess;
    const uint64_t freed = (dev ? bytes : 0u) + (host ? bytes : 0u);
    *this = Scratch{};
    if (error && *error == hipSuccess) *error = d != hipSuccess ? d : h;
    return freed;
}

}  // namespace bt

using namespace bt;

extern "C" {

uint32_t bt_abi_version(void) { return BT_ABI_VERSION; }
const char* bt_last_error(void) { return g_error; }

bt_status bt_ctx_create(int32_t device, void* stream, bt_ctx** out) {
    if (!out) return BT_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    int count = 0;
    BT_HIP(hipGetDeviceCount(&count));
    if (device < 0 || device >= count) {
        set_error("device %d out of range (%d visible)", device, count);
        return BT_ERR_INVALID_ARGUMENT;
    }
    BT_HIP(hipSetDevice(device));
    bt_ctx* ctx = new bt_ctx();
    ctx->device = device;
    if (stream) {
        ctx->stream = hipStream_t(stream);
    } else {
        hipError_t e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
        if (e != hipSuccess) {
            delete ctx;
            return hip_fail(e, "hipStreamCreateWithFlags");
        }
        ctx->own_stream = true;
    }
    hipEventCreate(&ctx->ev_begin);
    hipEventCreate(&ctx->ev_end);
    *out = ctx;
    return BT_OK;
}

void bt_ctx_destroy(bt_ctx* ctx) {
    if (!ctx) return;
    hipSetDevice(ctx->device);
    ctx->staging.release(true);
    if (ctx->ev_begin) hipEventDestroy(ctx->ev_begin);
    if (ctx->ev_end) hipEventDestroy(ctx->ev_end);
    if (ctx->own_stream && ctx->stream) hipStreamDestroy(ctx->stream);
    for (auto& kept : ctx->spare_rasters) hipFree(kept.first);
    for (bt::Scratch* s : ctx->scratch()) s->release();
    ctx->plan_ring.release();
    if (ctx->plan_ring.copied) hipEventDestroy(ctx->plan_ring.copied);
    if (ctx->copy_stream) hipStreamDestroy(ctx->copy_stream);
    if (ctx->save_stream) hipStreamDestroy(ctx->save_stream);
    delete ctx;
}

bt_status bt_ctx_set_stream(bt_ctx* ctx, void* stream) {
    if (!ctx) return BT_ERR_INVALID_ARGUMENT;
    // work queued on the outgoing stream (bt_atlas_create's zeroing memset, which a prev_zero launch relies on without reading the layer) is
    // not ordered before the new stream's: finish it first
    BT_HIP(hipSetDevice(ctx->device));
    if (ctx->stream) BT_HIP(hipStreamSynchronize(ctx->stream));
    if (ctx->own_stream && ctx->stream) hipStreamDestroy(ctx->stream);
    ctx->own_stream = false;
    ctx->stream = hipStream_t(stream);
    return BT_OK;
}

void* bt_ctx_stream(const bt_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

bt_status bt_ctx_synchronize(bt_ctx* ctx) {
    if (!ctx) return BT_ERR_INVALID_ARGUMENT;
    BT_HIP(hipSetDevice(ctx->device));
    BT_HIP(hipStreamSynchronize(ctx->stream));
    return BT_OK;
}

bt_status bt_ctx_trim(bt_ctx* ctx, uint64_t* freed_bytes) {
    if (!ctx) return BT_ERR_INVALID_ARGUMENT;
    BT_HIP(hipSetDevice(ctx->device));
    BT_HIP(hipStreamSynchronize(ctx->stream));
    if (ctx->copy_stream) BT_HIP(hipStreamSynchronize(ctx->copy_stream));
    if (ctx->save_stream) BT_HIP(hipStreamSynchronize(ctx->save_stream));
    uint64_t freed = 0;
    for (auto& kept : ctx->spare_rasters) {
        BT_HIP(hipFree(kept.first));
        freed += kept.second;
    }
    ctx->spare_rasters.clear();
    hipError_t failed = hipSuccess;
    freed += ctx->staging.release(false, &failed);  // (the events stay until bt_ctx_destroy)
    for (bt::Scratch* s : ctx->scratch()) freed += s->release(&failed);
    freed += ctx->plan_ring.release(&failed);
    BT_HIP(failed);
    if (freed_bytes) *freed_bytes = freed;
    return BT_OK;
}

bt_status bt_ctx_set_io_threads(bt_ctx* ctx, uint32_t threads) {
    if (!ctx || threads > 256u) return BT_ERR_INVALID_ARGUMENT;
    ctx->io_threads = threads;
    return BT_OK;
}

uint32_t bt_ctx_io_threads(const bt_ctx* ctx) { return ctx ? bt::ctx_io_threads(ctx) : 0u; }

bt_status bt_ctx_timer_begin(bt_ctx* ctx) {
    if (!ctx) return BT_ERR_INVALID_ARGUMENT;
    BT_HIP(hipEventRecord(ctx->ev_begin, ctx->stream));
    return BT_OK;
}

bt_status bt_ctx_timer_end(bt_ctx* ctx, float* elapsed_ms) {
    if (!ctx || !elapsed_ms) return BT_ERR_INVALID_ARGUMENT;
    BT_HIP(hipEventRecord(ctx->ev_end, ctx->stream));
    BT_HIP(hipEventSynchronize(ctx->ev_end));
    BT_HIP(hipEventElapsedTime(elapsed_ms, ctx->ev_begin, ctx->ev_end));
    return BT_OK;
}

bt_status bt_device_malloc(bt_ctx* ctx, size_t bytes, void** out) {
    if (!ctx || !out) return BT_ERR_INVALID_ARGUMENT;
    BT_HIP(hipSetDevice(ctx->device));
    BT_HIP(hipMalloc(out, bytes ? bytes : 1));
    return BT_OK;
}

bt_status bt_device_free(bt_ctx* ctx, void* ptr) {
    if (!ctx) return BT_ERR_INVALID_ARGUMENT;
    BT_HIP(hipSetDevice(ctx->device));
    BT_HIP(hipFree(ptr));
    return BT_OK;
}

bt_status bt_memcpy_h2d(bt_ctx* ctx, void* dst, const void* src, size_t bytes) {
    if (!ctx) return BT_ERR_INVALID_ARGUMENT;
    BT_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    BT_HIP(hipStreamSynchronize(ctx->stream));
    return BT_OK;
}

bt_status bt_memcpy_d2h(bt_ctx* ctx, void* dst, const void* src, size_t bytes) {
    if (!ctx) return BT_ERR_INVALID_ARGUMENT;
    BT_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    BT_HIP(hipStreamSynchronize(ctx->stream));
    return BT_OK;
}

}  // extern "C"

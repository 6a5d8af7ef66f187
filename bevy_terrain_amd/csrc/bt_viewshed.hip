// bt_atlas_viewshed: the kernels.  The host half is bt_viewshed.cpp; the definition is the VIEWSHED section of include/bevy_terrain_amd.h.
//
// viewshed_transpose_kernel   raw -> the same texels with the axes exchanged, through a 32 x 32 tile of LDS.
// viewshed_walk_kernel<X>     the line walk.  A wave owns 64 consecutive targets along the minor axis of one line of the major axis: a column
//                             of the window for the x-major lines (<true>, launched first, reading the transposed plane), a row for the
//                             y-major ones (<false>, reading the plane as it lies).  For one observer all its lanes share n, j and the trip
//                             count, and at step j they read one line of the plane within a span of 65 texels.  A lane whose line is of the
//                             other class is idle.  The observers are looped inside the wave and the minimum, the count and the mask are
//                             kept in registers: the first launch writes every cell, the second one reads what the first left and adds its
//                             own.  No atomic, and no result depends on a schedule.  27 VGPRs, no scratch.  Against a lane per target in
//                             row-major order on the plane as it lies, whose lanes differ in n and read up to 64 rows a step: 2.7 times
//                             faster on 2048 x 2048 (profiles/viewshed.txt), which is why that simpler form is not the one here.
// viewshed_finish_kernel      the counts of bt_viewshed_stats: integer sums and a maximum, folded per workgroup and added atomically, which
//                             is independent of the order.
//
// Everything is integer arithmetic.  The sample loop holds no division: q and r advance by a DDA, the largest S_j / j is kept as a pair and
// found by cross-multiplication of 32-bit factors, and the one division per line is the final ceiling.
#include "bt_internal.hpp"

namespace bt {

namespace {

constexpr uint32_t kViewshedThreads = 256;
constexpr uint32_t kWave = 64;
constexpr uint32_t kTransposeTile = 32;
constexpr uint32_t kFinishCells = 4;  // of one thread of the finish kernel
constexpr uint32_t kNone = BT_VIEWSHED_NONE;

// C_o(T) of the header for a line of n >= 0 steps.  z: a plane in which the observer sits at index `at`, one step of the major axis is
// major_step (signed) and one cell of the minor axis towards larger coordinates is minor_step.  m: the signed minor difference, |m| <= n.
// E: the eye; zt: z(T).
__device__ __forceinline__ uint32_t line_clearance(const uint16_t* __restrict__ z, uint32_t at, int32_t major_step, uint32_t minor_step, uint32_t n, int32_t m, uint32_t E,
                                                   uint32_t zt) {
    if (n <= 1u) return 0u;
    const uint32_t En = E * n;  // < 2^32: E < 2^17, n < 2^15; and > 0: the observer's cell is active
    int32_t r = 0;
    uint32_t Gb = 0u, jb = 0u;  // the largest (G_j - En) / j so far; jb = 0: none yet, and then the test below holds since En j > 0
    for (uint32_t j = 1u; j < n; j++) {
        at += uint32_t(major_step);
        r += m;  // |m| <= n: one of the two corrections at most
        if (r >= int32_t(n)) r -= int32_t(n), at += minor_step;
        if (r < 0) r += int32_t(n), at -= minor_step;
        const uint32_t za = z[at], zb = z[r ? at + minor_step : at];       // z_b has the weight 0 when r == 0, and may lie outside
        const uint32_t G = __umul24(za, n - uint32_t(r)) + __umul24(zb, uint32_t(r));  // < 2^31
        // S_j jb > S_b j with S = G - En, brought to unsigned terms (j > jb); each product < 2^47
        if (uint64_t(G) * jb + uint64_t(En) * (j - jb) > uint64_t(Gb) * j) Gb = G, jb = j;
    }
    const int64_t S = int64_t(Gb) - int64_t(En);  // in (-2^32, 2^31)
    const int64_t M = S >= 0 ? int64_t((uint32_t(S) + jb - 1u) / jb) : -int64_t(uint32_t(-S) / jb);  // the ceiling, towards +inf
    const int64_t C = int64_t(E) + M - int64_t(zt);
    return C > 0 ? uint32_t(C) : 0u;
}

__device__ __forceinline__ bool covers(const bt_viewshed_observer& o, int32_t dx, int32_t dy) {
    return o.radius == 0u || uint64_t(uint32_t(dx * dx) + uint32_t(dy * dy)) <= uint64_t(o.radius) * o.radius;  // dx^2 + dy^2 < 2^31
}

__device__ __forceinline__ uint32_t abs_u(int32_t v) { return uint32_t(v < 0 ? -v : v); }

__global__ __launch_bounds__(kTransposeTile * 8) void viewshed_transpose_kernel(ViewshedPlanes p) {
    __shared__ uint16_t tile[kTransposeTile][kTransposeTile + 1];
    const uint32_t bx = blockIdx.x * kTransposeTile, by = blockIdx.y * kTransposeTile;
    for (uint32_t k = threadIdx.y; k < kTransposeTile; k += 8u) {
        const uint32_t x = bx + threadIdx.x, y = by + k;
        if (x < p.width && y < p.height) tile[k][threadIdx.x] = p.raw[uint64_t(y) * p.width + x];
    }
    __syncthreads();
    for (uint32_t k = threadIdx.y; k < kTransposeTile; k += 8u) {
        const uint32_t x = bx + k, y = by + threadIdx.x;
        if (x < p.width && y < p.height) p.transposed[uint64_t(x) * p.height + y] = tile[threadIdx.x][k];
    }
}

// kXMajor: the major axis is x, a wave's line is a column and the plane is the transposed one; otherwise y, a row, the plane as it lies
template <bool kXMajor>
__global__ __launch_bounds__(kViewshedThreads) void viewshed_walk_kernel(ViewshedPlanes p) {
    const uint32_t major_len = kXMajor ? p.width : p.height, minor_len = kXMajor ? p.height : p.width;
    const uint16_t* __restrict__ z = kXMajor ? p.transposed : p.raw;  // cell (major, minor) at major * minor_len + minor
    const uint32_t chunks = (minor_len + kWave - 1u) / kWave;
    const uint32_t wave = blockIdx.x * (kViewshedThreads / kWave) + threadIdx.x / kWave;
    const uint32_t major = wave / chunks, minor = (wave % chunks) * kWave + threadIdx.x % kWave;
    if (major >= major_len) return;  // the whole wave
    const bool inside = minor < minor_len;
    const uint32_t zt = inside ? uint32_t(z[major * minor_len + minor]) : 0u;
    const bool live = zt != 0u;
    uint32_t best = kNone, count = 0u;
    uint64_t mask = 0u;
    bool any = false;
    for (uint32_t o = 0; o < p.observer_count; o++) {
        const bt_viewshed_observer& ob = p.observers[o];
        const uint32_t o_major = kXMajor ? ob.x : ob.y, o_minor = kXMajor ? ob.y : ob.x;
        const uint32_t at = o_major * minor_len + o_minor;
        const uint32_t zo = z[at];
        if (zo == 0u) continue;  // skipped: on a void cell
        const int32_t d_major = int32_t(major) - int32_t(o_major), d_minor = int32_t(minor) - int32_t(o_minor);
        const uint32_t n = abs_u(d_major);  // of every lane that works
        const bool mine = kXMajor ? abs_u(d_minor) <= n : abs_u(d_minor) < n;  // an exact diagonal is x-major
        if (!(live && mine && covers(ob, d_major, d_minor))) continue;  // the lane; a wave with no lane left goes on to the next observer
        const uint32_t E = zo + ob.eye_height;
        const uint32_t c = line_clearance(z, at, d_major < 0 ? -int32_t(minor_len) : int32_t(minor_len), 1u, n, d_minor, E, zt);
        any = true;
        best = min(best, c);
        if (c <= p.target_height) count++, mask |= uint64_t(1) << o;
    }
    if (!inside) return;
    const uint64_t i = kXMajor ? uint64_t(minor) * p.width + major : uint64_t(major) * p.width + minor;
    if (kXMajor) {  // the first launch: every cell
        p.clearance[i] = best;
        p.count[i] = uint8_t(count);
        if (p.mask) p.mask[i] = mask;
    } else if (any) {
        p.clearance[i] = min(p.clearance[i], best);
        if (count) {
            p.count[i] = uint8_t(p.count[i] + count);
            if (p.mask) p.mask[i] |= mask;
        }
    }
}

// the sum or the maximum of v over a workgroup, in thread 0; slot: four words of LDS of this fold's own
template <bool kMax>
__device__ __forceinline__ uint32_t group_fold(uint32_t v, uint32_t* slot) {
    for (int off = warpSize / 2; off > 0; off >>= 1) {
        const uint32_t o = __shfl_down(v, off);
        v = kMax ? max(v, o) : v + o;
    }
    if (threadIdx.x % kWave == 0u) slot[threadIdx.x / kWave] = v;
    __syncthreads();
    if (threadIdx.x != 0u) return 0u;
    for (uint32_t k = 1; k < kViewshedThreads / kWave; k++) v = kMax ? max(v, slot[k]) : v + slot[k];
    return v;
}

// A thread counts kFinishCells cells a workgroup's width apart, the workgroup folds, and its first thread adds to the counts: five atomics
// to a workgroup of 1024 cells
__global__ __launch_bounds__(kViewshedThreads) void viewshed_finish_kernel(ViewshedPlanes p, ViewshedCounts* __restrict__ counts) {
    __shared__ uint32_t slots[5][kViewshedThreads / kWave];
    const uint64_t cells = uint64_t(p.width) * p.height;
    uint32_t voids = 0u, covered = 0u, visible = 0u, clearance = 0u, samples = 0u;  // a cell's samples < 2^21, a workgroup's < 2^31
    for (uint32_t k = 0; k < kFinishCells; k++) {
        const uint64_t i = (uint64_t(blockIdx.x) * kFinishCells + k) * kViewshedThreads + threadIdx.x;
        if (i >= cells) break;
        voids += p.raw[i] == 0u;
        const uint32_t c = p.clearance[i];
        visible += p.count[i] != 0u;
        if (c == kNone) continue;  // void, or no used observer covers it
        covered++;
        clearance = max(clearance, c);
        const int32_t x = int32_t(i % p.width), y = int32_t(i / p.width);
        for (uint32_t o = 0; o < p.observer_count; o++) {
            const bt_viewshed_observer& ob = p.observers[o];
            if (p.raw[uint64_t(ob.y) * p.width + ob.x] == 0u) continue;
            const int32_t dx = x - int32_t(ob.x), dy = y - int32_t(ob.y);
            const uint32_t n = max(abs_u(dx), abs_u(dy));
            if (covers(ob, dx, dy) && n > 1u) samples += n - 1u;
        }
    }
    voids = group_fold<false>(voids, slots[0]), covered = group_fold<false>(covered, slots[1]), visible = group_fold<false>(visible, slots[2]);
    clearance = group_fold<true>(clearance, slots[3]), samples = group_fold<false>(samples, slots[4]);
    if (threadIdx.x != 0u) return;
    if (voids) atomicAdd(&counts->voids, voids);
    if (covered) atomicAdd(&counts->covered, covered);
    if (visible) atomicAdd(&counts->visible, visible);
    if (clearance) atomicMax(&counts->max_clearance, clearance);
    if (samples) atomicAdd(&counts->samples, (unsigned long long)samples);
    if (blockIdx.x == 0u) {
        uint32_t used = 0u;
        for (uint32_t o = 0; o < p.observer_count; o++) used += p.raw[uint64_t(p.observers[o].y) * p.width + p.observers[o].x] != 0u;
        counts->observers_used = used;
        counts->observers_skipped = p.observer_count - used;
    }
}

}  // namespace

bt_status launch_viewshed_transpose(hipStream_t stream, const ViewshedPlanes& p) {
    const dim3 grid((p.width + kTransposeTile - 1u) / kTransposeTile, (p.height + kTransposeTile - 1u) / kTransposeTile);
    viewshed_transpose_kernel<<<grid, dim3(kTransposeTile, 8), 0, stream>>>(p);
    return launched("viewshed_transpose_kernel");
}

bt_status launch_viewshed_walk(hipStream_t stream, const ViewshedPlanes& p) {
    constexpr uint32_t kWaves = kViewshedThreads / kWave;
    auto grid = [](uint32_t major_len, uint32_t minor_len) { return dim3(uint32_t((uint64_t(major_len) * ((minor_len + kWave - 1u) / kWave) + kWaves - 1u) / kWaves)); };
    viewshed_walk_kernel<true><<<grid(p.width, p.height), kViewshedThreads, 0, stream>>>(p);
    if (bt_status s = launched("viewshed_walk_kernel<x-major>")) return s;
    viewshed_walk_kernel<false><<<grid(p.height, p.width), kViewshedThreads, 0, stream>>>(p);
    return launched("viewshed_walk_kernel<y-major>");
}

bt_status launch_viewshed_finish(hipStream_t stream, const ViewshedPlanes& p, ViewshedCounts* counts) {
    const uint64_t per_group = uint64_t(kViewshedThreads) * kFinishCells;
    viewshed_finish_kernel<<<dim3(uint32_t((uint64_t(p.width) * p.height + per_group - 1u) / per_group)), kViewshedThreads, 0, stream>>>(p, counts);
    return launched("viewshed_finish_kernel");
}

}  // namespace bt

// bt_atlas_skyline: the kernels.  The host half is in bt_edit.cpp (the call, beside the other bakes) and bt_skyline.cpp (the line geometry
// and the plan); the definition is the SKYLINE section of include/bevy_terrain_amd.h.
//
// The transpose is the viewshed's (launch_viewshed_transpose), unchanged.
// skyline_walk_kernel     the hull walk.  blockIdx.y is a direction of the batch.  Along the major axis (x for an x-major direction, on
//                         the transposed plane; y otherwise, on the plane as it lies) the kernel steps against the direction, and at major
//                         coordinate u the cell of line j sits at minor coordinate j + off(u).  The lines j and j + M (M: the length of the
//                         minor axis) are never present at the same u, and the later one starts after the earlier one has ended, so a lane
//                         owns a residue c = j mod M and walks its lines one after the other: M lanes, every one busy at every step, and
//                         consecutive lanes read consecutive texels but where the residues wrap.  off(u) advances by a DDA that every lane
//                         shares.  The hull of the cells walked so far is a stack: the top two entries in registers, entry e below them at
//                         stack[e * M + c] of the direction's cell-sized plane, so lanes at equal depth touch one segment.  The next texel
//                         is fetched before the pops of this one, which are the only dependent loads.  (Holding the entries next under
//                         the registers in LDS as well was built and measured: slower in every case, profiles/skyline.txt.)  A workgroup is one wave, so that a
//                         call with few directions still spreads over the compute units.
// skyline_finish_kernel   a lane to a cell: the lit bits of the batch's directions ORed into the mask (one writer per cell), the sums of
//                         bt_skyline_stats folded per workgroup and added atomically, which is independent of the order; in the last
//                         batch's launch also count, the void count and the baked byte merged into the staged destination texels.
//
// Everything is integer arithmetic.  No atomics but the finish launch's counts; no result depends on a schedule.
#include "bt_internal.hpp"

namespace bt {

namespace {

constexpr uint32_t kWalkThreads = 64;  // one wave
constexpr uint32_t kFinishThreads = 256;
constexpr uint32_t kWave = 64;
constexpr uint32_t kFinishCells = 4;  // of one thread of the finish kernel

__device__ __forceinline__ int32_t abs_i(int32_t v) { return v < 0 ? -v : v; }

// floor(a / b) for b > 0, towards minus infinity
__device__ __forceinline__ int32_t floor_div(int32_t a, int32_t b) {
    const int32_t q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

__global__ __launch_bounds__(kWalkThreads) void skyline_walk_kernel(SkylinePlanes p) {
    const uint32_t k = blockIdx.y;
    const bt_skyline_direction& d = p.directions[p.first + k];
    const bool x_major = abs_i(d.dx) >= abs_i(d.dy);
    const int32_t L = int32_t(x_major ? p.width : p.height), M = int32_t(x_major ? p.height : p.width);  // the major and the minor length
    const int32_t c = int32_t(blockIdx.x * kWalkThreads + threadIdx.x);
    if (c >= M) return;
    const int32_t major_d = x_major ? d.dx : d.dy, minor_d = x_major ? d.dy : d.dx;
    const int32_t n = abs_i(major_d), m = major_d < 0 ? -minor_d : minor_d;
    const uint16_t* __restrict__ z = x_major ? p.transposed : p.raw;  // cell (u, v) at u * M + v
    const uint64_t cells = uint64_t(p.width) * p.height;
    uint32_t* __restrict__ stack = p.stack + k * cells + uint32_t(c);  // entry e below the registers at stack[e * M]
    uint16_t* __restrict__ steps = p.steps + k * cells;
    int32_t* __restrict__ rise = p.rise + k * cells;

    // against the direction: from the far end towards the near one, so that the cells ahead are the ones walked
    const int32_t du = major_d > 0 ? -1 : 1;
    int32_t u = major_d > 0 ? L - 1 : 0;
    // 2 u m + n = q * 2 n + r with 0 <= r < 2 n: q = off(u).  A step moves the left side by dr, |dr| <= 2 n: one correction at most
    const int32_t two_n = 2 * n, dr = du * 2 * m;
    int32_t q = floor_div(2 * u * m + n, two_n), r = 2 * u * m + n - q * two_n;  // |2 u m| < 2^26
    int32_t v = (c + q) % M;  // the lane's line at u: j = v - q, congruent to c
    if (v < 0) v += M;
    uint32_t depth = 0u, top_u = 0u, top_z = 0u, under_u = 0u, under_z = 0u;
    uint32_t za = z[uint32_t(u) * uint32_t(M) + uint32_t(v)];
    for (int32_t i = 0; i < L; i++) {
        // where the lane stands after this cell; a wrap of v is the end of its line and the start of the next one
        const int32_t next_u = u + du;
        int32_t next_r = r + dr, next_v = v;
        if (next_r >= two_n) next_r -= two_n, next_v++;
        else if (next_r < 0) next_r += two_n, next_v--;
        bool fresh = false;
        if (next_v >= M) next_v -= M, fresh = true;
        else if (next_v < 0) next_v += M, fresh = true;
        uint32_t next_z = 0u;
        if (i + 1 < L) next_z = z[uint32_t(next_u) * uint32_t(M) + uint32_t(next_v)];

        // pop the top p while the entry q under it has (z_q - z_a) t_p > (z_p - z_a) t_q: strict, a collinear p stays
        while (depth >= 2u) {
            const int64_t t_p = abs_i(int32_t(top_u) - u), t_q = abs_i(int32_t(under_u) - u);
            if (!((int64_t(under_z) - int64_t(za)) * t_p > (int64_t(top_z) - int64_t(za)) * t_q)) break;
            top_u = under_u, top_z = under_z;
            depth--;
            if (depth >= 2u) {
                const uint32_t e = stack[uint64_t(depth - 2u) * uint32_t(M)];
                under_u = e >> 16, under_z = e & 0xFFFFu;
            }
        }
        const uint64_t cell = x_major ? uint64_t(v) * p.width + uint32_t(u) : uint64_t(u) * p.width + uint32_t(v);
        steps[cell] = depth ? uint16_t(abs_i(int32_t(top_u) - u)) : uint16_t(0);
        rise[cell] = depth ? int32_t(top_z) - int32_t(za) : 0;
        // push a
        if (depth >= 2u) stack[uint64_t(depth - 2u) * uint32_t(M)] = under_u << 16 | under_z;
        under_u = top_u, under_z = top_z;
        top_u = uint32_t(u), top_z = za;
        depth = fresh ? 0u : depth + 1u;
        u = next_u, r = next_r, v = next_v, za = next_z;
    }
}

// the sum or the maximum of v over a workgroup, in thread 0; slot: four words of LDS of this fold's own
template <bool kMax, typename T>
__device__ __forceinline__ T group_fold(T v, T* slot) {
    for (int off = int(kWave) / 2; off > 0; off >>= 1) {
        const T o = __shfl_down(v, off);
        v = kMax ? max(v, o) : v + o;
    }
    if (threadIdx.x % kWave == 0u) slot[threadIdx.x / kWave] = v;
    __syncthreads();
    if (threadIdx.x != 0u) return T(0);
    for (uint32_t k = 1; k < kFinishThreads / kWave; k++) v = kMax ? max(v, slot[k]) : v + slot[k];
    return v;
}

// A thread takes kFinishCells cells a workgroup's width apart, the workgroup folds, and its first thread adds to the counts
__global__ __launch_bounds__(kFinishThreads) void skyline_finish_kernel(SkylinePlanes p, SkylineBake bake, uint32_t last, SkylineCounts* __restrict__ counts) {
    __shared__ uint32_t slots[3][kFinishThreads / kWave];
    __shared__ unsigned long long wide_slots[kFinishThreads / kWave];
    const uint32_t cells = p.width * p.height;
    uint32_t voids = 0u, longest = 0u, lit = 0u;  // a workgroup's lit <= 1024 * 64
    unsigned long long sum = 0u;
    for (uint32_t f = 0; f < kFinishCells; f++) {
        const uint32_t i = (blockIdx.x * kFinishCells + f) * kFinishThreads + threadIdx.x;
        if (i >= cells) break;
        uint64_t bits = 0u;
        for (uint32_t k = 0; k < p.batch; k++) {
            const bt_skyline_direction& d = p.directions[p.first + k];
            const uint32_t t = p.steps[uint64_t(k) * cells + i];
            const int32_t up = p.rise[uint64_t(k) * cells + i];
            // |up| sun_den < 2^32; t sun_num < 2^46
            bits |= uint64_t(int64_t(up) * int64_t(d.sun_den) <= int64_t(t) * int64_t(d.sun_num)) << (p.first + k);
            longest = max(longest, t);
            sum += t;
        }
        lit += uint32_t(__popcll(bits));
        const uint64_t mask = (p.first ? p.mask[i] : uint64_t(0)) | bits;
        p.mask[i] = mask;
        if (!last) continue;
        const uint32_t count = uint32_t(__popcll(mask));
        p.count[i] = uint8_t(count);
        voids += p.raw[i] == 0u;
        if (bake.texels) {
            const uint32_t b = 255u * count / p.direction_count, byte = bake.shade ? 255u - b : b;
            bake.texels[i] = (bake.texels[i] & ~(0xFFu << bake.shift)) | (byte << bake.shift);
        }
    }
    voids = group_fold<false>(voids, slots[0]), longest = group_fold<true>(longest, slots[1]), lit = group_fold<false>(lit, slots[2]);
    sum = group_fold<false>(sum, wide_slots);
    if (threadIdx.x != 0u) return;
    if (voids) atomicAdd(&counts->voids, voids);
    if (longest) atomicMax(&counts->max_steps, longest);
    if (lit) atomicAdd(&counts->lit, (unsigned long long)lit);
    if (sum) atomicAdd(&counts->sum_steps, sum);
}

}  // namespace

bt_status launch_skyline_transpose(hipStream_t stream, const SkylinePlanes& p) {
    ViewshedPlanes v{};  // the viewshed's transpose reads these four
    v.width = p.width, v.height = p.height, v.raw = p.raw, v.transposed = p.transposed;
    return launch_viewshed_transpose(stream, v);
}

bt_status launch_skyline_walk(hipStream_t stream, const SkylinePlanes& p) {
    const uint32_t lanes = max(p.width, p.height);  // of the longer minor axis; a direction whose minor axis is shorter leaves waves idle
    skyline_walk_kernel<<<dim3((lanes + kWalkThreads - 1u) / kWalkThreads, p.batch), kWalkThreads, 0, stream>>>(p);
    return launched("skyline_walk_kernel");
}

bt_status launch_skyline_finish(hipStream_t stream, const SkylinePlanes& p, const SkylineBake& bake, bool last, SkylineCounts* counts) {
    const uint32_t per_group = kFinishThreads * kFinishCells;
    skyline_finish_kernel<<<dim3((p.width * p.height + per_group - 1u) / per_group), kFinishThreads, 0, stream>>>(p, bake, last ? 1u : 0u, counts);
    return launched("skyline_finish_kernel");
}

}  // namespace bt

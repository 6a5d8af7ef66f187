// bt_atlas_distance_field: the kernels.  The host half is in bt_edit.cpp, beside bt_atlas_erode_height; the definition is the DISTANCE
// section of include/bevy_terrain_amd.h.
//
// The column phase finds r(x, y), the row of the nearest seed of column x to row y, the upper one on a tie.  A lane owns one column of one
// band of kDistanceBand = 32 rows, so a wave reads 64 consecutive texels of a row at a time and the seeds of its band are the bits of one
// register:
// distance_summary_kernel   the band's first and last seed row per column.
// distance_carry_kernel     a lane to a column walks the bands (256 at most) down and up and leaves, per band, the last seed row above it
//                           and the first one below it.
// distance_fill_kernel      the band's bits again, and r for its 32 rows from the bits and the two carried rows: the nearest bit at or above
//                           by a count of leading zeros, the nearest at or below by a count of trailing ones.
// The row phase:
// distance_rows_kernel      a workgroup to a row y, that row of r in LDS (16 KB at the widest).  A lane owns a cell and looks at the columns
//                           x, x -+ 1, x -+ 2, ... for the lexicographic minimum of (dx^2 + dy^2, index); it stops once dx^2 exceeds the
//                           best distance so far, and not when it equals it: a tie with a smaller index may lie there.  The lanes of a wave
//                           own 64 consecutive x, so their trip counts are close and their LDS reads consecutive.  A window without a seed
//                           is told from the row itself (a column without a seed has none in any row) and skips the search.
// distance_finish_kernel    the counts of bt_distance_stats: integer sums and a maximum, folded per workgroup and added atomically, which is
//                           independent of the order; and the baked byte merged into the staged destination texels.
//
// Everything is integer arithmetic.  No atomics but the finish launch's counts; no result depends on a schedule.
#include "bt_internal.hpp"

namespace bt {

namespace {

static_assert(kDistanceBand == 32u, "a band's seeds are the bits of one 32-bit word");
constexpr uint32_t kDistanceThreads = 256;
constexpr uint32_t kWave = 64;
constexpr uint32_t kFinishCells = 4;  // of one thread of the finish kernel
constexpr uint32_t kNone = BT_DISTANCE_NONE;
constexpr uint32_t kNoRow = 0xFFFFu;

__device__ __forceinline__ bool is_seed(const DistancePlanes& p, uint32_t i) {
    const uint32_t t = p.wide ? ((const uint32_t*)p.raw)[i] : uint32_t(((const uint16_t*)p.raw)[i]);
    const uint32_t v = (t >> p.shift) & p.value_mask;
    const bool s = (p.lo <= v && v <= p.hi) || (p.host && p.host[i] != 0u);
    return s != (p.invert != 0u);
}

// bit k: row band * kDistanceBand + k of column x is a seed
__device__ __forceinline__ uint32_t band_bits(const DistancePlanes& p, uint32_t x, uint32_t band) {
    const uint32_t y0 = band * kDistanceBand, rows = min(kDistanceBand, p.height - y0);
    uint32_t bits = 0u;
    for (uint32_t k = 0; k < rows; k++) bits |= uint32_t(is_seed(p, (y0 + k) * p.width + x)) << k;
    return bits;
}

__global__ __launch_bounds__(kDistanceThreads) void distance_summary_kernel(DistancePlanes p) {
    const uint32_t x = blockIdx.x * kDistanceThreads + threadIdx.x, band = blockIdx.y;
    if (x >= p.width) return;
    const uint32_t bits = band_bits(p, x, band), y0 = band * kDistanceBand;
    p.first[band * p.width + x] = uint16_t(bits ? y0 + uint32_t(__ffs(int(bits))) - 1u : kNoRow);
    p.last[band * p.width + x] = uint16_t(bits ? y0 + 31u - uint32_t(__clz(int(bits))) : kNoRow);
}

__global__ __launch_bounds__(kDistanceThreads) void distance_carry_kernel(DistancePlanes p) {
    const uint32_t x = blockIdx.x * kDistanceThreads + threadIdx.x;
    if (x >= p.width) return;
    uint32_t carry = kNoRow;
    for (uint32_t b = 0; b < p.bands; b++) {  // last: the band's own -> the last seed row above the band
        const uint32_t own = p.last[b * p.width + x];
        p.last[b * p.width + x] = uint16_t(carry);
        if (own != kNoRow) carry = own;
    }
    carry = kNoRow;
    for (uint32_t b = p.bands; b-- > 0u;) {  // first: the band's own -> the first seed row below the band
        const uint32_t own = p.first[b * p.width + x];
        p.first[b * p.width + x] = uint16_t(carry);
        if (own != kNoRow) carry = own;
    }
}

__global__ __launch_bounds__(kDistanceThreads) void distance_fill_kernel(DistancePlanes p) {
    const uint32_t x = blockIdx.x * kDistanceThreads + threadIdx.x, band = blockIdx.y;
    if (x >= p.width) return;
    const uint32_t bits = band_bits(p, x, band), y0 = band * kDistanceBand, rows = min(kDistanceBand, p.height - y0);
    const uint32_t up = p.last[band * p.width + x], down = p.first[band * p.width + x];
    for (uint32_t k = 0; k < rows; k++) {
        const uint32_t y = y0 + k;
        const uint32_t at_or_above = bits & (0xFFFFFFFFu >> (31u - k)), at_or_below = bits >> k;
        const uint32_t above = at_or_above ? y0 + 31u - uint32_t(__clz(int(at_or_above))) : up;
        const uint32_t below = at_or_below ? y + uint32_t(__ffs(int(at_or_below))) - 1u : down;
        uint32_t r;
        if (above == kNoRow) r = below;
        else if (below == kNoRow) r = above;
        else r = y - above <= below - y ? above : below;  // the upper one on a tie
        p.r[y * p.width + x] = uint16_t(r);
    }
}

__global__ __launch_bounds__(kDistanceThreads) void distance_rows_kernel(DistancePlanes p) {
    __shared__ uint16_t row[BT_DISTANCE_MAX_SIDE];
    const uint32_t y = blockIdx.x, width = p.width;
    const uint32_t base = y * width;
    int seen = 0;
    for (uint32_t x = threadIdx.x; x < width; x += kDistanceThreads) {
        const uint16_t r = p.r[base + x];
        row[x] = r;
        seen |= r != kNoRow;
    }
    if (!__syncthreads_or(seen)) {  // no column holds a seed: S is empty
        for (uint32_t x = threadIdx.x; x < width; x += kDistanceThreads) p.dist2[base + x] = kNone, p.nearest[base + x] = kNone;
        return;
    }
    for (uint32_t x = threadIdx.x; x < width; x += kDistanceThreads) {
        uint32_t best = kNone, best_index = kNone;
        auto look = [&](uint32_t i, uint32_t dx2) {
            const uint32_t r = row[i];
            if (r == kNoRow) return;
            const uint32_t dy = y > r ? y - r : r - y;
            const uint32_t d = dx2 + dy * dy, index = r * width + i;  // < 2^27; < 2^22
            if (d < best || (d == best && index < best_index)) best = d, best_index = index;
        };
        look(x, 0u);
        for (uint32_t dx = 1u;; dx++) {
            const uint32_t dx2 = dx * dx;
            if (dx2 > best) break;  // equal goes on: a smaller index at the same distance
            const bool left = dx <= x, right = x + dx < width;
            if (!left && !right) break;
            if (left) look(x - dx, dx2);
            if (right) look(x + dx, dx2);
        }
        p.dist2[base + x] = best;
        p.nearest[base + x] = best_index;
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
    for (uint32_t k = 1; k < kDistanceThreads / kWave; k++) v = kMax ? max(v, slot[k]) : v + slot[k];
    return v;
}

// b of the header: the largest b <= 255 with b^2 reach^2 <= 65025 dist2, which is min(255, isqrt(floor(65025 dist2 / reach^2)))
__device__ __forceinline__ uint32_t proximity(uint32_t dist2, uint64_t reach2) {
    if (dist2 == kNone) return 255u;
    const uint64_t n = uint64_t(dist2) * 65025u;  // < 2^43
    uint32_t b = 0u;
    for (uint32_t bit = 128u; bit; bit >>= 1) {
        const uint32_t c = b | bit;
        if (uint64_t(c * c) * reach2 <= n) b = c;  // < 2^16 * 2^32
    }
    return b;
}

// A thread counts kFinishCells cells a workgroup's width apart, the workgroup folds, and its first thread adds to the counts
__global__ __launch_bounds__(kDistanceThreads) void distance_finish_kernel(DistancePlanes p, DistanceBake bake, DistanceCounts* __restrict__ counts) {
    __shared__ uint32_t slots[2][kDistanceThreads / kWave];
    __shared__ unsigned long long wide_slots[kDistanceThreads / kWave];
    const uint32_t cells = p.width * p.height;
    uint32_t seeds = 0u, largest = 0u;
    unsigned long long sum = 0u;
    for (uint32_t k = 0; k < kFinishCells; k++) {
        const uint32_t i = (blockIdx.x * kFinishCells + k) * kDistanceThreads + threadIdx.x;
        if (i >= cells) break;
        const uint32_t d = p.dist2[i];
        if (bake.texels) {
            const uint32_t b = proximity(d, bake.reach2), byte = bake.near ? 255u - b : b;
            bake.texels[i] = (bake.texels[i] & ~(0xFFu << bake.shift)) | (byte << bake.shift);
        }
        if (d == kNone) continue;
        seeds += d == 0u;
        largest = max(largest, d);
        sum += d;
    }
    seeds = group_fold<false>(seeds, slots[0]), largest = group_fold<true>(largest, slots[1]), sum = group_fold<false>(sum, wide_slots);
    if (threadIdx.x != 0u) return;
    if (seeds) atomicAdd(&counts->seeds, seeds);
    if (largest) atomicMax(&counts->max_dist2, largest);
    if (sum) atomicAdd(&counts->sum_dist2, sum);
}

}  // namespace

bt_status launch_distance_columns(hipStream_t stream, const DistancePlanes& p) {
    const uint32_t groups = (p.width + kDistanceThreads - 1u) / kDistanceThreads;
    distance_summary_kernel<<<dim3(groups, p.bands), kDistanceThreads, 0, stream>>>(p);
    if (bt_status s = launched("distance_summary_kernel")) return s;
    distance_carry_kernel<<<dim3(groups), kDistanceThreads, 0, stream>>>(p);
    if (bt_status s = launched("distance_carry_kernel")) return s;
    distance_fill_kernel<<<dim3(groups, p.bands), kDistanceThreads, 0, stream>>>(p);
    return launched("distance_fill_kernel");
}

bt_status launch_distance_rows(hipStream_t stream, const DistancePlanes& p) {
    distance_rows_kernel<<<dim3(p.height), kDistanceThreads, 0, stream>>>(p);
    return launched("distance_rows_kernel");
}

bt_status launch_distance_finish(hipStream_t stream, const DistancePlanes& p, const DistanceBake& bake, DistanceCounts* counts) {
    const uint32_t per_group = kDistanceThreads * kFinishCells;
    distance_finish_kernel<<<dim3((p.width * p.height + per_group - 1u) / per_group), kDistanceThreads, 0, stream>>>(p, bake, counts);
    return launched("distance_finish_kernel");
}

}  // namespace bt

// bt_atlas_drainage: the kernels.  The host half is bt_drain.cpp; the definition is the DRAINAGE section of include/bevy_terrain_amd.h.
//
// drain_prepare_kernel    raw texels + the caller's mask -> z (0 = void), the initial X of the fill in W (z on outlets, 65535 on the other
//                         active cells, 0 on void ones), the counts of void cells and outlets.
// relax_kernel            <FillRule>, <FlatRule>, <AccumulateRule>: one sweep of the block relaxation, described in bt_relax.hpp.  The rules
//                         and why a halo value read while a neighbour rewrites it, or a stale one, cannot move the fixed point: at each
//                         rule below.
// drain_flat_seed_kernel  the final W -> F = 0 on drain cells (and void ones), 0xFFFFFFFF elsewhere.
// drain_direction_kernel  the direction plane by the header's rule, and A = w.
// drain_finish_kernel     the counts of bt_drainage_stats that need the final planes.
//
// Everything is integer arithmetic.  The relaxations: 38 VGPRs at most, no scratch: the 256 threads, not the registers or the LDS, bound the
// workgroups of a CU (tools/kernel_resources.sh relax bt_drain.hip).
#include "bt_relax.hpp"

namespace bt {

namespace {

constexpr uint32_t kDrainThreads = 256;  // of the per-cell kernels (prepare, seed, direction, finish)
constexpr uint32_t kNone = 0xFFFFFFFFu;

__device__ __forceinline__ bool drain_inside(const DrainPlanes& p, int x, int y) { return x >= 0 && y >= 0 && x < int(p.width) && y < int(p.height); }

// The three rules.  What all of them share: the cell's state is its fixed word a, and x is kNone outside the window.
struct DrainRuleBase {
    DrainPlanes p;
    using Cell = uint32_t;
    static constexpr uint32_t kOutsideX = kNone;
    __device__ __forceinline__ uint32_t cell(const uint32_t* s_a, uint32_t t) const { return s_a[t]; }
};

// X = max(z, min over neighbours), descending.  a = z (0: void or outside), x = X (kNone on void cells: a void neighbour never is the
// minimum that counts, and an outlet, which has one, starts at z and cannot fall).  Every X held anywhere, at any time, is 65535 or the
// bottleneck of a real path to an outlet, hence >= W; a stale or half-way halo value is such a value too, so a block can only stop above W
// or at it, never below, and the flags bring it back until nothing can fall.
struct FillRule : DrainRuleBase {
    static constexpr uint32_t kOutsideA = 0u;
    __device__ __forceinline__ void load(uint64_t c, uint32_t& a, uint32_t& x) const {
        a = p.z[c];
        x = a ? uint32_t(p.W[c]) : kNone;
    }
    __device__ __forceinline__ uint32_t relax(const uint32_t*, const uint32_t* s_x, uint32_t t, uint32_t a, uint32_t x) const {
        if (a == 0u) return x;
        uint32_t m = kNone;
#pragma unroll
        for (int k = 0; k < 8; k++) m = min(m, s_x[tile_neighbour(t, k)]);
        return min(x, max(a, m));
    }
    __device__ __forceinline__ void store(uint64_t c, uint32_t x) const { p.W[c] = uint16_t(x); }
};

// X = 1 + min over the neighbours of equal W, descending.  a = the final W (kNone: void or outside, equal to no cell's), x = F (0 on drain
// cells, which never move, kNone = not reached yet).  Every finite X held is the length of a real walk through cells of one W to a drain
// cell, hence >= F; a stale or half-way halo value is one too.
struct FlatRule : DrainRuleBase {
    static constexpr uint32_t kOutsideA = kNone;
    __device__ __forceinline__ void load(uint64_t c, uint32_t& a, uint32_t& x) const {
        const bool is_void = p.z[c] == 0u;
        a = is_void ? kNone : uint32_t(p.W[c]);
        x = is_void ? kNone : p.F[c];
    }
    __device__ __forceinline__ uint32_t relax(const uint32_t* s_a, const uint32_t* s_x, uint32_t t, uint32_t a, uint32_t x) const {
        if (a == kNone || x == 0u) return x;
        uint32_t m = kNone;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int n = tile_neighbour(t, k);
            if (s_a[n] == a) m = min(m, s_x[n]);
        }
        return m == kNone ? x : min(x, m + 1u);
    }
    __device__ __forceinline__ void store(uint64_t c, uint32_t x) const { p.F[c] = x; }
};

// X = w + the sum over the neighbours whose direction points at the cell, ascending from X = w.  a = direction | w << 8 (direction
// BT_DRAIN_VOID: void or outside), x = A.  The receivers form a forest, so the equations have one solution, by induction from the leaves; a
// value only grows, every value held is w plus a sum of values its donors held at some time, hence <= A, and a stale or half-way halo value
// is one such: a block can only stop below A or at it, and a donor that grows afterwards flags the block again.
struct AccumulateRule : DrainRuleBase {
    static constexpr uint32_t kOutsideA = BT_DRAIN_VOID;
    __device__ __forceinline__ void load(uint64_t c, uint32_t& a, uint32_t& x) const {
        a = uint32_t(p.dir[c]) | (p.weight ? uint32_t(p.weight[c]) : 1u) << 8;
        x = p.A[c];
    }
    __device__ __forceinline__ uint32_t relax(const uint32_t* s_a, const uint32_t* s_x, uint32_t t, uint32_t a, uint32_t x) const {
        if ((a & 255u) == BT_DRAIN_VOID) return x;
        uint32_t sum = a >> 8;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int n = tile_neighbour(t, k);
            if ((s_a[n] & 255u) == uint32_t((k + 4) & 7)) sum += s_x[n];  // neighbour k steps by -(dx, dy) of k: it points here
        }
        return sum;
    }
    __device__ __forceinline__ void store(uint64_t c, uint32_t x) const { p.A[c] = x; }
};

__global__ __launch_bounds__(kDrainThreads) void drain_prepare_kernel(DrainPlanes p, DrainCounts* __restrict__ counts) {
    const uint64_t cells = uint64_t(p.width) * p.height;
    const uint64_t i = uint64_t(blockIdx.x) * kDrainThreads + threadIdx.x;
    bool is_void = false, outlet = false;
    if (i < cells) {
        auto active = [&](int cx, int cy) {
            if (!drain_inside(p, cx, cy)) return false;
            const uint64_t c = uint64_t(cy) * p.width + uint32_t(cx);
            return p.raw[c] != 0u && !(p.mask && p.mask[c] != 0u);
        };
        const int x = int(i % p.width), y = int(i / p.width);
        is_void = !active(x, y);
        if (!is_void)
            for (int k = 0; k < 8; k++) outlet |= !active(x + neighbour_dx(k), y + neighbour_dy(k));
        const uint16_t z = is_void ? uint16_t(0) : p.raw[i];
        p.z[i] = z;
        p.W[i] = is_void ? uint16_t(0) : outlet ? z : uint16_t(65535);
    }
    const uint32_t voids = __syncthreads_count(is_void), outlets = __syncthreads_count(outlet);
    if (threadIdx.x == 0 && voids) atomicAdd(&counts->voids, voids);
    if (threadIdx.x == 0 && outlets) atomicAdd(&counts->outlets, outlets);
}

__global__ __launch_bounds__(kDrainThreads) void drain_flat_seed_kernel(DrainPlanes p) {
    const uint64_t cells = uint64_t(p.width) * p.height;
    const uint64_t i = uint64_t(blockIdx.x) * kDrainThreads + threadIdx.x;
    if (i >= cells) return;
    uint32_t f = 0u;
    if (p.z[i] != 0u) {
        const int x = int(i % p.width), y = int(i / p.width);
        const uint32_t w = p.W[i];
        bool drain = false;
        for (int k = 0; k < 8; k++) {
            const int nx = x + neighbour_dx(k), ny = y + neighbour_dy(k);
            if (!drain_inside(p, nx, ny)) {
                drain = true;
                continue;
            }
            const uint64_t c = uint64_t(ny) * p.width + uint32_t(nx);
            drain |= p.z[c] == 0u || p.W[c] < w;  // an outlet, or a lower neighbour
        }
        f = drain ? 0u : kNone;
    }
    p.F[i] = f;
}

__global__ __launch_bounds__(kDrainThreads) void drain_direction_kernel(DrainPlanes p) {
    const uint64_t cells = uint64_t(p.width) * p.height;
    const uint64_t i = uint64_t(blockIdx.x) * kDrainThreads + threadIdx.x;
    if (i >= cells) return;
    uint32_t out = BT_DRAIN_VOID, weight = 0u;
    if (p.z[i] != 0u) {
        weight = p.weight ? uint32_t(p.weight[i]) : 1u;
        const int x = int(i % p.width), y = int(i / p.width);
        const uint32_t w = p.W[i], f = p.F[i];
        bool outlet = false;
        uint64_t best = 0u;
        uint32_t steepest = kNone, level = kNone;
        for (int k = 7; k >= 0; k--) {  // descending k: the smallest stays on a tie
            const int nx = x + neighbour_dx(k), ny = y + neighbour_dy(k);
            if (!drain_inside(p, nx, ny)) {
                outlet = true;
                continue;
            }
            const uint64_t c = uint64_t(ny) * p.width + uint32_t(nx);
            if (p.z[c] == 0u) {
                outlet = true;
                continue;
            }
            const uint32_t wn = p.W[c];
            if (wn < w) {
                const uint64_t d = w - wn, score = d * d * ((k & 1) ? 1u : 2u);
                if (score >= best) best = score, steepest = uint32_t(k);
            } else if (wn == w && f != 0u && p.F[c] == f - 1u) {
                level = uint32_t(k);
            }
        }
        out = outlet ? uint32_t(BT_DRAIN_OUTLET) : steepest != kNone ? steepest : level;  // level is a k: F is finite on every active cell
    }
    p.dir[i] = uint8_t(out);
    p.A[i] = weight;
}

// the sum or the maximum of v over a wave, in lane 0
template <bool kMax>
__device__ __forceinline__ uint32_t wave_fold(uint32_t v) {
    for (int off = warpSize / 2; off > 0; off >>= 1) {
        const uint32_t o = __shfl_down(v, off);
        v = kMax ? max(v, o) : v + o;
    }
    return v;
}

__global__ __launch_bounds__(kDrainThreads) void drain_finish_kernel(DrainPlanes p, DrainCounts* __restrict__ counts) {
    const uint64_t cells = uint64_t(p.width) * p.height;
    const uint64_t i = uint64_t(blockIdx.x) * kDrainThreads + threadIdx.x;
    bool filled = false, flat = false;
    uint32_t f = 0u, a = 0u, out = 0u;
    if (i < cells && p.z[i] != 0u) {
        filled = p.W[i] > p.z[i];
        f = p.F[i];
        flat = f > 0u;
        a = p.A[i];
        out = p.dir[i] == BT_DRAIN_OUTLET ? a : 0u;
    }
    const uint32_t filled_here = __syncthreads_count(filled), flats_here = __syncthreads_count(flat);
    if (threadIdx.x == 0 && filled_here) atomicAdd(&counts->filled, filled_here);
    if (threadIdx.x == 0 && flats_here) atomicAdd(&counts->flats, flats_here);
    f = wave_fold<true>(f), a = wave_fold<true>(a), out = wave_fold<false>(out);
    if (threadIdx.x % warpSize == 0) {
        if (f) atomicMax(&counts->max_flat_distance, f);
        if (a) atomicMax(&counts->max_accumulation, a);
        if (out) atomicAdd(&counts->outflow, out);
    }
}

uint32_t flat_grid(const DrainPlanes& p) { return uint32_t((uint64_t(p.width) * p.height + kDrainThreads - 1u) / kDrainThreads); }

}  // namespace

bt_status launch_drain_prepare(hipStream_t stream, const DrainPlanes& p, DrainCounts* counts) {
    drain_prepare_kernel<<<dim3(flat_grid(p)), kDrainThreads, 0, stream>>>(p, counts);
    return launched("drain_prepare_kernel");
}

bt_status launch_drain_relax(hipStream_t stream, DrainRule rule, const DrainPlanes& p, uint32_t rounds, uint32_t* active, uint32_t* activate, uint32_t* marked) {
    const dim3 grid(p.blocks_x, p.blocks_y);
    if (rule == kDrainFill)
        relax_kernel<<<grid, kRelaxThreads, 0, stream>>>(FillRule{{p}}, RelaxGrid(p), rounds, active, activate, marked);
    else if (rule == kDrainFlat)
        relax_kernel<<<grid, kRelaxThreads, 0, stream>>>(FlatRule{{p}}, RelaxGrid(p), rounds, active, activate, marked);
    else
        relax_kernel<<<grid, kRelaxThreads, 0, stream>>>(AccumulateRule{{p}}, RelaxGrid(p), rounds, active, activate, marked);
    return launched("drain_relax_kernel");  // relax_kernel<Rule>, under the name bt_last_error() has always given it
}

bt_status launch_drain_flat_seed(hipStream_t stream, const DrainPlanes& p) {
    drain_flat_seed_kernel<<<dim3(flat_grid(p)), kDrainThreads, 0, stream>>>(p);
    return launched("drain_flat_seed_kernel");
}

bt_status launch_drain_direction(hipStream_t stream, const DrainPlanes& p) {
    drain_direction_kernel<<<dim3(flat_grid(p)), kDrainThreads, 0, stream>>>(p);
    return launched("drain_direction_kernel");
}

bt_status launch_drain_finish(hipStream_t stream, const DrainPlanes& p, DrainCounts* counts) {
    drain_finish_kernel<<<dim3(flat_grid(p)), kDrainThreads, 0, stream>>>(p, counts);
    return launched("drain_finish_kernel");
}

}  // namespace bt

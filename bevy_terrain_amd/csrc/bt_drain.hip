// bt_atlas_drainage: the kernels.  The host half is bt_drain.cpp; the definition is the DRAINAGE section of include/bevy_terrain_amd.h.
//
// drain_prepare_kernel    raw texels + the caller's mask -> z (0 = void), the initial X of the fill in W (z on outlets, 65535 on the other
//                         active cells, 0 on void ones), the counts of void cells and outlets.
// drain_relax_kernel      one sweep of one of three rules, the block scheme of bt_path.hip.  A workgroup owns kDrainBlock x kDrainBlock cells; it
//                         leaves at once unless its flag is set.  It stages two words per cell, a fixed one (`a`) and the value that moves (`x`),
//                         for its cells plus a one-cell halo in LDS, and relaxes in LDS until nothing changed in the workgroup or `rounds` rounds
//                         (kDrainRounds) have run.  It writes back the cells it changed (one writer per cell, naturally aligned stores, no global
//                         atomics), and flags the blocks whose halo those cells are in, and itself when it stopped at the round limit.  Sweeps are
//                         ordered by the kernel boundary alone.  The rules and why a halo value read while a neighbour rewrites it, or a stale
//                         one, cannot move the fixed point: at each rule below.
// drain_flat_seed_kernel  the final W -> F = 0 on drain cells (and void ones), 0xFFFFFFFF elsewhere.
// drain_direction_kernel  the direction plane by the header's rule, and A = w.
// drain_finish_kernel     the counts of bt_drainage_stats that need the final planes.
//
// Everything is integer arithmetic.  LDS: 2 x 34 x 34 dwords = 9248 bytes a workgroup (9512 with the words of the barrier reductions); a
// half-wave reads 32 consecutive dwords of a row (ds_read_b32 banks by dword mod 32 within a 32-lane half: no conflict).  38 VGPRs at most,
// no scratch: the 256 threads, not the registers or the LDS, bound the workgroups of a CU (tools/kernel_resources.sh drain bt_drain.hip).
#include "bt_internal.hpp"

namespace bt {

namespace {

constexpr uint32_t kDrainThreads = 256;
constexpr uint32_t kDrainTile = kDrainBlock + 2u;  // the block and its halo
constexpr uint32_t kDrainOwn = kDrainBlock * kDrainBlock / kDrainThreads;  // cells of a thread: rows ly, ly + 8, ly + 16, ly + 24
constexpr uint32_t kNone = 0xFFFFFFFFu;
// neighbour k = 0..7: (1,0), (1,1), (0,1), (-1,1), (-1,0), (-1,-1), (0,-1), (1,-1)
__host__ __device__ constexpr int drain_dx(int k) { return k == 0 || k == 1 || k == 7 ? 1 : k >= 3 && k <= 5 ? -1 : 0; }
__host__ __device__ constexpr int drain_dy(int k) { return k >= 1 && k <= 3 ? 1 : k >= 5 ? -1 : 0; }

__device__ __forceinline__ bool drain_inside(const DrainPlanes& p, int x, int y) { return x >= 0 && y >= 0 && x < int(p.width) && y < int(p.height); }

// The three rules.  load: the two words of a cell inside the window (outside it: kOutsideA, kNone); relax: the new x of a cell from its own
// words and the tile (t: its index in the tile); store: x back into its plane.

// X = max(z, min over neighbours), descending.  a = z (0: void or outside), x = X (kNone on void cells: a void neighbour never is the
// minimum that counts, and an outlet, which has one, starts at z and cannot fall).  Every X held anywhere, at any time, is 65535 or the
// bottleneck of a real path to an outlet, hence >= W; a stale or half-way halo value is such a value too, so a block can only stop above W
// or at it, never below, and the flags bring it back until nothing can fall.
struct FillRule {
    static constexpr uint32_t kOutsideA = 0u;
    static __device__ __forceinline__ void load(const DrainPlanes& p, uint64_t c, uint32_t& a, uint32_t& x) {
        a = p.z[c];
        x = a ? uint32_t(p.W[c]) : kNone;
    }
    static __device__ __forceinline__ uint32_t relax(const uint32_t* s_a, const uint32_t* s_x, uint32_t t, uint32_t a, uint32_t x) {
        if (a == 0u) return x;
        uint32_t m = kNone;
#pragma unroll
        for (int k = 0; k < 8; k++) m = min(m, s_x[int(t) + drain_dy(k) * int(kDrainTile) + drain_dx(k)]);
        return min(x, max(a, m));
    }
    static __device__ __forceinline__ void store(const DrainPlanes& p, uint64_t c, uint32_t x) { p.W[c] = uint16_t(x); }
};

// X = 1 + min over the neighbours of equal W, descending.  a = the final W (kNone: void or outside, equal to no cell's), x = F (0 on drain
// cells, which never move, kNone = not reached yet).  Every finite X held is the length of a real walk through cells of one W to a drain
// cell, hence >= F; a stale or half-way halo value is one too.
struct FlatRule {
    static constexpr uint32_t kOutsideA = kNone;
    static __device__ __forceinline__ void load(const DrainPlanes& p, uint64_t c, uint32_t& a, uint32_t& x) {
        const bool is_void = p.z[c] == 0u;
        a = is_void ? kNone : uint32_t(p.W[c]);
        x = is_void ? kNone : p.F[c];
    }
    static __device__ __forceinline__ uint32_t relax(const uint32_t* s_a, const uint32_t* s_x, uint32_t t, uint32_t a, uint32_t x) {
        if (a == kNone || x == 0u) return x;
        uint32_t m = kNone;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int n = int(t) + drain_dy(k) * int(kDrainTile) + drain_dx(k);
            if (s_a[n] == a) m = min(m, s_x[n]);
        }
        return m == kNone ? x : min(x, m + 1u);
    }
    static __device__ __forceinline__ void store(const DrainPlanes& p, uint64_t c, uint32_t x) { p.F[c] = x; }
};

// X = w + the sum over the neighbours whose direction points at the cell, ascending from X = w.  a = direction | w << 8 (direction
// BT_DRAIN_VOID: void or outside), x = A.  The receivers form a forest, so the equations have one solution, by induction from the leaves; a
// value only grows, every value held is w plus a sum of values its donors held at some time, hence <= A, and a stale or half-way halo value
// is one such: a block can only stop below A or at it, and a donor that grows afterwards flags the block again.
struct AccumulateRule {
    static constexpr uint32_t kOutsideA = BT_DRAIN_VOID;
    static __device__ __forceinline__ void load(const DrainPlanes& p, uint64_t c, uint32_t& a, uint32_t& x) {
        a = uint32_t(p.dir[c]) | (p.weight ? uint32_t(p.weight[c]) : 1u) << 8;
        x = p.A[c];
    }
    static __device__ __forceinline__ uint32_t relax(const uint32_t* s_a, const uint32_t* s_x, uint32_t t, uint32_t a, uint32_t x) {
        if ((a & 255u) == BT_DRAIN_VOID) return x;
        uint32_t sum = a >> 8;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int n = int(t) + drain_dy(k) * int(kDrainTile) + drain_dx(k);
            if ((s_a[n] & 255u) == uint32_t((k + 4) & 7)) sum += s_x[n];  // neighbour k steps by -(dx, dy) of k: it points here
        }
        return sum;
    }
    static __device__ __forceinline__ void store(const DrainPlanes& p, uint64_t c, uint32_t x) { p.A[c] = x; }
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
            for (int k = 0; k < 8; k++) outlet |= !active(x + drain_dx(k), y + drain_dy(k));
        const uint16_t z = is_void ? uint16_t(0) : p.raw[i];
        p.z[i] = z;
        p.W[i] = is_void ? uint16_t(0) : outlet ? z : uint16_t(65535);
    }
    const uint32_t voids = __syncthreads_count(is_void), outlets = __syncthreads_count(outlet);
    if (threadIdx.x == 0 && voids) atomicAdd(&counts->voids, voids);
    if (threadIdx.x == 0 && outlets) atomicAdd(&counts->outlets, outlets);
}

// bits of the flag mask a block collects: the neighbour blocks in whose halo a changed cell lies, and the block itself
enum : uint32_t { kLeft = 1, kRight = 2, kUp = 4, kDown = 8, kUpLeft = 16, kUpRight = 32, kDownLeft = 64, kDownRight = 128, kSelf = 256 };

template <class Rule>
__global__ __launch_bounds__(kDrainThreads) void drain_relax_kernel(DrainPlanes p, uint32_t rounds, uint32_t* active, uint32_t* activate, uint32_t* marked) {
    const uint32_t block = blockIdx.y * p.blocks_x + blockIdx.x;
    if (active[block] == 0u) return;  // the same word for every thread, and only this workgroup writes it (below, behind a barrier)
    __shared__ uint32_t s_a[kDrainTile * kDrainTile];
    __shared__ uint32_t s_x[kDrainTile * kDrainTile];
    __shared__ uint32_t s_mask;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) s_mask = 0u;
    const int gx0 = int(blockIdx.x * kDrainBlock) - 1, gy0 = int(blockIdx.y * kDrainBlock) - 1;
    for (uint32_t i = tid; i < kDrainTile * kDrainTile; i += kDrainThreads) {
        const int gx = gx0 + int(i % kDrainTile), gy = gy0 + int(i / kDrainTile);
        uint32_t a = Rule::kOutsideA, x = kNone;
        if (drain_inside(p, gx, gy)) Rule::load(p, uint64_t(gy) * p.width + uint32_t(gx), a, x);
        s_a[i] = a;
        s_x[i] = x;
    }
    __syncthreads();
    if (tid == 0) active[block] = 0u;

    const uint32_t lx = tid % kDrainBlock, ly0 = tid / kDrainBlock;
    uint32_t a[kDrainOwn], x[kDrainOwn], x_in[kDrainOwn];
#pragma unroll
    for (uint32_t j = 0; j < kDrainOwn; j++) {
        const uint32_t t = (ly0 + j * (kDrainThreads / kDrainBlock) + 1u) * kDrainTile + lx + 1u;
        a[j] = s_a[t];
        x[j] = x_in[j] = s_x[t];
    }
    int more = 1;
    for (uint32_t round = 0; round < rounds && more; round++) {
        int changed = 0;
#pragma unroll
        for (uint32_t j = 0; j < kDrainOwn; j++) {
            const uint32_t t = (ly0 + j * (kDrainThreads / kDrainBlock) + 1u) * kDrainTile + lx + 1u;
            const uint32_t next = Rule::relax(s_a, s_x, t, a[j], x[j]);
            if (next != x[j]) {
                x[j] = next;
                s_x[t] = next;
                changed = 1;
            }
        }
        more = __syncthreads_or(changed);
    }
    uint32_t mask = 0u;
#pragma unroll
    for (uint32_t j = 0; j < kDrainOwn; j++) {
        if (x[j] == x_in[j]) continue;
        const uint32_t ly = ly0 + j * (kDrainThreads / kDrainBlock);
        // inside the window: a cell outside it holds kOutsideA and no rule moves it
        Rule::store(p, uint64_t(blockIdx.y * kDrainBlock + ly) * p.width + blockIdx.x * kDrainBlock + lx, x[j]);
        const bool l = lx == 0u, r = lx == kDrainBlock - 1u, u = ly == 0u, dn = ly == kDrainBlock - 1u;
        mask |= (l ? kLeft : 0u) | (r ? kRight : 0u) | (u ? kUp : 0u) | (dn ? kDown : 0u) | (l && u ? kUpLeft : 0u) | (r && u ? kUpRight : 0u) |
                (l && dn ? kDownLeft : 0u) | (r && dn ? kDownRight : 0u);
    }
    if (mask) atomicOr(&s_mask, mask);
    __syncthreads();
    if (tid != 0) return;
    mask = s_mask | (more ? uint32_t(kSelf) : 0u);
    const uint32_t bx = blockIdx.x, by = blockIdx.y;
    const bool hl = bx > 0u, hr = bx + 1u < p.blocks_x, hu = by > 0u, hd = by + 1u < p.blocks_y;
    uint32_t set = 0u;
    auto flag = [&](uint32_t bit, bool exists, int dx, int dy) {
        if (!(mask & bit) || !exists) return;
        activate[uint32_t(int(by) + dy) * p.blocks_x + uint32_t(int(bx) + dx)] = 1u;
        set = 1u;
    };
    flag(kLeft, hl, -1, 0), flag(kRight, hr, 1, 0), flag(kUp, hu, 0, -1), flag(kDown, hd, 0, 1);
    flag(kUpLeft, hl && hu, -1, -1), flag(kUpRight, hr && hu, 1, -1), flag(kDownLeft, hl && hd, -1, 1), flag(kDownRight, hr && hd, 1, 1);
    flag(kSelf, true, 0, 0);
    if (set) atomicAdd(marked, 1u);
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
            const int nx = x + drain_dx(k), ny = y + drain_dy(k);
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
            const int nx = x + drain_dx(k), ny = y + drain_dy(k);
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

bt_status drain_launched(const char* what) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? BT_OK : hip_fail(e, what);
}

uint32_t flat_grid(const DrainPlanes& p) { return uint32_t((uint64_t(p.width) * p.height + kDrainThreads - 1u) / kDrainThreads); }

}  // namespace

bt_status launch_drain_prepare(hipStream_t stream, const DrainPlanes& p, DrainCounts* counts) {
    drain_prepare_kernel<<<dim3(flat_grid(p)), kDrainThreads, 0, stream>>>(p, counts);
    return drain_launched("drain_prepare_kernel");
}

bt_status launch_drain_relax(hipStream_t stream, DrainRule rule, const DrainPlanes& p, uint32_t rounds, uint32_t* active, uint32_t* activate, uint32_t* marked) {
    const dim3 grid(p.blocks_x, p.blocks_y);
    if (rule == kDrainFill)
        drain_relax_kernel<FillRule><<<grid, kDrainThreads, 0, stream>>>(p, rounds, active, activate, marked);
    else if (rule == kDrainFlat)
        drain_relax_kernel<FlatRule><<<grid, kDrainThreads, 0, stream>>>(p, rounds, active, activate, marked);
    else
        drain_relax_kernel<AccumulateRule><<<grid, kDrainThreads, 0, stream>>>(p, rounds, active, activate, marked);
    return drain_launched("drain_relax_kernel");
}

bt_status launch_drain_flat_seed(hipStream_t stream, const DrainPlanes& p) {
    drain_flat_seed_kernel<<<dim3(flat_grid(p)), kDrainThreads, 0, stream>>>(p);
    return drain_launched("drain_flat_seed_kernel");
}

bt_status launch_drain_direction(hipStream_t stream, const DrainPlanes& p) {
    drain_direction_kernel<<<dim3(flat_grid(p)), kDrainThreads, 0, stream>>>(p);
    return drain_launched("drain_direction_kernel");
}

bt_status launch_drain_finish(hipStream_t stream, const DrainPlanes& p, DrainCounts* counts) {
    drain_finish_kernel<<<dim3(flat_grid(p)), kDrainThreads, 0, stream>>>(p, counts);
    return drain_launched("drain_finish_kernel");
}

}  // namespace bt

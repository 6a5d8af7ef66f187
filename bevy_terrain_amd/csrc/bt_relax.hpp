// The block relaxation of bt_atlas_path_field and bt_atlas_drainage: one kernel skeleton and one host loop, the text of bt_path.hip / bt_path.cpp and
// bt_drain.hip / bt_drain.cpp (not compiled on its own).  A field over a width x height window is brought to the fixed point of a local rule:
// every cell's value is a function of its own fixed word and of its eight neighbours' words.
//
// relax_kernel<Rule>  one sweep.  A workgroup owns kRelaxBlock x kRelaxBlock cells; it leaves at once unless its flag is set.  It stages two words
//                     per cell, a fixed one (`a`) and the value that moves (`x`), for its cells plus a one-cell halo in LDS (the rule's outside words
//                     beyond the window), forms each cell's state once, in registers, and relaxes in LDS until nothing changed in the workgroup
//                     or `rounds` rounds (kRelaxRounds) have run.  It writes back the cells it changed (one writer per cell, naturally aligned
//                     stores, no global atomics), and flags the blocks whose halo those cells are in (a corner cell is in a diagonal block's
//                     too), and itself when it stopped at the round limit: until no block is flagged, some block still has work.  A halo value
//                     may be read while a neighbour rewrites it, or be stale; why that cannot move the fixed point is a property of the rule
//                     and stands at each Rule.  Sweeps are ordered by the kernel boundary alone.
// relax_sweeps        the host loop: sweeps in batches (4, 8, 16, then 32 at a time); after each batch the LAST sweep's count of blocks that
//                     flagged work for the sweep after it comes back, and 0 ends the loop.  A sweep in which no block is flagged does nothing, so
//                     sweeps past convergence cost a launch each and change nothing.
//
// LDS: 2 x 34 x 34 dwords = 9248 bytes a workgroup (9512 with the words of the barrier reductions); a half-wave reads 32 consecutive dwords of a
// row (ds_read_b32 banks by dword mod 32 within a 32-lane half: no conflict).
#pragma once

#include <cstdlib>

#include "bt_internal.hpp"

namespace bt {

constexpr uint32_t kRelaxThreads = 256;
constexpr uint32_t kRelaxTile = kRelaxBlock + 2u;                          // the block and its halo
constexpr uint32_t kRelaxOwn = kRelaxBlock * kRelaxBlock / kRelaxThreads;  // cells of a thread: rows ly, ly + 8, ly + 16, ly + 24
constexpr uint32_t kRelaxRounds = 64;                                      // rounds of one block in one sweep, at most
constexpr uint32_t kBatchFirst = 4, kBatchMax = 32;                        // sweeps between two looks at the count of flagged blocks

// neighbour k = 0..7: (1,0), (1,1), (0,1), (-1,1), (-1,0), (-1,-1), (0,-1), (1,-1)
__host__ __device__ constexpr int neighbour_dx(int k) { return k == 0 || k == 1 || k == 7 ? 1 : k >= 3 && k <= 5 ? -1 : 0; }
__host__ __device__ constexpr int neighbour_dy(int k) { return k >= 1 && k <= 3 ? 1 : k >= 5 ? -1 : 0; }
// neighbour k of tile cell t
__device__ __forceinline__ int tile_neighbour(uint32_t t, int k) { return int(t) + neighbour_dy(k) * int(kRelaxTile) + neighbour_dx(k); }

// bits of the flag mask a block collects: the neighbour blocks in whose halo a changed cell lies, and the block itself
enum : uint32_t { kLeft = 1, kRight = 2, kUp = 4, kDown = 8, kUpLeft = 16, kUpRight = 32, kDownLeft = 64, kDownRight = 128, kSelf = 256 };

// A Rule is a small value type that holds its planes by value (a reference to a kernel argument costs registers) and supplies
//   kOutsideA, kOutsideX                 the two words of a cell outside the window;
//   load(c, a, x)                        the two words of cell c inside it;
//   Cell, cell(s_a, t)                   what relax needs of the cell at tile index t besides x, formed once from the staged tile;
//   relax(s_a, s_x, t, cell, x) -> x'    the cell's new value from the tile as it stands; x' == x (as words) says "unchanged";
//   store(c, x)                          x back into its plane.
// No rule moves a cell outside the window (the kernel stores without a bounds test).
template <class Rule>
__global__ __launch_bounds__(kRelaxThreads) void relax_kernel(Rule rule, RelaxGrid g, uint32_t rounds, uint32_t* active, uint32_t* activate, uint32_t* marked) {
    const uint32_t block = blockIdx.y * g.blocks_x + blockIdx.x;
    if (active[block] == 0u) return;  // the same word for every thread, and only this workgroup writes it (below, behind a barrier)
    __shared__ uint32_t s_a[kRelaxTile * kRelaxTile];
    __shared__ uint32_t s_x[kRelaxTile * kRelaxTile];
    __shared__ uint32_t s_mask;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) s_mask = 0u;
    const int gx0 = int(blockIdx.x * kRelaxBlock) - 1, gy0 = int(blockIdx.y * kRelaxBlock) - 1;
    for (uint32_t i = tid; i < kRelaxTile * kRelaxTile; i += kRelaxThreads) {
        const int gx = gx0 + int(i % kRelaxTile), gy = gy0 + int(i / kRelaxTile);
        uint32_t a = Rule::kOutsideA, x = Rule::kOutsideX;
        if (gx >= 0 && gy >= 0 && gx < int(g.width) && gy < int(g.height)) rule.load(uint64_t(gy) * g.width + uint32_t(gx), a, x);
        s_a[i] = a;
        s_x[i] = x;
    }
    __syncthreads();
    if (tid == 0) active[block] = 0u;

    const uint32_t lx = tid % kRelaxBlock, ly0 = tid / kRelaxBlock;
    typename Rule::Cell cell[kRelaxOwn];
    uint32_t x[kRelaxOwn], x_in[kRelaxOwn];
#pragma unroll
    for (uint32_t j = 0; j < kRelaxOwn; j++) {
        const uint32_t t = (ly0 + j * (kRelaxThreads / kRelaxBlock) + 1u) * kRelaxTile + lx + 1u;
        cell[j] = rule.cell(s_a, t);
        x[j] = x_in[j] = s_x[t];
    }
    int more = 1;
    for (uint32_t round = 0; round < rounds && more; round++) {
        int changed = 0;
#pragma unroll
        for (uint32_t j = 0; j < kRelaxOwn; j++) {
            const uint32_t t = (ly0 + j * (kRelaxThreads / kRelaxBlock) + 1u) * kRelaxTile + lx + 1u;
            const uint32_t next = rule.relax(s_a, s_x, t, cell[j], x[j]);
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
    for (uint32_t j = 0; j < kRelaxOwn; j++) {
        if (x[j] == x_in[j]) continue;
        const uint32_t ly = ly0 + j * (kRelaxThreads / kRelaxBlock);
        rule.store(uint64_t(blockIdx.y * kRelaxBlock + ly) * g.width + blockIdx.x * kRelaxBlock + lx, x[j]);  // inside the window: no rule moves a cell outside it
        const bool l = lx == 0u, r = lx == kRelaxBlock - 1u, u = ly == 0u, dn = ly == kRelaxBlock - 1u;
        mask |= (l ? kLeft : 0u) | (r ? kRight : 0u) | (u ? kUp : 0u) | (dn ? kDown : 0u) | (l && u ? kUpLeft : 0u) | (r && u ? kUpRight : 0u) |
                (l && dn ? kDownLeft : 0u) | (r && dn ? kDownRight : 0u);
    }
    if (mask) atomicOr(&s_mask, mask);
    __syncthreads();
    if (tid != 0) return;
    mask = s_mask | (more ? uint32_t(kSelf) : 0u);
    const uint32_t bx = blockIdx.x, by = blockIdx.y;
    const bool hl = bx > 0u, hr = bx + 1u < g.blocks_x, hu = by > 0u, hd = by + 1u < g.blocks_y;
    uint32_t set = 0u;
    auto flag = [&](uint32_t bit, bool exists, int dx, int dy) {
        if (!(mask & bit) || !exists) return;
        activate[uint32_t(int(by) + dy) * g.blocks_x + uint32_t(int(bx) + dx)] = 1u;
        set = 1u;
    };
    flag(kLeft, hl, -1, 0), flag(kRight, hr, 1, 0), flag(kUp, hu, 0, -1), flag(kDown, hd, 0, 1);
    flag(kUpLeft, hl && hu, -1, -1), flag(kUpRight, hr && hu, 1, -1), flag(kDownLeft, hl && hd, -1, 1), flag(kDownRight, hr && hd, 1, 1);
    flag(kSelf, true, 0, 0);
    if (set) atomicAdd(marked, 1u);
}

// rounds of a block per sweep.  The profiling build (tools/, -DBT_DEBUG_HOOKS) takes it from `variable` (BT_PATH_ROUNDS for tools/path_bench.py,
// BT_DRAIN_ROUNDS for tools/drainage_bench.py)
inline uint32_t relax_rounds(const char* variable) {
#ifdef BT_DEBUG_HOOKS
    if (const char* v = getenv(variable)) return uint32_t(std::min(std::max(atoi(v), 1), 4096));
#endif
    return kRelaxRounds;
}

// Sweeps from the flags the caller has set in flags[0] (flags[1]: zeros) until one flags nothing, `cells` sweeps at the most.  enqueue(active,
// activate, marked) launches one sweep; `marked` are kBatchMax counters on the device, `marked_host` the pinned word the last one of a
// batch comes back in.  *sweeps: how many were launched; *converged: whether the last one flagged nothing
template <class Enqueue>
bt_status relax_sweeps(hipStream_t stream, uint64_t cells, uint32_t* const flags[2], uint32_t* marked, const uint32_t* marked_host, Enqueue enqueue, uint32_t* sweeps,
                       bool* converged) {
    *sweeps = 0, *converged = false;
    for (uint32_t batch = kBatchFirst; !*converged && *sweeps < cells; batch = std::min(2u * batch, kBatchMax)) {
        const uint32_t n = uint32_t(std::min<uint64_t>(batch, cells - *sweeps));
        BT_HIP(hipMemsetAsync(marked, 0, n * 4u, stream));
        for (uint32_t i = 0; i < n; i++, ++*sweeps)
            if (bt_status s = enqueue(flags[*sweeps & 1u], flags[(*sweeps + 1u) & 1u], marked + i)) return s;
        BT_HIP(hipMemcpyAsync((void*)marked_host, marked + (n - 1u), 4u, hipMemcpyDeviceToHost, stream));
        BT_HIP(hipStreamSynchronize(stream));
        *converged = marked_host[0] == 0u;
    }
    return BT_OK;
}

}  // namespace bt

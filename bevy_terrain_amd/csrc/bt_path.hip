// bt_atlas_path_field: the kernels.  The host half is bt_path.cpp; the definition is the PATH FIELD section of include/bevy_terrain_amd.h.
//
// path_prepare_kernel  raw texels + the caller's mask -> the height plane (NaN = blocked; a free cell's height is finite, the host refuses
//                      what could make it otherwise) and the count of blocked cells; the goal list -> D by atomicMin on the bits
//                      (non-negative floats order as their bit patterns), a mark in the next plane on every cell a goal names, and the
//                      flags of the 3 x 3 blocks around it (a goal on a block's edge may change nothing inside its own block).
// relax_kernel         <PathRule>: one sweep of the block relaxation, described in bt_relax.hpp.  PathRule below is what it relaxes: heights
//                      and D staged in LDS (NaN / +inf outside the window), the eight weights of a cell formed once, in registers.
// path_next_kernel     the next plane by the header's rule, and the count of reachable cells.
//
// Arithmetic contract: IEEE binary32, one rounding per written operation; this file is compiled with -ffp-contract=off, `/` is the
// correctly rounded division.
#include "bt_relax.hpp"

namespace bt {

namespace {

constexpr uint32_t kPathThreads = 256;  // of the per-cell kernels (prepare, next)
constexpr uint32_t kInfBits = 0x7F800000u;

// w(a -> b) of the header line by line, or +inf where the grade test fails (a NaN height on either side fails it)
__device__ __forceinline__ float path_weight(float ha, float hb, float run, const bt_path_cost& c) {
    const float rise = hb - ha;
    const float g = fabsf(rise) / run;
    if (!(g <= c.max_grade)) return __builtin_inff();
    const float up = rise > 0.0f ? rise : 0.0f;
    const float down = rise < 0.0f ? -rise : 0.0f;
    return ((run * (1.0f + c.grade_weight * g)) + c.climb_weight * up) + c.descend_weight * down;
}

__global__ __launch_bounds__(kPathThreads) void path_prepare_kernel(PathPlanes p, bt_path_cost cost, const bt_path_goal* __restrict__ goals, uint32_t goal_count,
                                                                    uint32_t* __restrict__ flags, PathCounts* __restrict__ counts) {
    const uint64_t cells = uint64_t(p.width) * p.height;
    const uint64_t i = uint64_t(blockIdx.x) * kPathThreads + threadIdx.x;
    bool blocked = false;
    if (i < cells) {
        const uint32_t raw = p.raw[i];
        blocked = raw == 0u || (p.mask && p.mask[i] != 0u);
        const float h = cost.min_height + (cost.max_height - cost.min_height) * (float(raw) / 65535.0f);
        p.h[i] = blocked ? __builtin_nanf("") : h;
    }
    const uint32_t blocked_here = __syncthreads_count(blocked);
    if (threadIdx.x == 0 && blocked_here) atomicAdd(&counts->blocked, blocked_here);
    if (i < goal_count) {
        const bt_path_goal g = goals[i];
        const uint64_t c = uint64_t(g.y) * p.width + g.x;
        if (p.raw[c] == 0u || (p.mask && p.mask[c] != 0u)) {
            atomicAdd(&counts->goals_blocked, 1u);
        } else {
            atomicMin(&p.D[c], __float_as_uint(g.cost0));
            p.next[c] = 1u;
            const uint32_t bx = g.x / kRelaxBlock, by = g.y / kRelaxBlock;
            for (int dy = -1; dy <= 1; dy++)
                for (int dx = -1; dx <= 1; dx++) {
                    const uint32_t nx = bx + uint32_t(dx), ny = by + uint32_t(dy);  // wraps below 0: fails the test
                    if (nx < p.blocks_x && ny < p.blocks_y) flags[ny * p.blocks_x + nx] = 1u;
                }
        }
    }
}

// D = min(D, min over neighbours of D + w), descending.  a = the bits of the height (NaN: blocked or outside), x = the bits of D (+inf: not
// reached, and outside).  The cell's state is its eight weights, formed once: +inf where the grade test fails, where either height is NaN,
// and on a diagonal beside a blocked cell, so a blocked or outside cell never falls below +inf.  Every D held anywhere, at any time, is
// +inf or the cost of a real path to a goal, hence >= the field; a halo value read while a neighbour rewrites it (an aligned dword), or a
// stale one, is such a cost too, so a block can only stop above the field or at it, and the flags bring it back until nothing can fall.
// "Changed" is a comparison of words: a value only falls, is never NaN, and the host turns a goal's -0 into +0, so next != x says what
// next < x says on the floats.
struct PathRule {
    PathPlanes p;
    bt_path_cost cost;
    float cell_diag;
    struct Cell {
        float w[8];
    };
    static constexpr uint32_t kOutsideA = 0x7FC00000u, kOutsideX = kInfBits;  // NaN, +inf
    __device__ __forceinline__ void load(uint64_t c, uint32_t& a, uint32_t& x) const {
        a = __float_as_uint(p.h[c]);
        x = p.D[c];
    }
    __device__ __forceinline__ Cell cell(const uint32_t* s_a, uint32_t t) const {
        Cell c;
        const float ha = __uint_as_float(s_a[t]);
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const float hb = __uint_as_float(s_a[tile_neighbour(t, k)]);
            float wk = path_weight(ha, hb, (k & 1) ? cell_diag : cost.cell_size, cost);
            if (k & 1) {  // no corner cutting: both cells beside the diagonal are free
                const float hx = __uint_as_float(s_a[int(t) + neighbour_dx(k)]), hy = __uint_as_float(s_a[int(t) + neighbour_dy(k) * int(kRelaxTile)]);
                if (hx != hx || hy != hy) wk = __builtin_inff();
            }
            c.w[k] = wk;
        }
        return c;
    }
    __device__ __forceinline__ uint32_t relax(const uint32_t*, const uint32_t* s_x, uint32_t t, const Cell& c, uint32_t x) const {
        float best = __uint_as_float(x);
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const float cand = __uint_as_float(s_x[tile_neighbour(t, k)]) + c.w[k];
            if (cand < best) best = cand;
        }
        return __float_as_uint(best);
    }
    __device__ __forceinline__ void store(uint64_t c, uint32_t x) const { p.D[c] = x; }
};

__global__ __launch_bounds__(kPathThreads) void path_next_kernel(PathPlanes p, bt_path_cost cost, float cell_diag, const bt_path_goal* __restrict__ goals, uint32_t goal_count,
                                                                 PathCounts* __restrict__ counts) {
    const uint64_t cells = uint64_t(p.width) * p.height;
    const uint64_t i = uint64_t(blockIdx.x) * kPathThreads + threadIdx.x;
    bool reachable = false;
    if (i < cells) {
        const int x = int(i % p.width), y = int(i / p.width);
        const float ha = p.h[i];
        const uint32_t dbits = p.D[i];
        uint32_t out = BT_PATH_UNREACHABLE;
        if (ha != ha) {
            out = BT_PATH_BLOCKED;
        } else if (dbits != kInfBits) {
            reachable = true;
            const float d = __uint_as_float(dbits);
            bool goal = false;
            if (p.next[i] == 1u) {  // some goal entry names the cell: the cheapest of them is the cell's goal cost
                for (uint32_t g = 0; g < goal_count; g++)
                    if (goals[g].x == uint32_t(x) && goals[g].y == uint32_t(y) && goals[g].cost0 == d) goal = true;
            }
            if (goal) {
                out = BT_PATH_GOAL;
            } else {
                auto height = [&](int cx, int cy) { return cx >= 0 && cy >= 0 && cx < int(p.width) && cy < int(p.height) ? p.h[uint64_t(cy) * p.width + uint32_t(cx)] : __builtin_nanf(""); };
                for (int k = 7; k >= 0; k--) {
                    const int nx = x + neighbour_dx(k), ny = y + neighbour_dy(k);
                    const float hb = height(nx, ny);
                    if (hb != hb) continue;
                    if (k & 1) {
                        const float hx = height(nx, y), hy = height(x, ny);
                        if (hx != hx || hy != hy) continue;
                    }
                    const float wk = path_weight(ha, hb, (k & 1) ? cell_diag : cost.cell_size, cost);
                    if (__uint_as_float(p.D[uint64_t(ny) * p.width + uint32_t(nx)]) + wk == d) out = uint32_t(k);  // descending k: the smallest stays
                }
            }
        }
        p.next[i] = uint8_t(out);
    }
    const uint32_t reachable_here = __syncthreads_count(reachable);
    if (threadIdx.x == 0 && reachable_here) atomicAdd(&counts->reachable, reachable_here);
}

}  // namespace

bt_status launch_path_prepare(hipStream_t stream, const PathPlanes& p, const bt_path_cost& cost, const bt_path_goal* goals, uint32_t goal_count, uint32_t* flags, PathCounts* counts) {
    const uint64_t threads = std::max<uint64_t>(uint64_t(p.width) * p.height, goal_count);
    path_prepare_kernel<<<dim3(uint32_t((threads + kPathThreads - 1u) / kPathThreads)), kPathThreads, 0, stream>>>(p, cost, goals, goal_count, flags, counts);
    return launched("path_prepare_kernel");
}

bt_status launch_path_relax(hipStream_t stream, const PathPlanes& p, const bt_path_cost& cost, float cell_diag, uint32_t rounds, uint32_t* active, uint32_t* activate, uint32_t* marked) {
    relax_kernel<<<dim3(p.blocks_x, p.blocks_y), kRelaxThreads, 0, stream>>>(PathRule{p, cost, cell_diag}, RelaxGrid(p), rounds, active, activate, marked);
    return launched("path_relax_kernel");  // relax_kernel<PathRule>, under the name bt_last_error() has always given it
}

bt_status launch_path_next(hipStream_t stream, const PathPlanes& p, const bt_path_cost& cost, float cell_diag, const bt_path_goal* goals, uint32_t goal_count, PathCounts* counts) {
    const uint64_t cells = uint64_t(p.width) * p.height;
    path_next_kernel<<<dim3(uint32_t((cells + kPathThreads - 1u) / kPathThreads)), kPathThreads, 0, stream>>>(p, cost, cell_diag, goals, goal_count, counts);
    return launched("path_next_kernel");
}

}  // namespace bt

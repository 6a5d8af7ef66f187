// bt_atlas_path_field: the kernels.  The host half is bt_path.cpp; the definition is the PATH FIELD section of include/bevy_terrain_amd.h.
//
// path_prepare_kernel  raw texels + the caller's mask -> the height plane (NaN = blocked; a free cell's height is finite, the host refuses
//                      what could make it otherwise) and the count of blocked cells; the goal list -> D by atomicMin on the bits
//                      (non-negative floats order as their bit patterns), a mark in the next plane on every cell a goal names, and the
//                      flags of the 3 x 3 blocks around it (a goal on a block's edge may change nothing inside its own block).
// path_relax_kernel    one sweep.  A workgroup owns kPathBlock x kPathBlock cells; it leaves at once unless its flag is set.  It stages
//                      heights and D of its cells plus a one-cell halo in LDS (NaN / +inf outside the window), forms the eight weights of
//                      each of its cells once, in registers, and relaxes in LDS until nothing changed in the workgroup or `rounds`
//                      rounds (kPathRounds) have run.  It writes back the cells it lowered (one writer per cell: no global atomics), and flags the
//                      blocks whose halo those cells are in, and itself when it stopped at the round limit.  A halo value read while a
//                      neighbour rewrites it, or a stale one, is still the cost of a real path, so the fixed point does not move; the
//                      loads and stores are aligned dwords.  Sweeps are ordered by the kernel boundary alone.
// path_next_kernel     the next plane by the header's rule, and the count of reachable cells.
//
// Arithmetic contract: IEEE binary32, one rounding per written operation; this file is compiled with -ffp-contract=off, `/` is the
// correctly rounded division.
#include "bt_internal.hpp"

namespace bt {

namespace {

constexpr uint32_t kPathThreads = 256;
constexpr uint32_t kPathTile = kPathBlock + 2u;   // the block and its halo
constexpr uint32_t kPathOwn = kPathBlock * kPathBlock / kPathThreads;  // cells of a thread: rows ly, ly + 8, ly + 16, ly + 24
constexpr uint32_t kInfBits = 0x7F800000u;
// neighbour k = 0..7: (1,0), (1,1), (0,1), (-1,1), (-1,0), (-1,-1), (0,-1), (1,-1)
__host__ __device__ constexpr int path_dx(int k) { return k == 0 || k == 1 || k == 7 ? 1 : k >= 3 && k <= 5 ? -1 : 0; }
__host__ __device__ constexpr int path_dy(int k) { return k >= 1 && k <= 3 ? 1 : k >= 5 ? -1 : 0; }

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
            const uint32_t bx = g.x / kPathBlock, by = g.y / kPathBlock;
            for (int dy = -1; dy <= 1; dy++)
                for (int dx = -1; dx <= 1; dx++) {
                    const uint32_t nx = bx + uint32_t(dx), ny = by + uint32_t(dy);  // wraps below 0: fails the test
                    if (nx < p.blocks_x && ny < p.blocks_y) flags[ny * p.blocks_x + nx] = 1u;
                }
        }
    }
}

// bits of the flag mask a block collects: the neighbour blocks in whose halo a lowered cell lies, and the block itself
enum : uint32_t { kLeft = 1, kRight = 2, kUp = 4, kDown = 8, kUpLeft = 16, kUpRight = 32, kDownLeft = 64, kDownRight = 128, kSelf = 256 };

__global__ __launch_bounds__(kPathThreads) void path_relax_kernel(PathPlanes p, bt_path_cost cost, float cell_diag, uint32_t rounds, uint32_t* active, uint32_t* activate, uint32_t* marked) {
    const uint32_t block = blockIdx.y * p.blocks_x + blockIdx.x;
    if (active[block] == 0u) return;  // the same word for every thread, and only this workgroup writes it (below, behind a barrier)
    __shared__ float s_h[kPathTile * kPathTile];
    __shared__ float s_d[kPathTile * kPathTile];
    __shared__ uint32_t s_mask;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) s_mask = 0u;
    const int gx0 = int(blockIdx.x * kPathBlock) - 1, gy0 = int(blockIdx.y * kPathBlock) - 1;
    for (uint32_t i = tid; i < kPathTile * kPathTile; i += kPathThreads) {
        const int gx = gx0 + int(i % kPathTile), gy = gy0 + int(i / kPathTile);
        float h = __builtin_nanf(""), d = __builtin_inff();
        if (gx >= 0 && gy >= 0 && gx < int(p.width) && gy < int(p.height)) {
            const uint64_t c = uint64_t(gy) * p.width + uint32_t(gx);
            h = p.h[c];
            d = __uint_as_float(p.D[c]);
        }
        s_h[i] = h;
        s_d[i] = d;
    }
    __syncthreads();
    if (tid == 0) active[block] = 0u;

    const uint32_t lx = tid % kPathBlock, ly0 = tid / kPathBlock;
    float w[kPathOwn][8], d[kPathOwn], d_in[kPathOwn];
#pragma unroll
    for (uint32_t j = 0; j < kPathOwn; j++) {
        const uint32_t t = (ly0 + j * (kPathThreads / kPathBlock) + 1u) * kPathTile + lx + 1u;
        const float ha = s_h[t];
        d[j] = d_in[j] = s_d[t];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const float hb = s_h[int(t) + path_dy(k) * int(kPathTile) + path_dx(k)];
            float wk = path_weight(ha, hb, (k & 1) ? cell_diag : cost.cell_size, cost);
            if (k & 1) {  // no corner cutting: both cells beside the diagonal are free
                const float hx = s_h[int(t) + path_dx(k)], hy = s_h[int(t) + path_dy(k) * int(kPathTile)];
                if (hx != hx || hy != hy) wk = __builtin_inff();
            }
            w[j][k] = wk;
        }
    }
    int more = 1;
    for (uint32_t round = 0; round < rounds && more; round++) {
        int lowered = 0;
#pragma unroll
        for (uint32_t j = 0; j < kPathOwn; j++) {
            const uint32_t t = (ly0 + j * (kPathThreads / kPathBlock) + 1u) * kPathTile + lx + 1u;
            float best = d[j];
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const float cand = s_d[int(t) + path_dy(k) * int(kPathTile) + path_dx(k)] + w[j][k];
                if (cand < best) best = cand;
            }
            if (best < d[j]) {
                d[j] = best;
                s_d[t] = best;
                lowered = 1;
            }
        }
        more = __syncthreads_or(lowered);
    }
    uint32_t mask = 0u;
#pragma unroll
    for (uint32_t j = 0; j < kPathOwn; j++) {
        if (!(d[j] < d_in[j])) continue;
        const uint32_t ly = ly0 + j * (kPathThreads / kPathBlock);
        p.D[uint64_t(blockIdx.y * kPathBlock + ly) * p.width + blockIdx.x * kPathBlock + lx] = __float_as_uint(d[j]);  // inside the window: a cell outside is NaN and never lowered
        const bool l = lx == 0u, r = lx == kPathBlock - 1u, u = ly == 0u, dn = ly == kPathBlock - 1u;
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
                    const int nx = x + path_dx(k), ny = y + path_dy(k);
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

bt_status path_launched(const char* what) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? BT_OK : hip_fail(e, what);
}

}  // namespace

bt_status launch_path_prepare(hipStream_t stream, const PathPlanes& p, const bt_path_cost& cost, const bt_path_goal* goals, uint32_t goal_count, uint32_t* flags, PathCounts* counts) {
    const uint64_t threads = std::max<uint64_t>(uint64_t(p.width) * p.height, goal_count);
    path_prepare_kernel<<<dim3(uint32_t((threads + kPathThreads - 1u) / kPathThreads)), kPathThreads, 0, stream>>>(p, cost, goals, goal_count, flags, counts);
    return path_launched("path_prepare_kernel");
}

bt_status launch_path_relax(hipStream_t stream, const PathPlanes& p, const bt_path_cost& cost, float cell_diag, uint32_t rounds, uint32_t* active, uint32_t* activate, uint32_t* marked) {
    path_relax_kernel<<<dim3(p.blocks_x, p.blocks_y), kPathThreads, 0, stream>>>(p, cost, cell_diag, rounds, active, activate, marked);
    return path_launched("path_relax_kernel");
}

bt_status launch_path_next(hipStream_t stream, const PathPlanes& p, const bt_path_cost& cost, float cell_diag, const bt_path_goal* goals, uint32_t goal_count, PathCounts* counts) {
    const uint64_t cells = uint64_t(p.width) * p.height;
    path_next_kernel<<<dim3(uint32_t((cells + kPathThreads - 1u) / kPathThreads)), kPathThreads, 0, stream>>>(p, cost, cell_diag, goals, goal_count, counts);
    return path_launched("path_next_kernel");
}

}  // namespace bt

// bt_atlas_label_regions: the kernels.  The host half is in bt_edit.cpp, beside bt_atlas_distance_field; the definition is the REGIONS
// section of include/bevy_terrain_amd.h.
//
// A union-find over the u32 parent plane P of the window.  P[c] <= c at all times and a link is only ever made from a root to a smaller
// index, so no cycle can form and the root of a finished region is its smallest cell: the label needs no tie rule.  Six launches, each
// ordered by the kernel boundary alone; their number does not depend on the texels.
// regions_local_kernel      a workgroup of 256 lanes to a block of 32 x 32 cells, four cells a lane (cell k of the block at lane k % 256,
//                           so a row of the block is one half-wave's line of LDS).  v and the member bit are staged in LDS, the block's
//                           own components resolved there (every member united with its left and upper neighbours, with EIGHT its
//                           upper-left and upper-right ones, by LDS atomicMin), and P[c] written as the window index of the local root,
//                           NONE for the rest.  Nothing global is contended.
// regions_seam_kernel       a wave to a block: a lane to each cell of its last column and of its last row, united with the linked
//                           neighbours across the seam (the last column: right, with EIGHT up-right and down-right; the last row: down,
//                           with EIGHT down-left and down-right; at a four-block corner that reaches the diagonal blocks).
// regions_flatten_kernel    from here on in linear index order, a workgroup to a chunk of 1024 consecutive cells, so that ranks come out
//                           row-major.  label(c) = find(c), written to the lane's own cell only; the chunk's roots are counted and ranked
//                           within the chunk, the members counted, the areas added into a plane indexed by label.
// regions_scan_kernel       one workgroup: the exclusive prefix sums of the chunks' root counts and their total.  No atomics.
// regions_emit_kernel       id(c) = the chunk offset of its label + the label's rank in that chunk; and every member of a region whose id
//                           is below region_cap folded into that region's accumulators.
// regions_finish_kernel     the largest region, the baked byte merged into the staged destination texels, and the accumulators written
//                           out as bt_region records.
//
// The global union (seam kernel) is the usual loop: find both roots, and while they differ old = atomicMin(&P[larger], smaller), relaxed,
// agent scope; the link is made if old == larger, otherwise the loop goes on from old (the cell that `larger` hung under in the meantime
// must end up in the same tree as `smaller`, and uniting the two does that).  A stale load is harmless: every value ever stored in P[c] is
// a cell of c's region with an index <= c, so a find that starts from one only starts elsewhere in the same tree, and whether a link was
// made is decided by the atomic's return value alone.  Hence no fence and no flag.
//
// Sums, minima and maxima are integer atomics: no result depends on a schedule.  Adds to one address are serial (about 14 ns each was
// measured: profiles/regions.txt), so what shares a label is reduced before it is added.  Lanes of a wave hold 64 consecutive cells: runs of
// neighbouring lanes with one label are reduced by a segmented scan (six steps whatever the number of runs); the runs that carry the
// label of the wave's first run are reduced across the wave, and those of the workgroup's sixteen waves-times-trips through LDS, so a
// corridor that crosses a chunk many times, or a region that fills it, adds once per chunk: 2^12 adds for a region of 2^22 cells.  The
// runs of other labels add one by one.
#include "bt_internal.hpp"

namespace bt {

namespace {

constexpr uint32_t kRegionsThreads = 256;
constexpr uint32_t kWave = 64;
constexpr uint32_t kBlock = kRegionsBlock;        // cells across a block of the local launch
constexpr uint32_t kBlockCells = kBlock * kBlock;
constexpr uint32_t kChunk = kRegionsChunk;        // cells of a chunk of the linear launches
constexpr uint32_t kCellsPerLane = kChunk / kRegionsThreads;
constexpr uint32_t kSegments = kChunk / kWave;    // the 64 consecutive cells a wave holds at a time, of a chunk
constexpr uint32_t kNone = BT_REGIONS_NONE;
constexpr uint32_t kMemberBit = 1u << 16;         // of a staged value
static_assert(kBlockCells == kChunk && kCellsPerLane == 4u && kBlock == 32u, "four cells a lane in both layouts");

__device__ __forceinline__ uint32_t value_at(const RegionsPlanes& p, uint32_t i) {
    const uint32_t t = p.wide ? ((const uint32_t*)p.raw)[i] : uint32_t(((const uint16_t*)p.raw)[i]);
    return (t >> p.shift) & p.value_mask;
}

__device__ __forceinline__ bool is_member(const RegionsPlanes& p, uint32_t i, uint32_t v) {
    const bool m = (p.lo <= v && v <= p.hi) || (p.host && p.host[i] != 0u);
    return m != (p.invert != 0u);
}

__device__ __forceinline__ bool within_step(const RegionsPlanes& p, uint32_t a, uint32_t b) { return (a > b ? a - b : b - a) <= p.max_step; }

// relaxed loads and stores of a parent plane that other lanes unite in at the same time
template <int kScope>
__device__ __forceinline__ uint32_t parent_of(const uint32_t* P, uint32_t c) {
    return __hip_atomic_load(P + c, __ATOMIC_RELAXED, kScope);
}

template <int kScope>
__device__ __forceinline__ uint32_t find_root(const uint32_t* P, uint32_t c) {
    for (uint32_t q; (q = parent_of<kScope>(P, c)) != c;) c = q;  // P[c] <= c: the chain falls until it stands
    return c;
}

// a and b, two members, into one tree
template <int kScope>
__device__ __forceinline__ void unite(uint32_t* P, uint32_t a, uint32_t b) {
    for (;;) {
        a = find_root<kScope>(P, a), b = find_root<kScope>(P, b);
        if (a == b) return;
        const uint32_t larger = max(a, b), smaller = min(a, b);
        const uint32_t old = __hip_atomic_fetch_min(P + larger, smaller, __ATOMIC_RELAXED, kScope);
        if (old == larger) return;  // it was a root and hangs under `smaller` now
        a = old, b = smaller;       // it was none any more: what it hung under and `smaller` are still to be united
    }
}

__global__ __launch_bounds__(kRegionsThreads) void regions_local_kernel(RegionsPlanes p) {
    __shared__ uint32_t parent[kBlockCells];
    __shared__ uint32_t staged[kBlockCells];  // v | kMemberBit
    const uint32_t bx = blockIdx.x * kBlock, by = blockIdx.y * kBlock;
    for (uint32_t j = 0; j < kCellsPerLane; j++) {
        const uint32_t k = j * kRegionsThreads + threadIdx.x, x = bx + k % kBlock, y = by + k / kBlock;
        uint32_t s = 0u;
        if (x < p.width && y < p.height) {
            const uint32_t i = y * p.width + x, v = value_at(p, i);
            s = v | (is_member(p, i, v) ? kMemberBit : 0u);
            p.area[i] = 0u;
        }
        staged[k] = s;
        parent[k] = (s & kMemberBit) ? k : kNone;
    }
    __syncthreads();
    for (uint32_t j = 0; j < kCellsPerLane; j++) {
        const uint32_t k = j * kRegionsThreads + threadIdx.x, lx = k % kBlock, ly = k / kBlock, s = staged[k];
        if (!(s & kMemberBit)) continue;
        auto link = [&](uint32_t n) {
            const uint32_t t = staged[n];
            if ((t & kMemberBit) && within_step(p, s & 0xFFFFu, t & 0xFFFFu)) unite<__HIP_MEMORY_SCOPE_WORKGROUP>(parent, k, n);
        };
        if (lx > 0u) link(k - 1u);
        if (ly > 0u) link(k - kBlock);
        if (p.eight && ly > 0u) {
            if (lx > 0u) link(k - kBlock - 1u);
            if (lx + 1u < kBlock) link(k - kBlock + 1u);
        }
    }
    __syncthreads();
    for (uint32_t j = 0; j < kCellsPerLane; j++) {  // the flatten: reads of `parent` only
        const uint32_t k = j * kRegionsThreads + threadIdx.x, x = bx + k % kBlock, y = by + k / kBlock;
        if (x >= p.width || y >= p.height) continue;
        uint32_t root = kNone;
        if (staged[k] & kMemberBit) {
            const uint32_t r = find_root<__HIP_MEMORY_SCOPE_WORKGROUP>(parent, k);
            root = (by + r / kBlock) * p.width + bx + r % kBlock;
        }
        p.P[y * p.width + x] = root;
    }
}

__global__ __launch_bounds__(kWave) void regions_seam_kernel(RegionsPlanes p) {
    const uint32_t t = threadIdx.x, column = t < kBlock;  // the lanes of the last column, then those of the last row
    const uint32_t x = blockIdx.x * kBlock + (column ? kBlock - 1u : t - kBlock), y = blockIdx.y * kBlock + (column ? t : kBlock - 1u);
    if (x >= p.width || y >= p.height) return;
    const uint32_t i = y * p.width + x, v = value_at(p, i);
    if (!is_member(p, i, v)) return;
    auto link = [&](int dx, int dy) {
        const int nx = int(x) + dx, ny = int(y) + dy;
        if (nx < 0 || ny < 0 || nx >= int(p.width) || ny >= int(p.height)) return;
        const uint32_t n = uint32_t(ny) * p.width + uint32_t(nx), w = value_at(p, n);
        if (is_member(p, n, w) && within_step(p, v, w)) unite<__HIP_MEMORY_SCOPE_AGENT>(p.P, i, n);
    };
    if (column) {
        link(1, 0);
        if (p.eight) link(1, -1), link(1, 1);
    } else {
        link(0, 1);
        if (p.eight) {
            link(-1, 1);
            if (t != kWave - 1u) link(1, 1);  // the corner cell's is the last column's
        }
    }
}

// The lanes of a wave hold consecutive cells.  A run: neighbouring lanes with one key.  *start: the first lane of this lane's run;
// returns whether this lane is the last of its run
__device__ __forceinline__ bool run_of(uint32_t key, uint32_t lane, uint32_t* start) {
    const uint32_t before = __shfl_up(key, 1);
    const unsigned long long heads = __ballot(lane == 0u || key != before);
    *start = 63u - uint32_t(__clzll(heads & (~0ull >> (63u - lane))));
    return lane == kWave - 1u || ((heads >> (lane + 1u)) & 1u);
}

__global__ __launch_bounds__(kRegionsThreads) void regions_flatten_kernel(RegionsPlanes p, RegionsCounts* __restrict__ counts) {
    __shared__ uint32_t roots_of[kSegments], members_of[kSegments], lead_of[kSegments], lead_area[kSegments];
    const uint32_t cells = p.width * p.height, lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    uint32_t label[kCellsPerLane];
    unsigned long long root_lanes[kCellsPerLane];
    for (uint32_t j = 0; j < kCellsPerLane; j++) {  // 64 consecutive cells are segment j * 4 + wave of the chunk
        const uint32_t i = blockIdx.x * kChunk + j * kRegionsThreads + threadIdx.x, segment = j * (kRegionsThreads / kWave) + wave;
        uint32_t L = kNone;
        if (i < cells && parent_of<__HIP_MEMORY_SCOPE_AGENT>(p.P, i) != kNone) {
            L = find_root<__HIP_MEMORY_SCOPE_AGENT>(p.P, i);
            __hip_atomic_store(p.P + i, L, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // its own cell only: what others read there stays an ancestor
        }
        label[j] = L;
        root_lanes[j] = __ballot(L == i && L != kNone);
        const unsigned long long member_lanes = __ballot(L != kNone);
        // the areas: a run adds once; the runs of the wave's first label add once for the wave, and (below) once for the workgroup
        uint32_t start;
        const bool tail = run_of(L, lane, &start) && L != kNone;
        const unsigned long long tails = __ballot(tail);
        const uint32_t lead = tails ? __shfl(L, __ffsll(tails) - 1) : kNone;
        uint32_t n = tail && L == lead ? lane - start + 1u : 0u;
        for (uint32_t off = kWave / 2u; off > 0u; off >>= 1) n += __shfl_xor(n, off);
        if (tail && L != lead) atomicAdd(&p.area[L], lane - start + 1u);
        if (lane == 0u) {
            roots_of[segment] = uint32_t(__popcll(root_lanes[j])), members_of[segment] = uint32_t(__popcll(member_lanes));
            lead_of[segment] = lead, lead_area[segment] = n;
        }
    }
    __syncthreads();
    for (uint32_t j = 0; j < kCellsPerLane; j++) {
        const uint32_t i = blockIdx.x * kChunk + j * kRegionsThreads + threadIdx.x, segment = j * (kRegionsThreads / kWave) + wave;
        if (label[j] != i || label[j] == kNone) continue;
        uint32_t rank = uint32_t(__popcll(root_lanes[j] & ((1ull << lane) - 1ull)));
        for (uint32_t s = 0; s < segment; s++) rank += roots_of[s];
        p.rank[i] = rank;
    }
    if (threadIdx.x < kSegments && lead_of[threadIdx.x] != kNone) {  // the first segment with a label adds for every segment with it
        const uint32_t s = threadIdx.x, L = lead_of[s];
        bool first = true;
        for (uint32_t t = 0; t < s; t++) first = first && lead_of[t] != L;
        if (first) {
            uint32_t n = 0u;
            for (uint32_t t = s; t < kSegments; t++) n += lead_of[t] == L ? lead_area[t] : 0u;
            atomicAdd(&p.area[L], n);
        }
    }
    if (threadIdx.x == 0u) {
        uint32_t roots = 0u, members = 0u;
        for (uint32_t s = 0; s < kSegments; s++) roots += roots_of[s], members += members_of[s];
        p.chunk_roots[blockIdx.x] = roots;
        if (members) atomicAdd(&counts->members, members);
    }
}

__global__ __launch_bounds__(kRegionsThreads) void regions_scan_kernel(RegionsPlanes p, RegionsCounts* __restrict__ counts) {
    __shared__ uint32_t sums[kRegionsThreads];
    const uint32_t chunks = (p.width * p.height + kChunk - 1u) / kChunk, per = (chunks + kRegionsThreads - 1u) / kRegionsThreads;
    const uint32_t first = min(threadIdx.x * per, chunks), end = min(first + per, chunks);
    uint32_t sum = 0u;
    for (uint32_t c = first; c < end; c++) sum += p.chunk_roots[c];
    sums[threadIdx.x] = sum;
    __syncthreads();
    uint32_t before = 0u;
    for (uint32_t t = 0; t < threadIdx.x; t++) before += sums[t];
    for (uint32_t c = first; c < end; c++) {
        const uint32_t own = p.chunk_roots[c];
        p.chunk_roots[c] = before;
        before += own;
    }
    if (threadIdx.x == kRegionsThreads - 1u) counts->regions = before;
}

// what some cells of one region add to its record
struct RegionFold {
    uint32_t n, x_min, y_min, x_max, y_max, v_min, v_max, v_sum, edges;  // at most 1024 cells: the sum of v fits
};

__device__ __forceinline__ RegionFold nothing_folded() { return RegionFold{0u, kNone, kNone, 0u, 0u, kNone, 0u, 0u, 0u}; }

__device__ __forceinline__ RegionFold folded(const RegionFold& a, const RegionFold& b) {
    return RegionFold{a.n + b.n, min(a.x_min, b.x_min), min(a.y_min, b.y_min), max(a.x_max, b.x_max), max(a.y_max, b.y_max), min(a.v_min, b.v_min), max(a.v_max, b.v_max),
                      a.v_sum + b.v_sum, a.edges + b.edges};
}

template <typename Shuffle>
__device__ __forceinline__ RegionFold shuffled(const RegionFold& f, Shuffle&& sh) {
    return RegionFold{sh(f.n), sh(f.x_min), sh(f.y_min), sh(f.x_max), sh(f.y_max), sh(f.v_min), sh(f.v_max), sh(f.v_sum), sh(f.edges)};
}

__device__ __forceinline__ void add_to(RegionAccum* r, const RegionFold& f) {
    atomicAdd(&r->area, f.n);
    atomicMax(&r->not_x_min, ~f.x_min), atomicMax(&r->not_y_min, ~f.y_min), atomicMax(&r->not_v_min, ~f.v_min);
    atomicMax(&r->x_max, f.x_max), atomicMax(&r->y_max, f.y_max), atomicMax(&r->v_max, f.v_max);
    if (f.edges) atomicAdd(&r->edges, f.edges);
    if (f.v_sum) atomicAdd(&r->v_sum, (unsigned long long)f.v_sum);
}

__global__ __launch_bounds__(kRegionsThreads) void regions_emit_kernel(RegionsPlanes p) {
    __shared__ uint32_t lead_of[kSegments];
    __shared__ RegionFold lead_fold[kSegments];
    const uint32_t cells = p.width * p.height, lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    for (uint32_t j = 0; j < kCellsPerLane; j++) {
        const uint32_t i = blockIdx.x * kChunk + j * kRegionsThreads + threadIdx.x;
        const bool inside = i < cells;
        const uint32_t L = inside ? p.P[i] : kNone;
        const uint32_t id = L != kNone ? p.chunk_roots[L / kChunk] + p.rank[L] : kNone;
        if (inside) p.id[i] = id;
        if (!p.region_cap) continue;
        // what this cell adds to its region's record
        const uint32_t key = id < p.region_cap ? id : kNone;  // NONE is above every cap
        RegionFold f = nothing_folded();
        if (key != kNone) {
            const uint32_t x = i % p.width, y = i / p.width, v = value_at(p, i);
            const uint32_t edges = uint32_t(x == 0u || p.P[i - 1u] != L) + uint32_t(x + 1u == p.width || p.P[i + 1u] != L) + uint32_t(y == 0u || p.P[i - p.width] != L) +
                                   uint32_t(y + 1u == p.height || p.P[i + p.width] != L);
            f = RegionFold{1u, x, y, x, y, v, v, v, edges};
            if (L == i) p.accum[key].label = L;  // the root's lane alone
        }
        // a run of equal keys first: a segmented scan, six steps whatever the number of runs; its last lane holds the run
        uint32_t start;
        const bool tail = run_of(key, lane, &start) && key != kNone;
        for (uint32_t off = 1u; off < kWave; off <<= 1) {
            const RegionFold below = shuffled(f, [off](uint32_t v) { return __shfl_up(v, off); });
            if (lane >= start + off) f = folded(f, below);  // the lane `off` below is of this run
        }
        // then the runs of the wave's first key into one (a corridor that crosses the wave many times), kept for the workgroup's fold below
        const unsigned long long tails = __ballot(tail);
        const uint32_t lead = tails ? __shfl(key, __ffsll(tails) - 1) : kNone;
        if (tail && key != lead) add_to(p.accum + key, f);
        RegionFold whole = tail && key == lead ? f : nothing_folded();
        if (lead != kNone)
            for (uint32_t off = kWave / 2u; off > 0u; off >>= 1) whole = folded(whole, shuffled(whole, [off](uint32_t v) { return __shfl_xor(v, off); }));
        if (lane == 0u) lead_of[j * (kRegionsThreads / kWave) + wave] = lead, lead_fold[j * (kRegionsThreads / kWave) + wave] = whole;
    }
    if (!p.region_cap) return;
    __syncthreads();
    if (threadIdx.x >= kSegments || lead_of[threadIdx.x] == kNone) return;
    const uint32_t s = threadIdx.x, key = lead_of[s];  // the first segment with a key adds for every segment with it
    for (uint32_t t = 0; t < s; t++)
        if (lead_of[t] == key) return;
    RegionFold f = lead_fold[s];
    for (uint32_t t = s + 1u; t < kSegments; t++)
        if (lead_of[t] == key) f = folded(f, lead_fold[t]);
    add_to(p.accum + key, f);
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
    for (uint32_t k = 1; k < kRegionsThreads / kWave; k++) v = kMax ? max(v, slot[k]) : v + slot[k];
    return v;
}

__global__ __launch_bounds__(kRegionsThreads) void regions_finish_kernel(RegionsPlanes p, RegionsBake bake, RegionsCounts* __restrict__ counts, bt_region* __restrict__ table) {
    __shared__ uint32_t slots[kRegionsThreads / kWave];
    __shared__ unsigned long long wide_slots[kRegionsThreads / kWave];
    const uint32_t cells = p.width * p.height;
    uint32_t baked = 0u;
    unsigned long long largest = 0u;  // area << 32 | ~label: the largest area, then the smallest label
    for (uint32_t j = 0; j < kCellsPerLane; j++) {
        const uint32_t i = blockIdx.x * kChunk + j * kRegionsThreads + threadIdx.x;
        if (i >= cells) break;
        const uint32_t L = p.P[i];
        if (L == kNone) continue;
        const uint32_t area = p.area[L];
        if (L == i) largest = max(largest, (unsigned long long)area << 32 | (kNone - L));
        if (bake.texels && bake.min_area <= area && area <= bake.max_area) {
            bake.texels[i] = (bake.texels[i] & ~(0xFFu << bake.shift)) | (bake.value << bake.shift);
            baked++;
        }
    }
    // the records: the accumulators of the regions the table holds, a thread to a record
    const uint32_t written = min(counts->regions, p.region_cap);
    for (uint32_t r = blockIdx.x * kRegionsThreads + threadIdx.x; r < written; r += gridDim.x * kRegionsThreads) {
        const RegionAccum a = p.accum[r];
        bt_region out;
        out.label = a.label, out.area = a.area;
        out.x_min = uint16_t(~a.not_x_min), out.y_min = uint16_t(~a.not_y_min), out.x_max = uint16_t(a.x_max), out.y_max = uint16_t(a.y_max);
        out.v_min = uint16_t(~a.not_v_min), out.v_max = uint16_t(a.v_max);
        out.edges = a.edges, out.v_sum = a.v_sum;
        table[r] = out;
    }
    baked = group_fold<false>(baked, slots), largest = group_fold<true>(largest, wide_slots);
    if (threadIdx.x != 0u) return;
    if (baked) atomicAdd(&counts->baked, baked);
    if (largest) atomicMax(&counts->largest, largest);
}

}  // namespace

bt_status launch_regions_label(hipStream_t stream, const RegionsPlanes& p, RegionsCounts* counts) {
    const dim3 blocks((p.width + kBlock - 1u) / kBlock, (p.height + kBlock - 1u) / kBlock);
    const uint32_t chunks = (p.width * p.height + kChunk - 1u) / kChunk;
    regions_local_kernel<<<blocks, kRegionsThreads, 0, stream>>>(p);
    if (bt_status s = launched("regions_local_kernel")) return s;
    regions_seam_kernel<<<blocks, kWave, 0, stream>>>(p);
    if (bt_status s = launched("regions_seam_kernel")) return s;
    regions_flatten_kernel<<<dim3(chunks), kRegionsThreads, 0, stream>>>(p, counts);
    if (bt_status s = launched("regions_flatten_kernel")) return s;
    regions_scan_kernel<<<dim3(1), kRegionsThreads, 0, stream>>>(p, counts);
    return launched("regions_scan_kernel");
}

bt_status launch_regions_emit(hipStream_t stream, const RegionsPlanes& p) {
    regions_emit_kernel<<<dim3((p.width * p.height + kChunk - 1u) / kChunk), kRegionsThreads, 0, stream>>>(p);
    return launched("regions_emit_kernel");
}

bt_status launch_regions_finish(hipStream_t stream, const RegionsPlanes& p, const RegionsBake& bake, RegionsCounts* counts, bt_region* table) {
    regions_finish_kernel<<<dim3((p.width * p.height + kChunk - 1u) / kChunk), kRegionsThreads, 0, stream>>>(p, bake, counts, table);
    return launched("regions_finish_kernel");
}

}  // namespace bt

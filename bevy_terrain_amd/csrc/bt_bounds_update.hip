// bt_height_bounds_update: the height-bounds table of the culling test brought up to date from a list of changed tiles.
//
// An entry is own(tile) united with the four children's entries, and own of a tile the atlas does not hold is own of its nearest held
// ancestor.  The table alone cannot be updated (own is gone once united), so the library keeps a shadow beside it (HeightBoundsImpl):
// own of every held tile, kBoundsNotHeld elsewhere.  With U the distinct listed tiles of the table's levels:
//   - own changes for U only: the grid-1 reduction of a held tile's layer (launch_tile_bounds, into device scratch), not-held otherwise;
//   - the filled own (own after the walk up to the nearest held tile) changes for U and for everything that looks up through a tile of U:
//     the subtrees below the children of U the atlas does not hold ("fill roots"), taken whole, down to the last level;
//   - the entry changes for those and for the ancestors of U.
// The host plan (bt_height_bounds.cpp: index arithmetic, O(count * levels)) turns that set into windows per level: a single entry, or the 2^s x 2^s square a fill
// root covers s levels below it.  Windows nested in a fill root's are dropped, so every entry has one writer.  The kernels:
//   scatter   shadow[slot] = the new own or not-held, for U;
//   fill      for every affected entry, of all levels at once: walk up the shadow to the nearest held tile (a root that is not held
//             gives (0, 65535)) and store the filled own in the table entry itself;
//   unite     per level from levels - 2 up to 0: entry = entry (its filled own) united with the four children's entries as they stand.
// At or below kBoundsUpdateSmall affected entries one workgroup runs all three with workgroup barriers in between (one launch); above it
// scatter, fill and every level's unite are launches of their own: kernel boundaries are the only order between workgroups.
#include "bt_height_bounds.hpp"

namespace bt {

namespace {

constexpr uint32_t kSmallThreads = 1024;  // the one workgroup of the small form
constexpr uint32_t kWideThreads = 256;

// the kernels' argument: BoundsUpdateArgs under the name, and in the unnamed namespace, that the kernels' symbols spell
struct UpdateArgs : BoundsUpdateArgs {};

__device__ __forceinline__ uint32_t level_offset(uint32_t sides, uint32_t level) { return sides * (((1u << (2u * level)) - 1u) / 3u); }

// entry `w` of the affected entries of `level` -> its table index and coordinate (windows: a.windows, or the small form's copy in LDS)
__device__ __forceinline__ uint32_t locate(const UpdateArgs& a, const Window* windows, uint32_t level, uint32_t w, uint32_t& side, uint32_t& x, uint32_t& y) {
    uint32_t lo = a.level_window[level], hi = a.level_window[level + 1u];  // the last window with first <= w
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) / 2u;
        if (windows[mid].first <= w) lo = mid;
        else hi = mid;
    }
    const Window win = windows[lo];
    const uint32_t shift = win.side_shift >> 8, local = w - win.first;
    side = win.side_shift & 0xFFu;
    x = win.x0 + (local & ((1u << shift) - 1u));
    y = win.y0 + (local >> shift);
    return level_offset(a.sides, level) + ((((side << level) + y) << level) + x);
}

__device__ void scatter_one(const UpdateArgs& a, uint32_t i) {
    const Scatter s = a.scatter[i];
    a.shadow[s.slot] = s.source == kNoSource ? kBoundsNotHeld : a.own[s.source];
}

// w: an index into the affected entries of all levels
__device__ __forceinline__ void fill_one(const UpdateArgs& a, const Window* windows, uint32_t w) {
    uint32_t level = 0;
    while (level + 1u < a.levels && a.level_work[level + 1u] <= w) level++;
    uint32_t side, x, y;
    const uint32_t slot = locate(a, windows, level, w - a.level_work[level], side, x, y);
    uint32_t v = a.shadow[slot];
    for (uint32_t l = level; v == kBoundsNotHeld && l > 0u;) {  // the nearest held ancestor's own
        l--;
        x >>= 1, y >>= 1;
        v = a.shadow[level_offset(a.sides, l) + ((((side << l) + y) << l) + x)];
    }
    a.table[slot] = v == kBoundsNotHeld ? 0xFFFF0000u : v;
}

// w: an index into the affected entries of `level` < levels - 1
__device__ __forceinline__ void unite_one(const UpdateArgs& a, const Window* windows, uint32_t level, uint32_t w) {
    uint32_t side, x, y;
    const uint32_t slot = locate(a, windows, level, w, side, x, y);
    const uint32_t v = a.table[slot], cl = level + 1u;
    const uint32_t c0 = level_offset(a.sides, cl) + ((((side << cl) + 2u * y) << cl) + 2u * x);
    uint32_t mn = v & 0xFFFFu, mx = v >> 16;
    for (uint32_t c : {c0, c0 + 1u, c0 + (1u << cl), c0 + (1u << cl) + 1u}) {
        const uint32_t e = a.table[c];
        mn = min(mn, e & 0xFFFFu);
        mx = max(mx, e >> 16);
    }
    a.table[slot] = mn | (mx << 16);
}

// the whole update in one workgroup: the barriers order the steps (and the levels) among its waves.  The windows (at most one per
// affected entry: kBoundsUpdateSmall * 16 bytes) are copied to LDS once, so the searches of every step stay out of global memory.
__global__ __launch_bounds__(kSmallThreads) void bounds_update_small(UpdateArgs a) {
    extern __shared__ uint32_t lds[];
    Window* windows = reinterpret_cast<Window*>(lds);
    for (uint32_t i = threadIdx.x; i < a.level_window[a.levels]; i += kSmallThreads) windows[i] = a.windows[i];
    for (uint32_t i = threadIdx.x; i < a.scatter_count; i += kSmallThreads) scatter_one(a, i);
    __syncthreads();
    for (uint32_t w = threadIdx.x; w < a.level_work[a.levels]; w += kSmallThreads) fill_one(a, windows, w);
    __syncthreads();
    for (uint32_t level = a.levels - 1u; level-- > 0u;) {
        const uint32_t work = a.level_work[level + 1u] - a.level_work[level];
        if (!work) continue;  // (uniform)
        for (uint32_t w = threadIdx.x; w < work; w += kSmallThreads) unite_one(a, windows, level, w);
        __syncthreads();
    }
}

__global__ __launch_bounds__(kWideThreads) void bounds_update_scatter(UpdateArgs a) {
    const uint32_t i = blockIdx.x * kWideThreads + threadIdx.x;
    if (i < a.scatter_count) scatter_one(a, i);
}

__global__ __launch_bounds__(kWideThreads) void bounds_update_fill(UpdateArgs a) {
    const uint32_t w = blockIdx.x * kWideThreads + threadIdx.x;
    if (w < a.level_work[a.levels]) fill_one(a, a.windows, w);
}

__global__ __launch_bounds__(kWideThreads) void bounds_update_unite(UpdateArgs a, uint32_t level) {
    const uint32_t w = blockIdx.x * kWideThreads + threadIdx.x;
    if (w < a.level_work[level + 1u] - a.level_work[level]) unite_one(a, a.windows, level, w);
}

}  // namespace

uint32_t launch_bounds_update(hipStream_t stream, const BoundsUpdateArgs& host_args) {
    UpdateArgs args;
    static_cast<BoundsUpdateArgs&>(args) = host_args;
    const uint32_t windows = args.level_window[args.levels], total = args.level_work[args.levels];
    if (total <= kBoundsUpdateSmall) {
        bounds_update_small<<<1, kSmallThreads, windows * sizeof(Window), stream>>>(args);
        return 1;
    }
    auto blocks = [](uint32_t n) { return (n + kWideThreads - 1u) / kWideThreads; };
    bounds_update_scatter<<<blocks(args.scatter_count), kWideThreads, 0, stream>>>(args);
    bounds_update_fill<<<blocks(total), kWideThreads, 0, stream>>>(args);
    uint32_t launches = 2;
    for (uint32_t l = args.levels - 1u; l-- > 0u;) {
        const uint32_t work = args.level_work[l + 1u] - args.level_work[l];
        if (!work) continue;
        bounds_update_unite<<<blocks(work), kWideThreads, 0, stream>>>(args, l);
        launches++;
    }
    return launches;
}

}  // namespace bt

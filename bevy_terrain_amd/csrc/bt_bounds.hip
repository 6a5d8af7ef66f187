// Per-tile min/max height pyramids of R16 atlas layers (bt_atlas_tile_bounds).
//
// Cell (cx, cy) of level k (size s_k = (T / g) << k) covers texels x in [cx*s_k, min((cx+1)*s_k, T-1)], y likewise: its own block plus
// the first column to its right and the first row below it (the max-mipmap rule: every bilinear patch whose top-left texel lies in the
// block).  With this rule a level-(k+1) cell is exactly the min / max of its four level-k children.
//
// One workgroup per listed layer.  Level 0 is reduced into LDS by ds_min_u32 / ds_max_u32 (order-independent, so the result is
// deterministic), the coarser levels are composed from it in LDS, and the layer's whole pyramid leaves in one coalesced write.
//
// Fast path (T % 8 == 0 and s % 8 == 0 with s dividing 512 or a multiple of it): each lane loads 8 texels (16 bytes) of a row, a wave
// one 512-texel row segment per instruction.  A lane keeps the elementwise min / max of its 8 columns over the rows of the current cell
// row (v_pk_min_u16 / v_pk_max_u16), so the first of its columns is at hand for the cell to the left.  At the end of a cell row the lanes
// of one cell combine by __shfl_xor over s/8 lanes (at most the wave) and one lane merges the cell into LDS; a lane whose first column
// starts a cell also merges that column into the cell to its left.  The row below a cell row is the next cell row's first row: a band
// reads it once more only when it ends on a cell boundary, so every texel is read once apart from one row per band.
// Plain path (any other T or s): every texel merges into each of the up to four cells that cover it.
//
// BT_BOUNDS_SKIP_ZERO: minimums are taken over v - 1 (mod 2^16), which sends 0 above every other value; 0xFFFF then means "no texel",
// and the output adds the 1 back.  Maximums need nothing: 0 is their identity.
#include "bt_internal.hpp"

namespace bt {

namespace {

typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kBoundsThreads = 512;  // 8 waves; one layer per workgroup

struct BoundsArgs {
    const uint16_t* atlas;
    const uint32_t* layers;  // count entries
    uint32_t* out;           // count * cells words: (min | max << 16) per cell, levels finest first
    uint32_t T, s, g, cells, skip_zero;
};

__device__ __forceinline__ u16x2 as_u16x2(uint32_t v) { return __builtin_bit_cast(u16x2, v); }

// the stored minimum of a cell: the texel minimum, or (skip-zero) the minimum of v - 1 -> the texel minimum, 0xFFFF for no texel
__device__ __forceinline__ uint32_t out_min(uint32_t m, uint32_t skip_zero) { return skip_zero && m != 0xFFFFu ? m + 1u : m; }

__device__ __forceinline__ void merge_cell(uint32_t* lmin, uint32_t* lmax, uint32_t cell, uint32_t mn, uint32_t mx) {
    atomicMin(&lmin[cell], mn);
    atomicMax(&lmax[cell], mx);
}

// Level 0 by the fast path: (band of the layer's rows, one per wave, + its closing boundary row) x 512-texel row segment.
__device__ void level0_fast(const BoundsArgs& a, const uint16_t* __restrict__ tile, uint32_t* lmin, uint32_t* lmax) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t T = a.T, s = a.s, g = a.g;
    const uint32_t chunks = T / 8u;                 // 8-texel chunks per row
    const uint32_t segments = (chunks + 63u) / 64u; // 512-texel row segments
    const uint32_t bands = kBoundsThreads / 64u;
    const uint32_t band_rows = (T + bands - 1u) / bands;
    const uint32_t width = min(s / 8u, 64u);        // lanes of one cell inside a segment (a power of two)
    const u16x2 zero_pair = as_u16x2(0u), one_pair = as_u16x2(0x00010001u);
    for (uint32_t item = wave; item < bands * segments; item += bands) {
        const uint32_t band = item / segments, seg = item % segments;
        const uint32_t r0 = band * band_rows;
        if (r0 >= T) continue;
        const uint32_t r1 = min(r0 + band_rows, T);
        const uint32_t last = (r1 < T && r1 % s == 0u) ? r1 : r1 - 1u;  // the closing boundary row is read by this band too
        const uint32_t chunk = seg * 64u + lane;
        const bool valid = chunk < chunks;
        const uint32_t x = chunk * 8u;
        const uint32_t cx = x / s;
        const u32x4* src = reinterpret_cast<const u32x4*>(tile + x);
        u16x2 mn[4], mx[4];
        auto reset = [&]() {
            for (int j = 0; j < 4; j++) {
                mn[j] = as_u16x2(0xFFFFFFFFu);
                mx[j] = zero_pair;
            }
        };
        auto merge_row = [&](const u32x4& v) {
            for (int j = 0; j < 4; j++) {
                u16x2 t = as_u16x2(v[j]);
                mx[j] = __builtin_elementwise_max(mx[j], t);
                if (a.skip_zero) t = t - one_pair;  // v_pk_sub_u16: 0 -> 0xFFFF
                mn[j] = __builtin_elementwise_min(mn[j], t);
            }
        };
        // one cell row's accumulators -> LDS cells (cy, *)
        auto flush = [&](uint32_t cy) {
            const u16x2 m2 = __builtin_elementwise_min(__builtin_elementwise_min(mn[0], mn[1]), __builtin_elementwise_min(mn[2], mn[3]));
            const u16x2 x2 = __builtin_elementwise_max(__builtin_elementwise_max(mx[0], mx[1]), __builtin_elementwise_max(mx[2], mx[3]));
            uint32_t p = uint32_t(min(m2[0], m2[1])) | (uint32_t(max(x2[0], x2[1])) << 16);
            for (uint32_t off = 1; off < width; off <<= 1) {
                const uint32_t q = __shfl_xor(p, int(off));
                p = min(p & 0xFFFFu, q & 0xFFFFu) | (max(p >> 16, q >> 16) << 16);
            }
            if (!valid) return;
            if ((lane & (width - 1u)) == 0u) merge_cell(lmin, lmax, cy * g + cx, p & 0xFFFFu, p >> 16);
            if (x % s == 0u && x > 0u) merge_cell(lmin, lmax, cy * g + cx - 1u, mn[0][0], mx[0][0]);  // column x closes the cell to the left
        };
        reset();
        uint32_t cy = r0 / s;
        bool pending = false;  // rows merged since the last flush
        constexpr uint32_t kBatch = 8;  // rows in flight per lane
        for (uint32_t y0 = r0; y0 <= last; y0 += kBatch) {
            u32x4 rows[kBatch];
#pragma unroll
            for (uint32_t i = 0; i < kBatch; i++) {
                const uint32_t y = y0 + i;
                rows[i] = (valid && y <= last) ? src[uint64_t(y) * chunks] : u32x4{0u, 0u, 0u, 0u};
            }
#pragma unroll
            for (uint32_t i = 0; i < kBatch; i++) {
                const uint32_t y = y0 + i;
                if (y > last) break;
                merge_row(rows[i]);
                pending = true;
                if (y > r0 && y % s == 0u) {  // row y closes cell row y/s - 1 and, unless it is the band's closing row r1, opens y/s
                    flush(cy);
                    cy = y / s;
                    reset();
                    pending = y < r1;
                    if (pending) merge_row(rows[i]);
                }
            }
        }
        if (pending) flush(cy);
    }
}

// Level 0 by the plain path: every texel into the up to four cells that cover it.
__device__ void level0_plain(const BoundsArgs& a, const uint16_t* __restrict__ tile, uint32_t* lmin, uint32_t* lmax) {
    const uint32_t T = a.T, s = a.s, g = a.g;
    const uint64_t texels = uint64_t(T) * T;
    for (uint64_t i = threadIdx.x; i < texels; i += kBoundsThreads) {
        const uint32_t y = uint32_t(i / T), x = uint32_t(i % T);
        const uint32_t v = tile[i];
        const uint32_t mn = a.skip_zero ? ((v - 1u) & 0xFFFFu) : v;
        const uint32_t cx = min(x / s, g - 1u), cy = min(y / s, g - 1u);
        const bool left = x % s == 0u && x > 0u, up = y % s == 0u && y > 0u;
        merge_cell(lmin, lmax, cy * g + cx, mn, v);
        if (left) merge_cell(lmin, lmax, cy * g + cx - 1u, mn, v);
        if (up) merge_cell(lmin, lmax, (cy - 1u) * g + cx, mn, v);
        if (left && up) merge_cell(lmin, lmax, (cy - 1u) * g + cx - 1u, mn, v);
    }
}

// LDS: lmin[g*g], lmax[g*g] (level 0, by atomics), then levels 1.. packed (min | max << 16), (g*g - 1) / 3 words
template <bool kFast>
__global__ __launch_bounds__(kBoundsThreads) void tile_bounds_kernel(BoundsArgs a) {
    extern __shared__ uint32_t lds[];
    const uint32_t g = a.g, g2 = g * g;
    uint32_t* lmin = lds;
    uint32_t* lmax = lds + g2;
    uint32_t* coarse = lds + 2u * g2;
    for (uint32_t i = threadIdx.x; i < g2; i += kBoundsThreads) {
        lmin[i] = 0xFFFFu;
        lmax[i] = 0u;
    }
    __syncthreads();
    const uint16_t* tile = a.atlas + uint64_t(a.layers[blockIdx.x]) * a.T * a.T;  // 64-bit layer offset
    if (kFast)
        level0_fast(a, tile, lmin, lmax);
    else
        level0_plain(a, tile, lmin, lmax);
    __syncthreads();
    // levels 1..log2(g): the 2x2 children of the level below (level 1 reads lmin / lmax, level k > 1 reads coarse[below..])
    for (uint32_t n = g / 2u, base = 0, below = 0; n >= 1u; below = base, base += n * n, n /= 2u) {
        const uint32_t cn = n * 2u;
        for (uint32_t i = threadIdx.x; i < n * n; i += kBoundsThreads) {
            const uint32_t c0 = 2u * (i / n) * cn + 2u * (i % n);
            uint32_t mn = 0xFFFFu, mx = 0u;
            for (uint32_t c : {c0, c0 + 1u, c0 + cn, c0 + cn + 1u}) {
                mn = min(mn, cn == g ? lmin[c] : coarse[below + c] & 0xFFFFu);
                mx = max(mx, cn == g ? lmax[c] : coarse[below + c] >> 16);
            }
            coarse[base + i] = mn | (mx << 16);
        }
        __syncthreads();
    }
    uint32_t* out = a.out + uint64_t(blockIdx.x) * a.cells;
    for (uint32_t i = threadIdx.x; i < a.cells; i += kBoundsThreads) {
        const uint32_t mn = i < g2 ? lmin[i] : coarse[i - g2] & 0xFFFFu;
        const uint32_t mx = i < g2 ? lmax[i] : coarse[i - g2] >> 16;
        out[i] = out_min(mn, a.skip_zero) | (mx << 16);
    }
}

}  // namespace

static bool tile_bounds_fast(uint32_t T, uint32_t grid) {
    const uint32_t s = T / grid;
    return T % 8u == 0u && s % 8u == 0u && (512u % s == 0u || s % 512u == 0u);
}

static size_t tile_bounds_lds_bytes(uint32_t grid) { return 4u * (2u * grid * grid + (grid * grid - 1u) / 3u); }

bt_status launch_tile_bounds(hipStream_t stream, const void* atlas, uint32_t T, const uint32_t* layers, uint32_t count, uint32_t grid,
                             bool skip_zero, uint32_t* out) {
    if (!count) return BT_OK;
    BoundsArgs a{(const uint16_t*)atlas, layers, out, T, T / grid, grid, uint32_t((4u * grid * grid - 1u) / 3u), skip_zero ? 1u : 0u};
    const size_t lds = tile_bounds_lds_bytes(grid);
    if (tile_bounds_fast(T, grid))
        tile_bounds_kernel<true><<<count, kBoundsThreads, lds, stream>>>(a);
    else
        tile_bounds_kernel<false><<<count, kBoundsThreads, lds, stream>>>(a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? BT_OK : hip_fail(e, "tile_bounds_kernel");
}

}  // namespace bt

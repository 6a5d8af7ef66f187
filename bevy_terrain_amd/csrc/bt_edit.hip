// In-place editing of atlas layers (bt_atlas_edit_height / bt_atlas_paint / bt_atlas_write_region / bt_atlas_read_region): the kernels.  The planning is in bt_edit.cpp.
//
// An item is ONE tile's dirty rectangle of one launch: (layer, inclusive rectangle in centre texels, mosaic origin of the tile's centre).
// grid = (items, row blocks of the tallest rectangle); a workgroup of four waves takes kEditRows rows of its item, a wave one row at a
// time, lanes along x: a row is one coalesced run of dwords.
//   R16: a lane owns one ALIGNED 32-bit pair of texels; the rule is stated, and carried out, at for_each_pair.
//   Rgba8: a lane owns one texel.
//
// edit_brush_kernel   the stamps of bt_atlas_edit_height on the texels of the rectangle; the stamp array is indexed by the loop counter
//                     only (wave-uniform: scalar loads), and a stamp whose side is not the item's is skipped by the whole wave.
// edit_paint_kernel   the stamps of bt_atlas_paint on the Rgba8 texels of the rectangle, in the same way: one dword read, four channels in
//                     registers, one dword written.
// edit_region_kernel  the same layout, copying from the staged rectangle of bt_atlas_write_region.
// edit_gather_kernel  its mirror for bt_atlas_read_region: layers -> the staged rectangle.
// edit_smooth_kernel<K>  the box mean of bt_atlas_smooth_height (kernel_radius K) and its stamps.  It READS the layers and writes the new dwords
//                     of every item's rectangle into device scratch: other workgroups read the rows it would write (as halo), so nothing of
//                     the call may land in a layer before every workgroup has read.  edit_smooth_copy_kernel, the next launch, moves them in.
//                     A workgroup stages its row block in LDS; see the kernel.
// edit_downsample_kernel  the rectangle of a parent's centre from its four children: downsample_texel of bt_downsample.hpp, the device
//                     function downsample_kernel runs.  One launch per LOD (a level reads what the level below wrote).
//
// Arithmetic contract of the brush (include/bevy_terrain_amd.h): IEEE binary32, one rounding per written operation; this file is compiled
// with -ffp-contract=off, `/` is the correctly rounded division.
#include "bt_internal.hpp"

namespace bt {

namespace {

#include "bt_downsample.hpp"  // unorm16_to_float, float_to_unorm, Texel, downsample_texel

constexpr uint32_t kEditThreads = 256;
constexpr uint32_t kEditRows = 16;  // rows of a rectangle per workgroup: four per wave

// the disc test and the falloff weight of a stamp (bt_edit_stamp or bt_smooth_stamp) at texel (fx, fy), the header's BRUSH section line
// by line: false outside the disc, else w
template <typename Stamp>
__device__ __forceinline__ bool stamp_weight(const Stamp& s, float r2, float fx, float fy, float& w) {
    const float dx = fx - s.center[0];
    const float dy = fy - s.center[1];
    const float d2 = (dx * dx) + (dy * dy);
    if (!(d2 < r2)) return false;
    w = 1.0f;
    if (s.falloff == BT_EDIT_FALLOFF_SMOOTH) {
        const float q = d2 / r2;
        const float sm = 1.0f - q;
        w = sm * sm;
    }
    return true;
}

// t -> t' of one stamp that has passed the side test
__device__ __forceinline__ uint32_t stamp_texel(const bt_edit_stamp& s, float r2, float fx, float fy, uint32_t t) {
    float w;
    if (!stamp_weight(s, r2, fx, fy, w) || t == 0u) return t;
    const float h = unorm16_to_float(t);  // == f32(t) / 65535 for every t (bt_selftest)
    const float hn = s.mode == BT_EDIT_FLATTEN ? h + (s.amount - h) * w : h + s.amount * w;
    return max(1u, float_to_unorm(hn, 65535.0f));
}

// u -> u' of one paint stamp that has passed the side test: the header's PAINT section line by line
__device__ __forceinline__ uint32_t paint_texel(const bt_paint_stamp& s, float r2, float fx, float fy, uint32_t u) {
    float w;
    if ((u & 0x00FFFFFFu) == 0u || !stamp_weight(s, r2, fx, fy, w)) return u;
    const float a = s.opacity * w;
    uint32_t out = u;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
        if (!((s.channel_mask >> k) & 1u)) continue;
        const float c = unorm8_to_float((u >> (8u * k)) & 0xFFu);  // == f32(u[k]) / 255 (bt_selftest)
        const float cn = s.mode == BT_PAINT_BLEND ? c + (s.color[k] - c) * a : c + s.color[k] * a;
        out = (out & ~(0xFFu << (8u * k))) | (float_to_unorm(cn, 255.0f) << (8u * k));
    }
    // never a hole: the channels of the mask among r, g, b (all 0 here) become 1
    if ((out & 0x00FFFFFFu) == 0u) out |= (s.channel_mask & 1u) | ((s.channel_mask & 2u) << 7) | ((s.channel_mask & 4u) << 14);
    return out;
}

// the rows and the dword range a workgroup's waves walk: calls body(row y, dword p) for every (row of this workgroup, dword of the row)
// first / last: the first and last dword index (inside the tile row) that holds a texel of the rectangle
template <typename Body>
__device__ __forceinline__ void for_each_dword(const EditItem& it, uint32_t first, uint32_t last, Body body) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t y_begin = it.y0 + blockIdx.y * kEditRows;
    if (y_begin > it.y1) return;
    const uint32_t y_end = min(y_begin + kEditRows - 1u, it.y1);
    for (uint32_t y = y_begin + wave; y <= y_end; y += kEditThreads / 64u)
        for (uint32_t p = first + lane; p <= last; p += 64u) body(y, p);
}

__device__ __forceinline__ uint32_t pair_of(uint32_t t0, uint32_t t1) { return t0 | (t1 << 16); }

// R16: a lane owns one ALIGNED 32-bit pair of texels, (px, px + 1) with px = 2p a column of the layer (T is even: an odd centre size is
// refused, so rows start on a dword).  At an odd rectangle edge half of the pair lies outside the rectangle (another centre texel, or an
// apron texel): the lane writes that half back from its own read; the read is skipped when both halves are inside, unless the body wants
// the old texels (kAlwaysRead).  Items of a launch are different layers and rows are different dwords, so no two lanes touch the same
// dword.  body(y, p, px, in0, in1, old) returns the fresh pair; what it puts in a half that is outside (in0 / in1 false) is dropped.
template <bool kAlwaysRead, typename Body>
__device__ __forceinline__ void for_each_pair(const AttachmentMeta& m, uint16_t* atlas, const EditItem& it, Body body) {
    const uint32_t Tsz = m.texture_size, b = m.border_size;
    uint32_t* tile = reinterpret_cast<uint32_t*>(atlas + uint64_t(it.layer) * Tsz * Tsz);
    const uint32_t px0 = b + it.x0, px1 = b + it.x1;
    for_each_dword(it, px0 >> 1, px1 >> 1, [&](uint32_t y, uint32_t p) {
        uint32_t* dst = tile + (uint64_t(b + y) * Tsz) / 2u + p;
        const uint32_t px = 2u * p;
        const bool in0 = px >= px0, in1 = px + 1u <= px1;  // (px <= px1 and px + 1 >= px0 hold for every dword of the range)
        const uint32_t old = (kAlwaysRead || !(in0 && in1)) ? *dst : 0u;
        const uint32_t fresh = body(y, p, px, in0, in1, old);
        *dst = pair_of(in0 ? (fresh & 0xFFFFu) : (old & 0xFFFFu), in1 ? (fresh >> 16) : (old >> 16));
    });
}

__global__ __launch_bounds__(kEditThreads) void edit_brush_kernel(AttachmentMeta m, uint16_t* __restrict__ atlas, const EditItem* __restrict__ items,
                                                                  const bt_edit_stamp* __restrict__ stamps, uint32_t stamp_count) {
    const EditItem it = items[blockIdx.x];
    const uint32_t b = m.border_size;
    for_each_pair<true>(m, atlas, it, [&](uint32_t y, uint32_t, uint32_t px, bool in0, bool in1, uint32_t old) {
        uint32_t t0 = old & 0xFFFFu, t1 = old >> 16;
        const float fy = float(it.gy0 + y);
        const float fx0 = float(it.gx0 + px - b), fx1 = float(it.gx0 + px + 1u - b);  // (the half outside the rectangle is not used)
        for (uint32_t k = 0; k < stamp_count; k++) {
            const bt_edit_stamp s = stamps[k];
            if (s.side != it.side) continue;
            const float r2 = s.radius * s.radius;
            if (in0) t0 = stamp_texel(s, r2, fx0, fy, t0);
            if (in1) t1 = stamp_texel(s, r2, fx1, fy, t1);
        }
        return pair_of(t0, t1);
    });
}

__global__ __launch_bounds__(kEditThreads) void edit_paint_kernel(AttachmentMeta m, uint32_t* __restrict__ atlas, const EditItem* __restrict__ items,
                                                                  const bt_paint_stamp* __restrict__ stamps, uint32_t stamp_count) {
    const EditItem it = items[blockIdx.x];
    const uint32_t Tsz = m.texture_size, b = m.border_size;
    uint32_t* tile = atlas + uint64_t(it.layer) * Tsz * Tsz;
    for_each_dword(it, b + it.x0, b + it.x1, [&](uint32_t y, uint32_t px) {
        uint32_t* dst = tile + uint64_t(b + y) * Tsz + px;
        uint32_t u = *dst;
        const float fx = float(it.gx0 + px - b), fy = float(it.gy0 + y);
        for (uint32_t k = 0; k < stamp_count; k++) {
            const bt_paint_stamp s = stamps[k];
            if (s.side != it.side) continue;
            u = paint_texel(s, s.radius * s.radius, fx, fy, u);
        }
        *dst = u;
    });
}

template <uint32_t FORMAT>
__global__ __launch_bounds__(kEditThreads) void edit_region_kernel(AttachmentMeta m, void* __restrict__ atlas_, const EditItem* __restrict__ items,
                                                                   const void* __restrict__ src_, uint32_t rx0, uint32_t ry0, uint32_t src_width) {
    const EditItem it = items[blockIdx.x];
    const uint32_t Tsz = m.texture_size, b = m.border_size;
    if constexpr (FORMAT == BT_FORMAT_R16) {
        const uint16_t* src = (const uint16_t*)src_;
        for_each_pair<false>(m, (uint16_t*)atlas_, it, [&](uint32_t y, uint32_t, uint32_t px, bool in0, bool in1, uint32_t) {
            const uint16_t* row = src + uint64_t(it.gy0 + y - ry0) * src_width;
            // (the column of the half outside the rectangle may lie outside the staged rows: it is not read)
            return pair_of(in0 ? uint32_t(row[it.gx0 + px - b - rx0]) : 0u, in1 ? uint32_t(row[it.gx0 + px + 1u - b - rx0]) : 0u);
        });
    } else {
        const uint32_t px0 = b + it.x0, px1 = b + it.x1;
        uint32_t* tile = (uint32_t*)atlas_ + uint64_t(it.layer) * Tsz * Tsz;
        const uint32_t* src = (const uint32_t*)src_;
        for_each_dword(it, px0, px1, [&](uint32_t y, uint32_t px) {
            tile[uint64_t(b + y) * Tsz + px] = src[uint64_t(it.gy0 + y - ry0) * src_width + (it.gx0 + px - b - rx0)];
        });
    }
}

// The mirror of edit_region_kernel: the texels of every item's rectangle go from the layers into the staged rectangle (`dst_width` texels per
// row, tightly packed, texel (0, 0) = mosaic texel (rx0, ry0)).  R16: a lane owns one aligned pair of the LAYER row and reads it as one dword;
// the staged rectangle is written PER TEXEL (16-bit stores of the halves inside the rectangle), so an odd x0 or width, where the staged
// rows are not dword-aligned with the layer's, needs no case of its own.  Rgba8: one dword in, one dword out.
template <uint32_t FORMAT>
__global__ __launch_bounds__(kEditThreads) void edit_gather_kernel(AttachmentMeta m, const void* __restrict__ atlas_, const EditItem* __restrict__ items,
                                                                   void* __restrict__ dst_, uint32_t rx0, uint32_t ry0, uint32_t dst_width) {
    const EditItem it = items[blockIdx.x];
    const uint32_t Tsz = m.texture_size, b = m.border_size;
    const uint32_t px0 = b + it.x0, px1 = b + it.x1;
    if constexpr (FORMAT == BT_FORMAT_R16) {
        const uint32_t* tile = reinterpret_cast<const uint32_t*>((const uint16_t*)atlas_ + uint64_t(it.layer) * Tsz * Tsz);
        uint16_t* dst = (uint16_t*)dst_;
        for_each_dword(it, px0 >> 1, px1 >> 1, [&](uint32_t y, uint32_t p) {
            const uint32_t pair = tile[(uint64_t(b + y) * Tsz) / 2u + p], px = 2u * p;
            uint16_t* row = dst + uint64_t(it.gy0 + y - ry0) * dst_width;
            if (px >= px0) row[it.gx0 + px - b - rx0] = uint16_t(pair & 0xFFFFu);
            if (px + 1u <= px1) row[it.gx0 + px + 1u - b - rx0] = uint16_t(pair >> 16);
        });
    } else {
        const uint32_t* tile = (const uint32_t*)atlas_ + uint64_t(it.layer) * Tsz * Tsz;
        uint32_t* dst = (uint32_t*)dst_;
        for_each_dword(it, px0, px1, [&](uint32_t y, uint32_t px) {
            dst[uint64_t(it.gy0 + y - ry0) * dst_width + (it.gx0 + px - b - rx0)] = tile[uint64_t(b + y) * Tsz + px];
        });
    }
}

// ---- smoothing.  A texel in LDS is one dword, already in the form the sums add: (1 << 24) | u for u != 0, 0 for a hole, so a tap is ONE
// integer add and the total carries the count in bits 24.. (<= 81) and the sum below (<= 81 * 65535 < 2^23).  A lane owns the aligned pair
// (2p, 2p + 1) as everywhere in this file and reads whole pairs (8 bytes): the 32 lanes of a half wave read 256 consecutive bytes of one
// staged row, which is one pass of the 64 banks whatever the row pitch, so the pitch is just the window's width.  The staging stores are
// 8-byte stores of consecutive lanes as well.
//
// The window of a workgroup: its kEditRows rows plus K above and below, by one trip of the lanes (64 pairs) plus kHalo = ceil(K / 2) pairs
// left and right; a wider rectangle is walked in such column chunks, each staged with its own halo.  K <= border_size keeps every row
// and every texel a data texel taps inside the layer; a PAIR of the halo may lie outside the row (odd K at the layer's edge): it is
// staged as holes and only the discarded half of an edge pair ever taps it.
// Separable: a wave takes four consecutive rows; per pair it forms the row sums of the 4 + 2K staged rows those need, once each, and adds
// 2K + 1 of them per output row.  Integer sums: every order gives the same bits.
template <uint32_t K>
struct SmoothWindow {
    static constexpr uint32_t kHalo = (K + 1u) / 2u;          // pairs
    static constexpr uint32_t kPairs = 64u + 2u * kHalo;      // pitch, in pairs
    static constexpr uint32_t kRows = kEditRows + 2u * K;
    static constexpr uint32_t kWaveRows = kEditRows / (kEditThreads / 64u);  // output rows of a wave
};

__device__ __forceinline__ uint32_t smooth_pack(uint32_t u) { return u ? (1u << 24) | u : 0u; }

// steps 1 - 3 of the header's SMOOTHING section for one texel: t0 its value before the call, acc the packed box total
__device__ __forceinline__ uint32_t smooth_texel(const bt_smooth_stamp* __restrict__ stamps, uint32_t stamp_count, uint32_t side, float fx, float fy, uint32_t t0,
                                                 uint32_t acc) {
    if (t0 == 0u) return 0u;
    const float mean = float(acc & 0xFFFFFFu) / (65535.0f * float(acc >> 24));
    uint32_t t = t0;
    for (uint32_t k = 0; k < stamp_count; k++) {
        const bt_smooth_stamp s = stamps[k];
        if (s.side != side) continue;
        float w;
        if (!stamp_weight(s, s.radius * s.radius, fx, fy, w)) continue;
        const float a = s.strength * w;
        const float h = unorm16_to_float(t);
        const float hn = h + (mean - h) * a;
        t = max(1u, float_to_unorm(hn, 65535.0f));
    }
    return t;
}

template <uint32_t K>
__global__ __launch_bounds__(kEditThreads) void edit_smooth_kernel(AttachmentMeta m, const uint16_t* __restrict__ atlas, const EditItem* __restrict__ items,
                                                                   const uint64_t* __restrict__ offsets, const bt_smooth_stamp* __restrict__ stamps,
                                                                   uint32_t stamp_count, uint32_t* __restrict__ scratch) {
    using W = SmoothWindow<K>;
    __shared__ uint2 window[W::kRows][W::kPairs];
    const EditItem it = items[blockIdx.x];
    const uint32_t y_begin = it.y0 + blockIdx.y * kEditRows;
    if (y_begin > it.y1) return;  // (the whole workgroup: no barrier is skipped by a part of it)
    const uint32_t y_end = min(y_begin + kEditRows - 1u, it.y1);
    const uint32_t Tsz = m.texture_size, b = m.border_size, row_pairs = Tsz / 2u;
    const uint32_t* tile = reinterpret_cast<const uint32_t*>(atlas + uint64_t(it.layer) * Tsz * Tsz);
    const uint32_t px0 = b + it.x0, px1 = b + it.x1, first = px0 >> 1, last = px1 >> 1, width = last - first + 1u;
    uint32_t* out = scratch + offsets[blockIdx.x];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t staged_rows = y_end - y_begin + 1u + 2u * K;  // staged row r is layer row b + y_begin - K + r
    for (uint32_t chunk = first; chunk <= last; chunk += 64u) {
        if (chunk != first) __syncthreads();  // the window of the previous chunk has been read
        const uint32_t staged_pairs = min(64u, last - chunk + 1u) + 2u * W::kHalo;  // staged pair i is pair chunk - kHalo + i of the row
        for (uint32_t r = wave; r < staged_rows; r += kEditThreads / 64u) {
            const uint32_t* row = tile + uint64_t(b + y_begin - K + r) * row_pairs;
            for (uint32_t i = lane; i < staged_pairs; i += 64u) {
                const uint32_t p = chunk + i - W::kHalo;  // (wraps below 0: then it is not < row_pairs either)
                const uint32_t pair = p < row_pairs ? row[p] : 0u;
                window[r][i] = make_uint2(smooth_pack(pair & 0xFFFFu), smooth_pack(pair >> 16));
            }
        }
        __syncthreads();
        const uint32_t p = chunk + lane, j0 = wave * W::kWaveRows;  // the wave's output rows are y_begin + j0 ..
        if (p > last || y_begin + j0 > y_end) continue;
        uint32_t row0[W::kWaveRows + 2u * K], row1[W::kWaveRows + 2u * K], centre[W::kWaveRows];
#pragma unroll
        for (uint32_t r = 0; r < W::kWaveRows + 2u * K; r++) {  // (rows past the staged ones hold stale words: their sums feed rows past y_end only)
            uint32_t e[2u * (2u * W::kHalo + 1u)];
#pragma unroll
            for (uint32_t i = 0; i <= 2u * W::kHalo; i++) {
                const uint2 v = window[j0 + r][lane + i];
                e[2u * i] = v.x, e[2u * i + 1u] = v.y;
            }
            uint32_t s0 = 0, s1 = 0;
#pragma unroll
            for (uint32_t d = 0; d <= 2u * K; d++) {
                s0 += e[2u * W::kHalo - K + d];
                s1 += e[2u * W::kHalo + 1u - K + d];
            }
            row0[r] = s0, row1[r] = s1;
            if (r >= K && r < K + W::kWaveRows) centre[r - K] = (e[2u * W::kHalo] & 0xFFFFu) | (e[2u * W::kHalo + 1u] << 16);
        }
        const uint32_t px = 2u * p;
        const bool in0 = px >= px0, in1 = px + 1u <= px1;
        const float fx0 = float(it.gx0 + px - b), fx1 = float(it.gx0 + px + 1u - b);  // (the half outside the rectangle is not used)
#pragma unroll
        for (uint32_t j = 0; j < W::kWaveRows; j++) {
            const uint32_t y = y_begin + j0 + j;
            if (y > y_end) break;
            uint32_t a0 = 0, a1 = 0;
#pragma unroll
            for (uint32_t d = 0; d <= 2u * K; d++) a0 += row0[j + d], a1 += row1[j + d];
            uint32_t t0 = centre[j] & 0xFFFFu, t1 = centre[j] >> 16;
            const float fy = float(it.gy0 + y);
            if (in0) t0 = smooth_texel(stamps, stamp_count, it.side, fx0, fy, t0, a0);
            if (in1) t1 = smooth_texel(stamps, stamp_count, it.side, fx1, fy, t1, a1);
            out[uint64_t(y - it.y0) * width + (p - first)] = t0 | (t1 << 16);
        }
    }
}

// scratch -> layers, the source being item-relative
__global__ __launch_bounds__(kEditThreads) void edit_smooth_copy_kernel(AttachmentMeta m, uint16_t* __restrict__ atlas, const EditItem* __restrict__ items,
                                                                        const uint64_t* __restrict__ offsets, const uint32_t* __restrict__ scratch) {
    const EditItem it = items[blockIdx.x];
    const uint32_t b = m.border_size, first = (b + it.x0) >> 1, width = ((b + it.x1) >> 1) - first + 1u;
    const uint32_t* src = scratch + offsets[blockIdx.x];
    for_each_pair<false>(m, atlas, it, [&](uint32_t y, uint32_t p, uint32_t, bool, bool, uint32_t) { return src[uint64_t(y - it.y0) * width + (p - first)]; });
}

// centre texel (tx, ty) of a parent: the child it lies in and the 2x2 block of that child's centre (downsample_kernel's mapping).  The child
// layers come as four scalars selected by comparisons: a dynamically indexed copy of the item would be promoted to LDS.
struct EditChildren {
    uint32_t c0, c1, c2, c3;
};
template <uint32_t FORMAT>
__device__ __forceinline__ uint32_t parent_texel(const AttachmentMeta& m, const typename Texel<FORMAT>::type* __restrict__ base, EditChildren ch, uint32_t tx, uint32_t ty) {
    const uint32_t Tsz = m.texture_size, b = m.border_size, child_size = m.center_size / 2u;
    const bool right = tx >= child_size, low = ty >= child_size;
    const uint32_t layer = low ? (right ? ch.c3 : ch.c2) : (right ? ch.c1 : ch.c0);
    const typename Texel<FORMAT>::type* child = layer < m.atlas_size ? base + uint64_t(layer) * Tsz * Tsz : nullptr;
    return downsample_texel<FORMAT>(child, Tsz, 2u * (right ? tx - child_size : tx) + b, 2u * (low ? ty - child_size : ty) + b);
}

template <uint32_t FORMAT>
__global__ __launch_bounds__(kEditThreads) void edit_downsample_kernel(AttachmentMeta m, void* __restrict__ atlas_, const EditItem* __restrict__ items) {
    using T = typename Texel<FORMAT>::type;
    const EditItem it = items[blockIdx.x];
    const uint32_t Tsz = m.texture_size, b = m.border_size;
    T* base = (T*)atlas_;
    const EditChildren ch = {it.child[0], it.child[1], it.child[2], it.child[3]};
    if constexpr (FORMAT == BT_FORMAT_R16) {
        for_each_pair<false>(m, base, it, [&](uint32_t y, uint32_t, uint32_t px, bool in0, bool in1, uint32_t) {
            // (the half of a dword outside the rectangle: its texel is computed from a clamped column and dropped)
            return pair_of(parent_texel<FORMAT>(m, base, ch, in0 ? px - b : it.x0, y), parent_texel<FORMAT>(m, base, ch, in1 ? px + 1u - b : it.x1, y));
        });
    } else {
        const uint32_t px0 = b + it.x0, px1 = b + it.x1;
        T* tile = base + uint64_t(it.layer) * Tsz * Tsz;
        for_each_dword(it, px0, px1, [&](uint32_t y, uint32_t px) { tile[uint64_t(b + y) * Tsz + px] = parent_texel<FORMAT>(m, base, ch, px - b, y); });
    }
}

dim3 edit_grid(uint32_t n, uint32_t max_rows) { return dim3(n, (max_rows + kEditRows - 1u) / kEditRows); }

}  // namespace

bt_status launch_edit_brush(hipStream_t stream, const AttachmentMeta& m, void* atlas, const EditItem* items, uint32_t n, uint32_t max_rows,
                            const bt_edit_stamp* stamps, uint32_t stamp_count) {
    if (!n || !max_rows) return BT_OK;
    edit_brush_kernel<<<edit_grid(n, max_rows), kEditThreads, 0, stream>>>(m, (uint16_t*)atlas, items, stamps, stamp_count);
    return launched("edit_brush_kernel");
}

bt_status launch_edit_paint(hipStream_t stream, const AttachmentMeta& m, void* atlas, const EditItem* items, uint32_t n, uint32_t max_rows,
                            const bt_paint_stamp* stamps, uint32_t stamp_count) {
    if (!n || !max_rows) return BT_OK;
    edit_paint_kernel<<<edit_grid(n, max_rows), kEditThreads, 0, stream>>>(m, (uint32_t*)atlas, items, stamps, stamp_count);
    return launched("edit_paint_kernel");
}

bt_status launch_edit_gather(hipStream_t stream, const AttachmentMeta& m, const void* atlas, const EditItem* items, uint32_t n, uint32_t max_rows,
                             void* dst, uint32_t rx0, uint32_t ry0, uint32_t dst_width) {
    if (!n || !max_rows) return BT_OK;
    const auto kernel = m.format == BT_FORMAT_R16 ? edit_gather_kernel<BT_FORMAT_R16> : edit_gather_kernel<BT_FORMAT_RGBA8>;
    kernel<<<edit_grid(n, max_rows), kEditThreads, 0, stream>>>(m, atlas, items, dst, rx0, ry0, dst_width);
    return launched("edit_gather_kernel");
}

bt_status launch_edit_region(hipStream_t stream, const AttachmentMeta& m, void* atlas, const EditItem* items, uint32_t n, uint32_t max_rows,
                             const void* src, uint32_t rx0, uint32_t ry0, uint32_t src_width) {
    if (!n || !max_rows) return BT_OK;
    const auto kernel = m.format == BT_FORMAT_R16 ? edit_region_kernel<BT_FORMAT_R16> : edit_region_kernel<BT_FORMAT_RGBA8>;
    kernel<<<edit_grid(n, max_rows), kEditThreads, 0, stream>>>(m, atlas, items, src, rx0, ry0, src_width);
    return launched("edit_region_kernel");
}

bt_status launch_edit_smooth(hipStream_t stream, const AttachmentMeta& m, void* atlas, const EditItem* items, const uint64_t* offsets, uint32_t n, uint32_t max_rows,
                             const bt_smooth_stamp* stamps, uint32_t stamp_count, uint32_t kernel_radius, void* scratch) {
    if (!n || !max_rows) return BT_OK;
    const dim3 grid = edit_grid(n, max_rows);
    switch (kernel_radius) {
        case 1: edit_smooth_kernel<1><<<grid, kEditThreads, 0, stream>>>(m, (const uint16_t*)atlas, items, offsets, stamps, stamp_count, (uint32_t*)scratch); break;
        case 2: edit_smooth_kernel<2><<<grid, kEditThreads, 0, stream>>>(m, (const uint16_t*)atlas, items, offsets, stamps, stamp_count, (uint32_t*)scratch); break;
        case 3: edit_smooth_kernel<3><<<grid, kEditThreads, 0, stream>>>(m, (const uint16_t*)atlas, items, offsets, stamps, stamp_count, (uint32_t*)scratch); break;
        case 4: edit_smooth_kernel<4><<<grid, kEditThreads, 0, stream>>>(m, (const uint16_t*)atlas, items, offsets, stamps, stamp_count, (uint32_t*)scratch); break;
        default: set_error("edit_smooth_kernel: kernel_radius %u", kernel_radius); return BT_ERR_INVALID_ARGUMENT;
    }
    if (bt_status s = launched("edit_smooth_kernel")) return s;
    edit_smooth_copy_kernel<<<grid, kEditThreads, 0, stream>>>(m, (uint16_t*)atlas, items, offsets, (const uint32_t*)scratch);
    return launched("edit_smooth_copy_kernel");
}

bt_status launch_edit_downsample(hipStream_t stream, const AttachmentMeta& m, void* atlas, const EditItem* items, uint32_t n, uint32_t max_rows) {
    if (!n || !max_rows) return BT_OK;
    const auto kernel = m.format == BT_FORMAT_R16 ? edit_downsample_kernel<BT_FORMAT_R16> : edit_downsample_kernel<BT_FORMAT_RGBA8>;
    kernel<<<edit_grid(n, max_rows), kEditThreads, 0, stream>>>(m, atlas, items);
    return launched("edit_downsample_kernel");
}

}  // namespace bt

// bt_atlas_splat_from_height (include/bevy_terrain_amd.h, SPLAT): the first step of its plan.  The kernel reads the layers of an R16
// attachment H and writes, for every texel of the items' rectangles, one Rgba8 texel of the attachment G of the same atlas: up to eight
// height-and-slope rules evaluated on the texel's height and on steep = 1 - s.z of its TILE NORMAL (tile_normal of bt_normal_device.hpp,
// the one definition the normal bake and the normal query evaluate).  The planning is in bt_edit.cpp: the items, the grid and the
// ownership are those of edit_paint_kernel (bt_edit.hip): grid = (items, blocks of kSplatRows rows of the tallest rectangle), a wave
// takes one row at a time, a lane owns one target texel = one dword, a row is one coalesced run of dwords.
//
// The four taps of a texel read 16 height texels, most of them shared with its neighbours'.  A workgroup therefore stages the rows of its
// block plus `halo` rows above and below, by one trip of the lanes (64 columns) plus `halo` columns left and right, in LDS: every global
// texel is fetched once per workgroup and column chunk; a wider rectangle is walked in such chunks, each staged with its own halo.  The
// halo is the bake's (T / (2c) + 2 texels: the tap offset, the bilinear pair, one for the rounding of the tap position); the window is cut
// to the layer, and a texel one of whose (clamped) tap texels falls outside it takes all its taps from HBM instead - one test per texel
// - so the bytes are the definition's whatever the window.  A halo beyond kSplatMaxHalo (a centre smaller than a tenth of the texture)
// is not staged at all.  The window is 32 x 80 texels of 2 bytes = 5 KiB: no limit on occupancy.  Lanes read adjacent 16-bit texels of
// a window row (two lanes share a dword: a broadcast), so the row pitch is free of bank conflicts.
//
// The rules travel through the plan ring and are indexed by the (unrolled) loop counter only: wave-uniform scalar loads.
// Arithmetic: IEEE binary32, one rounding per written operation (-ffp-contract=off), `/` is the correctly rounded division.
#include "bt_band_device.hpp"
#include "bt_internal.hpp"
#include "bt_model.hpp"
#include "bt_normal_device.hpp"

namespace bt {

namespace {

constexpr uint32_t kSplatThreads = 256;
constexpr uint32_t kSplatRows = 16;    // rows of a rectangle per workgroup: four per wave (the paint kernel's)
constexpr uint32_t kSplatColumns = 64;  // columns of a chunk: one trip of the lanes
constexpr uint32_t kSplatMaxHalo = 8;
constexpr uint32_t kWindowRows = kSplatRows + 2u * kSplatMaxHalo, kWindowColumns = kSplatColumns + 2u * kSplatMaxHalo;

struct SplatParams {
    NormalModel nm;
    uint32_t lod, halo, mode, count;
    uint32_t fallback;  // the four bytes as the texel's dword
};

// (band() of step 4: bt_band_device.hpp, shared with the scatter kernels of bt_scatter.hip)

// steps 2 and 4 - 7 for a data texel: its raw height, the z of its tile normal -> the target dword
__device__ __forceinline__ uint32_t splat_texel(const SplatParams& P, const bt_splat_rule* __restrict__ rules, uint32_t raw, float sz) {
    const float v = unorm16_to_float(raw);  // == f32(raw) / 65535 for every raw (bt_selftest)
    const float h = P.nm.min_height + (P.nm.max_height - P.nm.min_height) * v;
    const float steep = 1.0f - sz;
    float w[BT_SPLAT_MAX_WEIGHT_RULES] = {0.0f, 0.0f, 0.0f, 0.0f}, colour[3] = {0.0f, 0.0f, 0.0f}, sum = 0.0f;
#pragma unroll
    for (uint32_t k = 0; k < BT_SPLAT_MAX_RULES; k++) {
        if (k >= P.count) break;
        const bt_splat_rule rule = rules[k];
        // (weight * 0) * band is 0 for every finite band: a wave none of whose lanes is inside the rule's heights skips its other band
        const float wh = rule.weight * band(h, rule.height_lo, rule.height_hi, rule.height_fade);
        float wk = 0.0f;
        if (__builtin_amdgcn_ballot_w64(wh != 0.0f) != 0ull) wk = wh * band(steep, rule.steep_lo, rule.steep_hi, rule.steep_fade);
        sum = sum + wk;  // (0 + w_0 is w_0)
        if (P.mode == BT_SPLAT_COLOUR) {
#pragma unroll
            for (uint32_t ch = 0; ch < 3; ch++) colour[ch] = colour[ch] + wk * rule.colour[ch];  // (0 + x is x up to the sign of a zero, which enc8 drops)
        } else if (k < BT_SPLAT_MAX_WEIGHT_RULES) {
            w[k] = wk;
        }
    }
    uint32_t texel = P.fallback;
    if (sum > 0.0f) {
        if (P.mode == BT_SPLAT_COLOUR)
            texel = enc8(colour[0] / sum) | (enc8(colour[1] / sum) << 8) | (enc8(colour[2] / sum) << 16) | (255u << 24);
        else
            texel = enc8(w[0] / sum) | (enc8(w[1] / sum) << 8) | (enc8(w[2] / sum) << 16) | (enc8(w[3] / sum) << 24);  // (w_k = 0 from `count` on)
    }
    if ((texel & 0x00FFFFFFu) == 0u) texel |= 1u;  // the zero rule: a data texel stays one
    return texel;
}

// m: the meta of H; G has its texture_size and border_size (the entry point refuses anything else), and a tile has ONE layer index in
// every attachment of its atlas
__global__ __launch_bounds__(kSplatThreads) void edit_splat_kernel(AttachmentMeta m, const uint16_t* __restrict__ heights, uint32_t* __restrict__ target,
                                                                   const EditItem* __restrict__ items, const bt_splat_rule* __restrict__ rules, SplatParams P) {
    __shared__ uint16_t window[kWindowRows][kWindowColumns];
    const EditItem it = items[blockIdx.x];
    const uint32_t y_begin = it.y0 + blockIdx.y * kSplatRows;
    if (y_begin > it.y1) return;  // (the whole workgroup: no barrier is skipped by a part of it)
    const uint32_t y_end = min(y_begin + kSplatRows - 1u, it.y1);
    const uint32_t T = m.texture_size, b = m.border_size, c = m.center_size;
    const uint16_t* __restrict__ tile = heights + uint64_t(it.layer) * T * T;
    uint32_t* __restrict__ out = target + uint64_t(it.layer) * T * T;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const NormalTaps tp = normal_taps(m);
    const float dist = normal_dist(m, P.nm, P.lod);
    const bool windowed = P.halo <= kSplatMaxHalo;
    // the window's rows: texture rows [wy0, wy0 + wrows), at most kSplatRows + 2 * halo of them, inside the layer
    const uint32_t wy0 = windowed && b + y_begin > P.halo ? b + y_begin - P.halo : 0u;
    const uint32_t wrows = windowed ? min(b + y_end + P.halo, T - 1u) - wy0 + 1u : 0u;
    const uint32_t px0 = b + it.x0, px1 = b + it.x1;
    for (uint32_t chunk = px0; chunk <= px1; chunk += kSplatColumns) {
        const uint32_t chunk_last = min(chunk + kSplatColumns - 1u, px1);
        // its columns: texture columns [wx0, wx0 + wcolumns), at most kSplatColumns + 2 * halo
        const uint32_t wx0 = windowed && chunk > P.halo ? chunk - P.halo : 0u;
        const uint32_t wcolumns = windowed ? min(chunk_last + P.halo, T - 1u) - wx0 + 1u : 0u;
        if (windowed) {
            if (chunk != px0) __syncthreads();  // the window of the previous chunk has been read
            for (uint32_t r = wave; r < wrows; r += kSplatThreads / 64u) {
                const uint16_t* row = tile + uint64_t(wy0 + r) * T + wx0;
                for (uint32_t i = lane; i < wcolumns; i += 64u) window[r][i] = row[i];
            }
            __syncthreads();
        }
        const uint32_t px = chunk + lane;
        if (px > chunk_last) continue;
        const uint32_t i = px - b;
        for (uint32_t y = y_begin + wave; y <= y_end; y += kSplatThreads / 64u) {
            const uint32_t py = b + y;
            const uint32_t raw = windowed ? uint32_t(window[py - wy0][px - wx0]) : uint32_t(tile[uint64_t(py) * T + px]);
            uint32_t texel = 0u;  // no data in, no data out
            if (raw != 0u) {
                const float uv[2] = {(float(i) + 0.5f) / float(c), (float(y) + 0.5f) / float(c)};
                const TapSplit sp = tap_split(tp, uv);
                // ONE window test per texel: the columns and rows its taps touch, after the clamp (first[a][0] <= [1] <= [2])
                const uint32_t lo_x = texel_clamp(sp.first[0][0], T), hi_x = texel_clamp(sp.first[0][2] + 1, T);
                const uint32_t lo_y = texel_clamp(sp.first[1][0], T), hi_y = texel_clamp(sp.first[1][2] + 1, T);
                F3 s;
                if (lo_x >= wx0 && hi_x - wx0 < wcolumns && lo_y >= wy0 && hi_y - wy0 < wrows)
                    s = tile_normal(tp, P.nm, dist, sp, [&](uint32_t x, uint32_t yy) -> uint32_t { return window[yy - wy0][x - wx0]; });
                else  // a tap outside the window (or no window): the layer in HBM
                    s = tile_normal(tp, P.nm, dist, sp, [&](uint32_t x, uint32_t yy) -> uint32_t { return tile[uint64_t(yy) * T + x]; });
                texel = splat_texel(P, rules, raw, s.z);
            }
            out[uint64_t(py) * T + px] = texel;
        }
    }
}

}  // namespace

uint32_t splat_reach(const AttachmentMeta& m) { return m.texture_size / (2u * m.center_size) + 2u; }

bt_status launch_edit_splat(hipStream_t stream, const AttachmentMeta& m, void* atlas, const EditItem* items, uint32_t n, uint32_t max_rows, const SplatSource& src,
                            const bt_splat_rule* rules) {
    if (!n || !max_rows) return BT_OK;
    const model::Model model = model::make_model(*src.model);
    SplatParams P{};
    P.nm = {model.min_height, model.max_height, normal_side_length(model)};
    P.lod = src.lod, P.halo = splat_reach(src.meta), P.mode = src.mode, P.count = src.count, P.fallback = src.fallback;
    edit_splat_kernel<<<dim3(n, (max_rows + kSplatRows - 1u) / kSplatRows), kSplatThreads, 0, stream>>>(src.meta, (const uint16_t*)src.level0, (uint32_t*)atlas, items, rules, P);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? BT_OK : hip_fail(e, "edit_splat_kernel");
}

}  // namespace bt

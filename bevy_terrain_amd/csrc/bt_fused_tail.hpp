// fused_tail: the remaining LODs from the atlas, the apron rows of the LODs above and a cube's cross-face seam regions.  Device code only;
// included by bt_fused.hip inside namespace bt { namespace { ... } }, behind fused_main and before fused_direct; not a unit of its own.
#pragma once

// ---- fused_tail: up to three LODs below `A.lod`, read from the atlas ---------------------------------
// Workgroup = 64 x 64 pixels of the LOD-`lod` mosaic, 16 x 16 threads, 4 x 4 input pixels per thread: a thread
// owns 2 x 2 pixels of lod-1 and one pixel of lod-2 in registers; 2 x 2 neighbouring threads (lanes l, l+1,
// l+16, l+17 of one wave) combine into one pixel of lod-3 with three shuffles.  No LDS, no barrier, one tile
// lookup per thread and LOD (c % 4 == 0: a 4 x 4 block never straddles a tile).
// Top / bottom apron rows (whole rows, corners included) of the tiles of the LODs fused_main produced below the
// finest one: stitch.wgsl:53-118 for same-side neighbours — neighbour's centre rows, or the own centre clamped
// when it is absent.  (Cube face edges are re-stitched afterwards by the generic kernel.)  One thread per pixel pair.
__device__ __forceinline__ void tail_apron_rows(const FusedArgs& A, uint32_t side, uint32_t e) {
    const uint32_t T = A.m.texture_size, b = A.m.border_size, c = A.m.center_size, o = b + c;
    const uint32_t pairs = b * T, per_block = 256u * kApronPairsPerThread, blocks_per_tile = (pairs + per_block - 1u) / per_block;
    for (uint32_t k = 0; k < A.apron_lods; k++) {
        const uint32_t lod = A.lod + k, n = 1u << lod, blocks = n * n * blocks_per_tile;
        if (e >= blocks) {
            e -= blocks;
            continue;
        }
        const uint32_t tile = e / blocks_per_tile, i0 = (e % blocks_per_tile) * per_block + threadIdx.x;
        const uint32_t tx = tile / n, ty = tile % n;
        const uint32_t self = grid_lookup(A, side, lod, int(tx), int(ty));
        if (self == kInvalid) return;
        // every load first (unconditional, from clamped addresses), then the stores: one round trip for the thread's four pairs
        uint32_t v[kApronPairsPerThread][2], dst[kApronPairsPerThread];
        bool live[kApronPairsPerThread];
#pragma unroll
        for (uint32_t q = 0; q < kApronPairsPerThread; q++) {
            const uint32_t i = i0 + 256u * q;
            live[q] = i < pairs;
            const uint32_t ii = live[q] ? i : 0u;
            const uint32_t r = ii / (T / 2u), px = 2u * (ii % (T / 2u)), py = r < b ? r : c + r;
            const int rx = px < b ? -1 : (px >= o ? 1 : 0), ry = r < b ? -1 : 1;
            if (A.seam_skip) {
                // cube: a neighbour beyond ONE edge of the face lives on another face and a seam workgroup of this launch writes the region
                // (beyond two edges — the cube's corner — there is none: clamped below like any absent neighbour)
                const bool out_x = int(tx) + rx < 0 || int(tx) + rx >= int(n), out_y = int(ty) + ry < 0 || int(ty) + ry >= int(n);
                if (out_x != out_y) live[q] = false;
            }
            const uint32_t nb = grid_lookup(A, side, lod, int(tx) + rx, int(ty) + ry);
#pragma unroll
            for (uint32_t h = 0; h < 2; h++) {
                const uint32_t x = px + h;
                const uint32_t sx = nb != kInvalid ? uint32_t(int(x) - rx * int(c)) : min(max(x, b), o - 1u);
                const uint32_t sy = nb != kInvalid ? uint32_t(int(py) - ry * int(c)) : min(max(py, b), o - 1u);
                v[q][h] = A.atlas[uint64_t(nb != kInvalid ? nb : self) * T * T + sy * T + sx];
            }
            dst[q] = py * T + px;
        }
#pragma unroll
        for (uint32_t q = 0; q < kApronPairsPerThread; q++)
            if (live[q]) *reinterpret_cast<uint32_t*>(A.atlas + uint64_t(self) * T * T + dst[q]) = v[q][0] | (v[q][1] << 16);
        return;
    }
}

// Rgba8 twin (one 4-byte texel per thread) that also does the left / right apron columns: after fused_direct, which writes
// the centres of the two parent LODs only, these workgroups are the whole stitch of those tiles (stitch.wgsl:53-118 for
// same-face neighbours; cube seams are re-stitched by the batched kernel afterwards, like everywhere in the fused plans).
__device__ __forceinline__ uint32_t tail_apron_texels_per_tile(const FusedArgs& A) {
    return 2u * A.m.border_size * A.m.texture_size + (A.apron_cols ? 2u * A.m.border_size * A.m.center_size : 0u);
}
__device__ __forceinline__ void tail_aprons_rgba8(const FusedArgs& A, uint32_t side, uint32_t e) {
    const uint32_t T = A.m.texture_size, b = A.m.border_size, c = A.m.center_size, o = b + c;
    const uint32_t per_tile = tail_apron_texels_per_tile(A), blocks_per_tile = (per_tile + 255u) / 256u;
    uint32_t* atlas = reinterpret_cast<uint32_t*>(A.atlas);
    for (uint32_t k = 0; k < A.apron_lods; k++) {
        const uint32_t lod = A.lod + k, n = 1u << lod, blocks = n * n * blocks_per_tile;
        if (e >= blocks) {
            e -= blocks;
            continue;
        }
        const uint32_t tile = e / blocks_per_tile, i = (e % blocks_per_tile) * 256u + threadIdx.x;
        if (i >= per_tile) return;
        const uint32_t tx = tile / n, ty = tile % n;
        const uint32_t self = grid_lookup(A, side, lod, int(tx), int(ty));
        if (self == kInvalid) return;
        uint32_t px, py;
        if (i < 2u * b * T) {  // whole apron rows (with the corners)
            const uint32_t r = i / T;
            px = i % T;
            py = r < b ? r : c + r;
        } else {  // apron columns of the centre rows
            const uint32_t j = i - 2u * b * T, kk = j % (2u * b);
            px = kk < b ? kk : c + kk;
            py = b + j / (2u * b);
        }
        const int rx = px < b ? -1 : (px >= o ? 1 : 0), ry = py < b ? -1 : (py >= o ? 1 : 0);
        if (A.seam_skip) {  // cube: a region beyond exactly ONE face edge belongs to a seam workgroup of this launch (see tail_apron_rows)
            const bool out_x = int(tx) + rx < 0 || int(tx) + rx >= int(n), out_y = int(ty) + ry < 0 || int(ty) + ry >= int(n);
            if (out_x != out_y) return;
        }
        const uint32_t nb = grid_lookup(A, side, lod, int(tx) + rx, int(ty) + ry);
        const uint32_t sx = nb != kInvalid ? uint32_t(int(px) - rx * int(c)) : min(max(px, b), o - 1u);
        const uint32_t sy = nb != kInvalid ? uint32_t(int(py) - ry * int(c)) : min(max(py, b), o - 1u);
        atlas[uint64_t(self) * T * T + py * T + px] = atlas[uint64_t(nb != kInvalid ? nb : self) * T * T + sy * T + sx];
        return;
    }
}

// kRegular: the atlas indices follow the closed form (FusedArgs::regular) — as a compile-time fact the table lookups and their
// registers fall away (64 VGPRs: eight waves per SIMD)
// downsample.wgsl:25-39 for R16 in the 2^16-scaled domain of fused_main's fast loop (round 5; downsample4 above is the plain form).
// F(t) = fma(x, r, x) = 65536 * RN(t / 65535) and F(0) = 0: a no-data texel adds an exact 0 to the running sum, so ((F00 + F01) + F10) + F11
// IS the sum over the valid texels in OFFSETS order, rounding for rounding; what differs is the divisor.  All four valid (the common case):
// 0.5 + (0.25 * k) * sum with k = 65535 / 65536 (sum * 0.25 is exact).  Otherwise ONE IEEE division by the count — scaling by a power of two
// commutes with it, and an average of values <= 1 needs no clamp — and count 0 gives 0.5 + k * (0 / 1) -> 0, the defined "no data".
typedef float tail_f2 __attribute__((ext_vector_type(2)));
typedef uint16_t tail_u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ tail_f2 tail_conv2(uint32_t a, uint32_t bq) {
    const tail_f2 x = {float(a), float(bq)}, kr = {1.0f / 65535.0f, 1.0f / 65535.0f};
    return __builtin_elementwise_fma(x, kr, x);
}
// two 2 x 2 averages at once: block A = a_top over a_bot, packed texel pairs (low half = x0), block B likewise
__device__ __forceinline__ void down_pair_r16(uint32_t a_top, uint32_t a_bot, uint32_t b_top, uint32_t b_bot, uint32_t& qa, uint32_t& qb) {
    const tail_f2 khalf = {0.5f, 0.5f}, kn = {65535.0f / 65536.0f, 65535.0f / 65536.0f}, knq = {0.25f * (65535.0f / 65536.0f), 0.25f * (65535.0f / 65536.0f)};
    const tail_u16x2 one = {1, 1};
    const tail_u16x2 at = __builtin_bit_cast(tail_u16x2, a_top), ab = __builtin_bit_cast(tail_u16x2, a_bot), bt2 = __builtin_bit_cast(tail_u16x2, b_top), bb = __builtin_bit_cast(tail_u16x2, b_bot);
    const tail_u16x2 m = __builtin_elementwise_min(__builtin_elementwise_min(at, ab), __builtin_elementwise_min(bt2, bb));
    // OFFSETS order (0,0),(0,1),(1,0),(1,1) of (dx, dy): ((x0y0 + x0y1) + x1y0) + x1y1
    const tail_f2 sum = ((tail_conv2(a_top & 0xFFFFu, b_top & 0xFFFFu) + tail_conv2(a_bot & 0xFFFFu, b_bot & 0xFFFFu)) + tail_conv2(a_top >> 16, b_top >> 16)) + tail_conv2(a_bot >> 16, b_bot >> 16);
    tail_f2 w = khalf + knq * sum;
    if (__builtin_expect(m.x == 0 || m.y == 0, 0)) {  // (rare) some texel has no data: the valid-average
        const tail_u16x2 ca = __builtin_elementwise_min(at, one) + __builtin_elementwise_min(ab, one), cb = __builtin_elementwise_min(bt2, one) + __builtin_elementwise_min(bb, one);
        const tail_f2 d = {sum.x / float(max(uint32_t(ca.x) + uint32_t(ca.y), 1u)), sum.y / float(max(uint32_t(cb.x) + uint32_t(cb.y), 1u))};
        w = khalf + kn * d;
    }
    qa = uint32_t(w.x);
    qb = uint32_t(w.y);
}
__device__ __forceinline__ uint32_t down_one_r16(uint32_t t00, uint32_t t01, uint32_t t10, uint32_t t11) {
    const float r = 1.0f / 65535.0f;
    const float x00 = float(t00), x01 = float(t01), x10 = float(t10), x11 = float(t11);
    const float sum = ((__builtin_fmaf(x00, r, x00) + __builtin_fmaf(x01, r, x01)) + __builtin_fmaf(x10, r, x10)) + __builtin_fmaf(x11, r, x11);
    float w = 0.5f + (0.25f * (65535.0f / 65536.0f)) * sum;
    if (__builtin_expect(min(min(t00, t01), min(t10, t11)) == 0, 0)) {
        const uint32_t count = min(t00, 1u) + min(t01, 1u) + min(t10, 1u) + min(t11, 1u);
        w = 0.5f + (65535.0f / 65536.0f) * (sum / float(max(count, 1u)));
    }
    return uint32_t(w);
}

// Pixel (mx, my) of the LOD-`lod` mosaic of face `side`, evaluated from the tail's INPUT LOD (lod + K, complete when the launch starts) with the
// tail's own reduction in its own order — (x, y), (x, y + 1), (x + 1, y), (x + 1, y + 1), downsample.wgsl:25-39 per level, every level quantised —
// i.e. bit for bit what the mosaic workgroups of this launch write into that tile's centre (R16).
template <typename TT>
__device__ __forceinline__ uint32_t tail_down(uint32_t t00, uint32_t t01, uint32_t t10, uint32_t t11) {  // the tail's reduction of one level, per format
    if constexpr (std::is_same<TT, uint16_t>::value) return down_one_r16(t00, t01, t10, t11);
    else return downsample4_rgba8(t00, t01, t10, t11);
}
template <int K, typename TT>
__device__ __forceinline__ uint32_t pull_value(const FusedArgs& A, uint32_t side, uint32_t lod, uint32_t mx, uint32_t my) {
    if constexpr (K == 0) {
        const uint32_t T = A.m.texture_size, b = A.m.border_size, c = A.m.center_size;
        const uint32_t tx = mx / c, ty = my / c;
        const uint32_t idx = grid_lookup(A, side, lod, int(tx), int(ty));
        if (idx == kInvalid) return 0u;  // an absent tile reads as no data, like the mosaic workgroups' loads
        return reinterpret_cast<const TT*>(A.atlas)[uint64_t(idx) * T * T + uint64_t(b + my - ty * c) * T + b + mx - tx * c];
    } else {
        const uint32_t t00 = pull_value<K - 1, TT>(A, side, lod + 1u, 2u * mx, 2u * my), t01 = pull_value<K - 1, TT>(A, side, lod + 1u, 2u * mx, 2u * my + 1u);
        const uint32_t t10 = pull_value<K - 1, TT>(A, side, lod + 1u, 2u * mx + 1u, 2u * my), t11 = pull_value<K - 1, TT>(A, side, lod + 1u, 2u * mx + 1u, 2u * my + 1u);
        return tail_down<TT>(t00, t01, t10, t11);
    }
}

// ONE cross-face apron region of a tile the tail itself produces (stitch.wgsl:12-51, 79-118), pulled: the texel the reference copies out of
// the neighbour face's centre is evaluated from the tail's input instead (task.raster = LODs between the tile and the input; the neighbour
// tile's coordinate rides in rel_index[region] as x << 16 | y).  One workgroup of 256 threads; kPack = 2: two adjacent pixels per dword store.
template <typename TT, uint32_t kPack>
__device__ __forceinline__ void stitch_region_pull(const FusedArgs& A, const TaskDev& task) {
    const uint32_t Tsz = A.m.texture_size, b = A.m.border_size, c = A.m.center_size, o = b + c;
    const uint32_t region = uint32_t(__ffs(int(task.regions))) - 1u;  // 0 top, 1 right, 2 bottom, 3 left, 4 TL, 5 TR, 6 BR, 7 BL
    const uint32_t x0 = (region == 0u || region == 2u) ? b : ((region == 1u || region == 5u || region == 6u) ? o : 0u);
    const uint32_t y0 = (region == 1u || region == 3u) ? b : ((region == 2u || region == 6u || region == 7u) ? o : 0u);
    const uint32_t w = (region == 0u || region == 2u) ? c : b, h = (region == 1u || region == 3u) ? c : b;
    const int rx = (region == 1u || region == 5u || region == 6u) ? 1 : ((region == 3u || region == 4u || region == 7u) ? -1 : 0);
    const int ry = (region == 2u || region == 6u || region == 7u) ? 1 : ((region == 0u || region == 4u || region == 5u) ? -1 : 0);
    const uint32_t other = task.rel_side[region], nx = task.rel_index[region] >> 16, ny = task.rel_index[region] & 0xFFFFu;
    // task.raster = levels | part << 8 | parts << 16: a region is shared out over `parts` workgroups (a thread then evaluates one pixel pair:
    // the pull workgroups are the longest of the launch — 4^levels dependent-free loads per pixel — and must not outlast the mosaic's)
    const uint32_t levels = task.raster & 0xFFu, part = (task.raster >> 8) & 0xFFu, parts = max(1u, task.raster >> 16);
    const uint32_t count = (w / kPack) * h, share = (count + parts - 1u) / parts, i_end = min(count, (part + 1u) * share);
    // levels <= 2: the 2^levels x 2^levels input block of a pixel lies in ONE input tile (c is a multiple of 4): one tile lookup, one division per axis
    const uint32_t in_lod = task.lod + levels, cn = c >> levels;  // cn: pixels of this LOD one input tile's centre covers
    for (uint32_t i = part * share + threadIdx.x; i < i_end; i += 256u) {
        const uint32_t px = x0 + kPack * (i % (w / kPack)), py = y0 + i / (w / kPack);
        if (py >= A.m.row_limit) continue;
        uint32_t v[kPack];
#pragma unroll
        for (uint32_t e = 0; e < kPack; e++) {
            // neighbour_data of stitch.wgsl: the apron texel as a texel of the neighbour tile (its centre: [b, b + c) on both axes), then as a pixel of its face's mosaic
            const uint2 q = project_to_side(uint32_t(int(px + e) - rx * int(c)), uint32_t(int(py) - ry * int(c)), Tsz, task.side, other);
            const uint32_t mx = nx * c + (q.x - b), my = ny * c + (q.y - b);
            if (BT_ABLATE(A, 2147483648u)) {  // (2147483648: pull workgroups store zeros without evaluating anything — timing experiment)
                v[e] = 0;
            } else if (levels <= 2u && (c & 3u) == 0) {
                const uint32_t tx = mx / cn, ty = my / cn;  // the input tile, and the block's first pixel in it
                const uint32_t idx = grid_lookup(A, other, in_lod, int(tx), int(ty));
                const TT* src = reinterpret_cast<const TT*>(A.atlas) + uint64_t(idx == kInvalid ? 0u : idx) * Tsz * Tsz + uint64_t(b + ((my - ty * cn) << levels)) * Tsz + b + ((mx - tx * cn) << levels);
                // every load unconditional and issued before the first use (a conditional load becomes its own divergent block with a wait behind it:
                // sixteen dependent round trips per pixel made these the longest workgroups of the launch); an absent tile reads as no data
                const uint32_t keep = idx == kInvalid ? 0u : 0xFFFFFFFFu;
                if (levels == 1u) {
                    const uint32_t t00 = src[0], t01 = src[Tsz], t10 = src[1], t11 = src[Tsz + 1u];
                    v[e] = tail_down<TT>(t00 & keep, t01 & keep, t10 & keep, t11 & keep);
                } else {
                    uint32_t t[4][4];  // [dy][dx]
#pragma unroll
                    for (uint32_t dy = 0; dy < 4; dy++)
#pragma unroll
                        for (uint32_t dx = 0; dx < 4; dx++) t[dy][dx] = uint32_t(src[dy * Tsz + dx]) & keep;
                    auto two = [&](uint32_t dx, uint32_t dy) -> uint32_t { return tail_down<TT>(t[dy][dx], t[dy + 1][dx], t[dy][dx + 1], t[dy + 1][dx + 1]); };
                    v[e] = tail_down<TT>(two(0u, 0u), two(0u, 2u), two(2u, 0u), two(2u, 2u));
                }
            } else {
                v[e] = levels == 1u ? pull_value<1, TT>(A, other, task.lod, mx, my) : levels == 2u ? pull_value<2, TT>(A, other, task.lod, mx, my) : pull_value<3, TT>(A, other, task.lod, mx, my);
            }
        }
        TT* dst = reinterpret_cast<TT*>(A.atlas) + uint64_t(task.atlas_index) * Tsz * Tsz + uint64_t(py) * Tsz + px;
        if (BT_ABLATE(A, 4194304u) && (v[0] | v[kPack - 1]) != 0x12345u) continue;  // (4194304: evaluated, not stored — timing experiment)
        if constexpr (kPack == 2) *reinterpret_cast<uint32_t*>(dst) = v[0] | (v[1] << 16);
        else *dst = TT(v[0]);
    }
}

template <uint32_t kFormat, bool kRegular>
__global__ __launch_bounds__(256) void fused_tail_kernel(FusedArgs A_in) {
    FusedArgs A = A_in;
    A.regular = kRegular ? 1u : 0u;
    constexpr bool kR16 = kFormat == BT_FORMAT_R16;
    using TT = typename std::conditional<kR16, uint16_t, uint32_t>::type;  // texel
    // Workgroup -> work, XCD-aware (round 5).  Workgroups go to the XCDs round robin (blockIdx.x % 8) and every XCD has its own L2; a
    // 64-pixel-wide mosaic column starts b texels into a tile row, i.e. it shares its first and last 128-byte line with the workgroup
    // beside it — dispatched in mosaic order the two sit on different XCDs and every line is fetched from HBM twice
    // (profiles/r05_pmc_summary.json: the tail read 67.7 MB for 33.5 MB of texels).  So: XCD k takes the k-th eighth of the mosaic
    // workgroups (whole rows of them, neighbours in x back to back on one L2), and in front of those its eighth of the extra workgroups —
    // apron rows (Rgba8: and columns) of the LODs above, on a cube the cross-face seam regions first: short dependent chains that run
    // beside the mosaic work instead of behind the last of it.
    // The extras of an XCD, in dispatch order: its share of the cross-face seam regions (task f = j * 8 + xcd: the list's head — the pulled
    // regions, the launch's longest workgroups — spreads over all eight XCDs; round 6: with all of them on XCD 0 the launch ended 4 us late),
    // then its eighth of the apron blocks (side-major), then its eighth of the mosaic.
    const uint32_t nx = ((1u << A.lod) * A.m.center_size + 63u) / 64u, per_side_m = nx * nx, per_side_a = A.tail_extras;
    const uint32_t total_m = A.sides * per_side_m, total_a = A.sides * per_side_a, chunk_m = (total_m + 7u) / 8u, chunk_a = (total_a + 7u) / 8u;
    const uint32_t chunk_s = (A.seam_count + 7u) / 8u, chunk_e = chunk_s + chunk_a;
    uint32_t side, block_x, block_y;
    {
        const uint32_t xcd = blockIdx.x % 8u, j = blockIdx.x / 8u;
        if (j < chunk_e) {
            if (BT_ABLATE(A, 268435456u)) return;  // (268435456: no extra workgroups — timing experiment)
            if (j < chunk_s) {  // one cross-face region
                const uint32_t f = j * 8u + xcd;
                if (f < A.seam_count) {
                    const bool pulled = A.seam_tasks[f].raster != 0u;  // a region of a tile this launch produces: pulled from the input LOD
                    if constexpr (kR16) {
                        const bool pairs = (A.m.border_size & 1u) == 0 && (A.m.texture_size & 1u) == 0;
                        if (pulled) {
                            if (pairs) stitch_region_pull<uint16_t, 2>(A, A.seam_tasks[f]);
                            else stitch_region_pull<uint16_t, 1>(A, A.seam_tasks[f]);
                        } else if (pairs) stitch_region_body<uint16_t, 2>(A.m, A.atlas, A.seam_tasks[f]);
                        else stitch_region_body<uint16_t, 1>(A.m, A.atlas, A.seam_tasks[f]);
                    } else {
                        if (pulled) stitch_region_pull<uint32_t, 1>(A, A.seam_tasks[f]);
                        else stitch_region_body<uint32_t, 1>(A.m, A.atlas, A.seam_tasks[f]);
                    }
                }
                return;
            }
            const uint32_t id = xcd * chunk_a + (j - chunk_s);
            if (id >= total_a) return;
            side = id / per_side_a;
            const uint32_t e = id - side * per_side_a;
            if constexpr (kR16) tail_apron_rows(A, side, e);
            else tail_aprons_rgba8(A, side, e);
            return;
        }
        const uint32_t id = xcd * chunk_m + (j - chunk_e);
        if (id >= total_m) return;
        side = id / per_side_m;
        const uint32_t r = id - side * per_side_m;
        block_y = r / nx;
        block_x = r - block_y * nx;
    }
    const uint32_t T = A.m.texture_size, b = A.m.border_size, c = A.m.center_size;
    const uint32_t tile_texels = T * T;
    const uint32_t size = (1u << A.lod) * c;  // mosaic extent of the input LOD (a multiple of 4)
    const uint32_t tx = threadIdx.x & 15u, ty = threadIdx.x >> 4;
    const uint32_t gx = block_x * 64u + 4u * tx, gy = block_y * 64u + 4u * ty;  // first input pixel
    const bool active = gx < size && gy < size;
    // ONE division per axis: c is a multiple of 4, so the 4 x 4 block lies in one tile, and the tile / in-tile coordinates
    // of its pixel at LOD-k follow by shifts: tile >> k, ((tile & (2^k - 1)) * c + rem) >> k
    const uint32_t tile_x = gx / c, tile_y = gy / c, rem_x = gx - tile_x * c, rem_y = gy - tile_y * c;
    const uint32_t rx1 = ((tile_x & 1u) * c + rem_x) >> 1, ry1 = ((tile_y & 1u) * c + rem_y) >> 1;
    TT* atlas = reinterpret_cast<TT*>(A.atlas);
    auto down = [](uint32_t t00, uint32_t t01, uint32_t t10, uint32_t t11) -> uint32_t {
        if constexpr (kR16) return down_one_r16(t00, t01, t10, t11);
        else return downsample4_rgba8(t00, t01, t10, t11);
    };

    uint32_t t[4][4];  // [row][col]  (R16: t[r][0], t[r][1] hold the row's two DWORDS — pixels 0 | 1 and 2 | 3 — as loaded)
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int k = 0; k < 4; k++) t[r][k] = 0;
    // all tile lookups up front (independent of the data): one round of memory latency instead of four
    uint32_t idx = kInvalid, self1 = kInvalid, self2 = kInvalid, self3 = kInvalid;
    if (active) {
        idx = grid_lookup(A, side, A.lod, int(tile_x), int(tile_y));
        self1 = grid_lookup(A, side, A.lod - 1, int(tile_x >> 1), int(tile_y >> 1));
        if (A.levels >= 2) self2 = grid_lookup(A, side, A.lod - 2, int(tile_x >> 2), int(tile_y >> 2));
        if (A.levels >= 3) self3 = grid_lookup(A, side, A.lod - 3, int(tile_x >> 3), int(tile_y >> 3));
    }
    // ... and the neighbour tiles the four lod-1 pixels will be pushed into (edge pixels only), while nothing has been stored yet.
    // b even: the 2 x 2 block (even coordinates) lies in one edge region and shares its targets; b odd: per pixel, push_pixel
    const bool pre = (b & 1u) == 0;
    const PushNb nb1 = push_targets(A, side, A.lod - 1, tile_x >> 1, tile_y >> 1, rx1, ry1, active && pre);
    if (active) {
        if (idx != kInvalid && !BT_ABLATE(A, 33554432u)) {  // an absent tile reads as no data  (33554432: no texel loads — timing experiment)
            const TT* p = atlas + uint64_t(idx) * tile_texels + (b + rem_y) * T + b + rem_x;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                if constexpr (kR16) {  // 4-byte aligned (b even)
                    const uint2 w = *reinterpret_cast<const uint2 __attribute__((aligned(4)))*>(p + r * T);  // one 8-byte load from a dword-aligned address
                    t[r][0] = w.x;
                    t[r][1] = w.y;
                } else {  // 8-byte aligned (b even or not: (b + 4k) texels of 4 bytes; pairs need b even) — two texels per load
                    if ((b & 1u) == 0) {
                        const uint2 lo = *reinterpret_cast<const uint2*>(p + r * T), hi = *reinterpret_cast<const uint2*>(p + r * T + 2);
                        t[r][0] = lo.x;
                        t[r][1] = lo.y;
                        t[r][2] = hi.x;
                        t[r][3] = hi.y;
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; k++) t[r][k] = p[r * T + k];
                    }
                }
            }
        }
    }
    // lod-1: 2 x 2 pixels, each from a 2 x 2 block in OFFSETS order (0,0),(0,1),(1,0),(1,1) of (dx, dy)
    uint32_t q[2][2];  // [row][col]
#pragma unroll
    for (int r = 0; r < 2; r++) {
        if constexpr (kR16) {  // the row pair's two pixels at once, from the packed dwords
            down_pair_r16(t[2 * r][0], t[2 * r + 1][0], t[2 * r][1], t[2 * r + 1][1], q[r][0], q[r][1]);
        } else {
#pragma unroll
            for (int k = 0; k < 2; k++) q[r][k] = down(t[2 * r][2 * k], t[2 * r + 1][2 * k], t[2 * r][2 * k + 1], t[2 * r + 1][2 * k + 1]);
        }
    }
    if (active) {
        const uint32_t self = self1;
        if (self != kInvalid && !BT_ABLATE(A, 1073741824u)) {  // (1073741824: no lod-1 stores — timing experiment)
            // R16: the two pixels of a row are one aligned dword of the tile (x1, b, c even); aprons per pixel, edge pixels only
            TT* centre = atlas + uint64_t(self) * tile_texels + (b + ry1) * T + b + rx1;
#pragma unroll
            for (int r = 0; r < 2; r++) {
                if constexpr (kR16) {
                    *reinterpret_cast<uint32_t*>(centre + r * T) = q[r][0] | (q[r][1] << 16);
                } else {
                    centre[r * T] = q[r][0];
                    centre[r * T + 1] = q[r][1];
                }
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    if (BT_ABLATE(A, 536870912u)) continue;  // (536870912: no apron pushes of lod-1 — timing experiment)
                    if (pre) push_store<TT>(A, nb1, self, rx1 + k, ry1 + r, TT(q[r][k]));
                    else push_pixel<false, TT>(A, side, A.lod - 1, tile_x >> 1, tile_y >> 1, self, rx1 + k, ry1 + r, TT(q[r][k]));
                }
            }
        }
    }
    if (A.levels < 2 || BT_ABLATE(A, 67108864u)) return;  // (67108864: lod-1 only — timing experiment)
    const uint32_t v2 = down(q[0][0], q[1][0], q[0][1], q[1][1]);
    if (active) {
        const uint32_t self = self2;
        if (self != kInvalid)
            push_pixel<true, TT>(A, side, A.lod - 2, tile_x >> 2, tile_y >> 2, self, ((tile_x & 3u) * c + rem_x) >> 2, ((tile_y & 3u) * c + rem_y) >> 2, TT(v2));
    }
    if (A.levels < 3) return;
    // lod-3: threads (tx, ty) with both even own the pixel; partners are lanes +1 (dx), +16 (dy), +17
    const uint32_t right = __shfl_down(v2, 1), below = __shfl_down(v2, 16), diag = __shfl_down(v2, 17);
    if (active && ((tx | ty) & 1u) == 0) {
        const uint32_t v3 = down(v2, below, right, diag);
        const uint32_t self = self3;
        if (self != kInvalid)
            push_pixel<true, TT>(A, side, A.lod - 3, tile_x >> 3, tile_y >> 3, self, ((tile_x & 7u) * c + rem_x) >> 3, ((tile_y & 7u) * c + rem_y) >> 3, TT(v3));
    }
}

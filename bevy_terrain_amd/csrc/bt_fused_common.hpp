// The fused kernels' shared device vocabulary: the unorm conversions, the grid lookup, the apron push, the 2 x 2 reductions.  Device code only;
// included by bt_fused.hip inside namespace bt { namespace { ... } }, behind bt_fused_args.hpp and before the kernel families, whose order
// of definition it keeps (so push_pixel / push_targets / push_store, used by fused_tail alone, and load_tile_nb / split_value_slow, used by
// fused_main alone, stand where they stood).
#pragma once

// Ablation switches of the profiling build (tools/, -DBT_DEBUG_HOOKS): compiled out of the product library, where
// the branches they guard fold away and no environment variable is read.
#ifdef BT_DEBUG_HOOKS
#define BT_ABLATE(A, bits) ((A).ablate & (bits))
#else
#define BT_ABLATE(A, bits) 0u
#endif

// t / 65535.0f, correctly rounded, in 3 VALU ops (see bt_fused.hip's header)
__device__ __forceinline__ float unorm16_to_float(uint32_t t) {
    const float x = float(t);
    const float r = 1.0f / 65535.0f;
    const float q0 = x * r;
    const float e = __builtin_fmaf(-q0, 65535.0f, x);
    return __builtin_fmaf(e, r, q0);
}
// floor(0.5 + 65535 * clamp(e, 0, 1)): med3 clamps (no NaN reaches here); the u32 conversion truncates,
// which is floor for the non-negative argument
__device__ __forceinline__ uint32_t float_to_unorm16(float e) {
    const float cl = __builtin_amdgcn_fmed3f(e, 0.0f, 1.0f);
    return uint32_t(0.5f + 65535.0f * cl);
}
__device__ __forceinline__ float mixf(float a, float b, float t) { return a * (1.0f - t) + b * t; }

__device__ __forceinline__ uint32_t grid_lookup(const FusedArgs& A, uint32_t side, uint32_t lod, int x, int y) {
    const int n = int(1u << lod);
    if (x < 0 || y < 0 || x >= n || y >= n) return kInvalid;
    if (lod < A.grid_lod_lo || lod > A.grid_lod_hi || side >= A.grid_sides) return kInvalid;
    if (A.regular) {  // sum of 4^l for lod < l <= lod_hi tiles precede the LOD's on its side, lod_lo .. lod_hi make a side
        const uint32_t hi4 = 4u << (2u * A.grid_lod_hi);
        return A.reg_first + side * ((hi4 - (1u << (2u * A.grid_lod_lo))) / 3u) + (hi4 - (4u << (2u * lod))) / 3u + uint32_t(x) * uint32_t(n) + uint32_t(y);
    }
    // offset of the (side, lod) grid: computed, not looked up (one dependent load less in every lookup chain):
    // sum of 4^l for lod_lo <= l < lod = (4^lod - 4^lod_lo) / 3
    const uint32_t lo4 = 1u << (2u * A.grid_lod_lo), per_side = ((4u << (2u * A.grid_lod_hi)) - lo4) / 3u;
    const uint32_t off = side * per_side + ((1u << (2u * lod)) - lo4) / 3u;
    return A.grids[off + uint32_t(x) * uint32_t(n) + uint32_t(y)];
}

// A tile of some LOD together with its 8 same-face neighbours (stitch.wgsl:57-66 regions N, E, S, W, NW,
// NE, SE, SW).  Out-of-face neighbours count as absent here; on a cube the face-edge tiles are re-stitched
// afterwards by the generic kernel.  Named members: indexed arrays would be demoted to scratch / LDS.
struct TileNb {
    uint32_t self, n, e, s, w;
};

__device__ __forceinline__ TileNb load_tile_nb(const FusedArgs& A, uint32_t side, uint32_t lod, uint32_t x, uint32_t y) {
    const int ix = int(x), iy = int(y);
    TileNb t;
    t.self = grid_lookup(A, side, lod, ix, iy);
    t.n = grid_lookup(A, side, lod, ix, iy - 1);
    t.e = grid_lookup(A, side, lod, ix + 1, iy);
    t.s = grid_lookup(A, side, lod, ix, iy + 1);
    t.w = grid_lookup(A, side, lod, ix - 1, iy);
    return t;
}

// Write centre pixel (cx, cy) of tile (side, lod, tx, ty) — atlas layer `self_index` — and every apron
// texel that copies it (stitch.wgsl:53-118 inverted):
//  - the tile's own apron where the neighbour on that side is absent (repeat_data clamps into the centre),
//  - the facing apron of each existing neighbour whose b-wide strip contains the pixel.
// Neighbours are looked up only for the few pixels within b of a tile edge.
template <bool kCentre = true, typename TT = uint16_t>
__device__ __forceinline__ void push_pixel(const FusedArgs& A, uint32_t side, uint32_t lod, uint32_t tx, uint32_t ty,
                                           uint32_t self_index, uint32_t cx, uint32_t cy, TT v) {
    const uint32_t T = A.m.texture_size, b = A.m.border_size, c = A.m.center_size;
    const uint64_t tile_texels = uint64_t(T) * T;
    TT* atlas = reinterpret_cast<TT*>(A.atlas);
    TT* self = atlas + uint64_t(self_index) * tile_texels;
    if (kCentre) self[uint64_t(b + cy) * T + b + cx] = v;  // (false: the caller stored the centre texel, e.g. as half of a pair)
    const int ex = cx < b ? -1 : (cx >= c - b ? 1 : 0);
    const int ey = cy < b ? -1 : (cy >= c - b ? 1 : 0);
    if (ex == 0 && ey == 0) return;
    const uint32_t o = b + c;
    const int ix = int(tx), iy = int(ty);
    // a neighbour at offset (dx, dy) sees our centre (cx, cy) at texture (b + cx - dx*c, b + cy - dy*c)
    const uint32_t ax = uint32_t(int(b + cx) - ex * int(c)), ay = uint32_t(int(b + cy) - ey * int(c));
    // (cube, A.seam_pull: a neighbour beyond exactly ONE face edge lives on another face and a pull workgroup of this launch writes that region)
    const int nn = int(1u << lod);
    auto cross_face = [&](int x, int y) { return A.seam_pull != 0 && ((x < 0 || x >= nn) != (y < 0 || y >= nn)); };
    if (ex != 0) {
        const uint32_t n = grid_lookup(A, side, lod, ix + ex, iy);
        if (n != kInvalid) {
            atlas[uint64_t(n) * tile_texels + uint64_t(b + cy) * T + ax] = v;
        } else if (cross_face(ix + ex, iy)) {
        } else if (cx == 0 || cx == c - 1) {  // absent: our outermost column is replicated into our own apron
            const uint32_t x0 = ex < 0 ? 0u : o;
            for (uint32_t j = 0; j < b; j++) self[uint64_t(b + cy) * T + x0 + j] = v;
        }
    }
    if (ey != 0) {
        const uint32_t n = grid_lookup(A, side, lod, ix, iy + ey);
        if (n != kInvalid) {
            atlas[uint64_t(n) * tile_texels + uint64_t(ay) * T + b + cx] = v;
        } else if (cross_face(ix, iy + ey)) {
        } else if (cy == 0 || cy == c - 1) {
            const uint32_t y0 = ey < 0 ? 0u : o;
            for (uint32_t j = 0; j < b; j++) self[uint64_t(y0 + j) * T + b + cx] = v;
        }
    }
    if (ex != 0 && ey != 0) {
        const uint32_t n = grid_lookup(A, side, lod, ix + ex, iy + ey);
        if (n != kInvalid) {
            atlas[uint64_t(n) * tile_texels + uint64_t(ay) * T + ax] = v;
        } else if (cross_face(ix + ex, iy + ey)) {
        } else if ((cx == 0 || cx == c - 1) && (cy == 0 || cy == c - 1)) {  // corner region clamps both axes
            const uint32_t x0 = ex < 0 ? 0u : o, y0 = ey < 0 ? 0u : o;
            for (uint32_t j = 0; j < b; j++)
                for (uint32_t i = 0; i < b; i++) self[uint64_t(y0 + j) * T + x0 + i] = v;
        }
    }
}

// push_pixel in two halves for fused_tail, which is a latency chain: push_targets does the neighbour LOOKUPS of a centre pixel —
// coordinates only, no data — so that they are in flight together with the thread's other loads; push_store does the stores.
// (One memory counter covers loads and stores on this ISA: a lookup issued after a store waits for that store, so four
// push_pixel calls in a row cost an edge thread four round trips.)  A 2 x 2 pixel block with even coordinates shares its
// targets when b is even.
struct PushNb {
    int ex, ey;
    uint32_t nx, ny, nxy;
    uint32_t skip;  // bit 0 / 1 / 2: the x / y / diagonal neighbour lies beyond exactly one face edge of a cube and a pull workgroup writes that region (A.seam_pull)
};
__device__ __forceinline__ PushNb push_targets(const FusedArgs& A, uint32_t side, uint32_t lod, uint32_t tx, uint32_t ty, uint32_t cx, uint32_t cy, bool active) {
    const uint32_t b = A.m.border_size, c = A.m.center_size;
    PushNb t{0, 0, kInvalid, kInvalid, kInvalid, 0u};
    if (!active) return t;
    t.ex = cx < b ? -1 : (cx >= c - b ? 1 : 0);
    t.ey = cy < b ? -1 : (cy >= c - b ? 1 : 0);
    if (t.ex != 0) t.nx = grid_lookup(A, side, lod, int(tx) + t.ex, int(ty));
    if (t.ey != 0) t.ny = grid_lookup(A, side, lod, int(tx), int(ty) + t.ey);
    if (t.ex != 0 && t.ey != 0) t.nxy = grid_lookup(A, side, lod, int(tx) + t.ex, int(ty) + t.ey);
    if (A.seam_pull) {
        const int nn = int(1u << lod), x = int(tx) + t.ex, y = int(ty) + t.ey;
        const bool out_x = x < 0 || x >= nn, out_y = y < 0 || y >= nn;
        t.skip = (t.ex != 0 && out_x ? 1u : 0u) | (t.ey != 0 && out_y ? 2u : 0u) | (t.ex != 0 && t.ey != 0 && out_x != out_y ? 4u : 0u);
    }
    return t;
}
template <typename TT = uint16_t>
__device__ __forceinline__ void push_store(const FusedArgs& A, const PushNb& t, uint32_t self_index, uint32_t cx, uint32_t cy, TT v) {
    if (t.ex == 0 && t.ey == 0) return;
    const uint32_t T = A.m.texture_size, b = A.m.border_size, c = A.m.center_size, o = b + c;
    const uint64_t tile_texels = uint64_t(T) * T;
    TT* atlas = reinterpret_cast<TT*>(A.atlas);
    TT* self = atlas + uint64_t(self_index) * tile_texels;
    const uint32_t ax = uint32_t(int(b + cx) - t.ex * int(c)), ay = uint32_t(int(b + cy) - t.ey * int(c));
    if (t.ex != 0) {
        if (t.nx != kInvalid) {
            atlas[uint64_t(t.nx) * tile_texels + uint64_t(b + cy) * T + ax] = v;
        } else if (t.skip & 1u) {
        } else if (cx == 0 || cx == c - 1) {
            const uint32_t x0 = t.ex < 0 ? 0u : o;
            for (uint32_t j = 0; j < b; j++) self[uint64_t(b + cy) * T + x0 + j] = v;
        }
    }
    if (t.ey != 0) {
        if (t.ny != kInvalid) {
            atlas[uint64_t(t.ny) * tile_texels + uint64_t(ay) * T + b + cx] = v;
        } else if (t.skip & 2u) {
        } else if (cy == 0 || cy == c - 1) {
            const uint32_t y0 = t.ey < 0 ? 0u : o;
            for (uint32_t j = 0; j < b; j++) self[uint64_t(y0 + j) * T + b + cx] = v;
        }
    }
    if (t.ex != 0 && t.ey != 0) {
        if (t.nxy != kInvalid) {
            atlas[uint64_t(t.nxy) * tile_texels + uint64_t(ay) * T + ax] = v;
        } else if (t.skip & 4u) {
        } else if ((cx == 0 || cx == c - 1) && (cy == 0 || cy == c - 1)) {
            const uint32_t x0 = t.ex < 0 ? 0u : o, y0 = t.ey < 0 ? 0u : o;
            for (uint32_t j = 0; j < b; j++)
                for (uint32_t i = 0; i < b; i++) self[uint64_t(y0 + j) * T + x0 + i] = v;
        }
    }
}

// downsample.wgsl:25-39 on four texels in OFFSETS order (0,0),(0,1),(1,0),(1,1) of (dx, dy)
__device__ __forceinline__ uint32_t downsample4(uint32_t t00, uint32_t t01, uint32_t t10, uint32_t t11) {
    if (t00 != 0 && t01 != 0 && t10 != 0 && t11 != 0) {
        // all four valid (the common case): ((((0 + a) + b) + c) + d) / 4, and x / 4 == x * 0.25 exactly
        const float value = ((unorm16_to_float(t00) + unorm16_to_float(t01)) + unorm16_to_float(t10)) + unorm16_to_float(t11);
        return float_to_unorm16(value * 0.25f);
    }
    float value = 0.0f, count = 0.0f;
    if (t00 != 0) { value += unorm16_to_float(t00); count += 1.0f; }
    if (t01 != 0) { value += unorm16_to_float(t01); count += 1.0f; }
    if (t10 != 0) { value += unorm16_to_float(t10); count += 1.0f; }
    if (t11 != 0) { value += unorm16_to_float(t11); count += 1.0f; }
    if (count == 0.0f) return 0;
    return float_to_unorm16(value / count);
}

// the same for packed Rgba8 texels: a texel counts when any of r, g, b is non-zero (downsample.wgsl:31), all four
// channels are averaged; operation order of bt_kernels.hip downsample_texel<BT_FORMAT_RGBA8>
__device__ __forceinline__ float unorm8_to_float(uint32_t t) {
    const float x = float(t), r = 1.0f / 255.0f;
    const float q0 = x * r;
    return __builtin_fmaf(__builtin_fmaf(-q0, 255.0f, x), r, q0);
}
__device__ __forceinline__ uint32_t downsample4_rgba8(uint32_t t00, uint32_t t01, uint32_t t10, uint32_t t11) {
    const uint32_t t[4] = {t00, t01, t10, t11};
    if ((t00 & 0x00FFFFFFu) != 0 && (t01 & 0x00FFFFFFu) != 0 && (t10 & 0x00FFFFFFu) != 0 && (t11 & 0x00FFFFFFu) != 0) {
        // all four count (the common case): ((((0 + a) + b) + c) + d) / 4, and x / 4 == x * 0.25 exactly; the sum of four
        // values in [0, 1] stays in [0, 4], so the clamp of pack4x8unorm is a no-op.  Evaluated in the 2^8-scaled domain:
        // F(t) = fma(x, RN(1 / 255), x) == 256 * RN(t / 255) for all 256 inputs (bt_selftest), additions and the exact
        // factor 0.25 commute with the power-of-two scale, and 255 * v == (255 / 256) * (256 v) as real numbers, so every
        // rounding sees the value the unscaled expression sees — the same texel for a third of the conversion work.
        uint32_t out = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t sh = 8 * k;
            const float a = float((t00 >> sh) & 0xFFu), bq = float((t01 >> sh) & 0xFFu), cq = float((t10 >> sh) & 0xFFu), d = float((t11 >> sh) & 0xFFu);
            const float r = 1.0f / 255.0f;
            const float sum = ((__builtin_fmaf(a, r, a) + __builtin_fmaf(bq, r, bq)) + __builtin_fmaf(cq, r, cq)) + __builtin_fmaf(d, r, d);
            out |= uint32_t(0.5f + (255.0f / 256.0f) * (sum * 0.25f)) << sh;
        }
        return out;
    }
    float value[4] = {0.0f, 0.0f, 0.0f, 0.0f}, count = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; i++)
        if ((t[i] & 0x00FFFFFFu) != 0) {
#pragma unroll
            for (int k = 0; k < 4; k++) value[k] += unorm8_to_float((t[i] >> (8 * k)) & 0xFFu);
            count += 1.0f;
        }
    if (count == 0.0f) return 0;
    uint32_t out = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float e = value[k] / count;
        const float cl = e < 0.0f ? 0.0f : (e > 1.0f ? 1.0f : e);
        out |= uint32_t(floorf(0.5f + 255.0f * cl)) << (8 * k);
    }
    return out;
}

// general (slow) evaluation of the finest-LOD mosaic pixel (tile, r) from the source; used for the
// b x b corner aprons only.  `home` = atlas tile holding that pixel (for the keep-previous rule).
__device__ __forceinline__ uint32_t split_value_slow(const FusedArgs& A, const RasterDev& r, uint32_t tx, uint32_t rx, uint32_t ty,
                                                  uint32_t ry, uint32_t home_index) {
    const float scale = float(1u << A.lod);
    const uint32_t c = A.m.center_size, b = A.m.border_size, T = A.m.texture_size;
    const Axis ax = split_axis(rx, c, tx, scale, A.tlx, A.brx, r.width);
    const Axis ay = split_axis(ry, c, ty, scale, A.tly, A.bry, r.height);
    typedef const uint8_t __attribute__((address_space(1))) * global_bytes;
    typedef const uint16_t __attribute__((address_space(1))) * global_u16;
    const global_u16 row0 = (global_u16)((global_bytes)r.data + uint64_t(ay.i0) * r.pitch);
    const global_u16 row1 = (global_u16)((global_bytes)r.data + uint64_t(ay.i1) * r.pitch);
    const uint32_t t00 = row0[ax.i0], t10 = row0[ax.i1], t01 = row1[ax.i0], t11 = row1[ax.i1];
    if (t00 == 0 || t10 == 0 || t01 == 0 || t11 == 0) {
        if (home_index == kInvalid || A.prev_zero) return 0;
        return A.atlas[uint64_t(home_index) * T * T + uint64_t(b + ry) * T + b + rx];
    }
    const float top = mixf(unorm16_to_float(t00), unorm16_to_float(t10), ax.fr);
    const float bot = mixf(unorm16_to_float(t01), unorm16_to_float(t11), ax.fr);
    return float_to_unorm16(mixf(top, bot, ay.fr));
}

// blockIdx -> logical work id such that each XCD (blocks b, b+8, b+16, ... run on XCD b % 8) walks a
// contiguous range of work: neighbouring row groups / tiles then share source halos through one L2.
__device__ __forceinline__ uint32_t xcd_remap(uint32_t bid, uint32_t total) {
    const uint32_t q = total / 8u, r = total % 8u, xcd = bid % 8u, i = bid / 8u;
    return (xcd < r ? xcd * (q + 1u) : r * (q + 1u) + (xcd - r) * q) + i;
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

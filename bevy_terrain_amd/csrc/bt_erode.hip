// bt_atlas_erode_height: the kernels.  The host half is beside the region calls in bt_edit.cpp; the definition is the EROSION section of
// include/bevy_terrain_amd.h.
//
// erode_init_kernel    raw texels -> b, the four flux planes (0) and the activity bytes of ping-pong side 0; d and s hold the caller's water
//                      and sediment (staged into them) or are set to 0.  An inactive cell (raw 0: no data or a tile the atlas does not hold) holds zeros in every plane.
// erode_step_kernel    one step.  A workgroup owns kErodeBlock x kErodeBlock cells and stages them plus a halo of kHalo = 3 cells in LDS (7
//                      float planes and the activity bytes; d is staged as d1 = d + rain_dt; a cell outside the window or inactive is staged
//                      as zeros, so a wall reads as "no flux" without a test).  Phase A runs on the cells up to 2 out (the new fluxes,
//                      written over the old ones in place: A reads no other cell's flux), phase B on the cells up to 1 out (each thread its four
//                      own cells, whose b1, d2 and s1 stay in registers, and the first 132 threads one cell of the ring around the block, of
//                      which only s1 is wanted; s1 goes over s in place: B reads no other cell's s), phase C on the block.  A barrier stands
//                      between the phases.  What a workgroup recomputes of its neighbours' cells is the same arithmetic on the same
//                      inputs, so the result does not depend on the block size.  Every plane is written once, by the cell's owner: no atomics.
// erode_finish_kernel  the blend with the weight plane and the quantisation -> the staged rectangle of R16 texels (ctx->edit_region) that
//                      edit_region_kernel copies into the layers; a texel that keeps its value is copied from the gathered texels.
//
// LDS: 38 * 38 * (7 * 4 + 1) = 41876 bytes, three workgroups on a CU's 160 KiB.  ds_read_b32 / ds_write_b32 bank by (address / 4) % 32 within a
// 32-lane half: a half-wave is one row of 32 consecutive cells in phases B and C (any pitch is free of conflicts) and 32 consecutive cells
// of the strided loops of the load and phase A, which wrap at most once (two runs of consecutive addresses: 2-way on the 2 or 6 banks they share).
//
// Arithmetic contract: IEEE binary32 with subnormals kept (the default mode of a gfx950 kernel), one rounding per written operation; this
// file is compiled with -ffp-contract=off, `/` and sqrtf are correctly rounded.
#include "bt_internal.hpp"

namespace bt {

namespace {

constexpr uint32_t kErodeThreads = 256;
constexpr uint32_t kHalo = 3;
constexpr uint32_t kTile = kErodeBlock + 2u * kHalo;  // 38
constexpr uint32_t kTileCells = kTile * kTile;
constexpr uint32_t kOwn = kErodeBlock * kErodeBlock / kErodeThreads;  // cells of a thread: rows ly, ly + 8, ly + 16, ly + 24
constexpr uint32_t kRing = 4u * (kErodeBlock + 1u);                   // the cells one out of the block
static_assert(kRing <= kErodeThreads && kErodeThreads % kErodeBlock == 0, "one ring cell per thread, whole rows per trip");

// neighbour k = 0..3: (1,0), (0,1), (-1,0), (0,-1), as an offset in the tile
__device__ __forceinline__ int erode_off(int k) { return k == 0 ? 1 : k == 1 ? int(kTile) : k == 2 ? -1 : -int(kTile); }

__device__ __forceinline__ float erode_height(uint32_t raw, const ErodeConsts& c) { return c.min_height + c.range * (float(raw) / 65535.0f); }

struct ErodeLds {
    float b[kTileCells], d[kTileCells], s[kTileCells], f[4][kTileCells];
    uint8_t a[kTileCells];
};

// phase B of the active cell at tile index t: b1, d2, s1
__device__ __forceinline__ void erode_exchange(const ErodeLds& l, uint32_t t, const ErodeConsts& c, float& b1, float& d2, float& s1) {
    const float b = l.b[t], d1 = l.d[t], s = l.s[t];
    float f[4], in[4], bn[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t n = uint32_t(int(t) + erode_off(k));
        f[k] = l.f[k][t];
        in[k] = l.f[(k + 2) & 3][n];  // a wall holds 0
        bn[k] = l.a[n] ? l.b[n] : b;
    }
    const float out = ((f[0] + f[1]) + f[2]) + f[3];
    const float inflow = ((in[0] + in[1]) + in[2]) + in[3];
    const float dn = d1 + (c.dt * (inflow - out)) / c.l2;
    d2 = dn > 0.0f ? dn : 0.0f;
    float dm = 0.5f * (d1 + d2);
    dm = dm > c.min_depth ? dm : c.min_depth;
    const float wx = 0.5f * ((in[2] - f[2]) + (f[0] - in[0]));
    const float wy = 0.5f * ((in[3] - f[3]) + (f[1] - in[1]));
    const float vx = wx / (c.cell_size * dm), vy = wy / (c.cell_size * dm);
    const float speed = sqrtf(vx * vx + vy * vy);
    const float gx = (bn[0] - bn[2]) / c.two_l, gy = (bn[1] - bn[3]) / c.two_l;
    const float g2 = gx * gx + gy * gy;
    float sin_a = sqrtf(g2 / (1.0f + g2));
    sin_a = sin_a > c.min_tilt ? sin_a : c.min_tilt;
    const float C = (c.capacity * sin_a) * speed;
    if (C > s) {
        const float x = c.erode * (C - s);
        b1 = b - x, s1 = s + x;
    } else {
        const float x = c.deposit * (s - C);
        b1 = b + x, s1 = s - x;
    }
}

// m[k] of phase C for a cell with sediment s1, flux f and d1: what it sends towards k
__device__ __forceinline__ float erode_sent(float s1, float f, float d1, const ErodeConsts& c) {
    const float vol = d1 * c.l2;
    return vol > 0.0f ? s1 * ((f * c.dt) / vol) : 0.0f;
}

__global__ __launch_bounds__(kErodeThreads) void erode_init_kernel(const uint16_t* __restrict__ raw, bool water, bool sediment, ErodePlanes p, uint8_t* __restrict__ act,
                                                                   uint32_t cells, ErodeConsts c) {
    const uint32_t i = blockIdx.x * kErodeThreads + threadIdx.x;
    if (i >= cells) return;
    const uint32_t t = raw[i];
    const bool a = t != 0u;
    act[i] = a ? 1u : 0u;
    p.b[i] = a ? erode_height(t, c) : 0.0f;
    p.d[i] = a && water ? p.d[i] : 0.0f;  // the caller's planes were staged into d and s themselves
    p.s[i] = a && sediment ? p.s[i] : 0.0f;
#pragma unroll
    for (int k = 0; k < 4; k++) p.f[k][i] = 0.0f;
}

__global__ __launch_bounds__(kErodeThreads) void erode_step_kernel(ErodePlanes in, ErodePlanes out, const uint8_t* __restrict__ act, uint32_t width, uint32_t height, ErodeConsts c) {
    __shared__ ErodeLds l;
    const uint32_t tid = threadIdx.x;
    const int gx0 = int(blockIdx.x * kErodeBlock) - int(kHalo), gy0 = int(blockIdx.y * kErodeBlock) - int(kHalo);
    for (uint32_t t = tid; t < kTileCells; t += kErodeThreads) {
        const int gx = gx0 + int(t % kTile), gy = gy0 + int(t / kTile);
        float b = 0.0f, d = 0.0f, s = 0.0f, f[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        bool a = false;
        if (gx >= 0 && gy >= 0 && gx < int(width) && gy < int(height)) {
            const uint32_t i = uint32_t(gy) * width + uint32_t(gx);
            a = act[i] != 0u;
            if (a) {
                b = in.b[i], d = in.d[i] + c.rain_dt, s = in.s[i];
#pragma unroll
                for (int k = 0; k < 4; k++) f[k] = in.f[k][i];
            }
        }
        l.a[t] = a ? 1u : 0u;
        l.b[t] = b, l.d[t] = d, l.s[t] = s;
#pragma unroll
        for (int k = 0; k < 4; k++) l.f[k][t] = f[k];
    }
    __syncthreads();

    // A: the fluxes of the cells up to 2 out
    constexpr uint32_t kA = kTile - 2u;
    for (uint32_t j = tid; j < kA * kA; j += kErodeThreads) {
        const uint32_t t = (1u + j / kA) * kTile + 1u + j % kA;
        if (!l.a[t]) continue;
        const float d1 = l.d[t], H = l.b[t] + d1;
        float f[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t n = uint32_t(int(t) + erode_off(k));
            f[k] = 0.0f;
            if (l.a[n]) {
                const float Hn = l.b[n] + l.d[n];
                const float v = l.f[k][t] + c.cf * (H - Hn);
                f[k] = v > 0.0f ? v : 0.0f;
            }
        }
        const float sum = ((f[0] + f[1]) + f[2]) + f[3];
        const float leaves = sum * c.dt, vol = d1 * c.l2;
        if (leaves > vol) {
            const float K = vol / leaves;
#pragma unroll
            for (int k = 0; k < 4; k++) f[k] = f[k] * K;
        }
#pragma unroll
        for (int k = 0; k < 4; k++) l.f[k][t] = f[k];
    }
    __syncthreads();

    // B: the exchange of the thread's own cells, and of one cell of the ring around the block
    const uint32_t lx = tid % kErodeBlock, ly0 = tid / kErodeBlock;
    float b1[kOwn], d2[kOwn], s1[kOwn];
#pragma unroll
    for (uint32_t j = 0; j < kOwn; j++) {
        const uint32_t t = (ly0 + j * (kErodeThreads / kErodeBlock) + kHalo) * kTile + lx + kHalo;
        b1[j] = d2[j] = s1[j] = 0.0f;
        if (l.a[t]) {
            erode_exchange(l, t, c, b1[j], d2[j], s1[j]);
            l.s[t] = s1[j];
        }
    }
    if (tid < kRing) {
        constexpr uint32_t lo = kHalo - 1u, hi = kHalo + kErodeBlock, side = kErodeBlock + 2u;
        const uint32_t r = tid;
        const uint32_t tx = r < side ? lo + r : r < 2u * side ? lo + r - side : r < 2u * side + kErodeBlock ? lo : hi;
        const uint32_t ty = r < side ? lo : r < 2u * side ? hi : r < 2u * side + kErodeBlock ? kHalo + r - 2u * side : kHalo + r - 2u * side - kErodeBlock;
        const uint32_t t = ty * kTile + tx;
        if (l.a[t]) {
            float ring_b1, ring_d2, ring_s1;
            erode_exchange(l, t, c, ring_b1, ring_d2, ring_s1);
            l.s[t] = ring_s1;
        }
    }
    __syncthreads();

    // C: transport and evaporation of the own cells
#pragma unroll
    for (uint32_t j = 0; j < kOwn; j++) {
        const uint32_t ly = ly0 + j * (kErodeThreads / kErodeBlock);
        const uint32_t gx = blockIdx.x * kErodeBlock + lx, gy = blockIdx.y * kErodeBlock + ly;
        if (gx >= width || gy >= height) continue;
        const uint32_t t = (ly + kHalo) * kTile + lx + kHalo, i = gy * width + gx;
        float f[4] = {0.0f, 0.0f, 0.0f, 0.0f}, d3 = 0.0f, s2 = 0.0f;
        if (l.a[t]) {
            const float d1 = l.d[t];
            float m[4], mn[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t n = uint32_t(int(t) + erode_off(k));
                f[k] = l.f[k][t];
                m[k] = erode_sent(s1[j], f[k], d1, c);
                mn[k] = l.a[n] ? erode_sent(l.s[n], l.f[(k + 2) & 3][n], l.d[n], c) : 0.0f;
            }
            const float mo = ((m[0] + m[1]) + m[2]) + m[3];
            const float mi = ((mn[0] + mn[1]) + mn[2]) + mn[3];
            const float sn = (s1[j] - mo) + mi;
            s2 = sn > 0.0f ? sn : 0.0f;
            d3 = d2[j] * c.keep;
        }
        out.b[i] = b1[j], out.d[i] = d3, out.s[i] = s2;
#pragma unroll
        for (int k = 0; k < 4; k++) out.f[k][i] = f[k];
    }
}

__global__ __launch_bounds__(kErodeThreads) void erode_finish_kernel(const uint16_t* __restrict__ raw, const float* __restrict__ bT, const uint8_t* __restrict__ weight,
                                                                     uint16_t* __restrict__ texels, uint32_t cells, ErodeConsts c) {
    const uint32_t i = blockIdx.x * kErodeThreads + threadIdx.x;
    if (i >= cells) return;
    const uint32_t t = raw[i];
    uint32_t o = t;
    const uint32_t wb = weight ? uint32_t(weight[i]) : 255u;
    if (t != 0u && wb != 0u) {
        const float w = weight ? float(wb) / 255.0f : 1.0f;
        const float b0 = erode_height(t, c), b = bT[i];
        const float h = b0 + (b - b0) * w;
        if (__float_as_uint(b) != __float_as_uint(b0) && fabsf(h) < __builtin_inff()) {  // (a NaN fails the test)
            const float q = (h - c.min_height) / c.range;
            const float q01 = q < 0.0f ? 0.0f : q > 1.0f ? 1.0f : q;
            const float v = floorf(0.5f + 65535.0f * q01);
            o = v > 1.0f ? uint32_t(v) : 1u;
        }
    }
    texels[i] = uint16_t(o);
}

}  // namespace

bt_status launch_erode_init(hipStream_t stream, const uint16_t* raw, bool water, bool sediment, const ErodePlanes& p, uint8_t* act, uint32_t cells, const ErodeConsts& c) {
    erode_init_kernel<<<dim3((cells + kErodeThreads - 1u) / kErodeThreads), kErodeThreads, 0, stream>>>(raw, water, sediment, p, act, cells, c);
    return launched("erode_init_kernel");
}

bt_status launch_erode_step(hipStream_t stream, const ErodePlanes& in, const ErodePlanes& out, const uint8_t* act, uint32_t width, uint32_t height, const ErodeConsts& c) {
    erode_step_kernel<<<dim3((width + kErodeBlock - 1u) / kErodeBlock, (height + kErodeBlock - 1u) / kErodeBlock), kErodeThreads, 0, stream>>>(in, out, act, width, height, c);
    return launched("erode_step_kernel");
}

bt_status launch_erode_finish(hipStream_t stream, const uint16_t* raw, const float* bT, const uint8_t* weight, uint16_t* texels, uint32_t cells, const ErodeConsts& c) {
    erode_finish_kernel<<<dim3((cells + kErodeThreads - 1u) / kErodeThreads), kErodeThreads, 0, stream>>>(raw, bT, weight, texels, cells, c);
    return launched("erode_finish_kernel");
}

}  // namespace bt

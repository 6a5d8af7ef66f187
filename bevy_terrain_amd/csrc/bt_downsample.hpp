// Texel conversions and the per-texel downsample arithmetic (downsample.wgsl:12-40) shared by the batched kernels (bt_kernels.hip) and the
// in-place edit kernels (bt_edit.hip): both run the SAME device function, so an incremental update cannot drift from a full run.
// Device code only; included inside namespace bt { namespace { ... } } of a file compiled with -ffp-contract=off.
#pragma once

// t / 65535 and t / 255, correctly rounded, as mul + two fma (Markstein): equal to the IEEE division for every
// input of the range — exhaustively checked on the device by bt_selftest and on the CPU by the oracle tests
__device__ __forceinline__ float unorm16_to_float(uint32_t t) {
    const float x = float(t), r = 1.0f / 65535.0f;
    const float q0 = x * r;
    return __builtin_fmaf(__builtin_fmaf(-q0, 65535.0f, x), r, q0);
}
__device__ __forceinline__ float unorm8_to_float(uint32_t t) {
    const float x = float(t), r = 1.0f / 255.0f;
    const float q0 = x * r;
    return __builtin_fmaf(__builtin_fmaf(-q0, 255.0f, x), r, q0);
}

// pack2x16unorm / pack4x8unorm component: floor(0.5 + N * clamp(e, 0, 1))
__device__ __forceinline__ uint32_t float_to_unorm(float e, float n) {
    const float cl = e < 0.0f ? 0.0f : (e > 1.0f ? 1.0f : e);
    return uint32_t(floorf(0.5f + n * cl));
}

template <uint32_t FORMAT>
struct Texel;

template <>
struct Texel<BT_FORMAT_R16> {
    using type = uint16_t;
    static constexpr uint32_t kPerEntry = 2;
};
template <>
struct Texel<BT_FORMAT_RGBA8> {
    using type = uint32_t;
    static constexpr uint32_t kPerEntry = 1;
};

template <uint32_t FORMAT>
__device__ __forceinline__ uint32_t downsample_texel(const typename Texel<FORMAT>::type* __restrict__ child,
                                                     uint32_t Tsz, uint32_t cx, uint32_t cy) {
    // OFFSETS (0,0),(0,1),(1,0),(1,1) as (dx,dy): downsample.wgsl:25
    uint32_t t[4];
    if (child) {
        t[0] = child[uint64_t(cy) * Tsz + cx];
        t[1] = child[uint64_t(cy + 1) * Tsz + cx];
        t[2] = child[uint64_t(cy) * Tsz + cx + 1];
        t[3] = child[uint64_t(cy + 1) * Tsz + cx + 1];
    } else {
        t[0] = t[1] = t[2] = t[3] = 0;  // child tile absent: the layer reads as zero
    }
    if constexpr (FORMAT == BT_FORMAT_R16) {
        float value = 0.0f, count = 0.0f;
#pragma unroll
        for (int i = 0; i < 4; i++)
            if (t[i] != 0) {  // any(child_value.xyz != 0) with xyz = (r, 0, 0)
                value += unorm16_to_float(t[i]);
                count += 1.0f;
            }
        if (count == 0.0f) return 0;  // 0/0: defined as "no data" (oracle)
        return float_to_unorm(value / count, 65535.0f);
    } else {
        float value[4] = {0.0f, 0.0f, 0.0f, 0.0f}, count = 0.0f;
#pragma unroll
        for (int i = 0; i < 4; i++)
            if ((t[i] & 0x00FFFFFFu) != 0) {  // rgb != 0, alpha ignored
#pragma unroll
                for (int k = 0; k < 4; k++) value[k] += unorm8_to_float((t[i] >> (8 * k)) & 0xFFu);
                count += 1.0f;
            }
        if (count == 0.0f) return 0;
        uint32_t out = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) out |= float_to_unorm(value[k] / count, 255.0f) << (8 * k);
        return out;
    }
}

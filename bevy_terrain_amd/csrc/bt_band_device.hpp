// band(x; lo, hi, fade) of SPLAT step 4 (include/bevy_terrain_amd.h): the height and slope bands of a rule.  One definition for the splat
// kernel (bt_splat.hip) and the scatter kernels (bt_scatter.hip), whose rules carry the same six bounds.
//
// Arithmetic: IEEE binary32, one rounding per written operation (-ffp-contract=off), `/` is the correctly rounded division.
#pragma once

#include <hip/hip_runtime.h>

namespace bt {

#if defined(__HIPCC__)

__device__ __forceinline__ float clamp01(float t) { return t > 0.0f ? (t > 1.0f ? 1.0f : t) : 0.0f; }  // (a NaN gives 0)
__device__ __forceinline__ float smooth01(float t) { return (t * t) * (3.0f - 2.0f * t); }
// clamp01(num / fade) for a finite fade > 0.  The division is correctly rounded, hence monotonic: num >= fade gives a quotient >= 1, which
// clamps to 1, and num <= 0 one <= 0, which clamps to 0; a NaN is neither and clamps to 0.  So only a lane with 0 < num < fade needs the
// quotient, and where no lane of the wave does (most waves: fades are narrow and neighbours alike) the wave branches around the division.
__device__ __forceinline__ float ramp01(float num, float fade) {
    const bool inside = num > 0.0f && num < fade;
    float t = num >= fade ? 1.0f : 0.0f;
    if (__builtin_amdgcn_ballot_w64(inside) != 0ull)
        if (inside) t = clamp01(num / fade);
    return t;
}
// band(x; lo, hi, fade) of SPLAT step 4; fade is wave-uniform
__device__ __forceinline__ float band(float x, float lo, float hi, float fade) {
    float r, q;
    if (fade > 0.0f) {
        r = ramp01(x - (lo - fade), fade);
        q = ramp01((hi + fade) - x, fade);
    } else {
        r = x >= lo ? 1.0f : 0.0f;
        q = x <= hi ? 1.0f : 0.0f;
    }
    return smooth01(r) * smooth01(q);
}

#endif  // __HIPCC__

}  // namespace bt

// POINT of a tile (include/bevy_terrain_amd.h, "frustum and height-bounds culling") and coordinate_change_lod, the binary32 device
// functions of the reference's shaders (src/shaders/functions.wgsl:14-29, 73-96, 164-188) shared by the tiling prepass (bt_refine.hip:
// the divide test, the culling tests) and the terrain geometry (bt_geometry.hip: the vertex stage).  One definition, so a vertex of a
// tile lies where the divide test of that tile measured its distance, bit for bit.
//
// Arithmetic contract: IEEE binary32, one rounding per written operation (-ffp-contract=off), same operation order as
// oracle/bt_oracle.c.
#pragma once

#include "bt_internal.hpp"

#if defined(__HIPCC__)

namespace bt {
namespace {

struct Coordinate {  // types.wgsl:31-40
    uint32_t side, lod, x, y;
    float u, v;
};

// functions.wgsl:164-188; pow(2.0, f32(d)) is exact (ldexpf)
__device__ __forceinline__ void coordinate_change_lod(Coordinate& c, uint32_t new_lod) {
    const int d = int(new_lod) - int(c.lod);
    if (d == 0) return;
    const uint32_t delta_count = 1u << uint32_t(d < 0 ? -d : d);
    const float delta_size = ldexpf(1.0f, d);
    c.lod = new_lod;
    if (d > 0) {
        const float su = c.u * delta_size, sv = c.v * delta_size;
        c.x = c.x * delta_count + uint32_t(su);
        c.y = c.y * delta_count + uint32_t(sv);
        c.u = su - truncf(su);
        c.v = sv - truncf(sv);
    } else {
        const uint32_t x = c.x, y = c.y, sh = uint32_t(-d);  // delta_count = 2^sh: quotient and remainder by shift and mask
        c.x = x >> sh;
        c.y = y >> sh;
        c.u = (float(x & (delta_count - 1u)) + c.u) * delta_size;
        c.v = (float(y & (delta_count - 1u)) + c.v) * delta_size;
    }
}

__device__ __forceinline__ float length3(float x, float y, float z) { return sqrtf(x * x + y * y + z * z); }

// REL(coordinate) (include/bevy_terrain_amd.h, HIGH PRECISION): compute_relative_position (functions.wgsl:98-115), the position of a
// coordinate relative to the view from the second-order series of its side.  The coordinate goes to origin_lod, its offset from the view's
// coordinate is taken in integers first (i32, wrapping), and the series is summed left to right as the WGSL expression is, componentwise.  The side indexes
// two by-value kernel arguments; callers pass a workgroup-uniform side (>= 6 cannot come from a list of the view's terrain: read as 5).
struct Rel {
    float x, y, z;
};
__device__ __forceinline__ Rel relative_position(const bt_view_state& v, const bt_model_approximation& a, Coordinate c) {
    coordinate_change_lod(c, a.origin_lod);
    const uint32_t side = c.side < 6u ? c.side : 5u;
    const bt_side_parameter& o = v.sides[side];
    const bt_side_coefficients& k = a.sides[side];
    const float inv_oc = __builtin_bit_cast(float, (127u - a.origin_lod) << 23);  // x / 2^origin_lod == x * 2^-origin_lod bit for bit
    const float s = ((float(int32_t(c.x - uint32_t(o.view_xy[0]))) + c.u) - o.view_uv[0]) * inv_oc;
    const float t = ((float(int32_t(c.y - uint32_t(o.view_xy[1]))) + c.v) - o.view_uv[1]) * inv_oc;
    float r[3];
#pragma unroll
    for (int i = 0; i < 3; i++) r[i] = ((((k.c[i] + k.c_s[i] * s) + k.c_t[i] * t) + (k.c_ss[i] * s) * s) + (k.c_st[i] * s) * t) + (k.c_tt[i] * t) * t;
    return {r[0], r[1], r[2]};
}

// A point of a tile's surface and the normal there: compute_local_position (functions.wgsl:73-96) of the tile coordinate (u, w) =
// (tile xy + uv) / tile_count, then position_local_to_world / normal_local_to_world (:117-121).  point(tile, uv, h) = world + h * normal:
// the divide test's and the culling test's (include/bevy_terrain_amd.h).  l is the local position itself (the unit sphere's when spherical):
// the horizon test works from it.
struct SurfacePoint {
    float wx, wy, wz, nx, ny, nz, lx, ly, lz;
};

__device__ __forceinline__ SurfacePoint tile_surface(const bt_view_state& v, uint32_t side, float u, float w) {
    float lx, ly, lz;
    if (v.spherical) {
        const float C_SQR = 0.87f * 0.87f;
        u = (u - 0.5f) * 2.0f;
        w = (w - 0.5f) * 2.0f;
        u = u / sqrtf(1.0f + C_SQR - C_SQR * u * u);
        w = w / sqrtf(1.0f + C_SQR - C_SQR * w * w);
        switch (side) {
            case 0: lx = -1.0f; ly = -w; lz = u; break;
            case 1: lx = u; ly = -w; lz = 1.0f; break;
            case 2: lx = u; ly = 1.0f; lz = w; break;
            case 3: lx = 1.0f; ly = -u; lz = w; break;
            case 4: lx = w; ly = -u; lz = -1.0f; break;
            case 5: lx = w; ly = -1.0f; lz = u; break;
            default: lx = ly = lz = 0.0f; break;
        }
        const float l = length3(lx, ly, lz);
        lx = lx / l;
        ly = ly / l;
        lz = lz / l;
    } else {
        lx = u - 0.5f;
        ly = 0.0f;
        lz = w - 0.5f;
    }
    SurfacePoint p;
    const float* m = v.world_from_local;  // 3 columns + translation
    p.wx = (m[0] * lx + m[3] * ly + m[6] * lz) + m[9];
    p.wy = (m[1] * lx + m[4] * ly + m[7] * lz) + m[10];
    p.wz = (m[2] * lx + m[5] * ly + m[8] * lz) + m[11];
    const float nx0 = v.spherical ? lx : 0.0f, ny0 = v.spherical ? ly : 1.0f, nz0 = v.spherical ? lz : 0.0f;
    const float* t = v.local_from_world_transpose;
    const float nx = t[0] * nx0 + t[3] * ny0 + t[6] * nz0;
    const float ny = t[1] * nx0 + t[4] * ny0 + t[7] * nz0;
    const float nz = t[2] * nx0 + t[5] * ny0 + t[8] * nz0;
    const float nl = length3(nx, ny, nz);
    p.nx = nx / nl;
    p.ny = ny / nl;
    p.nz = nz / nl;
    p.lx = lx;
    p.ly = ly;
    p.lz = lz;
    return p;
}

}  // namespace
}  // namespace bt

#endif  // __HIPCC__

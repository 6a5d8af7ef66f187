// TILE NORMAL (include/bevy_terrain_amd.h, "surface normals"): the tangent-space normal of one R16 tile at a centre uv, the reference
// shader's sample_normal (src/shaders/attachments.wgsl:51-107) up to its TBN.  One definition for the two kernels of bt_normal.hip: the
// query fetches its texels from the atlas in HBM, the bake from the band of rows it holds in LDS.  And WORLD NORMAL, the query's normal of
// a world position, which the render kernel (bt_render.hip) evaluates at its hit points.
//
// Arithmetic: IEEE binary32, one rounding per written operation (the library is compiled without contraction).
#pragma once

#include "bt_tile_tree_device.hpp"

namespace bt {

// side_length of sample_normal: config.scale is TerrainModel::scale() (terrain_model.rs:183-193) `as f32`, which for a planar model is
// HALF its side length — the reference's quirk, kept
BT_HD float normal_side_length(const model::Model& m) {
    const float scale = float(model::model_scale(m));
    return model::is_spherical(m) ? (3.14159265359f / 4.0f) * scale : scale;
}

#if defined(__HIPCC__)

struct F3 {
    float x, y, z;
};
__device__ __forceinline__ float dot3f(F3 a, F3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ F3 norm3f(F3 v) {
    const float r = 1.0f / sqrtf(dot3f(v, v));
    return {v.x * r, v.y * r, v.z * r};
}
__device__ __forceinline__ F3 cross3f(F3 a, F3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

// what TILE NORMAL needs besides the attachment: the height range and side_length of the model
struct NormalModel {
    float min_height, max_height, side_length;
};

// what the taps of one attachment share: uv -> texture uv, the tap offset, T as a float
struct NormalTaps {
    float scale, offset, o, T;
    uint32_t size;  // T
};
__device__ __forceinline__ NormalTaps normal_taps(const AttachmentMeta& m) {
    const float T = float(m.texture_size);
    return {float(m.center_size) / T, float(m.border_size) / T, 0.5f / float(m.center_size), T, m.texture_size};
}
// dist of TILE NORMAL
__device__ __forceinline__ float normal_dist(const AttachmentMeta& m, const NormalModel& nm, uint32_t lod) {
    return nm.side_length / (float(m.center_size) * float(1u << lod));
}

// where the taps of one centre uv fall: per axis and offset (-o, 0, +o) the lerp weight and the first texel of the pair
struct TapSplit {
    float rem[2][3];
    int first[2][3];
};
// rem = fmodf(t, 1.0f) is computed as t - truncf(t): the same value for every finite t (both are exact; they differ only in the sign of a
// zero, which the lerps absorb: v00 + (+-0) = v00 for the unorm values v00 >= +0) and NaN alike for the others
__device__ __forceinline__ TapSplit tap_split(const NormalTaps& tp, const float uv[2]) {
    TapSplit sp;
#pragma unroll
    for (int a = 0; a < 2; a++) {
        const float u = uv[a] * tp.scale + tp.offset;
        const float p[3] = {u - tp.o, u, u + tp.o};
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float t = p[k] * tp.T - 0.5f;
            sp.rem[a][k] = t - truncf(t);
            sp.first[a][k] = int(t);
        }
    }
    return sp;
}

// s(layer, lod, uv) from the split on: fetch(px, py) returns the raw texel (px, py) of the layer.  The taps left / right share their row
// pair and weight, up / down their column pair.
template <typename Fetch>
__device__ __forceinline__ F3 tile_normal(const NormalTaps& tp, const NormalModel& nm, float dist, const TapSplit& sp, Fetch fetch) {
    auto tap = [&](int kx, int ky) -> float {
        float v[2][2];
#pragma unroll
        for (int x = 0; x < 2; x++)
#pragma unroll
            for (int y = 0; y < 2; y++) v[x][y] = unorm16_to_float(fetch(texel_clamp(sp.first[0][kx] + x, tp.size), texel_clamp(sp.first[1][ky] + y, tp.size)));
        const float value = bilerp(v[0][0], v[0][1], v[1][0], v[1][1], sp.rem[0][kx], sp.rem[1][ky]);
        return nm.min_height + (nm.max_height - nm.min_height) * value;  // height_of_value
    };
    const float left = tap(0, 1), up = tap(1, 0), right = tap(2, 1), down = tap(1, 2);
    return norm3f({left - right, down - up, dist});
}

// n_i of WORLD NORMAL: the tile's tangent-space normal through the TBN of the position, normalised
__device__ __forceinline__ F3 lookup_normal(const AttachmentMeta& m, const uint16_t* __restrict__ atlas, const NormalModel& nm, const Lookup& l, bool spherical, F3 tan,
                                            F3 bit, F3 N) {
    F3 s = {0.0f, 0.0f, 1.0f};  // nothing loaded: every tap samples 0
    if (l.atlas_index < m.atlas_size) {
        const uint32_t T = m.texture_size;
        const uint16_t* tile = atlas + uint64_t(l.atlas_index) * T * T;
        const NormalTaps tp = normal_taps(m);
        s = tile_normal(tp, nm, normal_dist(m, nm, l.atlas_lod), tap_split(tp, l.uv), [&](uint32_t px, uint32_t py) -> uint32_t { return tile[uint64_t(py) * T + px]; });
    }
    if (!spherical) return norm3f({s.x, s.z, s.y});
    return norm3f({(tan.x * s.x + bit.x * s.y) + N.x * s.z, (tan.y * s.x + bit.y * s.y) + N.y * s.z, (tan.z * s.x + bit.z * s.y) + N.z * s.z});
}

// WORLD NORMAL at world position p (steps 1 - 10): the normal and, in `cosine`, up_dot.  One definition for tile_tree_normal_kernel
// (bt_normal.hip) and render_kernel (bt_render.hip).
__device__ __forceinline__ F3 world_normal(const Ground& G, const NormalModel& nm, model::V3 p, float& cosine) {
    using namespace model;
    const TreeParams& P = G.P;
    const uint16_t* atlas = (const uint16_t*)G.atlas;
    F3 out = {0.0f, 0.0f, 0.0f};
    cosine = 0.0f;
    if (isfinite(p.x) && isfinite(p.y) && isfinite(p.z)) {
        const bool spherical = is_spherical(P.model);
        const V3 local = position_world_to_local(P.model, p);
        const V3 surface = position_local_to_world(P.model, local, G.approximate_height);
        // normal_local_to_world: local_from_world_transpose * local, identity rotation
        F3 VN = {0.0f, 1.0f, 0.0f};
        if (spherical) {
            const V3 v = normalize3({local.x / P.model.scale.x, local.y / P.model.scale.y, local.z / P.model.scale.z});
            VN = {float(v.x), float(v.y), float(v.z)};
        }
        const F3 N = norm3f(VN);
        const Coordinate c = coordinate_from_world_position(surface, P.model);
        F3 tan = {0.0f, 0.0f, 0.0f}, bit = tan;
        if (spherical) {
            const uint32_t pair = c.side >> 1;  // FACE_UP (attachments.wgsl:55-62)
            const F3 face_up = {pair == 2u ? -1.0f : 0.0f, pair == 0u ? 1.0f : 0.0f, pair == 1u ? -1.0f : 0.0f};
            tan = cross3f(face_up, N);
            bit = cross3f(N, tan);
        }
        uint32_t lod;
        float ratio;
        compute_blend(P, surface, lod, ratio);
        F3 n = lookup_normal(G.m, atlas, nm, lookup_tile_at(P, G.entries, c, lod), spherical, tan, bit, N);
        if (ratio > 0.0f) {
            const F3 n2 = lookup_normal(G.m, atlas, nm, lookup_tile_at(P, G.entries, c, lod - 1u), spherical, tan, bit, N);
            n = {n.x + (n2.x - n.x) * ratio, n.y + (n2.y - n.y) * ratio, n.z + (n2.z - n.z) * ratio};
        }
        out = dot3f(n, n) > 0.0f ? norm3f(n) : N;
        cosine = dot3f(out, N);
    }
    return out;
}

// enc of the normal map: [-1, 1] -> a byte, round half up
__device__ __forceinline__ uint32_t normal_enc(float v) {
    const float x = 0.5f + 0.5f * v;
    const float cl = x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x);
    return uint32_t(floorf(0.5f + 255.0f * cl));
}

// enc8 of the render section: [0, 1] -> a byte, round half up (bt_render.hip's colour plane, bt_splat.hip's channels)
__device__ __forceinline__ uint32_t enc8(float v) {
    const float c = v > 0.0f ? (v > 1.0f ? 1.0f : v) : 0.0f;  // (a NaN encodes as 0)
    return uint32_t(floorf(0.5f + 255.0f * c));
}

#endif  // __HIPCC__

}  // namespace bt

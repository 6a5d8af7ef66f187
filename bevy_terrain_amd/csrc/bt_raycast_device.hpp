// The per-sample evaluation of a ray against the terrain (include/bevy_terrain_amd.h, "batched ray queries"): f(p) = altitude(p) - h(p)
// and the test f <= 0, one definition for the two kernels that march rays: raycast_kernel (bt_raycast.hip, one wave per ray) and
// render_kernel (bt_render.hip, one lane per pixel).  So a pixel of bt_tile_tree_render meets the ground where bt_tile_tree_raycast says
// its ray does, bit for bit.
#pragma once

#include "bt_tile_tree_device.hpp"

namespace bt {

#if defined(__HIPCC__)

struct RayEval {
    bool below;    // f(p) <= 0
    float height;  // h(p), when it was sampled (always when below)
    float value;   // the attachment value h was made of (bt_tile_tree_sample_attachment's first component at p); the render kernel's grey
};

__device__ __forceinline__ model::V3 ray_point(const bt_ray& r, double t) {
    return {r.origin[0] + t * r.direction[0], r.origin[1] + t * r.direction[1], r.origin[2] + t * r.direction[2]};
}

__device__ __forceinline__ RayEval ray_eval(const TreeParams& P, const bt_tile_tree_entry* __restrict__ entries, const AttachmentMeta& m,
                                            const void* __restrict__ atlas, model::V3 p, double approximate_height, bool skip_above, double ceiling) {
    using namespace model;
    const Model& model = P.model;
    const V3 local = position_world_to_local(model, p);
    const V3 n = normalize3(transform_vector(model, is_spherical(model) ? local : V3{0.0, 1.0, 0.0}));
    const V3 ground0 = position_local_to_world(model, local, 0.0);
    const double altitude = dot3({p.x - ground0.x, p.y - ground0.y, p.z - ground0.z}, n);
    if (skip_above && altitude > ceiling) return {false, 0.0f, 0.0f};
    // surface_position(model, p, approximate_height) with the local position at hand
    const V3 surface = position_local_to_world(model, local, approximate_height);
    float value[4];
    sample_surface(P, entries, m, atlas, surface, value);
    const float h = height_of_value(model, value[0]);
    const double f = altitude - double(h);
    return {f <= 0.0, h, value[0]};
}

__device__ __forceinline__ bool finite(double v) { return fabs(v) <= 1.7976931348623157e308; }  // false for NaN and the infinities

#endif  // __HIPCC__

}  // namespace bt

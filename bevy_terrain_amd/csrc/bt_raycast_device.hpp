// The per-sample evaluation of a ray against the terrain (include/bevy_terrain_amd.h, "batched ray queries"): f(p) = altitude(p) - h(p)
// and the test f <= 0, one definition for the kernels that march rays: raycast_kernel (bt_raycast.hip, one wave per ray), render_kernel
// (bt_render.hip, one lane per pixel) and occlusion_kernel (bt_shadow.hip, one lane per shadow ray).  So a pixel of bt_tile_tree_render
// meets the ground where bt_tile_tree_raycast says its ray does, bit for bit.
//
// SUN OCCLUSION (the header's section of that name) is here too: occlusion_status, the any-hit march of one shadow ray, which the query
// kernel and the shadowed render kernel both call.  Its origin is lifted along the n of ray_frame, the frame ray_eval measures altitude in.
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

// the frame altitude is measured in at a world point p: its local position, the altitude direction n and the height-0 ground under it
struct RayFrame {
    model::V3 local, n, ground0;
};

__device__ __forceinline__ RayFrame ray_frame(const model::Model& model, model::V3 p) {
    using namespace model;
    const V3 local = position_world_to_local(model, p);
    const V3 n = normalize3(transform_vector(model, is_spherical(model) ? local : V3{0.0, 1.0, 0.0}));
    return {local, n, position_local_to_world(model, local, 0.0)};
}

__device__ __forceinline__ RayEval ray_eval(const TreeParams& P, const bt_tile_tree_entry* __restrict__ entries, const AttachmentMeta& m,
                                            const void* __restrict__ atlas, model::V3 p, double approximate_height, bool skip_above, double ceiling) {
    using namespace model;
    const Model& model = P.model;
    const RayFrame frame = ray_frame(model, p);
    const V3 &local = frame.local, &n = frame.n, &ground0 = frame.ground0;
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

// SUN OCCLUSION of the world point q for the direction s towards the light: the status bt_tile_tree_raycast gives the ray
// {q + lift * n(q), s, 0.0, distance} at `steps` steps and no refinement.  Lane-private: the march stops at the first sample at or under
// the ground, nothing crosses lanes.  dt and the t_i are written as the ray definition writes them.  A non-finite q is refused before
// its frame is computed: its origin would not be finite either.
__device__ __forceinline__ uint32_t occlusion_status(const TreeParams& P, const bt_tile_tree_entry* __restrict__ entries, const AttachmentMeta& m,
                                                     const void* __restrict__ atlas, model::V3 q, model::V3 s, double lift, double distance, uint32_t steps,
                                                     double approximate_height, bool skip_above, double ceiling) {
    using namespace model;
    if (!(finite(q.x) && finite(q.y) && finite(q.z))) return BT_RAY_INVALID;
    const V3 n = ray_frame(P.model, q).n;
    bt_ray ray;
    ray.origin[0] = q.x + lift * n.x;
    ray.origin[1] = q.y + lift * n.y;
    ray.origin[2] = q.z + lift * n.z;
    ray.direction[0] = s.x;
    ray.direction[1] = s.y;
    ray.direction[2] = s.z;
    ray.t_min = 0.0;
    ray.t_max = distance;
    bool valid = finite(ray.t_max) && ray.t_max >= ray.t_min;
    bool nonzero = false;
    for (int a = 0; a < 3; a++) {
        valid = valid && finite(ray.origin[a]) && finite(ray.direction[a]);
        nonzero = nonzero || ray.direction[a] != 0.0;
    }
    if (!(valid && nonzero)) return BT_RAY_INVALID;
    const double dt = (ray.t_max - ray.t_min) / double(steps);
    for (uint32_t i = 0; i <= steps; i++)
        if (ray_eval(P, entries, m, atlas, ray_point(ray, ray.t_min + double(i) * dt), approximate_height, skip_above, ceiling).below)
            return i == 0u ? BT_RAY_INSIDE : BT_RAY_HIT;
    return BT_RAY_MISS;
}

#endif  // __HIPCC__

}  // namespace bt

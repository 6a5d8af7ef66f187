// The per-sample evaluation of a ray against the terrain (include/bevy_terrain_amd.h, "batched ray queries"): f(p) = altitude(p) - h(p)
// and the test f <= 0, one definition for the kernels that march rays: raycast_kernel (bt_raycast.hip, one wave per ray), render_kernel
// (bt_render.hip, one lane per pixel) and occlusion_kernel (bt_shadow.hip, one lane per shadow ray).  So a pixel of bt_tile_tree_render
// meets the ground where bt_tile_tree_raycast says its ray does, bit for bit.
//
// What those kernels and sweep_kernel (bt_collide.hip) share besides ray_eval is here once as well: ray_valid (the validity of a ray),
// lane_march (the coarse any-hit march of one lane: render, occlusion), refine_bracket (one refinement round's new bracket: raycast,
// render) and wave_count (the three status counters of a wave: render, occlusion).
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

__device__ __forceinline__ RayEval ray_eval(const Ground& G, model::V3 p) {
    using namespace model;
    const Model& model = G.P.model;
    const RayFrame frame = ray_frame(model, p);
    const V3 &local = frame.local, &n = frame.n, &ground0 = frame.ground0;
    const double altitude = dot3({p.x - ground0.x, p.y - ground0.y, p.z - ground0.z}, n);
    if (G.skip_above && altitude > G.ceiling) return {false, 0.0f, 0.0f};
    // surface_position(model, p, approximate_height) with the local position at hand
    const V3 surface = position_local_to_world(model, local, G.approximate_height);
    float value[4];
    sample_ground(G, surface, value);
    const float h = height_of_value(model, value[0]);
    const double f = altitude - double(h);
    return {f <= 0.0, h, value[0]};
}

__device__ __forceinline__ bool finite(double v) { return fabs(v) <= 1.7976931348623157e308; }  // false for NaN and the infinities

// a valid ray of the header: finite t_min, t_max, origin and direction, t_max >= t_min, a direction that is not zero
__device__ __forceinline__ bool ray_valid(const bt_ray& ray) {
    bool valid = finite(ray.t_min) && finite(ray.t_max) && ray.t_max >= ray.t_min;
    bool nonzero = false;
    for (int a = 0; a < 3; a++) {
        valid = valid && finite(ray.origin[a]) && finite(ray.direction[a]);
        nonzero = nonzero || ray.direction[a] != 0.0;
    }
    return valid && nonzero;
}

// The coarse march of one lane, any-hit: samples t_i = t_min + i * dt, i = 0 .. steps, as the ray definition writes them, until the first
// at or under the ground.  Lane-private: nothing crosses lanes.  status: INSIDE (i == 0), HIT or MISS; step and e: the i and the
// evaluation that found the ground (0 and nothing on a MISS).  (raycast_kernel's march is another algorithm: 64 steps a round, a ballot.)
struct LaneMarch {
    uint32_t status, step;
    RayEval e;
};
__device__ __forceinline__ LaneMarch lane_march(const Ground& G, const bt_ray& ray, double dt, uint32_t steps) {
    for (uint32_t i = 0; i <= steps; i++) {
        const RayEval e = ray_eval(G, ray_point(ray, ray.t_min + double(i) * dt));
        if (e.below) return {i == 0u ? uint32_t(BT_RAY_INSIDE) : uint32_t(BT_RAY_HIT), i, e};
    }
    return {BT_RAY_MISS, 0u, {false, 0.0f, 0.0f}};
}

// one refinement round's new bracket from k, the smallest k in 1 .. 63 with u_k = lo + (hi - lo) * (k / 64) at or under the ground
// (64: none): (u_{k-1}, u_k], with u_0 = lo and u_64 = hi taken as they stand
struct Bracket {
    double lo, hi;
};
__device__ __forceinline__ Bracket refine_bracket(double lo, double hi, uint32_t k) {
    const double width = hi - lo;
    const double new_hi = k == 64u ? hi : lo + width * (double(k) / 64.0);
    const double new_lo = k == 1u ? lo : lo + width * (double(k - 1u) / 64.0);
    return {new_lo, new_hi};
}

// the status counters of a launch, a wave's share: how many of its lanes say a, b, c go to counters[0 .. 2] by lane 0.  Three ballots:
// every lane of the wave has to be here, whatever it did before
__device__ __forceinline__ void wave_count(uint32_t* counters, uint32_t lane, bool a, bool b, bool c) {
    const unsigned long long as = __ballot(a), bs = __ballot(b), cs = __ballot(c);
    if (lane == 0u) {
        if (as) atomicAdd(&counters[0], uint32_t(__popcll(as)));
        if (bs) atomicAdd(&counters[1], uint32_t(__popcll(bs)));
        if (cs) atomicAdd(&counters[2], uint32_t(__popcll(cs)));
    }
}

// SUN OCCLUSION of the world point q for the direction s towards the light: the status bt_tile_tree_raycast gives the ray
// {q + lift * n(q), s, 0.0, distance} at `steps` steps and no refinement.  A non-finite q is refused before its frame is computed: its
// origin would not be finite either.
__device__ __forceinline__ uint32_t occlusion_status(const Ground& G, model::V3 q, model::V3 s, double lift, double distance, uint32_t steps) {
    using namespace model;
    if (!(finite(q.x) && finite(q.y) && finite(q.z))) return BT_RAY_INVALID;
    const V3 n = ray_frame(G.P.model, q).n;
    bt_ray ray;
    ray.origin[0] = q.x + lift * n.x;
    ray.origin[1] = q.y + lift * n.y;
    ray.origin[2] = q.z + lift * n.z;
    ray.direction[0] = s.x;
    ray.direction[1] = s.y;
    ray.direction[2] = s.z;
    ray.t_min = 0.0;
    ray.t_max = distance;
    if (!ray_valid(ray)) return BT_RAY_INVALID;
    return lane_march(G, ray, (ray.t_max - ray.t_min) / double(steps), steps).status;
}

#endif  // __HIPCC__

}  // namespace bt

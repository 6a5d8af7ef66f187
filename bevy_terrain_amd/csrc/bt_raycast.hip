// Batched ray queries against the terrain (bt_tile_tree_raycast; the definition is in include/bevy_terrain_amd.h).
//
// The ground is wherever sample_height says it is: f(p) = altitude(p) - h(p), h from the device functions the sample kernel uses
// (bt_tile_tree_device.hpp), so a reported hit agrees with bt_tile_tree_sample_attachment at the hit point bit for bit.
//
// One wave per ray.  In a coarse round the 64 lanes evaluate 64 consecutive steps t_i; a ballot of f <= 0 and a find-first give the hit
// step, so the loop over rounds is wave-uniform and no lane leaves it early.  A refinement round is the same ballot over u_1 .. u_63
// (lane 0 idles).  A 256-step march with two refinements is at most six rounds of one sample per lane.  `steps` not a multiple of 64
// leaves lanes idle in the last coarse round.  The ellipsoid projection (a bisection, bt_model.hpp) diverges between lanes as it does in
// the sample kernel.  The height at the hit is taken from the lane that evaluated it (__shfl), the result leaves by lane 0.
//
// A sample whose altitude is above lerp(min_height, max_height, 1.0f) has f > 0 whatever the atlas holds: a bilinear sample of unorm
// texels and the blend of two of them stay within [0, 1] (rounding is monotone and every weight is in [0, 1] once the tile has a border,
// border_size >= 1) and the f32 lerp is monotone in its weight for max_height >= min_height.  Such a sample fetches nothing.
//
// That skip (Ground::skip_above / ceiling, built by ground_view of bt_tile_tree_device.hpp) and the per-sample evaluation (ray_eval), the
// validity of a ray (ray_valid) and the refinement's bracket (refine_bracket) live in bt_raycast_device.hpp, shared with the render kernel
// (bt_render.hip), the occlusion kernel (bt_shadow.hip) and the sweep kernel (bt_collide.hip).
#include "bt_raycast_device.hpp"

namespace bt {

using namespace bt::model;

namespace {

constexpr uint32_t kRaycastThreads = 256;  // four rays per workgroup, no LDS, no barrier
constexpr uint32_t kRaysPerGroup = kRaycastThreads / 64u;

__global__ __launch_bounds__(kRaycastThreads) void raycast_kernel(TreeParams P, const bt_tile_tree_entry* __restrict__ entries, AttachmentMeta m,
                                                                  const void* __restrict__ atlas, const bt_ray* __restrict__ rays, uint32_t count,
                                                                  uint32_t steps, uint32_t refine_rounds, bt_ray_hit* __restrict__ hits,
                                                                  const float* __restrict__ height) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t index = blockIdx.x * kRaysPerGroup + uint32_t(__builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)));
    if (index >= count) return;  // the whole wave
    const Ground G = ground_view(P, entries, m, atlas, height);
    const bt_ray ray = rays[index];

    bt_ray_hit hit{};
    if (!ray_valid(ray)) {
        hit.status = BT_RAY_INVALID;
        if (lane == 0) hits[index] = hit;
        return;
    }

    // coarse march: lane l of round r evaluates step 64 r + l
    const double dt = (ray.t_max - ray.t_min) / double(steps);
    bool found = false;
    uint32_t step = 0;
    float h_hit = 0.0f;
    for (uint32_t base = 0; base <= steps && !found; base += 64u) {
        const uint32_t i = base + lane;
        RayEval e = {false, 0.0f, 0.0f};
        if (i <= steps) e = ray_eval(G, ray_point(ray, ray.t_min + double(i) * dt));
        const unsigned long long bits = __ballot(e.below);
        if (bits) {
            const uint32_t first = uint32_t(__ffsll(bits)) - 1u;
            found = true;
            step = base + first;
            h_hit = __shfl(e.height, int(first));
        }
    }
    if (!found) {
        hit.status = BT_RAY_MISS;
        if (lane == 0) hits[index] = hit;
        return;
    }
    double lo, hi;
    if (step == 0) {
        hit.status = BT_RAY_INSIDE;
        lo = hi = ray.t_min;
    } else {
        hit.status = BT_RAY_HIT;
        lo = ray.t_min + double(step - 1u) * dt;
        hi = ray.t_min + double(step) * dt;
        // refinement: lane k evaluates u_k, k = 1 .. 63
        for (uint32_t round = 0; round < refine_rounds; round++) {
            const double width = hi - lo;
            RayEval e = {false, 0.0f, 0.0f};
            if (lane != 0) e = ray_eval(G, ray_point(ray, lo + width * (double(lane) / 64.0)));
            const unsigned long long bits = __ballot(e.below);
            const uint32_t k = bits ? uint32_t(__ffsll(bits)) - 1u : 64u;
            if (k != 64u) h_hit = __shfl(e.height, int(k));
            const Bracket b = refine_bracket(lo, hi, k);
            hi = b.hi;
            lo = b.lo;
        }
    }
    hit.step = step;
    hit.t = hi;
    hit.t_above = lo;
    const V3 p = ray_point(ray, hi);
    hit.position[0] = p.x;
    hit.position[1] = p.y;
    hit.position[2] = p.z;
    hit.height = h_hit;
    if (lane == 0) hits[index] = hit;
}

}  // namespace

bt_status launch_raycast(hipStream_t stream, const TerrainRef& g, const bt_ray* rays, uint32_t count, uint32_t steps, uint32_t refine_rounds, bt_ray_hit* hits) {
    if (!count) return BT_OK;
    raycast_kernel<<<(count + kRaysPerGroup - 1u) / kRaysPerGroup, kRaycastThreads, 0, stream>>>(g.P, g.entries, g.m, g.atlas, rays, count, steps, refine_rounds, hits,
                                                                                             g.height);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? BT_OK : hip_fail(e, "raycast_kernel");
}

}  // namespace bt

// Terrain collision: sphere contacts and sphere sweeps against the terrain (bt_tile_tree_collide_spheres, bt_tile_tree_sweep_spheres; the
// definitions, SPHERE CONTACT and SPHERE SWEEP, are in include/bevy_terrain_amd.h).
//
// One wave per sphere or per sweep, four waves per workgroup; no LDS, no barrier.  A round of the contact search is an 8 x 8 stencil of
// ground points, one per lane (lane l is column l & 7, row l >> 3), reduced across the wave (sphere_contact, bt_collide_device.hpp).  A
// sweep is a sequence of contacts at wave-uniform t: the coarse march stops at the first blocked step, the bisection halves the bracket,
// one more contact at t is the result; they share one loop, so the contact is compiled once.  Everything a wave branches on (the sphere, the foot, every status) is wave-uniform, so no lane
// leaves before the last cross-lane operation; a wave past the batch's end leaves whole.  The result leaves by lane 0.
//
// NOT MEASURED: the workgroup size (256 against 64 or 128) is the ray kernel's choice taken over, and the lane-to-stencil mapping (row-major
// 8 x 8 against a Morton order, which would keep a lane's neighbours in both directions within a row of 16) is the plainest one; nobody
// has timed the alternatives.
#include "bt_collide_device.hpp"

namespace bt {

using namespace bt::model;

namespace {

// the wave's sphere or sweep of the batch (wave-uniform)
__device__ __forceinline__ uint32_t wave_index() { return blockIdx.x * kCollideWavesPerGroup + uint32_t(__builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6))); }

__global__ __launch_bounds__(kCollideThreads) void collide_kernel(TreeParams P, const bt_tile_tree_entry* __restrict__ entries, AttachmentMeta m,
                                                                  const void* __restrict__ atlas, const bt_sphere* __restrict__ spheres, uint32_t count,
                                                                  uint32_t refine_rounds, bt_sphere_contact* __restrict__ contacts,
                                                                  const float* __restrict__ height) {
    const uint32_t lane = threadIdx.x & 63u, index = wave_index();
    if (index >= count) return;  // the whole wave
    const Ground G = ground_view(P, entries, m, atlas, height);
    const bt_sphere sphere = spheres[index];
    const bt_sphere_contact contact = sphere_contact(G, {sphere.center[0], sphere.center[1], sphere.center[2]}, sphere.radius, refine_rounds, lane);
    if (lane == 0) contacts[index] = contact;
}

__global__ __launch_bounds__(kCollideThreads) void sweep_kernel(TreeParams P, const bt_tile_tree_entry* __restrict__ entries, AttachmentMeta m,
                                                                const void* __restrict__ atlas, const bt_sphere_sweep* __restrict__ sweeps, uint32_t count,
                                                                uint32_t steps, uint32_t bisections, uint32_t refine_rounds, bt_sweep_hit* __restrict__ hits,
                                                                const float* __restrict__ height) {
    const uint32_t lane = threadIdx.x & 63u, index = wave_index();
    if (index >= count) return;  // the whole wave
    const Ground G = ground_view(P, entries, m, atlas, height);
    const bt_sphere_sweep sweep = sweeps[index];
    bt_ray ray;
    for (int a = 0; a < 3; a++) ray.origin[a] = sweep.origin[a], ray.direction[a] = sweep.direction[a];
    ray.t_min = sweep.t_min;
    ray.t_max = sweep.t_max;

    bt_sweep_hit hit{};
    if (!(ray_valid(ray) && finite(sweep.radius) && sweep.radius >= 0.0)) {
        hit.status = BT_RAY_INVALID;
        if (lane == 0) hits[index] = hit;
        return;
    }
    // one loop over the sweep's contacts, so that sphere_contact is compiled once: the coarse march (phase 0: step i), the bisection
    // (phase 1) and the contact at t (phase 2).  The phase and everything it depends on are wave-uniform.
    const double dt = (ray.t_max - ray.t_min) / double(steps);
    uint32_t phase = 0, i = 0, round = 0;
    double lo = 0.0, hi = 0.0;
    for (;;) {
        const double t = phase == 0u ? ray.t_min + double(i) * dt : (phase == 1u ? lo + (hi - lo) * 0.5 : hi);
        const bt_sphere_contact contact = sphere_contact(G, ray_point(ray, t), sweep.radius, refine_rounds, lane);
        if (phase == 2u) {
            hit.contact = contact;
            break;
        }
        const uint32_t status = uint32_t(__builtin_amdgcn_readfirstlane(int(contact.status)));  // (the same in every lane)
        const bool blocked = status == BT_CONTACT_TOUCHING || status == BT_CONTACT_BELOW;
        if (phase == 0u) {
            if (blocked) {
                hit.step = i;
                if (i == 0u) {
                    hit.status = BT_RAY_INSIDE;
                    lo = hi = ray.t_min;
                    phase = 2u;
                } else {
                    hit.status = BT_RAY_HIT;
                    lo = ray.t_min + double(i - 1u) * dt;
                    hi = t;
                    phase = bisections ? 1u : 2u;
                }
            } else if (++i > steps) {
                hit.status = BT_RAY_MISS;
                if (lane == 0) hits[index] = hit;
                return;
            }
        } else {
            if (blocked) hi = t;
            else lo = t;
            if (++round == bisections) phase = 2u;
        }
    }
    hit.t = hi;
    hit.t_above = lo;
    if (lane == 0) hits[index] = hit;
}

}  // namespace

bt_status launch_collide(hipStream_t stream, const TerrainRef& g, const bt_sphere* spheres, uint32_t count, uint32_t refine_rounds, bt_sphere_contact* contacts) {
    if (!count) return BT_OK;
    collide_kernel<<<(count + kCollideWavesPerGroup - 1u) / kCollideWavesPerGroup, kCollideThreads, 0, stream>>>(g.P, g.entries, g.m, g.atlas, spheres, count,
                                                                                                             refine_rounds, contacts, g.height);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? BT_OK : hip_fail(e, "collide_kernel");
}

bt_status launch_sweep(hipStream_t stream, const TerrainRef& g, const bt_sphere_sweep* sweeps, uint32_t count, uint32_t steps, uint32_t bisections,
                       uint32_t refine_rounds, bt_sweep_hit* hits) {
    if (!count) return BT_OK;
    sweep_kernel<<<(count + kCollideWavesPerGroup - 1u) / kCollideWavesPerGroup, kCollideThreads, 0, stream>>>(g.P, g.entries, g.m, g.atlas, sweeps, count, steps,
                                                                                                           bisections, refine_rounds, hits, g.height);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? BT_OK : hip_fail(e, "sweep_kernel");
}

}  // namespace bt

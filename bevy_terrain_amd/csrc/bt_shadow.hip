// Sun occlusion of a batch of world points (bt_tile_tree_sun_occlusion; the definition, SUN OCCLUSION, is in include/bevy_terrain_amd.h).
//
// A shadow ray is an any-hit ray: only its status is wanted, and most are decided within a few samples, or never fetch at all because
// they climb above the ceiling (ray_eval's skip).  bt_tile_tree_raycast would spend a wave and whole rounds of 64 samples on each; here a
// lane marches one ray sample by sample (occlusion_status of bt_raycast_device.hpp, the function the shadowed render kernel calls too)
// and leaves at its first sample at or under the ground.
//
// One lane per ray, 256 threads per workgroup; no LDS, no barrier.  Ray g of the batch is point g % count, direction g / count: the
// lanes of a wave march parallel rays from consecutive points of the caller's array, so where the caller's points are neighbours on the
// ground (a grid, the hit points of an image) the lanes visit the same tiles and share their fetches' cache lines.  Nothing crosses
// lanes until the counters at the very end, which every lane of every wave reaches: lanes past the launch's last ray skip the work,
// never the ballots.  The status leaves by a plain byte store (point-major, so the stores of a wave are direction_count bytes apart).
//
// NOT MEASURED: the lane mapping (point-fastest against direction-fastest) and the block size (256 against 64 or 128) are the render
// kernel's choices taken over; nobody has timed the alternatives.
#include "bt_raycast_device.hpp"

namespace bt {

using namespace bt::model;

namespace {

__global__ __launch_bounds__(kOcclusionThreads) void occlusion_kernel(TreeParams P, const bt_tile_tree_entry* __restrict__ entries, AttachmentMeta m,
                                                                      const void* __restrict__ atlas, OcclusionArgs a, const float* __restrict__ height) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t in_launch = blockIdx.x * kOcclusionThreads + threadIdx.x;
    const bool active = in_launch < a.ray_count;
    uint32_t status = BT_RAY_INVALID;

    if (active) {
        const uint32_t ray = a.first_ray + in_launch;  // (< count * direction_count <= BT_OCCLUSION_MAX_RAYS)
        const uint32_t direction = ray / a.count, point = ray - direction * a.count;
        const Ground G = ground_view(P, entries, m, atlas, height);
        const double* q = a.positions + 3ull * point;
        const double* s = a.directions + 3ull * direction;
        status = occlusion_status(G, {q[0], q[1], q[2]}, {s[0], s[1], s[2]}, a.lift, a.distance, a.steps);
        a.status[uint64_t(point) * a.direction_count + direction] = uint8_t(status);
    }

    // the ray counters: the whole wave is here, whatever its lanes did above
    // (lit, occluded, invalid)
    wave_count(a.counters, lane, active && status == BT_RAY_MISS, active && (status == BT_RAY_HIT || status == BT_RAY_INSIDE), active && status == BT_RAY_INVALID);
}

}  // namespace

bt_status launch_occlusion(hipStream_t stream, const TerrainRef& g, const OcclusionArgs& a) {
    if (!a.ray_count) return BT_OK;
    occlusion_kernel<<<(a.ray_count + kOcclusionThreads - 1u) / kOcclusionThreads, kOcclusionThreads, 0, stream>>>(g.P, g.entries, g.m, g.atlas, a, g.height);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? BT_OK : hip_fail(e, "occlusion_kernel");
}

}  // namespace bt

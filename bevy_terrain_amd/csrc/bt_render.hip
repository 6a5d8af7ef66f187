// A camera's view of the terrain, ray-cast image-order (bt_tile_tree_render; the definition is in include/bevy_terrain_amd.h).
//
// Every plane is made of the library's existing definitions: a pixel's ray is marched as bt_tile_tree_raycast marches it (ray_eval,
// lane_march and refine_bracket of bt_raycast_device.hpp, ceiling skip included), the normal at the hit is WORLD NORMAL (world_normal of bt_normal_device.hpp), the colour
// is the attachment value sample_surface returns there (bt_tile_tree_device.hpp).  So the image agrees with the point queries bit for bit.
//
// One lane per pixel, one wave per 8 x 8 block of pixels, four blocks per workgroup; no LDS, no barrier.  Neighbouring pixels visit the
// same tiles and leave the march at similar steps, so a wave's lanes share their fetches' cache lines and idle little behind the slowest
// of them.  A lane runs the definition as it is written: the smallest i with f <= 0, then per refinement round the smallest k in 1 .. 63;
// nothing crosses lanes until the pixel counters at the very end, which every lane of the wave reaches: lanes of pixels outside the
// image, of finished rays and of INVALID rays skip the work, never the ballots.  The hit's value and height come from the evaluation that
// found it.  Shading and the stores of the planes the caller asked for happen in the same launch.
//
// kShadow (bt_tile_tree_render_shadowed): a pixel that met the ground also marches its shadow ray, SUN OCCLUSION at p(t) towards the
// camera's sun (occlusion_status of bt_raycast_device.hpp, the function bt_tile_tree_sun_occlusion runs), in the same lane and before the
// colour is made; the march is left out where nothing could show its result (no shadow plane, and no colour plane, no lighting or a
// surface that faces away from the sun).  The false instance is bt_tile_tree_render's kernel as it was: it reads no shadow field.
#include "bt_normal_device.hpp"
#include "bt_raycast_device.hpp"

namespace bt {

using namespace bt::model;

namespace {

// (enc8 of the colour plane: bt_normal_device.hpp, shared with the splat kernel of bt_splat.hip)

template <bool kShadow>
__global__ __launch_bounds__(kRenderThreads) void render_kernel(TreeParams P, const bt_tile_tree_entry* __restrict__ entries, AttachmentMeta m,
                                                                const void* __restrict__ atlas, AttachmentMeta albedo_meta, const void* __restrict__ albedo,
                                                                NormalModel nm, RenderArgs a, const float* __restrict__ height) {
    const bt_render_camera& cam = a.camera;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t in_launch = blockIdx.x * kRenderBlocksPerGroup + uint32_t(__builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)));
    // the wave's 8 x 8 block, the lane's pixel in it (row-major: lane & 7 along x)
    const uint32_t block = a.first_block + in_launch;
    const uint32_t by = block / a.blocks_x, bx = block - by * a.blocks_x;
    const uint32_t x = bx * 8u + (lane & 7u), y = by * 8u + (lane >> 3);
    const bool active = in_launch < a.block_count && x < cam.width && y < cam.height;
    uint32_t status = BT_RAY_INVALID;

    if (active) {
        const Ground G = ground_view(P, entries, m, atlas, height);
        // PIXEL RAY
        const double sx = (2.0 * (double(x) + 0.5)) / double(cam.width) - 1.0;
        const double sy = 1.0 - (2.0 * (double(y) + 0.5)) / double(cam.height);
        bt_ray ray;
        for (int k = 0; k < 3; k++) {
            if (cam.flags & BT_RENDER_ORTHOGRAPHIC) {
                ray.origin[k] = (cam.origin[k] + sx * cam.right[k]) + sy * cam.up[k];
                ray.direction[k] = cam.forward[k];
            } else {
                ray.origin[k] = cam.origin[k];
                ray.direction[k] = (cam.forward[k] + sx * cam.right[k]) + sy * cam.up[k];
            }
        }
        ray.t_min = cam.t_min;
        ray.t_max = cam.t_max;

        double t = 0.0;
        float value = 0.0f;
        if (ray_valid(ray)) {
            // MARCH, the lane's own: coarse steps 0 .. steps until the first at or under the ground
            const double dt = (ray.t_max - ray.t_min) / double(a.steps);
            const LaneMarch march = lane_march(G, ray, dt, a.steps);
            status = march.status;
            value = march.e.value;
            if (status == BT_RAY_INSIDE) t = ray.t_min;
            if (status == BT_RAY_HIT) {
                double lo = ray.t_min + double(march.step - 1u) * dt, hi = ray.t_min + double(march.step) * dt;
                for (uint32_t round = 0; round < a.refine_rounds; round++) {
                    const double width = hi - lo;
                    uint32_t k = 1;
                    for (; k < 64u; k++) {
                        const RayEval e = ray_eval(G, ray_point(ray, lo + width * (double(k) / 64.0)));
                        if (e.below) {
                            value = e.value;
                            break;
                        }
                    }
                    const Bracket b = refine_bracket(lo, hi, k);
                    hi = b.hi;
                    lo = b.lo;
                }
                t = hi;
            }
        }

        // the fragment stage at p(t), and the planes the caller asked for
        const bool hit = status == BT_RAY_HIT || status == BT_RAY_INSIDE;
        const bool lighting = (cam.flags & BT_RENDER_LIGHTING) != 0u;
        const uint64_t pixel = uint64_t(y) * cam.width + x;
        const V3 p = ray_point(ray, t);
        F3 n = {0.0f, 0.0f, 0.0f};
        if (hit && (a.normal || (a.rgba && lighting))) {
            float cosine;
            n = world_normal(G, nm, p, cosine);
        }
        // SHADOW PLANE
        bool occluded = false;
        if constexpr (kShadow) {
            uint32_t shadow = BT_SHADOW_NONE;
            if (hit && (a.shadow_plane || (a.rgba && lighting && dot3f(n, {cam.sun[0], cam.sun[1], cam.sun[2]}) > 0.0f))) {
                shadow = occlusion_status(G, p, {double(cam.sun[0]), double(cam.sun[1]), double(cam.sun[2])}, a.shadow.lift, a.shadow.distance, a.shadow.steps);
                occluded = shadow == BT_RAY_HIT || shadow == BT_RAY_INSIDE;
            }
            if (a.shadow_plane) a.shadow_plane[pixel] = uint8_t(shadow);
        }
        if (a.t) a.t[pixel] = t;
        if (a.status) a.status[pixel] = uint8_t(status);
        if (a.normal) {
            a.normal[3u * pixel] = n.x;
            a.normal[3u * pixel + 1u] = n.y;
            a.normal[3u * pixel + 2u] = n.z;
        }
        if (a.rgba) {
            uint32_t texel = uint32_t(cam.background[0]) | (uint32_t(cam.background[1]) << 8) | (uint32_t(cam.background[2]) << 16) | (uint32_t(cam.background[3]) << 24);
            if (hit) {
                float base[4];
                if (albedo) {
                    sample_surface(P, entries, albedo_meta, albedo, surface_position(P.model, p, G.approximate_height), base);
                } else {
                    const float g = 0.5f * value;  // sample_color (attachments.wgsl:109-113)
                    base[0] = base[1] = base[2] = g;
                    base[3] = 1.0f;
                }
                if (lighting) {  // a plain Lambert term
                    const float d = dot3f(n, {cam.sun[0], cam.sun[1], cam.sun[2]});
                    const float l = d > 0.0f ? d : 0.0f;
                    float k;
                    if constexpr (kShadow) {
                        const float sh = occluded ? 0.0f : 1.0f;
                        k = cam.ambient + (1.0f - cam.ambient) * (l * sh);
                    } else {
                        k = cam.ambient + (1.0f - cam.ambient) * l;
                    }
                    for (int c = 0; c < 3; c++) base[c] = base[c] * k;
                }
                texel = enc8(base[0]) | (enc8(base[1]) << 8) | (enc8(base[2]) << 16) | (enc8(base[3]) << 24);
            }
            a.rgba[pixel] = texel;
        }
    }

    // the pixel counters: the whole wave is here, whatever its lanes did above
    wave_count(a.counters, lane, active && status == BT_RAY_HIT, active && status == BT_RAY_INSIDE, active && status == BT_RAY_MISS);
}

}  // namespace

bt_status launch_render(hipStream_t stream, const TerrainRef& g, const AttachmentMeta& albedo_meta, const void* albedo, const RenderArgs& a, bool shadowed) {
    if (!a.block_count) return BT_OK;
    const NormalModel nm = {g.P.model.min_height, g.P.model.max_height, normal_side_length(g.P.model)};
    const uint32_t groups = (a.block_count + kRenderBlocksPerGroup - 1u) / kRenderBlocksPerGroup;
    if (shadowed)
        render_kernel<true><<<groups, kRenderThreads, 0, stream>>>(g.P, g.entries, g.m, g.atlas, albedo_meta, albedo, nm, a, g.height);
    else
        render_kernel<false><<<groups, kRenderThreads, 0, stream>>>(g.P, g.entries, g.m, g.atlas, albedo_meta, albedo, nm, a, g.height);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? BT_OK : hip_fail(e, "render_kernel");
}

}  // namespace bt

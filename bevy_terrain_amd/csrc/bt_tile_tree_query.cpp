// The queries that read the terrain through a tile tree: bt_tile_tree_raycast, bt_tile_tree_collide_spheres, bt_tile_tree_sweep_spheres,
// bt_tile_tree_sun_occlusion, bt_tile_tree_render(_shadowed), bt_tile_tree_sample_normal and the geometry calls.  Each validates, stages its
// inputs in scratch of the context (bt::Scratch: grown on demand, kept until bt_ctx_trim), calls the launcher of its kernel file
// (bt_raycast.hip, bt_collide.hip, bt_shadow.hip, bt_render.hip, bt_normal.hip, bt_geometry.hip) and copies the results back.  The two
// shapes that sequence takes are here once: staged_batch (one array in, one launch, one array out: ray casting, contacts, sweeps) and
// counted_run (counters and planes in scratch, the launches in pieces: rendering, sun occlusion).
#include <cmath>
#include <initializer_list>

#include "bt_tile_tree_host.hpp"

using namespace bt;

namespace bt {

bt_status query_handles(const char* who, const bt_tile_tree* t, const bt_atlas* a) {
    if (!t || !a) {
        set_error("%s: NULL %s", who, t ? "atlas" : "tile tree");
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (t->ctx != a->ctx) {
        set_error("%s: tile tree and atlas belong to different contexts", who);
        return BT_ERR_INVALID_ARGUMENT;
    }
    return BT_OK;
}

bt_status height_attachment(const char* who, const bt_atlas* a, uint32_t ai, const Attachment** height) {
    if (ai >= a->attachments.size()) {
        set_error("%s: attachment index %u out of range", who, ai);
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (a->attachments[ai].meta.format != BT_FORMAT_R16) {
        set_error("%s: attachment %u is not R16", who, ai);
        return BT_ERR_UNSUPPORTED;
    }
    *height = &a->attachments[ai];
    return BT_OK;
}

bt_status query_check(const char* who, const bt_tile_tree* t, const bt_atlas* a, uint32_t ai, const Attachment** height) {
    if (bt_status s = query_handles(who, t, a)) return s;
    return height_attachment(who, a, ai, height);
}

}  // namespace bt

namespace {
// what bt_tile_tree_raycast, bt_tile_tree_collide_spheres and bt_tile_tree_sweep_spheres share once their limits hold: the batch goes to
// the ray queries' scratch, `launch` runs on it (in, out on the device), the results come back.  in_name / out_name: what the call's
// message calls a NULL array
template <class In, class Out, class Launch>
bt_status staged_batch(const char* who, bt_tile_tree* t, const char* in_name, const In* in, uint32_t count, const char* out_name, Out* out, Launch launch) {
    if (!count) return BT_OK;
    if (!in || !out) {
        set_error("%s: NULL %s", who, in ? out_name : in_name);
        return BT_ERR_INVALID_ARGUMENT;
    }
    bt_ctx* ctx = t->ctx;
    BT_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const uint64_t in_bytes = sizeof(In) * uint64_t(count), out_bytes = sizeof(Out) * uint64_t(count);
    if (bt_status st = ctx->raycast.reserve(ctx, in_bytes + out_bytes)) return st;
    uint8_t* dev = (uint8_t*)ctx->raycast.dev;
    BT_HIP(hipMemcpyAsync(dev, in, in_bytes, hipMemcpyHostToDevice, s));
    if (bt_status st = launch(s, (const In*)dev, (Out*)(dev + in_bytes))) return st;
    BT_HIP(hipMemcpyAsync(out, dev + in_bytes, out_bytes, hipMemcpyDeviceToHost, s));
    BT_HIP(hipStreamSynchronize(s));
    synchronised(t);
    return BT_OK;
}

// a plane of results in scratch and where the caller wants it (host NULL: not wanted)
struct Plane {
    void* host;
    const void* dev;
    uint64_t bytes;
};

// What render() and bt_tile_tree_sun_occlusion share once their scratch is laid out: three counters in the first 16 bytes of the scratch
// `dev` (the planes start at byte 256), cleared here; `total` units of work issued as launch(first, n) in pieces of per_launch; then the
// counters and the planes come back, the stream is synchronised once, and *stats = {launches, the three counters}.
template <class Stats, class Launch>
bt_status counted_run(const char* who, bt_tile_tree* t, uint8_t* dev, uint64_t total, uint32_t per_launch, std::initializer_list<Plane> planes, Stats* stats,
                      Launch launch) {
    hipStream_t s = t->ctx->stream;
    BT_HIP(hipMemsetAsync(dev, 0, 16, s));
    uint32_t launches = 0;
    for (uint64_t first = 0; first < total; first += per_launch, launches++) {
        if (bt_status st = launch(uint32_t(first), uint32_t(std::min<uint64_t>(per_launch, total - first)))) {
            (void)hipStreamSynchronize(s);
            return st;
        }
    }
    // nothing is copied back before the last launch has been queued
    uint32_t counters[4] = {};
    hipError_t e = hipMemcpyAsync(counters, dev, 16, hipMemcpyDeviceToHost, s);
    for (const Plane& p : planes)
        if (e == hipSuccess && p.host) e = hipMemcpyAsync(p.host, p.dev, p.bytes, hipMemcpyDeviceToHost, s);
    const hipError_t w = hipStreamSynchronize(s);  // (also when a copy was refused: `counters` must not be written after the return)
    if (e != hipSuccess || w != hipSuccess) return hip_fail(e != hipSuccess ? e : w, who);
    synchronised(t);
    if (stats) *stats = {launches, counters[0], counters[1], counters[2]};
    return BT_OK;
}
}  // namespace

extern "C" {

bt_status bt_tile_tree_raycast(bt_tile_tree* t, bt_atlas* a, uint32_t ai, const bt_ray* rays, uint32_t count, uint32_t steps, uint32_t refine_rounds,
                               bt_ray_hit* hits) {
    const Attachment* height;
    if (bt_status s = query_check("bt_tile_tree_raycast", t, a, ai, &height)) return s;
    const Attachment& at = *height;
    if (steps < 1u || steps > uint32_t(BT_RAYCAST_MAX_STEPS) || refine_rounds > uint32_t(BT_RAYCAST_MAX_REFINE_ROUNDS)) {
        set_error("bt_tile_tree_raycast: steps %u (1 .. %u) / refine_rounds %u (at most %u)", steps, unsigned(BT_RAYCAST_MAX_STEPS), refine_rounds,
                  unsigned(BT_RAYCAST_MAX_REFINE_ROUNDS));
        return BT_ERR_INVALID_ARGUMENT;
    }
    // a ray costs whole rounds of 64 samples (one wave per ray): that is what the cap counts
    const uint64_t rounds = (uint64_t(steps) + 1u + 63u) / 64u;
    if (uint64_t(count) * rounds * 64u > uint64_t(BT_RAYCAST_MAX_SAMPLES)) {
        set_error("bt_tile_tree_raycast: %u rays x %u rounds of 64 samples exceed BT_RAYCAST_MAX_SAMPLES (%u): split the batch", count, unsigned(rounds),
                  unsigned(BT_RAYCAST_MAX_SAMPLES));
        return BT_ERR_INVALID_ARGUMENT;
    }
    return staged_batch("bt_tile_tree_raycast", t, "rays", rays, count, "hits_out", hits, [&](hipStream_t s, const bt_ray* in, bt_ray_hit* out) {
        return launch_raycast(s, make_ground(t, at), in, count, steps, refine_rounds, out);
    });
}

bt_status bt_tile_tree_collide_spheres(bt_tile_tree* t, bt_atlas* a, uint32_t ai, const bt_sphere* spheres, uint32_t count, uint32_t refine_rounds,
                                       bt_sphere_contact* contacts) {
    static_assert(sizeof(bt_sphere) == 32 && sizeof(bt_sphere_contact) == 80, "the layouts the header states");
    const char* who = "bt_tile_tree_collide_spheres";
    const Attachment* height;
    if (bt_status s = query_check(who, t, a, ai, &height)) return s;
    const Attachment& at = *height;
    if (refine_rounds > uint32_t(BT_COLLIDE_MAX_REFINE_ROUNDS)) {
        set_error("%s: refine_rounds %u (at most %u)", who, refine_rounds, unsigned(BT_COLLIDE_MAX_REFINE_ROUNDS));
        return BT_ERR_INVALID_ARGUMENT;
    }
    // a sphere costs R + 1 rounds of 64 samples (one wave per sphere)
    if (uint64_t(count) * 64u * (uint64_t(refine_rounds) + 1u) > uint64_t(BT_COLLIDE_MAX_SAMPLES)) {
        set_error("%s: %u spheres x %u rounds of 64 samples exceed BT_COLLIDE_MAX_SAMPLES (%u): split the batch", who, count, refine_rounds + 1u,
                  unsigned(BT_COLLIDE_MAX_SAMPLES));
        return BT_ERR_INVALID_ARGUMENT;
    }
    return staged_batch(who, t, "input array", spheres, count, "output array", contacts, [&](hipStream_t s, const bt_sphere* in, bt_sphere_contact* out) {
        return launch_collide(s, make_ground(t, at), in, count, refine_rounds, out);
    });
}

bt_status bt_tile_tree_sweep_spheres(bt_tile_tree* t, bt_atlas* a, uint32_t ai, const bt_sphere_sweep* sweeps, uint32_t count, uint32_t steps, uint32_t bisections,
                                     uint32_t refine_rounds, bt_sweep_hit* hits) {
    static_assert(sizeof(bt_sphere_sweep) == 72 && sizeof(bt_sweep_hit) == 104, "the layouts the header states");
    const char* who = "bt_tile_tree_sweep_spheres";
    const Attachment* height;
    if (bt_status s = query_check(who, t, a, ai, &height)) return s;
    const Attachment& at = *height;
    if (steps < 1u || steps > uint32_t(BT_SWEEP_MAX_STEPS) || bisections > uint32_t(BT_SWEEP_MAX_BISECTIONS) || refine_rounds > uint32_t(BT_COLLIDE_MAX_REFINE_ROUNDS)) {
        set_error("%s: steps %u (1 .. %u) / bisections %u (at most %u) / refine_rounds %u (at most %u)", who, steps, unsigned(BT_SWEEP_MAX_STEPS), bisections,
                  unsigned(BT_SWEEP_MAX_BISECTIONS), refine_rounds, unsigned(BT_COLLIDE_MAX_REFINE_ROUNDS));
        return BT_ERR_INVALID_ARGUMENT;
    }
    // a sweep costs at most steps + 1 + bisections + 1 contacts of R + 1 rounds of 64 samples each
    const uint64_t contacts = uint64_t(steps) + bisections + 2u;
    if (uint64_t(count) * 64u * (uint64_t(refine_rounds) + 1u) * contacts > uint64_t(BT_COLLIDE_MAX_SAMPLES)) {
        set_error("%s: %u sweeps x %u contacts x %u rounds of 64 samples exceed BT_COLLIDE_MAX_SAMPLES (%u): split the batch", who, count, unsigned(contacts),
                  refine_rounds + 1u, unsigned(BT_COLLIDE_MAX_SAMPLES));
        return BT_ERR_INVALID_ARGUMENT;
    }
    return staged_batch(who, t, "input array", sweeps, count, "output array", hits, [&](hipStream_t s, const bt_sphere_sweep* in, bt_sweep_hit* out) {
        return launch_sweep(s, make_ground(t, at), in, count, steps, bisections, refine_rounds, out);
    });
}

namespace {
// bt_tile_tree_render (shadowed false: shadow and out_shadow NULL) and bt_tile_tree_render_shadowed
bt_status render(const char* who, bool shadowed, bt_tile_tree* t, bt_atlas* a, uint32_t ai, const bt_render_camera* camera, uint32_t steps, uint32_t refine_rounds,
                 const bt_sun_shadow* shadow, double* out_t, uint8_t* out_status, float* out_normal, uint8_t* out_rgba, uint8_t* out_shadow, bt_render_stats* stats) {
    if (t && a && (!camera || (shadowed && !shadow))) {  // (refused before two contexts are)
        set_error("%s: NULL %s", who, camera ? "shadow" : "camera");
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (bt_status st = query_handles(who, t, a)) return st;
    if (!out_t && !out_status && !out_normal && !out_rgba && !out_shadow) {
        set_error("%s: every plane is NULL", who);
        return BT_ERR_INVALID_ARGUMENT;
    }
    const bt_render_camera& cam = *camera;
    const uint64_t pixels = uint64_t(cam.width) * cam.height;
    if (!cam.width || !cam.height || pixels > uint64_t(BT_RENDER_MAX_PIXELS)) {
        set_error("%s: %u x %u pixels (each at least 1, at most %u in all)", who, cam.width, cam.height, unsigned(BT_RENDER_MAX_PIXELS));
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (steps < 1u || steps > uint32_t(BT_RENDER_MAX_STEPS) || refine_rounds > uint32_t(BT_RAYCAST_MAX_REFINE_ROUNDS)) {
        set_error("%s: steps %u (1 .. %u) / refine_rounds %u (at most %u)", who, steps, unsigned(BT_RENDER_MAX_STEPS), refine_rounds, unsigned(BT_RAYCAST_MAX_REFINE_ROUNDS));
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (shadowed && (shadow->steps < 1u || shadow->steps > uint32_t(BT_RENDER_MAX_STEPS) || !std::isfinite(shadow->lift))) {
        // (a non-finite or negative distance is no error: those shadow rays are BT_RAY_INVALID)
        set_error("%s: shadow steps %u (1 .. %u) / lift %g (finite)", who, shadow->steps, unsigned(BT_RENDER_MAX_STEPS), shadow->lift);
        return BT_ERR_INVALID_ARGUMENT;
    }
    const bool has_albedo = cam.albedo_attachment != BT_RENDER_NO_ALBEDO;
    if (has_albedo && cam.albedo_attachment >= a->attachments.size()) {
        set_error("%s: albedo attachment index %u out of range", who, cam.albedo_attachment);
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (cam.flags & ~uint32_t(BT_RENDER_ORTHOGRAPHIC | BT_RENDER_LIGHTING)) {
        set_error("%s: unknown flag bits 0x%x", who, cam.flags);
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (!std::isfinite(cam.ambient) || !std::isfinite(cam.sun[0]) || !std::isfinite(cam.sun[1]) || !std::isfinite(cam.sun[2])) {
        set_error("%s: non-finite ambient / sun", who);
        return BT_ERR_INVALID_ARGUMENT;
    }
    // (the height's index is refused here, behind the other invalid arguments and before either format)
    const Attachment* height;
    if (bt_status st = height_attachment(who, a, ai, &height)) return st;
    const Attachment& at = *height;
    const Attachment& albedo = a->attachments[has_albedo ? cam.albedo_attachment : ai];
    if (has_albedo && albedo.meta.format != BT_FORMAT_RGBA8) {
        set_error("%s: albedo attachment %u is not Rgba8", who, cam.albedo_attachment);
        return BT_ERR_UNSUPPORTED;
    }
    bt_ctx* ctx = t->ctx;
    BT_HIP(hipSetDevice(ctx->device));
    // the scratch: the counters, then the planes that were asked for, each from a 256-byte boundary (the shadow plane last)
    const uint64_t t_off = 256u, n_off = t_off + (out_t ? align256(8u * pixels) : 0u), c_off = n_off + (out_normal ? align256(12u * pixels) : 0u),
                   s_off = c_off + (out_rgba ? align256(4u * pixels) : 0u), o_off = s_off + (out_status ? align256(pixels) : 0u),
                   need = o_off + (out_shadow ? align256(pixels) : 0u);
    if (bt_status st = ctx->render.reserve(ctx, need)) return st;
    uint8_t* dev = (uint8_t*)ctx->render.dev;
    RenderArgs args{};
    args.camera = cam;
    args.steps = steps;
    args.refine_rounds = refine_rounds;
    args.blocks_x = (cam.width + 7u) / 8u;
    args.counters = (uint32_t*)dev;
    args.t = out_t ? (double*)(dev + t_off) : nullptr;
    args.normal = out_normal ? (float*)(dev + n_off) : nullptr;
    args.rgba = out_rgba ? (uint32_t*)(dev + c_off) : nullptr;
    args.status = out_status ? dev + s_off : nullptr;
    args.shadow_plane = out_shadow ? dev + o_off : nullptr;
    if (shadowed) args.shadow = *shadow;
    // a launch: whole 8 x 8 blocks whose worst case (with the shadow ray's steps + 1 samples in the shadowed form) stays within
    // BT_RAYCAST_MAX_SAMPLES (at least one fits: 64 * (4349 + 4097) samples at most), cut to whole 8-row bands when it holds one
    const uint32_t blocks = args.blocks_x * ((cam.height + 7u) / 8u);
    const uint64_t block_samples = 64ull * (uint64_t(steps) + 1u + 63ull * refine_rounds + (shadowed ? uint64_t(shadow->steps) + 1u : 0u));
    uint32_t per_launch = uint32_t(std::min<uint64_t>(blocks, uint64_t(BT_RAYCAST_MAX_SAMPLES) / block_samples));
    if (per_launch >= args.blocks_x) per_launch -= per_launch % args.blocks_x;
    const TerrainRef ground = make_ground(t, at);
    return counted_run(who, t, dev, blocks, per_launch,
                       {{out_t, args.t, 8u * pixels}, {out_status, args.status, pixels}, {out_normal, args.normal, 12u * pixels}, {out_rgba, args.rgba, 4u * pixels},
                        {out_shadow, args.shadow_plane, pixels}},
                       stats, [&](uint32_t first, uint32_t n) {
                           args.first_block = first;
                           args.block_count = n;
                           return launch_render(ctx->stream, ground, albedo.meta, has_albedo ? albedo.level0 : nullptr, args, shadowed);
                       });
}
}  // namespace

bt_status bt_tile_tree_sun_occlusion(bt_tile_tree* t, bt_atlas* a, uint32_t ai, const double* positions, uint32_t count, const double* directions,
                                     uint32_t direction_count, double lift, double distance, uint32_t steps, uint8_t* out_status, bt_occlusion_stats* stats) {
    const char* who = "bt_tile_tree_sun_occlusion";
    const Attachment* height;
    if (bt_status s = query_check(who, t, a, ai, &height)) return s;
    const Attachment& at = *height;
    if (steps < 1u || steps > uint32_t(BT_RENDER_MAX_STEPS) || !std::isfinite(lift)) {
        // (a non-finite or negative distance is no error: those rays are BT_RAY_INVALID)
        set_error("%s: steps %u (1 .. %u) / lift %g (finite)", who, steps, unsigned(BT_RENDER_MAX_STEPS), lift);
        return BT_ERR_INVALID_ARGUMENT;
    }
    const uint64_t rays = uint64_t(count) * direction_count;
    if (rays > uint64_t(BT_OCCLUSION_MAX_RAYS)) {
        set_error("%s: %u points x %u directions exceed BT_OCCLUSION_MAX_RAYS (%u): split the batch", who, count, direction_count, unsigned(BT_OCCLUSION_MAX_RAYS));
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (!rays) {
        if (stats) *stats = {};
        return BT_OK;
    }
    if (!positions || !directions || !out_status) {
        set_error("%s: NULL %s", who, !positions ? "world_positions_xyz" : (directions ? "out_status" : "directions_xyz"));
        return BT_ERR_INVALID_ARGUMENT;
    }
    bt_ctx* ctx = t->ctx;
    BT_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    // the scratch (the ray queries': bt_ctx::raycast): the counters, the points, the directions, the statuses, each from a 256-byte boundary
    const uint64_t p_bytes = 24ull * count, d_bytes = 24ull * direction_count, p_off = 256u, d_off = p_off + align256(p_bytes), s_off = d_off + align256(d_bytes);
    if (bt_status st = ctx->raycast.reserve(ctx, s_off + align256(rays))) return st;
    uint8_t* dev = (uint8_t*)ctx->raycast.dev;
    BT_HIP(hipMemcpyAsync(dev + p_off, positions, p_bytes, hipMemcpyHostToDevice, s));
    BT_HIP(hipMemcpyAsync(dev + d_off, directions, d_bytes, hipMemcpyHostToDevice, s));
    OcclusionArgs args{};
    args.positions = (const double*)(dev + p_off);
    args.directions = (const double*)(dev + d_off);
    args.count = count;
    args.direction_count = direction_count;
    args.lift = lift;
    args.distance = distance;
    args.steps = steps;
    args.status = dev + s_off;
    args.counters = (uint32_t*)dev;
    // a launch: whole waves whose worst case, 64 * (steps + 1) samples each, stays within BT_RAYCAST_MAX_SAMPLES (63 waves at 4096 steps)
    const uint32_t per_launch = 64u * uint32_t(uint64_t(BT_RAYCAST_MAX_SAMPLES) / (64ull * (uint64_t(steps) + 1u)));
    const TerrainRef ground = make_ground(t, at);
    return counted_run(who, t, dev, rays, per_launch, {{out_status, args.status, rays}}, stats, [&](uint32_t first, uint32_t n) {
        args.first_ray = first;
        args.ray_count = n;
        return launch_occlusion(s, ground, args);
    });
}

bt_status bt_tile_tree_render(bt_tile_tree* t, bt_atlas* a, uint32_t ai, const bt_render_camera* camera, uint32_t steps, uint32_t refine_rounds, double* out_t,
                              uint8_t* out_status, float* out_normal, uint8_t* out_rgba, bt_render_stats* stats) {
    return render("bt_tile_tree_render", false, t, a, ai, camera, steps, refine_rounds, nullptr, out_t, out_status, out_normal, out_rgba, nullptr, stats);
}

bt_status bt_tile_tree_render_shadowed(bt_tile_tree* t, bt_atlas* a, uint32_t ai, const bt_render_camera* camera, uint32_t steps, uint32_t refine_rounds,
                                       const bt_sun_shadow* shadow, double* out_t, uint8_t* out_status, float* out_normal, uint8_t* out_rgba, uint8_t* out_shadow,
                                       bt_render_stats* stats) {
    return render("bt_tile_tree_render_shadowed", true, t, a, ai, camera, steps, refine_rounds, shadow, out_t, out_status, out_normal, out_rgba, out_shadow, stats);
}

bt_status bt_tile_tree_sample_normal(bt_tile_tree* t, bt_atlas* a, uint32_t ai, const double* positions, uint32_t count, float* normals, float* up_dot) {
    const Attachment* height;
    if (bt_status s = query_check("bt_tile_tree_sample_normal", t, a, ai, &height)) return s;
    const Attachment& at = *height;
    if (!count) return BT_OK;
    if (!positions || !normals) {
        set_error("bt_tile_tree_sample_normal: NULL %s", positions ? "out_normals_xyz" : "world_positions_xyz");
        return BT_ERR_INVALID_ARGUMENT;
    }
    bt_ctx* ctx = t->ctx;
    BT_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const uint64_t in_bytes = sizeof(double) * 3 * uint64_t(count), n_bytes = 12 * uint64_t(count), d_bytes = 4 * uint64_t(count);
    if (bt_status st = ctx->normal.reserve(ctx, in_bytes + n_bytes + d_bytes)) return st;
    uint8_t* dev = (uint8_t*)ctx->normal.dev;
    BT_HIP(hipMemcpyAsync(dev, positions, in_bytes, hipMemcpyHostToDevice, s));
    if (bt_status st = launch_sample_normal(s, make_ground(t, at), (const double*)dev, count, (float*)(dev + in_bytes),
                                            up_dot ? (float*)(dev + in_bytes + n_bytes) : nullptr))
        return st;
    BT_HIP(hipMemcpyAsync(normals, dev + in_bytes, n_bytes, hipMemcpyDeviceToHost, s));
    if (up_dot) BT_HIP(hipMemcpyAsync(up_dot, dev + in_bytes + n_bytes, d_bytes, hipMemcpyDeviceToHost, s));
    BT_HIP(hipStreamSynchronize(s));
    synchronised(t);
    return BT_OK;
}

namespace {
// what both geometry calls refuse before any device work, and what they hand the kernel: the tree's parameters (TerrainViewConfigUniform:
// the f64 distances x TerrainModel::scale(), `as f32`) and the view (the caller's, or the tree's own)
// hp: the HIGH PRECISION calls, which also accept BT_GEOMETRY_VIEW_RELATIVE and check the approximation they were given
bt_status geometry_check(const char* who, bt_tile_tree* t, bt_atlas* a, uint32_t ai, const bt_view_state* view, uint32_t flags, GeometryParams* G, bt_view_state* v,
                         bool hp = false, const bt_model_approximation* approximation = nullptr) {
    if (bt_status s = query_handles(who, t, a)) return s;
    // (unknown flags are refused before the attachment's format)
    if (flags & ~uint32_t(BT_GEOMETRY_GRID | BT_GEOMETRY_NO_MORPH | BT_GEOMETRY_NO_BLEND | (hp ? BT_GEOMETRY_VIEW_RELATIVE : 0))) {
        set_error("%s: unknown flags 0x%x", who, flags);
        return BT_ERR_INVALID_ARGUMENT;
    }
    const Attachment* height;  // (the callers take it from the atlas again once they launch)
    if (bt_status s = height_attachment(who, a, ai, &height)) return s;
    const bt_terrain_view_config& vc = t->view_config;
    if (vc.grid_size == 0u || vc.grid_size > uint32_t(BT_GEOMETRY_MAX_GRID)) {
        set_error("%s: grid_size %u (1 .. %u)", who, vc.grid_size, unsigned(BT_GEOMETRY_MAX_GRID));
        return BT_ERR_UNSUPPORTED;
    }
    if (!(flags & BT_GEOMETRY_NO_MORPH) && !(std::isfinite(vc.morph_range) && vc.morph_range > 0.0f)) {
        set_error("%s: morph_range %g (finite, > 0, or BT_GEOMETRY_NO_MORPH)", who, double(vc.morph_range));
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (!(flags & BT_GEOMETRY_NO_BLEND) && !(std::isfinite(vc.blend_range) && vc.blend_range > 0.0f)) {
        set_error("%s: blend_range %g (finite, > 0, or BT_GEOMETRY_NO_BLEND)", who, double(vc.blend_range));
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (view) {
        *v = *view;
    } else if (bt_status s = bt_tile_tree_view_state(t, v)) {
        return s;
    }
    if ((v->spherical ? 6u : 1u) != t->sides) {
        set_error("%s: a view of %u side(s) for a tile tree of %u", who, v->spherical ? 6u : 1u, t->sides);
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (hp) {
        if (!approximation) {
            set_error("%s: NULL approximation", who);
            return BT_ERR_INVALID_ARGUMENT;
        }
        if (t->sides != 6u) {
            set_error("%s: a planar terrain has no model approximation", who);
            return BT_ERR_UNSUPPORTED;
        }
        const float th = approximation->precision_threshold_distance;
        if (approximation->origin_lod != v->origin_lod || approximation->origin_lod > 31u || !std::isfinite(th) || th < 0.0f) {
            set_error("%s: approximation of origin_lod %u for a view of %u (equal, <= 31), or precision_threshold_distance %g (finite, >= 0)", who,
                      approximation->origin_lod, v->origin_lod, double(th));
            return BT_ERR_INVALID_ARGUMENT;
        }
    }
    G->grid_size = vc.grid_size;
    G->tree_size = vc.tree_size;
    G->lod_count = t->lod_count;
    G->sides = t->sides;
    G->flags = flags;
    G->morph_distance = float(t->morph_distance);
    G->blend_distance = float(t->blend_distance);
    G->morph_range = vc.morph_range;
    G->blend_range = vc.blend_range;
    G->min_height = t->model_c.min_height;
    G->max_height = t->model_c.max_height;
    return BT_OK;
}

uint64_t geometry_slots(const GeometryParams& G) {
    const uint64_t g = G.grid_size;
    return (G.flags & BT_GEOMETRY_GRID) ? (g + 1u) * (g + 1u) : 2u * g * (g + 2u);
}
}  // namespace

namespace {
// both forms, plain (hp false, approximation NULL) and HIGH PRECISION
bt_status build_geometry(const char* who, bool hp, bt_tile_tree* t, bt_atlas* a, uint32_t ai, const bt_view_state* view, const bt_model_approximation* approximation,
                         const bt_tiling_prepass* prepass, uint32_t flags, void* vertices_device, uint64_t vertex_capacity) {
    GeometryParams G{};
    bt_view_state v{};
    if (bt_status s = geometry_check(who, t, a, ai, view, flags, &G, &v, hp, approximation)) return s;
    if (!prepass || bt::tiling_prepass_ctx(prepass) != t->ctx) {
        // the kernel reads the list the prepass kernels leave: ordered only on one stream
        set_error("%s: %s", who, prepass ? "tile tree and tiling prepass belong to different contexts" : "NULL prepass");
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (!vertex_capacity) return BT_OK;
    if (!vertices_device || (uintptr_t(vertices_device) & 15u)) {
        set_error("%s: vertices_device is %s", who, vertices_device ? "not 16-byte aligned" : "NULL");
        return BT_ERR_INVALID_ARGUMENT;
    }
    const bt_tile_coordinate* tiles;
    const uint32_t* count;
    uint32_t capacity;
    bt::tiling_prepass_final(prepass, &tiles, &count, &capacity);
    BT_HIP(hipSetDevice(t->ctx->device));
    // a read of the atlas: level0 is passed on without marking any layer written
    const Attachment& at = a->attachments[ai];
    return launch_geometry(t->ctx->stream, v, G, t->d_entries, at.meta, at.level0, tiles, count, capacity, 0u, vertices_device, vertex_capacity, approximation);
}

bt_status tile_geometry(const char* who, bool hp, bt_tile_tree* t, bt_atlas* a, uint32_t ai, const bt_view_state* view, const bt_model_approximation* approximation,
                        const bt_tile_coordinate* tiles, uint32_t count, uint32_t flags, bt_terrain_vertex* out, uint64_t out_bytes) {
    static_assert(sizeof(bt_terrain_vertex) == 48, "three 16-byte stores per vertex");
    static_assert(sizeof(bt_model_approximation) == 448, "a by-value kernel argument, a multiple of 16 bytes");
    GeometryParams G{};
    bt_view_state v{};
    if (bt_status s = geometry_check(who, t, a, ai, view, flags, &G, &v, hp, approximation)) return s;
    if (!count) return BT_OK;
    if (!tiles || !out) {
        set_error("%s: NULL %s", who, tiles ? "out_host" : "tiles");
        return BT_ERR_INVALID_ARGUMENT;
    }
    const uint64_t slots = geometry_slots(G), tile_bytes = slots * sizeof(bt_terrain_vertex);
    if (out_bytes < uint64_t(count) * tile_bytes) {
        set_error("%s: out_bytes %llu < %u tiles x %llu vertices x 48", who, (unsigned long long)out_bytes, count, (unsigned long long)slots);
        return BT_ERR_INVALID_ARGUMENT;
    }
    for (uint32_t i = 0; i < count; i++) {
        const bt_tile_coordinate& c = tiles[i];
        if (c.side >= t->sides || c.lod >= t->lod_count || c.x >= (1u << c.lod) || c.y >= (1u << c.lod)) {
            set_error("%s: tile %u (%u, %u, %u, %u) is not a tile of this terrain", who, i, c.side, c.lod, c.x, c.y);
            return BT_ERR_INVALID_ARGUMENT;
        }
    }
    bt_ctx* ctx = t->ctx;
    BT_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    // one launch per 32 MiB of vertices (at least one tile); the scratch is the normals' (bt_ctx::normal), until bt_ctx_trim
    const uint32_t chunk = uint32_t(std::min<uint64_t>(count, std::max<uint64_t>(1u, (32ull << 20) / tile_bytes)));
    const uint64_t in_bytes = (sizeof(bt_tile_coordinate) * uint64_t(chunk) + 15u) & ~15ull, need = in_bytes + uint64_t(chunk) * tile_bytes;
    if (bt_status st = ctx->normal.reserve(ctx, need)) return st;
    uint8_t* dev = (uint8_t*)ctx->normal.dev;
    const Attachment& at = a->attachments[ai];
    for (uint32_t first = 0; first < count; first += chunk) {
        const uint32_t n = std::min(chunk, count - first);
        BT_HIP(hipMemcpyAsync(dev, tiles + first, sizeof(bt_tile_coordinate) * size_t(n), hipMemcpyHostToDevice, s));
        // a read of the atlas: level0 is passed on without marking any layer written
        if (bt_status st = launch_geometry(s, v, G, t->d_entries, at.meta, at.level0, (const bt_tile_coordinate*)dev, nullptr, n, first, dev + in_bytes, uint64_t(n) * slots,
                                           approximation))
            return st;
        BT_HIP(hipMemcpyAsync((uint8_t*)out + uint64_t(first) * tile_bytes, dev + in_bytes, uint64_t(n) * tile_bytes, hipMemcpyDeviceToHost, s));
        BT_HIP(hipStreamSynchronize(s));  // (the next chunk reuses the scratch, and `tiles` / `out` are pageable)
    }
    synchronised(t);
    return BT_OK;
}
}  // namespace

bt_status bt_tile_tree_build_geometry(bt_tile_tree* t, bt_atlas* a, uint32_t ai, const bt_view_state* view, const bt_tiling_prepass* prepass, uint32_t flags,
                                      void* vertices_device, uint64_t vertex_capacity) {
    return build_geometry("bt_tile_tree_build_geometry", false, t, a, ai, view, nullptr, prepass, flags, vertices_device, vertex_capacity);
}

bt_status bt_tile_tree_tile_geometry(bt_tile_tree* t, bt_atlas* a, uint32_t ai, const bt_view_state* view, const bt_tile_coordinate* tiles, uint32_t count,
                                     uint32_t flags, bt_terrain_vertex* out, uint64_t out_bytes) {
    return tile_geometry("bt_tile_tree_tile_geometry", false, t, a, ai, view, nullptr, tiles, count, flags, out, out_bytes);
}

bt_status bt_tile_tree_build_geometry_hp(bt_tile_tree* t, bt_atlas* a, uint32_t ai, const bt_view_state* view, const bt_model_approximation* approximation,
                                         const bt_tiling_prepass* prepass, uint32_t flags, void* vertices_device, uint64_t vertex_capacity) {
    return build_geometry("bt_tile_tree_build_geometry_hp", true, t, a, ai, view, approximation, prepass, flags, vertices_device, vertex_capacity);
}

bt_status bt_tile_tree_tile_geometry_hp(bt_tile_tree* t, bt_atlas* a, uint32_t ai, const bt_view_state* view, const bt_model_approximation* approximation,
                                        const bt_tile_coordinate* tiles, uint32_t count, uint32_t flags, bt_terrain_vertex* out, uint64_t out_bytes) {
    return tile_geometry("bt_tile_tree_tile_geometry_hp", true, t, a, ai, view, approximation, tiles, count, flags, out, out_bytes);
}

}  // extern "C"

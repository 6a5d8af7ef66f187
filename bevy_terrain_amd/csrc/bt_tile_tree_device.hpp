// Device half of sample_attachment / sample_height (terrain_data/mod.rs:265-307) shared by the kernels that sample the
// terrain through a tile tree: tile_tree_sample_kernel (bt_tile_tree.hip), raycast_kernel (bt_raycast.hip), render_kernel (bt_render.hip),
// occlusion_kernel (bt_shadow.hip), collide_kernel and sweep_kernel (bt_collide.hip), tile_tree_normal_kernel (bt_normal.hip).  One
// definition, so a height a ray meets is the height bt_tile_tree_sample_attachment reports there, bit for bit.
//
// What such a kernel is handed is one thing on either side of the launch: TerrainRef on the host (make_ground of bt_tile_tree_host.hpp
// builds it, every launch_* takes it), Ground on the device (ground_view builds it at kernel entry from the kernel's own parameters).
//
// Arithmetic: IEEE binary64 / binary32, one rounding per written operation, see bt_model.hpp for the definitions
// where the reference defers to glam / libm.  compute_blend's log2 is the platform's (OCML here, libm in the oracle).
#pragma once

#include "bt_internal.hpp"
#include "bt_model.hpp"

namespace bt {

struct TreeParams {
    model::Model model;
    uint32_t lod_count, tree_size, sides;
    double load_distance, blend_distance;
    float blend_range, approximate_height;
    model::V3 view_world_position;
    model::Coordinate view_coordinate[6];  // the view coordinate projected to every side
};

// The terrain a query kernel samples, as the host hands it to a launcher: the tree's parameters and entries (device), one R16 attachment
// (its meta and level 0, device) and the tree's device copy of approximate_height (may be NULL: P.approximate_height)
struct TerrainRef {
    TreeParams P;
    const bt_tile_tree_entry* entries;
    AttachmentMeta m;
    const void* atlas;
    const float* height;
};

// bt_raycast.hip: `count` rays (device) against the terrain -> hits (device)
bt_status launch_raycast(hipStream_t stream, const TerrainRef& g, const bt_ray* rays, uint32_t count, uint32_t steps, uint32_t refine_rounds, bt_ray_hit* hits);
// bt_normal.hip: the world normals (3 floats each) and, when up_dot is not NULL, their cosine against the mesh normal, of `count` world
// positions (device)
bt_status launch_sample_normal(hipStream_t stream, const TerrainRef& g, const double* positions, uint32_t count, float* normals, float* up_dot);

// bt_render.hip: one launch of bt_tile_tree_render.  A wave renders one 8 x 8 block of pixels, a workgroup kRenderBlocksPerGroup of them;
// the launch covers blocks first_block .. first_block + block_count - 1 of the image's blocks_x x ceil(height / 8) blocks, row-major.
constexpr uint32_t kRenderThreads = 256;
constexpr uint32_t kRenderBlocksPerGroup = kRenderThreads / 64u;
struct RenderArgs {
    bt_render_camera camera;
    uint32_t steps, refine_rounds;
    uint32_t blocks_x, first_block, block_count;
    // the planes (device, width * height pixels each; NULL: not wanted) and the HIT / INSIDE / MISS pixel counters
    double* t;
    uint8_t* status;
    float* normal;
    uint32_t* rgba;
    uint32_t* counters;
    // bt_tile_tree_render_shadowed only (read by the kernel's shadowed instance alone): the SHADOW PLANE (device, may be NULL) and its march
    uint8_t* shadow_plane;
    bt_sun_shadow shadow;
};
// albedo == NULL: the grey of the height attachment (BT_RENDER_NO_ALBEDO).  shadowed: the kernel instance that casts a shadow ray from
// every pixel that met the ground (bt_tile_tree_render_shadowed); false: bt_tile_tree_render's, which reads no shadow field
bt_status launch_render(hipStream_t stream, const TerrainRef& g, const AttachmentMeta& albedo_meta, const void* albedo, const RenderArgs& a, bool shadowed);

// bt_shadow.hip: one launch of bt_tile_tree_sun_occlusion.  Ray g = first_ray + r of the batch is point g % count, direction g / count; its
// status goes to status[point * direction_count + direction].  A lane marches one ray, a workgroup kOcclusionThreads of them.
constexpr uint32_t kOcclusionThreads = 256;
struct OcclusionArgs {
    const double* positions;   // count x 3 (device)
    const double* directions;  // direction_count x 3 (device)
    uint32_t count, direction_count;
    uint32_t first_ray, ray_count;
    double lift, distance;
    uint32_t steps;
    uint8_t* status;     // count * direction_count (device), point-major
    uint32_t* counters;  // lit, occluded, invalid
};
bt_status launch_occlusion(hipStream_t stream, const TerrainRef& g, const OcclusionArgs& a);

// bt_collide.hip: SPHERE CONTACT of `count` spheres / SPHERE SWEEP of `count` sweeps (device) against the terrain -> contacts / hits
// (device); one wave each, kCollideWavesPerGroup of them per workgroup
constexpr uint32_t kCollideThreads = 256;
constexpr uint32_t kCollideWavesPerGroup = kCollideThreads / 64u;
bt_status launch_collide(hipStream_t stream, const TerrainRef& g, const bt_sphere* spheres, uint32_t count, uint32_t refine_rounds, bt_sphere_contact* contacts);
bt_status launch_sweep(hipStream_t stream, const TerrainRef& g, const bt_sphere_sweep* sweeps, uint32_t count, uint32_t steps, uint32_t bisections,
                       uint32_t refine_rounds, bt_sweep_hit* hits);

// bt_geometry.hip: what TERRAIN GEOMETRY (include/bevy_terrain_amd.h) takes from the tree besides its entries
struct GeometryParams {
    uint32_t grid_size, tree_size, lod_count, sides, flags;  // flags: BT_GEOMETRY_*
    float morph_distance, blend_distance, morph_range, blend_range, min_height, max_height;
};
// the vertices (bt_terrain_vertex, device) of the tiles of a device list, in list order.  device_count != NULL: the list's length is read
// on the device, min(*device_count, count); otherwise it is `count`.  Tile k writes slots k * slots_per_tile .. of `vertices` and carries
// tile_index tile_base + k; a tile whose last slot lies beyond vertex_capacity is left out.  approximation != NULL: the HIGH PRECISION
// instantiation (the only one that reads BT_GEOMETRY_VIEW_RELATIVE); NULL: the plain one.
bt_status launch_geometry(hipStream_t stream, const bt_view_state& view, const GeometryParams& G, const bt_tile_tree_entry* entries, const AttachmentMeta& m,
                          const void* atlas, const bt_tile_coordinate* tiles, const uint32_t* device_count, uint32_t count, uint32_t tile_base,
                          void* vertices, uint64_t vertex_capacity, const bt_model_approximation* approximation);

#if defined(__HIPCC__)

__device__ __forceinline__ float unorm16_to_float(uint32_t t) {
    const float x = float(t), r = 1.0f / 65535.0f;
    const float q0 = x * r;
    return __builtin_fmaf(__builtin_fmaf(-q0, 65535.0f, x), r, q0);
}
__device__ __forceinline__ float unorm8_to_float(uint32_t t) {
    const float x = float(t), r = 1.0f / 255.0f;
    const float q0 = x * r;
    return __builtin_fmaf(__builtin_fmaf(-q0, 255.0f, x), r, q0);
}

struct Lookup {  // TileLookup (tile_tree.rs:67-81)
    uint32_t atlas_index, atlas_lod;
    float uv[2];
};

// TileTree::lookup_tile (tile_tree.rs:241-266) from the coordinate of the world position on
__device__ __forceinline__ Lookup lookup_tile_at(const TreeParams& P, const bt_tile_tree_entry* __restrict__ entries, model::Coordinate c, uint32_t tree_lod) {
    const double tile_count = double(1u << tree_lod);
    const model::V2 t = model::compute_tree_xy(c, tile_count);
    const uint32_t ts = P.tree_size;
    const uint64_t ix = uint64_t(t.x), iy = uint64_t(t.y);  // `as usize` (non-negative here)
    const bt_tile_tree_entry e = entries[((c.side * P.lod_count + tree_lod) * ts + uint32_t(ix % ts)) * ts + uint32_t(iy % ts)];
    if (e.atlas_lod == BT_INVALID_LOD) return {BT_INVALID_ATLAS_INDEX, BT_INVALID_LOD, {0.0f, 0.0f}};
    const double div = double(1u << (tree_lod - e.atlas_lod));
    const double qx = t.x / div, qy = t.y / div;
    return {e.atlas_index, e.atlas_lod, {float(qx - trunc(qx)), float(qy - trunc(qy))}};  // `% 1.0`, as_vec2
}
__device__ __forceinline__ Lookup lookup_tile(const TreeParams& P, const bt_tile_tree_entry* __restrict__ entries, model::V3 world_position, uint32_t tree_lod) {
    return lookup_tile_at(P, entries, model::coordinate_from_world_position(world_position, P.model), tree_lod);
}

// The bilinear sample of a tile from texel space on (AttachmentData::sample, terrain_data/mod.rs:220-263), in three pieces shared by
// sample_lookup and the tile normal (bt_normal_device.hpp): t = uv * T - 0.5 -> (rem, first texel); the clamped texel; the two lerps.
__device__ __forceinline__ void texel_split(float t, float& rem, int& first) {
    rem = fmodf(t, 1.0f);
    first = int(t);
}
__device__ __forceinline__ uint32_t texel_clamp(int i, uint32_t T) { return uint32_t(min(max(i, 0), int(T) - 1)); }
// v[x][y]: the four texels; rem[0] along x, rem[1] along y
__device__ __forceinline__ float bilerp(float v00, float v01, float v10, float v11, float rem_x, float rem_y) {
    const float a = v00 + (v01 - v00) * rem_y;
    const float b = v10 + (v11 - v10) * rem_y;
    return a + (b - a) * rem_x;
}

// AtlasAttachment::sample + AttachmentData::sample (tile_atlas.rs:249-258, terrain_data/mod.rs:220-263); the same
// code as bt_kernels.hip sample_kernel
__device__ __forceinline__ void sample_lookup(const AttachmentMeta& m, const void* __restrict__ atlas, const Lookup& l, float r[4]) {
    if (l.atlas_index >= m.atlas_size) {
        r[0] = r[1] = r[2] = r[3] = 0.0f;
        return;
    }
    const uint32_t T = m.texture_size;
    const float scale = float(m.center_size) / float(T), offset = float(m.border_size) / float(T);
    float rem[2];
    int ixy[2];
#pragma unroll
    for (int a = 0; a < 2; a++) {
        const float u = l.uv[a] * scale + offset;
        texel_split(u * float(T) - 0.5f, rem[a], ixy[a]);
    }
    float v[2][2][4];
#pragma unroll
    for (int x = 0; x < 2; x++)
#pragma unroll
        for (int y = 0; y < 2; y++) {
            const uint32_t px = texel_clamp(ixy[0] + x, T), py = texel_clamp(ixy[1] + y, T);
            const uint64_t index = uint64_t(l.atlas_index) * T * T + uint64_t(py) * T + px;
            if (m.format == BT_FORMAT_R16) {
                v[x][y][0] = unorm16_to_float(((const uint16_t*)atlas)[index]);
                v[x][y][1] = v[x][y][2] = v[x][y][3] = 0.0f;
            } else {
                const uint32_t t = ((const uint32_t*)atlas)[index];
#pragma unroll
                for (int k = 0; k < 4; k++) v[x][y][k] = unorm8_to_float((t >> (8 * k)) & 0xFFu);
            }
        }
#pragma unroll
    for (int k = 0; k < 4; k++) r[k] = bilerp(v[0][0][k], v[0][1][k], v[1][0][k], v[1][1][k], rem[0], rem[1]);
}

// TileTree::compute_blend (tile_tree.rs:223-239) of a surface position
__device__ __forceinline__ void compute_blend(const TreeParams& P, model::V3 surface, uint32_t& lod, float& ratio) {
    const double view_distance = model::distance3(P.view_world_position, surface);
    const double cap = double(P.lod_count) - 0.00001;
    const double l2 = log2(P.blend_distance / view_distance);
    const float target_lod = float(l2 < cap ? l2 : cap);
    lod = !(target_lod > 0.0f) ? 0u : uint32_t(target_lod);  // `as u32` saturates
    ratio = 0.0f;
    if (lod != 0) {  // inverse_mix(lod + blend_range, lod, target_lod) (util.rs:8-10)
        const float a = float(lod) + P.blend_range, b = float(lod);
        const float q = (target_lod - a) / (b - a);
        ratio = q < 0.0f ? 0.0f : (q > 1.0f ? 1.0f : q);
    }
}

// sample_attachment (terrain_data/mod.rs:265-295) from the surface position on: compute_blend, the lookups at lod and lod - 1,
// their samples and the blend.  surface = surface_position(model, sample position, approximate_height).
__device__ __forceinline__ void sample_surface(const TreeParams& P, const bt_tile_tree_entry* __restrict__ entries, const AttachmentMeta& m,
                                               const void* __restrict__ atlas, model::V3 surface, float value[4]) {
    uint32_t lod;
    float ratio;
    compute_blend(P, surface, lod, ratio);
    sample_lookup(m, atlas, lookup_tile(P, entries, surface, lod), value);
    if (ratio > 0.0f) {
        float value2[4];
        sample_lookup(m, atlas, lookup_tile(P, entries, surface, lod - 1u), value2);
#pragma unroll
        for (int k = 0; k < 4; k++) value[k] = value[k] + (value2[k] - value[k]) * ratio;  // Vec4::lerp
    }
}

// sample_height's last step (terrain_data/mod.rs:297-307): f32::lerp(min_height, max_height, value.x)
__device__ __forceinline__ float height_of_value(const model::Model& model, float value) { return model.min_height + (model.max_height - model.min_height) * value; }

// the tree's approximate_height as a kernel reads it: the device copy the frame chain writes on the stream (bt_frame_update: the host's
// copy in P may lag a frame), the host's where the caller has none
__device__ __forceinline__ float tree_height(float host_height, const float* height) { return height ? *height : host_height; }

// The terrain as a device function samples it: the kernel's own parameters and the three values every sample of a query derives from them.
// P and m are held by value: the copy dissolves into the kernel's argument loads, where a reference to the argument turned the height
// into a load through a generic pointer held in vector registers (ten more VGPRs in occlusion_kernel and render_kernel<true>).
// skip_above / ceiling, the ceiling skip of ray_eval and sphere_contact (bt_raycast.hip's header has the argument): a sample whose altitude
// is above `ceiling` = lerp(min_height, max_height, 1.0f) is above the ground whatever the atlas holds, provided the tiles have a border
// and the height range is not inverted.
struct Ground {
    TreeParams P;
    const bt_tile_tree_entry* entries;
    AttachmentMeta m;
    const void* atlas;
    double approximate_height;
    bool skip_above;
    double ceiling;
};
// at kernel entry, from the kernel's __restrict__ parameters: the ONE place these three expressions are written
__device__ __forceinline__ Ground ground_view(const TreeParams& P, const bt_tile_tree_entry* __restrict__ entries, const AttachmentMeta& m,
                                              const void* __restrict__ atlas, const float* __restrict__ height) {
    return {P, entries, m, atlas, double(tree_height(P.approximate_height, height)), m.border_size >= 1u && P.model.max_height >= P.model.min_height,
            double(height_of_value(P.model, 1.0f))};
}
// sample_surface of the ground's own attachment
__device__ __forceinline__ void sample_ground(const Ground& G, model::V3 surface, float value[4]) { sample_surface(G.P, G.entries, G.m, G.atlas, surface, value); }

#endif  // __HIPCC__

}  // namespace bt

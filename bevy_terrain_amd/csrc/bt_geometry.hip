// Terrain geometry (include/bevy_terrain_amd.h, TERRAIN GEOMETRY): the reference's vertex stage (src/shaders/render/vertex.wgsl with
// compute_tile_uv, compute_morph, compute_blend, lookup_tile and coordinate_change_lod of src/shaders/functions.wgsl and sample_height of
// attachments.wgsl) as a compute pass over a list of tiles, for hosts that have no wgpu draw to run it in: the vertices of the tiles the
// prepass selected, morphed and displaced exactly as the renderer would.
//
// One 256-thread workgroup per tile per trip of a plain grid-stride loop (no workgroup waits on another).  A tile's strip doubles every
// interior grid vertex (2 g (g + 2) slots for (g + 1)^2 vertices), so the workgroup evaluates each GRID vertex once — two surface points
// with their square roots and divisions, two f64 log2, one or two tile lookups of four texels — into LDS (48 bytes a vertex, 13.9 KB at
// g = 16, 52.3 KB at the cap g = 32), and then copies the tile's slots out of LDS in slot order, one 16-byte store per lane: a wave writes
// 1 KiB of consecutive bytes.  LDS image: vertex v = cy (g + 1) + cx at float4[3 v .. 3 v + 2] — the writers' ds_write_b128 at a 48-byte
// lane stride fall on distinct banks within each group of 8 lanes, and in the GRID layout the copy is the identity.
//
// POINT and coordinate_change_lod are bt_surface_device.hpp's (the prepass's own), the tile sample is sample_lookup of
// bt_tile_tree_device.hpp (bt_tile_tree_sample_attachment's own).  The view travels as an unmodified by-value argument (see
// should_be_divided in bt_refine.hip on what writing into it costs).
//
// HIGH PRECISION (bt_tile_tree_build_geometry_hp / _tile_geometry_hp) is an instantiation of its own (template <bool kHighPrecision>, as kCull
// in bt_refine.hip): the kernel the plain calls run is what it was.  A vertex nearer than precision_threshold_distance takes its position
// from REL (bt_surface_device.hpp), the reference's second-order series around the view, instead of scale * local + translation; the
// coefficients travel as a by-value argument of their own (448 bytes), never written, indexed by the tile's side, which is workgroup-
// uniform: they are read with scalar loads and stay out of the VGPRs.
//
// Arithmetic contract: IEEE binary32 unless marked, one rounding per written operation (-ffp-contract=off); the two log2 are OCML's f64.
#include "bt_internal.hpp"
#include "bt_surface_device.hpp"
#include "bt_tile_tree_device.hpp"

namespace bt {
namespace {

constexpr uint32_t kGeometryThreads = 256;
constexpr uint32_t kGeometryBlocks = 1024;  // the fixed launch of the device form: four workgroups a CU

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float mixf(float a, float b, float t) { return a * (1.0f - t) + b * t; }
__device__ __forceinline__ float satf(float x) { return x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x); }

// lookup(o) of the definition from the blend LOD on: the value (channel x) of the tile the tree's entry names, 0 without one
__device__ __forceinline__ float lookup_value(const GeometryParams& G, const bt_tile_tree_entry* __restrict__ entries, const AttachmentMeta& m,
                                              const void* __restrict__ atlas, Coordinate c, uint32_t lookup_lod) {
    if (c.side >= G.sides) return 0.0f;  // (a list that is not this tree's: no entry to read)
    coordinate_change_lod(c, lookup_lod);
    const uint32_t ts = G.tree_size;
    const bt_tile_tree_entry e = entries[((c.side * G.lod_count + lookup_lod) * ts + c.x % ts) * ts + c.y % ts];
    if (e.atlas_lod == BT_INVALID_LOD) return 0.0f;
    coordinate_change_lod(c, e.atlas_lod);
    float r[4];
    sample_lookup(m, atlas, Lookup{e.atlas_index, e.atlas_lod, {c.u, c.v}}, r);
    return r[0];
}

template <bool kHighPrecision>
struct HpArgs {};
template <>
struct HpArgs<true> {
    bt_model_approximation approximation;
};

// one grid vertex (cx, cy) of tile `tile`, the tile_index-th of its list: steps 1 - 6 of the definition (kHighPrecision: with steps 2h and
// 3h) -> the three 16-byte parts
template <bool kHighPrecision>
__device__ __forceinline__ void grid_vertex(const bt_view_state& view, const HpArgs<kHighPrecision>& hpa, const GeometryParams& G, const bt_tile_tree_entry* __restrict__ entries,
                                            const AttachmentMeta& m, const void* __restrict__ atlas, const bt_tile_coordinate& tile, uint32_t tile_index, uint32_t cx,
                                            uint32_t cy, f32x4* __restrict__ out) {
    const float g = float(G.grid_size);
    const float tu = float(cx) / g, tv = float(cy) / g;
    // 2: x / 2^lod == x * 2^-lod bit for bit (see should_be_divided)
    const float inv_tc = __builtin_bit_cast(float, (127u - tile.lod) << 23);
    SurfacePoint p = tile_surface(view, tile.side, (float(tile.x) + tu) * inv_tc, (float(tile.y) + tv) * inv_tc);
    const float dx = (p.wx + view.approximate_height * p.nx) - view.world_position[0];
    const float dy = (p.wy + view.approximate_height * p.ny) - view.world_position[1];
    const float dz = (p.wz + view.approximate_height * p.nz) - view.world_position[2];
    float d = length3(dx, dy, dz);
    // 2h: the distance once more, from the series
    bool hp = false;
    if constexpr (kHighPrecision) {
        hp = d < hpa.approximation.precision_threshold_distance;
        if (hp) {
            const Rel r = relative_position(view, hpa.approximation, Coordinate{tile.side, tile.lod, tile.x, tile.y, tu, tv});
            d = length3(r.x + view.approximate_height * p.nx, r.y + view.approximate_height * p.ny, r.z + view.approximate_height * p.nz);
        }
    }
    // 3
    float u = tu, v = tv;
    if (!(G.flags & BT_GEOMETRY_NO_MORPH)) {
        const float eu = float(uint32_t(tu * g) & ~1u) / g, ev = float(uint32_t(tv * g) & ~1u) / g;
        const float target = float(log2(double((2.0f * G.morph_distance) / d)));
        const float a = float(tile.lod) + G.morph_range;
        const float ratio = tile.lod == 0u ? 0.0f : satf((target - a) / (float(tile.lod) - a));
        u = mixf(tu, eu, ratio);
        v = mixf(tv, ev, ratio);
        if (!hp) p = tile_surface(view, tile.side, (float(tile.x) + u) * inv_tc, (float(tile.y) + v) * inv_tc);  // (3h keeps n0)
    }
    // 3h: world = view.world_position + REL at the morphed uv; the normal stays the unmorphed one (vertex.wgsl:55)
    Rel rel{0.0f, 0.0f, 0.0f};
    if constexpr (kHighPrecision) {
        if (hp) {
            rel = relative_position(view, hpa.approximation, Coordinate{tile.side, tile.lod, tile.x, tile.y, u, v});
            p.wx = view.world_position[0] + rel.x;
            p.wy = view.world_position[1] + rel.y;
            p.wz = view.world_position[2] + rel.z;
        }
    }
    // 4
    const float l2 = float(log2(double(G.blend_distance / d))), cap = float(G.lod_count) - 0.00001f;
    const float t = l2 < cap ? l2 : cap;
    const uint32_t bl = !(t > 0.0f) ? 0u : uint32_t(t);  // saturating; t < lod_count <= 31
    float ratio_b = 0.0f;
    if (bl != 0u && !(G.flags & BT_GEOMETRY_NO_BLEND)) {
        const float a = float(bl) + G.blend_range;
        ratio_b = satf((t - a) / (float(bl) - a));
    }
    // 5, 6
    const Coordinate c{tile.side, tile.lod, tile.x, tile.y, u, v};
    float height = mixf(G.min_height, G.max_height, lookup_value(G, entries, m, atlas, c, bl));
    if (ratio_b > 0.0f) {
        const float h1 = mixf(G.min_height, G.max_height, lookup_value(G, entries, m, atlas, c, bl - 1u));
        height = mixf(height, h1, ratio_b);
    }
    if constexpr (kHighPrecision) {
        if (G.flags & BT_GEOMETRY_VIEW_RELATIVE) {  // the base of the displacement relative to the view: the series itself where it was taken
            if (!hp) rel = Rel{p.wx - view.world_position[0], p.wy - view.world_position[1], p.wz - view.world_position[2]};
            p.wx = rel.x;
            p.wy = rel.y;
            p.wz = rel.z;
        }
    }
    out[0] = f32x4{p.wx + height * p.nx, p.wy + height * p.ny, p.wz + height * p.nz, height};
    out[1] = f32x4{p.nx, p.ny, p.nz, __builtin_bit_cast(float, tile_index)};
    out[2] = f32x4{u, v, d, ratio_b};
}

// tiles [0, n) of the list, n = min(*device_count, count) when device_count is given; tile k's vertices go to slots (k * slots_per_tile ..),
// its tile_index is tile_base + k
template <bool kHighPrecision>
__global__ __launch_bounds__(kGeometryThreads) void geometry_kernel(bt_view_state view, GeometryParams G, const bt_tile_tree_entry* __restrict__ entries, AttachmentMeta m,
                                                                    const void* __restrict__ atlas, const bt_tile_coordinate* __restrict__ tiles,
                                                                    const uint32_t* __restrict__ device_count, uint32_t count, uint32_t tile_base,
                                                                    f32x4* __restrict__ vertices, uint64_t vertex_capacity, HpArgs<kHighPrecision> hpa) {
    extern __shared__ __attribute__((aligned(16))) f32x4 s_vertex[];  // [(g + 1)^2][3]
    const uint32_t g = G.grid_size, row = g + 1u, grid_vertices = row * row;
    const bool grid_layout = (G.flags & BT_GEOMETRY_GRID) != 0u;
    const uint32_t vpr = 2u * (g + 2u), slots = grid_layout ? grid_vertices : g * vpr;
    const uint32_t n = device_count ? min(*device_count, count) : count;
    for (uint32_t k = blockIdx.x; k < n; k += gridDim.x) {
        if ((uint64_t(k) + 1u) * slots > vertex_capacity) break;  // left out whole (and so is every later tile of this workgroup)
        const bt_tile_coordinate tile = tiles[k];
        for (uint32_t vi = threadIdx.x; vi < grid_vertices; vi += kGeometryThreads) {
            const uint32_t cy = vi / row, cx = vi - cy * row;
            grid_vertex<kHighPrecision>(view, hpa, G, entries, m, atlas, tile, tile_base + k, cx, cy, s_vertex + 3u * vi);
        }
        __syncthreads();
        f32x4* __restrict__ dst = vertices + uint64_t(k) * slots * 3u;
        for (uint32_t q = threadIdx.x; q < slots * 3u; q += kGeometryThreads) {
            const uint32_t slot = q / 3u, part = q - slot * 3u;
            uint32_t vi = slot;
            if (!grid_layout) {  // compute_tile_uv: the first and the last vertex of a strip row twice
                const uint32_t col = slot / vpr, r = min(max(slot - col * vpr, 1u), vpr - 2u) - 1u;
                vi = (r >> 1) * row + col + (r & 1u);
            }
            dst[q] = s_vertex[3u * vi + part];
        }
        __syncthreads();  // the next trip overwrites the image
    }
}

}  // namespace

bt_status launch_geometry(hipStream_t stream, const bt_view_state& view, const GeometryParams& G, const bt_tile_tree_entry* entries, const AttachmentMeta& m,
                          const void* atlas, const bt_tile_coordinate* tiles, const uint32_t* device_count, uint32_t count, uint32_t tile_base,
                          void* vertices, uint64_t vertex_capacity, const bt_model_approximation* approximation) {
    if (!count) return BT_OK;
    const uint32_t row = G.grid_size + 1u, lds = row * row * 3u * uint32_t(sizeof(f32x4));
    const uint32_t blocks = device_count ? kGeometryBlocks : std::min(count, kGeometryBlocks);
    if (approximation)
        geometry_kernel<true><<<blocks, kGeometryThreads, lds, stream>>>(view, G, entries, m, atlas, tiles, device_count, count, tile_base, (f32x4*)vertices, vertex_capacity,
                                                                         HpArgs<true>{*approximation});
    else
        geometry_kernel<false><<<blocks, kGeometryThreads, lds, stream>>>(view, G, entries, m, atlas, tiles, device_count, count, tile_base, (f32x4*)vertices, vertex_capacity,
                                                                          HpArgs<false>{});
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "geometry_kernel");
    return BT_OK;
}

}  // namespace bt

// Surface normals (include/bevy_terrain_amd.h): bt_tile_tree_sample_normal, the reference fragment shader's normal (sample_normal of
// src/shaders/attachments.wgsl:51-107 blended over two LODs, render/fragment.wgsl:99-107) for a batch of world positions, and
// bt_atlas_tile_normals, the tangent-space normal map of the centre texels of listed tiles.  Both evaluate TILE NORMAL of
// bt_normal_device.hpp; the query reaches its tiles through lookup_tile / compute_blend of bt_tile_tree_device.hpp, so a normal belongs to
// the same tiles as the height bt_tile_tree_sample_attachment reports there.
//
// Query: one position per lane, shaped like tile_tree_sample_kernel; its 16 texel fetches per tile go to HBM / L2.
// Bake: one workgroup per band of centre rows of one tile.  The band's texture rows and `halo` rows above and below are copied into LDS
// once (16-byte loads when T % 8 == 0), lanes own adjacent texels of a row (two lanes share an LDS dword: a broadcast, no bank conflict),
// and each lane writes its texel as one dword: a wave stores 256 contiguous bytes.  A texel one of whose tap rows falls outside the LDS
// window (only possible when the rounding of a tap position passes the halo the host computed) takes all its texels from HBM instead —
// one test per texel — so the bytes are the definition's whatever the window.
#include <cstring>

#include "bt_internal.hpp"
#include "bt_model.hpp"
#include "bt_normal_device.hpp"

using namespace bt;
using namespace bt::model;

namespace {

// ---- the query ---------------------------------------------------------------------------------------------------

// (WORLD NORMAL itself: world_normal of bt_normal_device.hpp, shared with the render kernel of bt_render.hip)

__global__ __launch_bounds__(128) void tile_tree_normal_kernel(TreeParams P, const bt_tile_tree_entry* __restrict__ entries, AttachmentMeta m,
                                                               const uint16_t* __restrict__ atlas, NormalModel nm, const double* __restrict__ positions,
                                                               uint32_t count, float* __restrict__ normals, float* __restrict__ up_dot,
                                                               const float* __restrict__ height) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const V3 p = {positions[3 * i], positions[3 * i + 1], positions[3 * i + 2]};
    float cosine;
    const F3 out = world_normal(ground_view(P, entries, m, atlas, height), nm, p, cosine);
    normals[3 * uint64_t(i)] = out.x;
    normals[3 * uint64_t(i) + 1] = out.y;
    normals[3 * uint64_t(i) + 2] = out.z;
    if (up_dot) up_dot[i] = cosine;
}

// ---- the bake ----------------------------------------------------------------------------------------------------

constexpr uint32_t kBakeThreads = 256;
constexpr uint32_t kBakeBandRows = 32;           // centre rows of one workgroup at most
constexpr uint32_t kBakeLdsBytes = 40u << 10;    // its LDS window at most: four workgroups of a CU (160 KiB) hold theirs at once
constexpr uint32_t kNoWindow = 0xFFFFFFFFu;      // BakeArgs::halo when not even one centre row and its halo fit kBakeLdsBytes

struct BakeTile {
    uint32_t layer, lod;
};

struct BakeArgs {
    const uint16_t* atlas;
    const BakeTile* tiles;
    uint32_t* out;  // c * c dwords per tile
    AttachmentMeta m;
    NormalModel nm;
    uint32_t band_rows, halo, bands;  // centre rows per band, texture rows kept above and below them, bands per tile
};

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(kBakeThreads) void tile_normals_kernel(BakeArgs a) {
    extern __shared__ u32x4 lds_raw[];  // (16-byte aligned)
    uint16_t* lds = reinterpret_cast<uint16_t*>(lds_raw);
    const uint32_t T = a.m.texture_size, b = a.m.border_size, c = a.m.center_size;
    const uint32_t t = blockIdx.x / a.bands, band = blockIdx.x - t * a.bands;
    const BakeTile tile_info = a.tiles[t];
    const uint16_t* __restrict__ tile = a.atlas + uint64_t(tile_info.layer) * T * T;  // 64-bit layer offset
    const uint32_t j0 = band * a.band_rows, j1 = min(j0 + a.band_rows, c);
    // the window: texture rows [w0, w0 + rows) (halo == kNoWindow: none fits the LDS budget, rows = 0 and every fetch goes to HBM)
    uint32_t w0 = 0, rows = 0;
    if (a.halo != kNoWindow) {
        w0 = b + j0 > a.halo ? b + j0 - a.halo : 0u;
        rows = min(b + j1 - 1u + a.halo, T - 1u) - w0 + 1u;
        const uint16_t* src = tile + uint64_t(w0) * T;
        const uint32_t texels = rows * T;  // (at most kBakeLdsBytes / 2)
        if (T % 8u == 0u) {
            const u32x4* src4 = reinterpret_cast<const u32x4*>(src);
            for (uint32_t k = threadIdx.x; k < texels / 8u; k += kBakeThreads) lds_raw[k] = src4[k];
        } else {
            for (uint32_t k = threadIdx.x; k < texels; k += kBakeThreads) lds[k] = src[k];
        }
    }
    __syncthreads();
    const NormalTaps tp = normal_taps(a.m);
    const float dist = normal_dist(a.m, a.nm, tile_info.lod);
    uint32_t* __restrict__ out = a.out + uint64_t(t) * c * c;
    const uint32_t n = (j1 - j0) * c;
    for (uint32_t k = threadIdx.x; k < n; k += kBakeThreads) {
        const uint32_t row = k / c, j = j0 + row, i = k - row * c;
        const float uv[2] = {(float(i) + 0.5f) / float(c), (float(j) + 0.5f) / float(c)};
        const TapSplit sp = tap_split(tp, uv);
        // ONE window test per texel: the rows its taps and its own value touch, after the clamp
        const uint32_t lo = min(texel_clamp(sp.first[1][0], T), b + j), hi = max(texel_clamp(sp.first[1][2] + 1, T), b + j);
        uint32_t texel = 128u | (128u << 8) | (255u << 16);  // no data: (128, 128, 255, 0)
        if (lo >= w0 && hi - w0 < rows) {
            auto fetch = [&](uint32_t px, uint32_t py) -> uint32_t { return lds[(py - w0) * T + px]; };  // w0 <= lo <= py <= hi < w0 + rows
            if (fetch(b + i, b + j) != 0u) {
                const F3 s = tile_normal(tp, a.nm, dist, sp, fetch);
                texel = normal_enc(s.x) | (normal_enc(s.y) << 8) | (normal_enc(s.z) << 16) | (255u << 24);
            }
        } else {  // a tap row outside the window (or no window): the layer in HBM
            auto fetch = [&](uint32_t px, uint32_t py) -> uint32_t { return tile[uint64_t(py) * T + px]; };
            if (fetch(b + i, b + j) != 0u) {
                const F3 s = tile_normal(tp, a.nm, dist, sp, fetch);
                texel = normal_enc(s.x) | (normal_enc(s.y) << 8) | (normal_enc(s.z) << 16) | (255u << 24);
            }
        }
        out[uint64_t(j) * c + i] = texel;
    }
}

// texture rows a tap can lie from its centre texel: the offset o is T / (2c) texels, the bilinear pair adds one, one more for the rounding
// of the tap position
uint32_t bake_halo(const AttachmentMeta& m) { return m.texture_size / (2u * m.center_size) + 2u; }

}  // namespace

namespace bt {

bt_status launch_sample_normal(hipStream_t stream, const TerrainRef& g, const double* positions, uint32_t count, float* normals, float* up_dot) {
    if (!count) return BT_OK;
    const NormalModel nm = {g.P.model.min_height, g.P.model.max_height, normal_side_length(g.P.model)};
    tile_tree_normal_kernel<<<(count + 127u) / 128u, 128, 0, stream>>>(g.P, g.entries, g.m, (const uint16_t*)g.atlas, nm, positions, count, normals, up_dot, g.height);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? BT_OK : hip_fail(e, "tile_tree_normal_kernel");
}

}  // namespace bt

extern "C" bt_status bt_atlas_tile_normals(bt_atlas* a, uint32_t ai, const bt_terrain_model* model_c, const bt_tile_coordinate* coords, uint32_t count,
                                           uint8_t* out, uint64_t out_bytes) {
    const char* who = "bt_atlas_tile_normals";
    if (!a) {
        set_error("%s: NULL atlas", who);
        return BT_ERR_INVALID_ARGUMENT;
    }
    const Attachment* height;
    if (bt_status s = height_attachment(who, a, ai, &height)) return s;
    const Attachment& at = *height;
    if (!count) return BT_OK;
    if (bt_status s = check_model(model_c, who)) return s;
    if (!coords || !out) {
        set_error("%s: NULL %s", who, coords ? "out_host" : "coords");
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (at.meta.border_size == 0) {
        set_error("%s: attachment %u has no border (the taps of an edge texel need the neighbour's texels)", who, ai);
        return BT_ERR_UNSUPPORTED;
    }
    const uint32_t T = at.meta.texture_size, c = at.meta.center_size;
    const uint64_t tile_bytes = uint64_t(c) * c * 4u;
    if (out_bytes < uint64_t(count) * tile_bytes) {
        set_error("%s: out_bytes %llu below count * c * c * 4 = %llu", who, (unsigned long long)out_bytes, (unsigned long long)(uint64_t(count) * tile_bytes));
        return BT_ERR_INVALID_ARGUMENT;
    }
    const Model model = make_model(*model_c);
    std::vector<BakeTile> tiles(count);
    for (uint32_t i = 0; i < count; i++) {
        const bt_tile_coordinate& co = coords[i];
        if (co.side >= side_count(model) || co.lod >= a->config.lod_count || co.lod > 31u || (uint64_t(co.x) >> co.lod) || (uint64_t(co.y) >> co.lod)) {
            set_error("%s: coords[%u] = (%u, %u, %u, %u): side / lod / x / y out of range", who, i, co.side, co.lod, co.x, co.y);
            return BT_ERR_INVALID_ARGUMENT;
        }
        const auto it = a->tile_states.find(co);
        if (it == a->tile_states.end() || it->second.atlas_index >= at.meta.atlas_size) {
            set_error("%s: the atlas holds no layer for coords[%u] = (%u, %u, %u, %u)", who, i, co.side, co.lod, co.x, co.y);
            return BT_ERR_INVALID_ARGUMENT;
        }
        tiles[i] = {it->second.atlas_index, co.lod};
    }
    bt_ctx* ctx = a->ctx;
    BT_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    // chunks of tiles whose normal maps fit 32 MiB; each goes kernel -> device scratch -> pinned staging -> out, three in flight
    constexpr uint32_t kBuffers = StagingRing::kBuffers;
    const uint64_t chunk = std::min<uint64_t>(count, std::max<uint64_t>(1u, (32ull << 20) / tile_bytes));
    const uint64_t chunk_bytes = chunk * tile_bytes, list_bytes = (uint64_t(count) * sizeof(BakeTile) + 255u) & ~255ull;
    const uint32_t chunks = uint32_t((count + chunk - 1u) / chunk);
    const uint64_t need = list_bytes + std::min<uint64_t>(kBuffers, chunks) * chunk_bytes;
    if (bt_status st = ctx->normal.reserve(ctx, need)) return st;
    StagingRing& ring = ctx->staging;
    if (bt_status st = ring.reserve(size_t(chunk_bytes), 32ull << 20)) return st;
    uint8_t* dev = (uint8_t*)ctx->normal.dev;
    BakeArgs args{};
    args.atlas = (const uint16_t*)at.level0;  // a read: no layer is marked written
    args.m = at.meta;
    args.nm = {model.min_height, model.max_height, normal_side_length(model)};
    args.halo = bake_halo(at.meta);
    // the band: as many centre rows as the LDS budget holds beside the halo, at most kBakeBandRows; none fits: no window
    const uint64_t row_bytes = uint64_t(T) * 2u, window_rows = kBakeLdsBytes / row_bytes;
    if (window_rows > 2ull * args.halo) {
        args.band_rows = uint32_t(std::min<uint64_t>({kBakeBandRows, window_rows - 2ull * args.halo, c}));
    } else {
        args.band_rows = std::min(kBakeBandRows, c);
        args.halo = kNoWindow;
    }
    args.bands = (c + args.band_rows - 1u) / args.band_rows;
    const size_t lds = args.halo == kNoWindow ? 0 : size_t(std::min<uint64_t>(args.band_rows + 2ull * args.halo, T) * row_bytes);
    BT_HIP(hipMemcpyAsync(dev, tiles.data(), count * sizeof(BakeTile), hipMemcpyHostToDevice, s));
    auto tiles_of = [&](uint32_t ci) { return std::min<uint64_t>(chunk, count - ci * chunk); };
    auto enqueue = [&](uint32_t ci, uint32_t k) {
        args.tiles = (const BakeTile*)dev + ci * chunk;
        args.out = (uint32_t*)(dev + list_bytes + k * chunk_bytes);
        tile_normals_kernel<<<uint32_t(tiles_of(ci)) * args.bands, kBakeThreads, lds, s>>>(args);
        const hipError_t e = hipGetLastError();
        return e != hipSuccess ? e : hipMemcpyAsync(ring.buffer(k), args.out, tiles_of(ci) * tile_bytes, hipMemcpyDeviceToHost, s);
    };
    auto landed = [&](uint32_t ci, uint32_t k) { memcpy(out + ci * chunk * tile_bytes, ring.buffer(k), tiles_of(ci) * tile_bytes); };
    const bt_status rc = stage_out_chunks(ring, s, chunks, who, enqueue, landed);
    if (rc != BT_OK) (void)hipStreamSynchronize(s);  // (the kernels write the scratch; `tiles` leaves with this call)
    return rc;
}

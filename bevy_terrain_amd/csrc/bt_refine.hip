// Tiling prepass (UDLOD tile refinement) as ONE persistent launch.
//
// Reference: TilingPrepassNode::run (render/tiling_prepass.rs:204-272) records 2*refinement_count+3
// dependent dispatches per view per frame — prepare_root, then (refine_tiles indirect, prepare_next) x
// refinement_count, refine_tiles, prepare_render — with two global atomics per tile
// (shaders/tiling_prepass/refine_tiles.wgsl:5-15) and "very low" occupancy (docs/implementation.md:62-65).
//
// Here one 1024-thread workgroup (16 wavefronts of 64) runs the whole schedule: the per-pass state
// (`Parameters`, types.wgsl:43-48) lives in LDS, passes are separated by __syncthreads() instead of
// kernel boundaries, and the child / final appends are a stable compaction — wave64 __ballot +
// __popcll ranks inside a wave, a 16-entry LDS scan across waves — so there are no global atomics and
// the output order is exactly the order of the reference run with invocations taken in id order.
// The ping-pong layout of `temporary_tiles` (parents read from one end, children appended from the
// other, prepare_prepass.wgsl:25-36) is kept so the buffers are bit-compatible.
//
// Arithmetic contract: IEEE binary32, one rounding per written operation (-ffp-contract=off), same
// operation order as oracle/bt_oracle.c (functions.wgsl:14-29,73-96,117-188).
#include "bt_internal.hpp"
#include "bt_surface_device.hpp"  // Coordinate, coordinate_change_lod, length3, SurfacePoint, tile_surface

struct bt_tiling_prepass {
    bt_ctx* ctx = nullptr;
    uint32_t capacity = 0;
    bt_tile_coordinate* temporary_tiles = nullptr;
    bt_tile_coordinate* final_tiles = nullptr;
    bt_indirect* indirect = nullptr;
    uint32_t* counters = nullptr;  // [0] final count, [1] overflow flag, [2] tiles visited, [3] passes, [4] tiles culled; unordered form: [8..40) tiles visited per LOD, [40..72) dividing tiles per LOD
    unsigned long long* bits = nullptr;  // divide bits of every (side, lod) window, then their cull bits (allocated on first use)
    int window = 0;                      // window radius of the unordered form (0 = the default, kWinK)
    bool unordered = false;              // the last run was the unordered form: read() derives counters [1..3] from the per-LOD counts
    uint32_t unordered_capacity = 0;
    bool cull_set = false;                     // bt_tiling_prepass_set_culling
    bt_cull_view cull{};
    const bt_height_bounds* bounds = nullptr;  // borrowed
    bool culled_run = false;                   // the last run culled: counters[4] is its count
    bool horizon_set = false;                  // bt_tiling_prepass_set_horizon
    bt_horizon_view horizon{};
};

namespace bt {
namespace {

constexpr uint32_t kThreads = 1024;
constexpr uint32_t kWaves = kThreads / 64;

// refine_tiles.wgsl:17-22 -> compute_subdivision_coordinate (functions.wgsl:133-154) ->
// approximate_view_distance (:117-131) -> compute_local_position (:73-96)
// approximate_height: the view's (bt_view_state::approximate_height), or the value bt_frame_update left on the device — passed
// beside the view: writing it into the by-value kernel argument makes the compiler copy the whole struct to scratch (224 bytes,
// 14 -> 52 VGPRs in the divide-bits kernel: measured, round 4)
__device__ bool should_be_divided(const bt_view_state& v, const bt_tile_coordinate& tile, float approximate_height) {
    Coordinate vc{tile.side, v.origin_lod, uint32_t(v.sides[tile.side].view_xy[0]), uint32_t(v.sides[tile.side].view_xy[1]),
                  v.sides[tile.side].view_uv[0], v.sides[tile.side].view_uv[1]};
    coordinate_change_lod(vc, tile.lod);
    const int off_x = int(vc.x) - int(tile.x), off_y = int(vc.y) - int(tile.y);
    const float uv_x = off_x < 0 ? 0.0f : (off_x > 0 ? 1.0f : vc.u);
    const float uv_y = off_y < 0 ? 0.0f : (off_y > 0 ? 1.0f : vc.v);

    // tile_count(lod) = 2^lod: x / 2^lod == x * 2^-lod bit for bit (no underflow at these magnitudes), and so is / 0.5 == * 2 —
    // five of the function's eleven IEEE divisions (each ~10 instructions, and this kernel is one CU's VALU)
    const float inv_tc = __builtin_bit_cast(float, (127u - tile.lod) << 23);
    const SurfacePoint p = tile_surface(v, tile.side, (float(tile.x) + uv_x) * inv_tc, (float(tile.y) + uv_y) * inv_tc);
    const float dx = (p.wx + approximate_height * p.nx) - v.world_position[0];
    const float dy = (p.wy + approximate_height * p.ny) - v.world_position[1];
    const float dz = (p.wz + approximate_height * p.nz) - v.world_position[2];
    const float view_distance = length3(dx, dy, dz);
    return view_distance < v.subdivision_distance * inv_tc;
}

// ---- frustum and height-bounds culling (the definition: include/bevy_terrain_amd.h) --------------------------------------
// The culling kernels are instantiations of their own (template <bool kCull>): with culling off the kernels that run are what they
// were.  The cull view travels as a kernel argument of its own, never written, so its planes stay in SGPRs (see should_be_divided
// on what a modified by-value argument costs), the table as a pointer.
template <bool kCull>
struct CullArgs {};
template <>
struct CullArgs<true> {
    bt_cull_view cull;
    const uint32_t* table;  // bt_height_bounds::table, or nullptr: every tile spans (0, 65535)
    uint32_t levels, sides;
    uint32_t horizon_on;    // bt_tiling_prepass_set_horizon: the horizon test runs after the planes (a scalar branch)
    bt_horizon_view horizon;
};

__device__ __forceinline__ float unorm16_height(const bt_cull_view& c, uint32_t v) { return c.min_height + (c.max_height - c.min_height) * (float(v) / 65535.0f); }

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

// q(tile, uv, h) = l + h * (local_from_world * n): the point in scaled space (the unit sphere's frame), from l and never from the world point
struct ScaledPoint {
    float x, y, z;
};
__device__ __forceinline__ ScaledPoint scaled_point(const bt_view_state& v, const SurfacePoint& s, float h) {
    const float* t = v.local_from_world_transpose;
    const float gx = (t[0] * s.nx + t[1] * s.ny) + t[2] * s.nz;
    const float gy = (t[3] * s.nx + t[4] * s.ny) + t[5] * s.nz;
    const float gz = (t[6] * s.nx + t[7] * s.ny) + t[8] * s.nz;
    return {s.lx + h * gx, s.ly + h * gy, s.lz + h * gz};
}

// Five surface points (the four corners and the centre) carry all nine points of either test: both heights reuse them.
__device__ bool tile_culled(const bt_view_state& v, const CullArgs<true>& c, const bt_tile_coordinate& tile) {
    uint32_t range = 0xFFFF0000u;  // (0, 65535)
    if (c.table) {
        const uint32_t lb = min(tile.lod, c.levels - 1u), sh = tile.lod - lb, n = 1u << lb;
        const uint32_t base = c.sides * (((1u << (2u * lb)) - 1u) / 3u);
        range = c.table[base + (tile.side * n + (tile.y >> sh)) * n + (tile.x >> sh)];  // one 4-byte load per tile
    }
    const float h_lo = unorm16_height(c.cull, range & 0xFFFFu), h_hi = unorm16_height(c.cull, range >> 16);
    const float inv_tc = __builtin_bit_cast(float, (127u - tile.lod) << 23);
    const float u0 = (float(tile.x) + 0.0f) * inv_tc, u1 = (float(tile.x) + 1.0f) * inv_tc;
    const float w0 = (float(tile.y) + 0.0f) * inv_tc, w1 = (float(tile.y) + 1.0f) * inv_tc;
    const SurfacePoint s[4] = {tile_surface(v, tile.side, u0, w0), tile_surface(v, tile.side, u1, w0), tile_surface(v, tile.side, u0, w1),
                               tile_surface(v, tile.side, u1, w1)};
    float px[8], py[8], pz[8];
#pragma unroll
    for (uint32_t k = 0; k < 8; k++) {
        const float h = k < 4 ? h_lo : h_hi;
        px[k] = s[k & 3u].wx + h * s[k & 3u].nx;
        py[k] = s[k & 3u].wy + h * s[k & 3u].ny;
        pz[k] = s[k & 3u].wz + h * s[k & 3u].nz;
    }
    float slack = 0.0f;
    SurfacePoint m{};
    if (v.spherical) {
        m = tile_surface(v, tile.side, (float(tile.x) + 0.5f) * inv_tc, (float(tile.y) + 0.5f) * inv_tc);
        const float bx = (m.wx + h_hi * m.nx) - ((px[4] + px[5]) + (px[6] + px[7])) * 0.25f;
        const float by = (m.wy + h_hi * m.ny) - ((py[4] + py[5]) + (py[6] + py[7])) * 0.25f;
        const float bz = (m.wz + h_hi * m.nz) - ((pz[4] + pz[5]) + (pz[6] + pz[7])) * 0.25f;
        slack = length3(bx, by, bz);
    }
    slack = slack + c.cull.margin;
    bool culled = false;
    for (uint32_t i = 0; i < c.cull.plane_count; i++) {  // (uniform: the planes are scalar loads)
        const float a = c.cull.planes[i][0], b = c.cull.planes[i][1], cc = c.cull.planes[i][2], d = c.cull.planes[i][3];
        const float limit = -(slack * length3(a, b, cc));
        bool outside = true;
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) outside = outside && ((a * px[k] + b * py[k]) + cc * pz[k]) + d < limit;
        culled = culled || outside;
    }
    // the horizon test (uniform: the word and the view are kernel arguments; a spherical view, checked by the host)
    if (c.horizon_on && c.horizon.vh > 0.0f) {
        const bt_horizon_view& hv = c.horizon;
        float qx[8], qy[8], qz[8];
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) {
            const ScaledPoint q = scaled_point(v, s[k & 3u], k < 4 ? h_lo : h_hi);
            qx[k] = q.x;
            qy[k] = q.y;
            qz[k] = q.z;
        }
        const ScaledPoint qc = scaled_point(v, m, h_hi);
        const float dx = qc.x - ((qx[4] + qx[5]) + (qx[6] + qx[7])) * 0.25f;
        const float dy = qc.y - ((qy[4] + qy[5]) + (qy[6] + qy[7])) * 0.25f;
        const float dz = qc.z - ((qz[4] + qz[5]) + (qz[6] + qz[7])) * 0.25f;
        const float bulge = sqrtf(dot3(dx, dy, dz, dx, dy, dz));
        const float widen = (bulge + hv.margin) + BT_HORIZON_GUARD;  // (m of the definition)
        const float E = sqrtf(dot3(hv.eye[0], hv.eye[1], hv.eye[2], hv.eye[0], hv.eye[1], hv.eye[2])), sv = sqrtf(hv.vh), lim = widen * E;
        bool hidden = true;
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) {
            const float vx = qx[k] - hv.eye[0], vy = qy[k] - hv.eye[1], vz = qz[k] - hv.eye[2];
            const float ap = -dot3(vx, vy, vz, hv.eye[0], hv.eye[1], hv.eye[2]);
            const float along = ap / E;
            const float sq = dot3(vx, vy, vz, vx, vy, vz) - along * along;
            const float perp = sqrtf(sq > 0.0f ? sq : 0.0f);
            hidden = hidden && (ap - hv.vh) > lim && ((along * hv.occluder_radius) - (perp * sv)) > lim;
        }
        culled = culled || hidden;
    }
    return culled;
}

// ---- the divide test of every tile that can matter, computed up front ------------------------------------------------
// The schedule is a chain of up to refinement_count + 1 dependent passes, and a pass of the single-workgroup kernel costs
// ~2.5 us of pure latency: tile load (L2) -> ~200 dependent VALU instructions of should_be_divided -> ballot / scan /
// barrier.  But should_be_divided(tile) depends on the tile and the view alone, not on the pass: so a first launch
// evaluates it SPECULATIVELY for every tile inside a (2K+1)^2 window around the view's tile at every LOD of every side
// (tiles only divide close to the view: the criterion scales with the tile size) — ~1.3 k workgroups, one evaluation per
// thread, all independent — and leaves one bit per tile.  The ordered kernel then reads bits (from LDS) instead of running
// the arithmetic, keeps its frontier in LDS while it fits, and a pass shrinks to a few hundred nanoseconds.  A tile outside
// its window (possible, rare) is evaluated in place with the same function: the result is the same list in the same order.
constexpr int kWinK = 28;  // window radius in tiles: tiles DIVIDE within ~10 tiles of the view, so tiles EXIST within ~2 x 10 + 2 (more under the cube-sphere warp)
constexpr uint32_t kWinW = 2 * kWinK + 1, kWinBits = kWinW * kWinW;
constexpr uint32_t kWinChunks = (kWinBits + 255) / 256;      // 256-thread workgroups per (side, lod)
constexpr uint32_t kWinWords = kWinChunks * 4;               // 64-bit words per (side, lod): one per wave
constexpr uint32_t kMaxLods = 32;
constexpr uint32_t kFrontierCap = 2048;                      // tiles of a pass kept in LDS

// first tile (x, y) of the window of (side, lod): centred on the view's tile of that LOD, clamped into the face
__device__ __forceinline__ void window_origin(const bt_view_state& v, uint32_t side, uint32_t lod, int& ox, int& oy, int radius = kWinK) {
    // view_xy is signed: on a neighbouring cube face the view's tile lies outside [0, 2^origin_lod); the window belongs at the
    // face's NEAR edge then (cast to u32 first, a negative coordinate would end up clamped to the far one)
    const int olast = int((1u << min(v.origin_lod, 30u)) - 1u);
    const int vx = min(max(v.sides[side].view_xy[0], 0), olast), vy = min(max(v.sides[side].view_xy[1], 0), olast);
    Coordinate vc{side, v.origin_lod, uint32_t(vx), uint32_t(vy), v.sides[side].view_uv[0], v.sides[side].view_uv[1]};
    coordinate_change_lod(vc, lod);
    const int last = int((1u << lod) - 1u);  // lod <= 31
    const int cx = min(max(int(vc.x), 0), last), cy = min(max(int(vc.y), 0), last);
    ox = cx - radius;
    oy = cy - radius;
}

// lods: LODs 0 .. lods - 1 get their bits (the host's estimate of how deep this view can refine; anything deeper is
// evaluated in place by the ordered kernel — an estimate can only cost time, never change the result)
constexpr uint32_t kCntCulled = 4, kCntVisited = 8, kCntDivide = 40, kCounterWords = 72;  // (bt_tiling_prepass::counters)
constexpr size_t kBitsPlane = 6 * size_t(kMaxLods) * kWinWords;  // words of one bit plane (divide bits; the cull bits follow them)

// radius <= kWinK: the window actually used (storage is laid out for kWinK); counters != nullptr: also resets the counters and
// the indirect arguments the unordered collector (next launch) accumulates into.  kCull: the cull test of the same tiles next to the
// divide test, into the second bit plane
template <bool kCull>
__global__ __launch_bounds__(256) void tiling_divide_bits_kernel(bt_view_state view, uint32_t lods, int radius, unsigned long long* __restrict__ bits,
                                                                 uint32_t* __restrict__ counters, bt_indirect* __restrict__ indirect, const float* __restrict__ height,
                                                                 CullArgs<kCull> cull) {
    const float approximate_height = height ? *height : view.approximate_height;  // (bt_frame_update: the height sampled earlier on this stream, never seen by the host)
    const uint32_t W = 2u * uint32_t(radius) + 1u, chunks = (W * W + 255u) / 256u;
    const uint32_t chunk = blockIdx.x % chunks, lod = (blockIdx.x / chunks) % lods, side = blockIdx.x / (chunks * lods);
    if (counters && blockIdx.x == 0) {
        if (threadIdx.x < kCounterWords) counters[threadIdx.x] = 0;
        if (threadIdx.x == 0) *indirect = {0u, 1u, 0u, 0u};  // prepare_render's instance_count / bases; the vertex count accumulates
    }
    if (lod > view.refinement_count) return;
    int ox, oy;
    window_origin(view, side, lod, ox, oy, radius);
    const uint32_t b = chunk * 256u + threadIdx.x;
    const int tx = ox + int(b % W), ty = oy + int(b / W), last = int((1u << lod) - 1u);
    bool divide = false;
    if constexpr (kCull) {
        bool culled = false;
        if (b < W * W && tx >= 0 && ty >= 0 && tx <= last && ty <= last) {
            const bt_tile_coordinate tile{side, lod, uint32_t(tx), uint32_t(ty)};
            divide = should_be_divided(view, tile, approximate_height);
            culled = tile_culled(view, cull, tile);
        }
        const unsigned long long word = __ballot(divide), word_c = __ballot(culled);
        if ((threadIdx.x & 63u) == 0) {
            const size_t i = (size_t(side) * kMaxLods + lod) * kWinWords + chunk * 4u + (threadIdx.x >> 6);
            bits[i] = word;
            bits[kBitsPlane + i] = word_c;
        }
    } else {
        if (b < W * W && tx >= 0 && ty >= 0 && tx <= last && ty <= last) divide = should_be_divided(view, bt_tile_coordinate{side, lod, uint32_t(tx), uint32_t(ty)}, approximate_height);
        const unsigned long long word = __ballot(divide);
        if ((threadIdx.x & 63u) == 0) bits[(size_t(side) * kMaxLods + lod) * kWinWords + chunk * 4u + (threadIdx.x >> 6)] = word;
    }
}

// ---- the unordered form: the final SET straight from the bits ---------------------------------------------------------
// The reference appends final tiles in the arrival order of global atomics (refine_tiles.wgsl:13-15, 41): its contract is the
// set, not the order.  With every divide test known, membership needs no passes at all: a tile is visited iff all its
// ancestors divide, and it is final iff it is visited, does not divide itself and its LOD is a pass that runs
// (lod <= refinement_count; the children of tiles that still divide in the last pass are dropped, as in the reference).
// One thread per window tile walks its <= 31 ancestors' bits in LDS; finals are appended with one atomic per wave.  A
// visited, dividing tile whose child lies outside the child LOD's window (or deeper than the LODs that got bits) owns that
// child's whole subtree: a stackless depth-first walk evaluating should_be_divided in place, skipping anything that is
// inside a window (those tiles have their own thread) — so every tile is decided exactly once, whatever the window size.
// prepare_render's vertex count (prepare_prepass.wgsl:38-44) accumulates with the same reservations; per-LOD visit / divide
// counts let bt_tiling_prepass_read give the overflow verdict of the reference's buffers (a pass needs parents + children
// <= N, prepare_prepass.wgsl:25-36; the final list <= N).  No ticket, no fence: a "last workgroup" protocol made ~1500
// same-address atomics the longest thing in the kernel.

struct WindowBits {
    const unsigned long long* bits;  // LDS: [lod][kWinWords] of one side
    const int2* origin;              // LDS: [lod]
    uint32_t lods;
    int W;
    __device__ __forceinline__ bool inside(uint32_t lod, uint32_t x, uint32_t y, uint32_t& b) const {
        if (lod >= lods) return false;
        const int bx = int(x) - origin[lod].x, by = int(y) - origin[lod].y;
        b = uint32_t(by * W + bx);
        return bx >= 0 && by >= 0 && bx < W && by < W;
    }
    __device__ __forceinline__ bool bit(uint32_t lod, uint32_t b) const { return (bits[lod * kWinWords + (b >> 6)] >> (b & 63u)) & 1ull; }
};

// kCull: a second plane of bits says which window tiles are culled.  reach additionally wants every ancestor's cull bit clear; a
// reached tile whose own cull bit is set is visited and counted, and neither divides nor is final; the walk over the children no window
// covers applies the same test in place (so the result still does not depend on the window).
template <bool kCull>
__global__ __launch_bounds__(256) void tiling_collect_kernel(bt_view_state view, uint32_t lods, int radius, uint32_t capacity,
                                                             const unsigned long long* __restrict__ bits, bt_tile_coordinate* __restrict__ final_tiles,
                                                             bt_indirect* __restrict__ indirect, uint32_t* __restrict__ counters, const float* __restrict__ height,
                                                             CullArgs<kCull> cull) {
    constexpr uint32_t kPlane = kMaxLods * kWinWords;  // LDS words of one bit plane of one side
    __shared__ unsigned long long s_bits[(kCull ? 2u : 1u) * kPlane];
    const float approximate_height = height ? *height : view.approximate_height;
    __shared__ int2 s_origin[kMaxLods];
    const uint32_t W = 2u * uint32_t(radius) + 1u, chunks = (W * W + 255u) / 256u;
    const uint32_t chunk = blockIdx.x % chunks, lod = (blockIdx.x / chunks) % lods, side = blockIdx.x / (chunks * lods);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, rc = view.refinement_count;
    if (lod > rc) return;
    {
        if (tid < lods) {
            int ox, oy;
            window_origin(view, side, tid, ox, oy, radius);
            s_origin[tid] = int2{ox, oy};
        }
        const uint32_t words = min(lod + 2u, lods) * kWinWords;  // ancestors, the tile itself, its children's window
        for (uint32_t i = tid; i < words; i += 256u) s_bits[i] = bits[size_t(side) * kMaxLods * kWinWords + i];
        if constexpr (kCull)
            for (uint32_t i = tid; i < words; i += 256u) s_bits[kPlane + i] = bits[kBitsPlane + size_t(side) * kMaxLods * kWinWords + i];
    }
    __syncthreads();
    {
        const WindowBits wb{s_bits, s_origin, lods, int(W)};
        const WindowBits wc{s_bits + (kCull ? kPlane : 0u), s_origin, lods, int(W)};  // (kCull only)
        const uint32_t b = chunk * 256u + tid;
        const int tx = s_origin[lod].x + int(b % W), ty = s_origin[lod].y + int(b / W), last = int((1u << lod) - 1u);
        bool reach = b < W * W && tx >= 0 && ty >= 0 && tx <= last && ty <= last;
        for (uint32_t a = lod; reach && a-- > 0;) {  // all ancestors divide (order is irrelevant; an ancestor outside its window is evaluated in place)
            const uint32_t ax = uint32_t(tx) >> (lod - a), ay = uint32_t(ty) >> (lod - a);
            uint32_t ab;
            if constexpr (kCull) {
                if (wb.inside(a, ax, ay, ab)) {
                    reach = wb.bit(a, ab) && !wc.bit(a, ab);
                } else {
                    const bt_tile_coordinate at{side, a, ax, ay};
                    reach = !tile_culled(view, cull, at) && should_be_divided(view, at, approximate_height);
                }
            } else {
                reach = wb.inside(a, ax, ay, ab) ? wb.bit(a, ab) : should_be_divided(view, bt_tile_coordinate{side, a, ax, ay}, approximate_height);
            }
        }
        bool culled = false;
        if constexpr (kCull) {
            culled = reach && wc.bit(lod, b);
            const unsigned long long ballot_c = __ballot(culled);
            if (lane == 0 && ballot_c) atomicAdd(&counters[kCntCulled], uint32_t(__popcll(ballot_c)));
        }
        const bool divide = reach && !culled && wb.bit(lod, b);
        const bool fin = reach && !culled && !divide;
        // finals: one reservation per wave
        const unsigned long long ballot_f = __ballot(fin), ballot_r = __ballot(reach), ballot_d = __ballot(divide);
        uint32_t base = 0;
        if (lane == 0) {
            if (ballot_f) {
                base = atomicAdd(&counters[0], uint32_t(__popcll(ballot_f)));
                atomicAdd(&indirect->vertex_count, view.vertices_per_tile * uint32_t(__popcll(ballot_f)));
            }
            if (ballot_r) atomicAdd(&counters[kCntVisited + lod], uint32_t(__popcll(ballot_r)));
            if (ballot_d) atomicAdd(&counters[kCntDivide + lod], uint32_t(__popcll(ballot_d)));
        }
        base = __shfl(base, 0);
        if (fin) {
            const uint32_t fi = base + uint32_t(__popcll(ballot_f & ((1ull << lane) - 1ull)));
            if (fi < capacity) final_tiles[fi] = bt_tile_coordinate{side, lod, uint32_t(tx), uint32_t(ty)};
        }
        // children no thread owns: their subtrees, depth first, without a stack (child order 0..3 = (x & 1) | (y & 1) << 1)
        if (divide && lod < rc) {
            for (uint32_t i = 0; i < 4; i++) {
                uint32_t nl = lod + 1u, nx = (uint32_t(tx) << 1) + (i & 1u), ny = (uint32_t(ty) << 1) + (i >> 1), nb;
                if (wb.inside(nl, nx, ny, nb)) continue;
                for (;;) {
                    bool descend = false;
                    if (!wb.inside(nl, nx, ny, nb)) {
                        atomicAdd(&counters[kCntVisited + nl], 1u);
                        const bt_tile_coordinate node{side, nl, nx, ny};
                        bool node_culled = false;
                        if constexpr (kCull) node_culled = tile_culled(view, cull, node);
                        if (node_culled) {
                            atomicAdd(&counters[kCntCulled], 1u);
                        } else if (should_be_divided(view, node, approximate_height)) {
                            atomicAdd(&counters[kCntDivide + nl], 1u);
                            descend = nl < rc;
                        } else {
                            const uint32_t fi = atomicAdd(&counters[0], 1u);
                            atomicAdd(&indirect->vertex_count, view.vertices_per_tile);
                            if (fi < capacity) final_tiles[fi] = node;
                        }
                    }
                    if (descend) {
                        nl++;
                        nx <<= 1;
                        ny <<= 1;
                        continue;
                    }
                    bool done = false;
                    for (;;) {  // next sibling, or up until there is one; back at the start level: finished
                        if (nl == lod + 1u) {
                            done = true;
                            break;
                        }
                        const uint32_t c = (nx & 1u) | ((ny & 1u) << 1);
                        if (c < 3u) {
                            nx = (nx & ~1u) | ((c + 1u) & 1u);
                            ny = (ny & ~1u) | ((c + 1u) >> 1);
                            break;
                        }
                        nl--;
                        nx >>= 1;
                        ny >>= 1;
                    }
                    if (done) break;
                }
            }
        }
    }
}

// kAssist = false: the whole schedule from the arithmetic alone (the plain kernel: checker, and fallback for odd views).
// kAssist = true: `bits` holds tiling_divide_bits_kernel's answers; dynamic LDS = bits of every (side, lod) + the origin
// table + two frontier buffers.
// __syncthreads() also drains the wave's global stores (one memory counter): with the frontier in LDS nothing a pass stores to
// global memory is read back inside the kernel, so its barriers only have to order LDS — the store latency (~1.5 us per
// barrier) then stays off the chain of passes
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// kCull (the plain kernel only): refine_tiles drops a culled tile before the divide test — it is neither `divide` nor `fin`, it still
// counts as visited, and counters[kCntCulled] says how many there were.
template <bool kAssist, bool kCull>
__global__ __launch_bounds__(kThreads) void tiling_prepass_kernel(bt_view_state view, uint32_t capacity,
                                                                  bt_tile_coordinate* __restrict__ temporary_tiles,
                                                                  bt_tile_coordinate* __restrict__ final_tiles,
                                                                  bt_indirect* __restrict__ indirect,
                                                                  uint32_t* __restrict__ counters, const unsigned long long* __restrict__ bits, uint32_t assist_lods,
                                                                  const float* __restrict__ height, CullArgs<kCull> cull) {
    static_assert(!(kAssist && kCull), "the two-launch form has no culling variant");
    const float approximate_height = height ? *height : view.approximate_height;
    // The pass state (Parameters, types.wgsl:43-48) is uniform and kept in registers by every thread; only the
    // per-wave counts of a sweep go through LDS (double-buffered by sweep parity: ONE barrier per sweep).
    __shared__ uint32_t s_divide[2][kWaves], s_final[2][kWaves];
    __shared__ uint32_t s_culled[kCull ? 2 : 1][kWaves];
    uint32_t culled_total = 0;

    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const int N = int(capacity);

    // prepare_root (prepare_prepass.wgsl:4-23)
    int counter = -1, child_index = N - 1, final_index = 0;
    uint32_t tile_count = view.spherical ? 6u : 1u, visited = 0, sweep = 0;
    bool overflow = false;
    if (tid < tile_count) temporary_tiles[tid] = {tid, 0u, 0u, 0u};
    // kAssist: the answers of every window, the window origins and the LDS frontier
    extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];
    const uint32_t sides = view.spherical ? 6u : 1u;
    unsigned long long* s_bits = reinterpret_cast<unsigned long long*>(s_dyn);
    int2* s_origin = reinterpret_cast<int2*>(s_bits + size_t(sides) * kMaxLods * kWinWords);
    bt_tile_coordinate* s_tiles = reinterpret_cast<bt_tile_coordinate*>(s_origin + sides * kMaxLods);  // [2][kFrontierCap]
    if constexpr (kAssist) {
        for (uint32_t i = tid; i < sides * kMaxLods * kWinWords; i += kThreads)
            if ((i / kWinWords) % kMaxLods < assist_lods) s_bits[i] = bits[i];
        if (tid < sides * kMaxLods) {
            int ox, oy;
            window_origin(view, tid / kMaxLods, tid % kMaxLods, ox, oy);
            s_origin[tid] = int2{ox, oy};
        }
        if (tid < tile_count) s_tiles[tid] = {tid, 0u, 0u, 0u};
    }
    __syncthreads();

    for (uint32_t pass = 0; pass <= view.refinement_count; pass++) {
        const bool from_lds = kAssist && tile_count <= kFrontierCap;  // this pass's parents all sit in s_tiles[pass & 1]
        uint32_t pass_children = 0;                                    // children appended so far in this pass
        // refine_tiles (refine_tiles.wgsl:33-44), 1024 invocation ids per sweep
        for (uint32_t base = 0; base < tile_count; base += kThreads, sweep++) {
            const uint32_t id = base + tid;
            const bool active = id < tile_count;
            bt_tile_coordinate tile{};
            bool divide = false, culled = false;
            if (active) {
                const int parent_index = (N - 1) * (counter > 0 ? 1 : 0) - int(id) * counter;  // :9-11
                tile = from_lds ? s_tiles[(pass & 1u) * kFrontierCap + id] : temporary_tiles[parent_index];
                if constexpr (kAssist) {
                    const int2 o = s_origin[tile.side * kMaxLods + tile.lod];
                    const int bx = int(tile.x) - o.x, by = int(tile.y) - o.y;
                    if (bx >= 0 && by >= 0 && bx < int(kWinW) && by < int(kWinW) && tile.lod < assist_lods) {
                        const uint32_t b = uint32_t(by) * kWinW + uint32_t(bx);
                        divide = (s_bits[(tile.side * kMaxLods + tile.lod) * kWinWords + (b >> 6)] >> (b & 63u)) & 1ull;
                    } else {
                        divide = should_be_divided(view, tile, approximate_height);  // outside its window: the same function, in place
                    }
                } else if constexpr (kCull) {
                    culled = tile_culled(view, cull, tile);
                    divide = !culled && should_be_divided(view, tile, approximate_height);
                } else {
                    divide = should_be_divided(view, tile, approximate_height);
                }
            }
            const bool fin = active && !culled && !divide;
            const unsigned long long ballot_d = __ballot(divide), ballot_f = __ballot(fin);
            unsigned long long ballot_c = 0;
            if constexpr (kCull) ballot_c = __ballot(culled);
            if (lane == 0) {
                s_divide[sweep & 1u][wave] = uint32_t(__popcll(ballot_d));
                s_final[sweep & 1u][wave] = uint32_t(__popcll(ballot_f));
                if constexpr (kCull) s_culled[sweep & 1u][wave] = uint32_t(__popcll(ballot_c));
            }
            if constexpr (kAssist) lds_barrier();  // (the counts are LDS; this pass reads no global data it wrote)
            else __syncthreads();
            uint32_t before_d = 0, before_f = 0, total_d = 0, total_f = 0;
#pragma unroll
            for (uint32_t w = 0; w < kWaves; w++) {
                const uint32_t d = s_divide[sweep & 1u][w], f = s_final[sweep & 1u][w];
                before_d += w < wave ? d : 0u;
                before_f += w < wave ? f : 0u;
                total_d += d;
                total_f += f;
                if constexpr (kCull) culled_total += s_culled[sweep & 1u][w];
            }
            const unsigned long long below = (1ull << lane) - 1ull;
            if (divide) {  // subdivide (:24-31): 4 children at consecutive child_index() values
                const int rank = int(before_d + uint32_t(__popcll(ballot_d & below)));
#pragma unroll
                for (uint32_t i = 0; i < 4; i++) {
                    const int ci = child_index + counter * (4 * rank + int(i));
                    const bt_tile_coordinate child = {tile.side, tile.lod + 1u, (tile.x << 1) + (i & 1u), (tile.y << 1) + ((i >> 1) & 1u)};
                    if (ci >= 0 && ci < N) temporary_tiles[ci] = child;
                    if constexpr (kAssist) {  // the same order (append order = the next pass's id order)
                        const uint32_t li = pass_children + 4u * uint32_t(rank) + i;
                        if (li < kFrontierCap) s_tiles[((pass + 1u) & 1u) * kFrontierCap + li] = child;
                    }
                }
            }
            if (fin) {
                const int fi = final_index + int(before_f + uint32_t(__popcll(ballot_f & below)));
                if (fi < N) final_tiles[fi] = tile;
            }
            pass_children += 4u * total_d;
            child_index += counter * 4 * int(total_d);
            final_index += int(total_f);
            visited += min(kThreads, tile_count - base);
            // children may not run into the parents still to be read, nor finals past the buffer
            const int children_so_far = counter > 0 ? child_index : (N - 1 - child_index);
            if (children_so_far + int(tile_count) > N || final_index > N) overflow = true;
            if (overflow) break;  // uniform: the buffers are too small, stop before indices run wild
        }
        if (overflow || pass == view.refinement_count) break;
        // prepare_next (prepare_prepass.wgsl:25-36)
        if (counter == 1) {
            tile_count = uint32_t(child_index);
            child_index = N - 1;
        } else {
            tile_count = uint32_t(N - 1 - child_index);
            child_index = 0;
        }
        counter = -counter;
        if (tile_count == 0) break;  // nothing left to refine: the remaining passes of the reference are no-ops
        // orders this pass's child stores before the next pass's parent loads: LDS when the next pass reads its parents there
        if (kAssist && tile_count <= kFrontierCap) lds_barrier();
        else __syncthreads();
    }

    // prepare_render (prepare_prepass.wgsl:38-44)
    if (tid == 0) {
        *indirect = {view.vertices_per_tile * uint32_t(final_index), 1u, 0u, 0u};
        counters[0] = uint32_t(final_index);
        counters[1] = overflow ? 1u : 0u;
        counters[2] = visited;
        counters[3] = view.refinement_count + 1;
        if constexpr (kCull) counters[kCntCulled] = culled_total;
    }
}

}  // namespace
}  // namespace bt

using namespace bt;

namespace bt {
bt_ctx* tiling_prepass_ctx(const bt_tiling_prepass* t) { return t ? t->ctx : nullptr; }
void tiling_prepass_final(const bt_tiling_prepass* t, const bt_tile_coordinate** final_tiles, const uint32_t** final_count, uint32_t* capacity) {
    *final_tiles = t->final_tiles;
    *final_count = t->counters;  // counters[0]: what prepare_render counted (it may exceed the capacity after an overflow)
    *capacity = t->capacity;
}
}  // namespace bt

extern "C" {

bt_status bt_tiling_prepass_create(bt_ctx* ctx, uint32_t geometry_tile_count, bt_tiling_prepass** out) {
    if (!ctx || !out || geometry_tile_count < 8) return BT_ERR_INVALID_ARGUMENT;
    BT_HIP(hipSetDevice(ctx->device));
    bt_tiling_prepass* t = new bt_tiling_prepass();
    t->ctx = ctx;
    t->capacity = geometry_tile_count;
    // TerrainViewData::new: two buffers of geometry_tile_count TileCoordinates (terrain_view_bind_group.rs:130-142)
    hipError_t e = hipMalloc((void**)&t->temporary_tiles, sizeof(bt_tile_coordinate) * size_t(geometry_tile_count));
    if (e == hipSuccess) e = hipMalloc((void**)&t->final_tiles, sizeof(bt_tile_coordinate) * size_t(geometry_tile_count));
    if (e == hipSuccess) e = hipMalloc((void**)&t->indirect, sizeof(bt_indirect));
    if (e == hipSuccess) e = hipMalloc((void**)&t->counters, kCounterWords * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemsetAsync(t->counters, 0, kCounterWords * sizeof(uint32_t), ctx->stream);
    if (e != hipSuccess) {
        bt_tiling_prepass_destroy(t);
        return hip_fail(e, "tiling prepass buffers");
    }
    *out = t;
    return BT_OK;
}

void bt_tiling_prepass_destroy(bt_tiling_prepass* t) {
    if (!t) return;
    hipSetDevice(t->ctx->device);
    if (t->temporary_tiles) hipFree(t->temporary_tiles);
    if (t->final_tiles) hipFree(t->final_tiles);
    if (t->indirect) hipFree(t->indirect);
    if (t->counters) hipFree(t->counters);
    if (t->bits) hipFree(t->bits);
    delete t;
}

namespace {
// How deep can this view refine?  A tile of LOD l divides only within subdivision_distance / 2^l of the view, and nothing is
// closer to the view than its height over the (approximate) surface: beyond l = log2(subdivision_distance / height) no tile
// divides.  An ESTIMATE (f32 on the host, the surface taken as the unit sphere / plane of the mesh transform): it only
// decides how many LODs get their bits up front — anything deeper is evaluated in place, so it can cost time, never change
// the result.
uint32_t estimate_lods(const bt_view_state* view) {
    uint32_t lods = kMaxLods;
    const float* m = view->world_from_local;
    const float* it = view->local_from_world_transpose;
    const float d[3] = {view->world_position[0] - m[9], view->world_position[1] - m[10], view->world_position[2] - m[11]};
    float local[3];
    for (int i = 0; i < 3; i++) local[i] = it[3 * i] * d[0] + it[3 * i + 1] * d[1] + it[3 * i + 2] * d[2];
    const float sx = sqrtf(m[0] * m[0] + m[1] * m[1] + m[2] * m[2]), sy = sqrtf(m[3] * m[3] + m[4] * m[4] + m[5] * m[5]);
    const float height = view->spherical ? (sqrtf(local[0] * local[0] + local[1] * local[1] + local[2] * local[2]) - 1.0f) * std::min(sx, sy) : local[1] * sy;
    const float clearance = 0.5f * fabsf(height - view->approximate_height);
    if (clearance > 0.0f && view->subdivision_distance > 0.0f && std::isfinite(clearance)) {
        const float deepest = log2f(view->subdivision_distance / clearance);
        if (deepest < 30.0f) lods = uint32_t(std::max(0.0f, ceilf(deepest))) + 2u;
    }
    return std::min(std::min(lods, kMaxLods), view->refinement_count + 1u);
}

bt_status prepass_check(bt_tiling_prepass* t, const bt_view_state* view) {
    if (!t || !view) return BT_ERR_INVALID_ARGUMENT;
    if (view->refinement_count > 31 || view->origin_lod > 31) {
        set_error("refinement_count %u / origin_lod %u > 31 (tile x/y are u32)", view->refinement_count, view->origin_lod);
        return BT_ERR_INVALID_ARGUMENT;
    }
    BT_HIP(hipSetDevice(t->ctx->device));
    if (!t->bits) {
        BT_HIP(hipMalloc((void**)&t->bits, 2 * kBitsPlane * sizeof(unsigned long long)));  // divide bits, cull bits
        BT_HIP(hipMemsetAsync(t->bits, 0, 2 * kBitsPlane * sizeof(unsigned long long), t->ctx->stream));
        BT_HIP(hipFuncSetAttribute((const void*)tiling_prepass_kernel<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, int(6 * kMaxLods * (kWinWords * 8 + 8) + 2 * kFrontierCap * 16)));
    }
    return BT_OK;
}
}  // namespace

}  // extern "C"

namespace bt {
// form 0: two launches — every divide test that can matter (independent, chip-wide), then the ordered schedule over the bits;
//         shallow views (few hundred tiles) take the plain kernel, which saves them the second launch
// form 1: the unordered form — the same SET of final tiles and the same indirect arguments, in whatever order the waves arrive
//         (the reference's own order is the arrival order of its atomics); two chip-wide launches, no pass chain, flat ~10 us
//         whatever the frame; temporary_tiles is not written
// form 2: the plain form — one launch, every divide test evaluated inside the pass that needs it; same list, same order as form 0
bt_status tiling_prepass_enqueue(bt_tiling_prepass* t, const bt_view_state* view, const float* device_height, uint32_t form) {
    if (!t || !view) return BT_ERR_INVALID_ARGUMENT;
    if (view->refinement_count > 31 || view->origin_lod > 31) {
        set_error("refinement_count %u / origin_lod %u > 31 (tile x/y are u32)", view->refinement_count, view->origin_lod);
        return BT_ERR_INVALID_ARGUMENT;
    }
    BT_HIP(hipSetDevice(t->ctx->device));
    const uint32_t capacity = std::min(t->capacity, view->geometry_tile_count ? view->geometry_tile_count : t->capacity);
    const uint32_t sides = view->spherical ? 6u : 1u;
    // (with the height on the device the estimate works from the host's copy, one frame old: it decides how many LODs get their
    // bits up front and can only cost time)
    // culling (bt_tiling_prepass_set_culling): no planes cull nothing, and the kernels without the test give exactly that — unless a
    // horizon view is set (bt_tiling_prepass_set_horizon), whose test reads the culling state's heights and table
    if (t->horizon_set && (!t->cull_set || !view->spherical)) {
        set_error("tiling prepass horizon culling: %s", !t->cull_set ? "culling is not set (the horizon test reads its heights and table)" : "a planar view has no horizon");
        return BT_ERR_INVALID_ARGUMENT;
    }
    const bool cull = t->cull_set && (t->cull.plane_count > 0 || t->horizon_set);
    CullArgs<true> ca{};
    if (cull) {
        if (t->bounds && t->bounds->sides != sides) {
            set_error("tiling prepass culling: a height-bounds table of %u side(s) for a view of %u", t->bounds->sides, sides);
            return BT_ERR_INVALID_ARGUMENT;
        }
        ca.cull = t->cull;
        ca.table = t->bounds ? t->bounds->table : nullptr;
        ca.levels = t->bounds ? t->bounds->levels : 0u;
        ca.sides = sides;
        ca.horizon_on = t->horizon_set ? 1u : 0u;
        if (t->horizon_set) ca.horizon = t->horizon;
    }
    if (cull && form != 1u) {  // both ordered forms: the plain kernel (the same list in the same order)
        tiling_prepass_kernel<false, true><<<1, kThreads, 0, t->ctx->stream>>>(*view, capacity, t->temporary_tiles, t->final_tiles, t->indirect, t->counters, nullptr, 0u, device_height, ca);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(e, "tiling_prepass_kernel");
        t->unordered = false;
        t->culled_run = true;
        return BT_OK;
    }
    const uint32_t lods = form == 2u ? 0u : estimate_lods(view);
    if (form == 2u || (form == 0u && lods < 12u)) {
        tiling_prepass_kernel<false, false><<<1, kThreads, 0, t->ctx->stream>>>(*view, capacity, t->temporary_tiles, t->final_tiles, t->indirect, t->counters, nullptr, 0u, device_height, CullArgs<false>{});
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(e, "tiling_prepass_kernel");
        t->unordered = false;
        t->culled_run = false;
        return BT_OK;
    }
    if (bt_status s = prepass_check(t, view)) return s;
    if (form == 0u) {
        const size_t lds = size_t(sides) * kMaxLods * (kWinWords * sizeof(unsigned long long) + sizeof(int2)) + 2 * size_t(kFrontierCap) * sizeof(bt_tile_coordinate);
        tiling_divide_bits_kernel<false><<<sides * lods * kWinChunks, 256, 0, t->ctx->stream>>>(*view, lods, kWinK, t->bits, nullptr, nullptr, device_height, CullArgs<false>{});
        tiling_prepass_kernel<true, false><<<1, kThreads, lds, t->ctx->stream>>>(*view, capacity, t->temporary_tiles, t->final_tiles, t->indirect, t->counters, t->bits, lods, device_height, CullArgs<false>{});
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(e, "tiling_prepass_kernel");
        t->unordered = false;
        t->culled_run = false;
        return BT_OK;
    }
    const int radius = t->window ? t->window : kWinK;
    const uint32_t W = 2u * uint32_t(radius) + 1u, chunks = (W * W + 255u) / 256u;
    if (cull) {
        tiling_divide_bits_kernel<true><<<sides * lods * chunks, 256, 0, t->ctx->stream>>>(*view, lods, radius, t->bits, t->counters, t->indirect, device_height, ca);
        tiling_collect_kernel<true><<<sides * lods * chunks, 256, 0, t->ctx->stream>>>(*view, lods, radius, capacity, t->bits, t->final_tiles, t->indirect, t->counters, device_height, ca);
    } else {
        tiling_divide_bits_kernel<false><<<sides * lods * chunks, 256, 0, t->ctx->stream>>>(*view, lods, radius, t->bits, t->counters, t->indirect, device_height, CullArgs<false>{});
        tiling_collect_kernel<false><<<sides * lods * chunks, 256, 0, t->ctx->stream>>>(*view, lods, radius, capacity, t->bits, t->final_tiles, t->indirect, t->counters, device_height, CullArgs<false>{});
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "tiling_collect_kernel");
    t->unordered = true;
    t->culled_run = cull;
    t->unordered_capacity = capacity;
    return BT_OK;
}
}  // namespace bt

extern "C" {

bt_status bt_tiling_prepass_run(bt_tiling_prepass* t, const bt_view_state* view) { return bt::tiling_prepass_enqueue(t, view, nullptr, 0u); }
bt_status bt_tiling_prepass_run_unordered(bt_tiling_prepass* t, const bt_view_state* view) { return bt::tiling_prepass_enqueue(t, view, nullptr, 1u); }
bt_status bt_tiling_prepass_run_plain(bt_tiling_prepass* t, const bt_view_state* view) { return bt::tiling_prepass_enqueue(t, view, nullptr, 2u); }

bt_status bt_tiling_prepass_set_window(bt_tiling_prepass* t, uint32_t radius) {
    if (!t || radius > uint32_t(kWinK)) return BT_ERR_INVALID_ARGUMENT;
    t->window = int(radius);
    return BT_OK;
}

bt_status bt_tiling_prepass_set_culling(bt_tiling_prepass* t, const bt_cull_view* cull, const bt_height_bounds* bounds) {
    if (!t) {
        set_error("bt_tiling_prepass_set_culling: NULL prepass");
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (!cull) {
        t->cull_set = false;
        t->bounds = nullptr;
        return BT_OK;
    }
    if (cull->plane_count > 5u) {
        set_error("bt_tiling_prepass_set_culling: plane_count %u > 5", cull->plane_count);
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (!(cull->margin >= 0.0f) || !std::isfinite(cull->margin)) {
        set_error("bt_tiling_prepass_set_culling: margin %g (finite, >= 0)", double(cull->margin));
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (bounds && (!bounds->table || (bounds->sides != 1u && bounds->sides != 6u) || bounds->levels < 1u || bounds->levels > BT_HEIGHT_BOUNDS_MAX_LEVELS)) {
        set_error("bt_tiling_prepass_set_culling: not a height-bounds table");
        return BT_ERR_INVALID_ARGUMENT;
    }
    t->cull = *cull;
    t->bounds = bounds;
    t->cull_set = true;
    return BT_OK;
}

bt_status bt_tiling_prepass_set_horizon(bt_tiling_prepass* t, const bt_horizon_view* horizon) {
    if (!t) {
        set_error("bt_tiling_prepass_set_horizon: NULL prepass");
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (!horizon) {
        t->horizon_set = false;
        return BT_OK;
    }
    const bt_horizon_view& h = *horizon;
    if (!std::isfinite(h.eye[0]) || !std::isfinite(h.eye[1]) || !std::isfinite(h.eye[2]) || !std::isfinite(h.vh) || !std::isfinite(h.occluder_radius) ||
        !std::isfinite(h.margin)) {
        set_error("bt_tiling_prepass_set_horizon: a non-finite field");
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (!(h.occluder_radius > 0.0f && h.occluder_radius <= 1.0f) || !(h.margin >= 0.0f)) {
        set_error("bt_tiling_prepass_set_horizon: occluder_radius %g (in (0, 1]), margin %g (>= 0)", double(h.occluder_radius), double(h.margin));
        return BT_ERR_INVALID_ARGUMENT;
    }
    t->horizon = h;
    t->horizon_set = true;
    return BT_OK;
}

bt_status bt_tiling_prepass_cull_stats(bt_tiling_prepass* t, uint32_t* visited, uint32_t* culled) {
    if (!t) {
        set_error("bt_tiling_prepass_cull_stats: NULL prepass");
        return BT_ERR_INVALID_ARGUMENT;
    }
    uint32_t counters[kCounterWords] = {0};
    BT_HIP(hipSetDevice(t->ctx->device));
    BT_HIP(hipMemcpyAsync(counters, t->counters, sizeof counters, hipMemcpyDeviceToHost, t->ctx->stream));
    BT_HIP(hipStreamSynchronize(t->ctx->stream));
    uint32_t v = counters[2];
    if (t->unordered) {
        v = 0;
        for (uint32_t l = 0; l < kMaxLods; l++) v += counters[kCntVisited + l];
    }
    if (visited) *visited = v;
    if (culled) *culled = t->culled_run ? counters[kCntCulled] : 0u;
    return BT_OK;
}

bt_status bt_tiling_prepass_buffers(const bt_tiling_prepass* t, void** final_tiles, void** indirect) {
    if (!t) return BT_ERR_INVALID_ARGUMENT;
    if (final_tiles) *final_tiles = t->final_tiles;
    if (indirect) *indirect = t->indirect;
    return BT_OK;
}

bt_status bt_tiling_prepass_read(bt_tiling_prepass* t, bt_tile_coordinate* out, uint32_t cap, uint32_t* count, bt_indirect* indirect) {
    if (!t || !count) return BT_ERR_INVALID_ARGUMENT;
    uint32_t counters[kCounterWords] = {0};
    BT_HIP(hipMemcpyAsync(counters, t->counters, sizeof counters, hipMemcpyDeviceToHost, t->ctx->stream));
    if (indirect) BT_HIP(hipMemcpyAsync(indirect, t->indirect, sizeof(bt_indirect), hipMemcpyDeviceToHost, t->ctx->stream));
    BT_HIP(hipStreamSynchronize(t->ctx->stream));
    if (t->unordered) {  // the reference's buffers: a pass needs its parents + the children appended, the final list its tiles
        counters[1] = counters[0] > t->unordered_capacity;
        for (uint32_t l = 0; l < kMaxLods; l++)
            if (uint64_t(counters[kCntVisited + l]) + 4ull * counters[kCntDivide + l] > t->unordered_capacity) counters[1] = 1;
    }
    *count = counters[0];
    if (counters[1]) {
        set_error("tiling prepass overflowed its %u-entry tile buffers", t->capacity);
        return BT_ERR_OVERFLOW;
    }
    if (out && counters[0]) {
        const uint32_t n = std::min(cap, counters[0]);
        BT_HIP(hipMemcpyAsync(out, t->final_tiles, sizeof(bt_tile_coordinate) * size_t(n), hipMemcpyDeviceToHost, t->ctx->stream));
        BT_HIP(hipStreamSynchronize(t->ctx->stream));
    }
    return BT_OK;
}

}  // extern "C"

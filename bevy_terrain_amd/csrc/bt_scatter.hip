// bt_atlas_scatter_instances (include/bevy_terrain_amd.h, SCATTER): vegetation placement.  For every centre texel (a cell) of the listed
// tiles of an R16 attachment H the kernels decide, from a hash of the cell's mosaic position and up to eight height-and-slope rules,
// whether the cell places an instance and of which rule, and write the placing cells' instances (f64 world position, world normal,
// scale, yaw) as one ordered list.  The argument checks are in bt_edit.cpp beside SPLAT's; scatter_run below lays out the scratch and
// runs, per chunk of the list, three launches with no host round trip between them:
//
//   decide  grid = (tiles of the chunk, blocks of kScatterRows rows); the splat kernel's shape: a wave takes a row at a time, a lane a
//           cell, a row wider than 64 cells further trips, and the window of H (rows and columns of the block plus `halo` on every side)
//           is staged in LDS with the splat kernel's window test and HBM fallback.  One byte per cell goes to scratch (the rule, kNone,
//           kNoData) and one record per block: the cells placed per rule and the no-data cells, counted by ballot and popcount per wave
//           and summed through LDS.
//   scan    one workgroup: the block records -> exclusive offsets of the blocks in the list, the first instance of every tile, and
//           the running totals (ScatterState), which carry from chunk to chunk on the device.
//   emit    the same grid.  A placing lane's rank is its block's offset + the placing cells of the rows before it in the block + those
//           of the trips before it in its row + the lower lanes of its own ballot (mbcnt).  Only placing lanes with a rank below the
//           list's capacity recompute uv, h and s (their texels come from HBM / L2: at vegetation densities a window would be staged for
//           a few lanes) and evaluate the f64 position and the normal; each writes its 56-byte record.
//
// No atomic decides a position: the list's order is the definition's and its bytes are the same from run to run.
// The rules lie in the scratch and are indexed by the (unrolled) loop counter only: wave-uniform scalar loads.
// Arithmetic: IEEE binary32, one rounding per written operation (-ffp-contract=off), `/` is the correctly rounded division; f64 where
// the header says f64 (bt_model.hpp).
#include "bt_band_device.hpp"
#include "bt_internal.hpp"
#include "bt_model.hpp"
#include "bt_normal_device.hpp"

namespace bt {

namespace {

constexpr uint32_t kScatterThreads = 256;
constexpr uint32_t kScatterRows = 16;        // rows of a tile per workgroup: four per wave (the splat kernel's)
constexpr uint32_t kScatterColumns = 64;     // columns of a chunk of a row: one trip of the lanes
constexpr uint32_t kScatterMaxHalo = 8;      // a wider halo is not staged (the splat kernel's)
constexpr uint32_t kScatterChunkTiles = 1024;          // tiles of one chunk of the list at most: grid.x of decide and emit
constexpr uint64_t kScatterChunkCells = 64ull << 20;   // and cells: the bytes of the cell scratch
constexpr uint32_t kScanThreads = 256;
constexpr uint32_t kScanItems = kScanThreads;          // blocks per trip of the scan: one per thread
constexpr uint32_t kBlockWords = BT_SCATTER_MAX_RULES + 1u;  // a block's record: cells placed per rule, then its no-data cells
constexpr uint32_t kNone = 0xFFu, kNoData = 0xFEu;     // the cell bytes that are not a rule
constexpr uint32_t kWindowRows = kScatterRows + 2u * kScatterMaxHalo, kWindowColumns = kScatterColumns + 2u * kScatterMaxHalo;

struct ScatterParams {
    AttachmentMeta m;  // of H; M has its texture_size and border_size (the entry point refuses anything else)
    NormalModel nm;
    const uint16_t* heights;
    const uint32_t* mask;  // level 0 of M, or nullptr
    uint32_t halo, rule_count, seed;
    float jitter;
};

// the running totals of one call, on the device: the scan of a chunk starts from them and leaves them for the next
struct ScatterState {
    uint64_t total, no_data;
    uint64_t per_rule[BT_SCATTER_MAX_RULES];
};

// step 1
__device__ __forceinline__ uint32_t mix(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
__device__ __forceinline__ uint32_t draw(uint32_t key, uint32_t n) { return mix(key + n * 0x9E3779B9u); }
__device__ __forceinline__ float unit(uint32_t r) { return float(r >> 8) * 0x1p-24f; }  // exact, in [0, 1)

// steps 1 and 2 of cell (i, j) of a tile: its key, its mosaic texel and its uv
struct Cell {
    uint32_t key, gx, gy;
    float uv[2];
};
__device__ __forceinline__ Cell cell_of(const ScatterParams& P, const ScatterTile& t, uint32_t i, uint32_t j) {
    const uint32_t c = P.m.center_size;
    Cell cell;
    cell.gx = t.x * c + i, cell.gy = t.y * c + j;
    cell.key = mix(mix(mix(P.seed ^ (t.side << 8 | t.lod)) ^ cell.gx) ^ cell.gy);
    const float ax = 0.5f + (unit(draw(cell.key, 1u)) - 0.5f) * P.jitter;
    const float ay = 0.5f + (unit(draw(cell.key, 2u)) - 0.5f) * P.jitter;
    cell.uv[0] = (float(i) + ax) / float(c);
    cell.uv[1] = (float(j) + ay) / float(c);
    return cell;
}

// the centre tap (u_x, u_y) of TILE NORMAL: its bilinear value; false when one of its four texels is 0 (step 3)
template <typename Fetch>
__device__ __forceinline__ bool centre_tap(const NormalTaps& tp, const TapSplit& sp, Fetch fetch, float& value) {
    uint32_t raw[2][2];
#pragma unroll
    for (int x = 0; x < 2; x++)
#pragma unroll
        for (int y = 0; y < 2; y++) raw[x][y] = fetch(texel_clamp(sp.first[0][1] + x, tp.size), texel_clamp(sp.first[1][1] + y, tp.size));
    value = bilerp(unorm16_to_float(raw[0][0]), unorm16_to_float(raw[0][1]), unorm16_to_float(raw[1][0]), unorm16_to_float(raw[1][1]), sp.rem[0][1], sp.rem[1][1]);
    return raw[0][0] != 0u && raw[0][1] != 0u && raw[1][0] != 0u && raw[1][1] != 0u;
}

// steps 5 and 6 for a data cell: its height, the z of its tile normal, the dword of M in its place, u -> the rule, or kNone
__device__ __forceinline__ uint32_t select_rule(const ScatterParams& P, const bt_scatter_rule* __restrict__ rules, float h, float sz, uint32_t mask_texel, float u) {
    const float steep = 1.0f - sz;
    float A = 0.0f;
    uint32_t code = kNone;
#pragma unroll
    for (uint32_t k = 0; k < BT_SCATTER_MAX_RULES; k++) {
        if (k >= P.rule_count) break;
        const bt_scatter_rule rule = rules[k];
        // (density * 0) * band is 0 for every band: a wave none of whose lanes is inside the rule's heights skips its other band
        const float ph = rule.density * band(h, rule.height_lo, rule.height_hi, rule.height_fade);
        float p = 0.0f;
        if (__builtin_amdgcn_ballot_w64(ph != 0.0f) != 0ull) {
            p = ph * band(steep, rule.steep_lo, rule.steep_hi, rule.steep_fade);
            const float m = rule.mask_channel == BT_SCATTER_NO_MASK ? 1.0f : float((mask_texel >> (8u * (rule.mask_channel & 3u))) & 0xFFu) / 255.0f;
            p = p * m;
        }
        A = A + p;  // (0 + p_0 is p_0)
        if (code == kNone && u < A) code = k;
    }
    return code;
}

__global__ __launch_bounds__(kScatterThreads) void scatter_decide_kernel(ScatterParams P, const bt_scatter_rule* __restrict__ rules, const ScatterTile* __restrict__ tiles,
                                                                         uint8_t* __restrict__ codes, uint32_t* __restrict__ block_words) {
    __shared__ uint16_t window[kWindowRows][kWindowColumns];
    __shared__ uint32_t wave_words[kScatterThreads / 64u][kBlockWords];
    const ScatterTile t = tiles[blockIdx.x];
    const uint32_t T = P.m.texture_size, b = P.m.border_size, c = P.m.center_size;
    const uint32_t y_begin = blockIdx.y * kScatterRows;  // (< c: grid.y is the blocks of c rows)
    const uint32_t y_end = min(y_begin + kScatterRows - 1u, c - 1u);
    const uint16_t* __restrict__ tile = P.heights + uint64_t(t.layer) * T * T;
    const uint32_t* __restrict__ mask = P.mask ? P.mask + uint64_t(t.layer) * T * T : nullptr;
    uint8_t* __restrict__ out = codes + uint64_t(blockIdx.x) * c * c;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const NormalTaps tp = normal_taps(P.m);
    const float dist = normal_dist(P.m, P.nm, t.lod);
    const bool windowed = P.halo <= kScatterMaxHalo;
    // the window's rows: texture rows [wy0, wy0 + wrows), at most kScatterRows + 2 * halo of them, inside the layer
    const uint32_t wy0 = windowed && b + y_begin > P.halo ? b + y_begin - P.halo : 0u;
    const uint32_t wrows = windowed ? min(b + y_end + P.halo, T - 1u) - wy0 + 1u : 0u;
    const uint32_t px0 = b, px1 = b + c - 1u;
    uint32_t placed[BT_SCATTER_MAX_RULES] = {}, no_data = 0u;  // of this wave's rows: wave-uniform
    for (uint32_t chunk = px0; chunk <= px1; chunk += kScatterColumns) {
        const uint32_t chunk_last = min(chunk + kScatterColumns - 1u, px1);
        // its columns: texture columns [wx0, wx0 + wcolumns), at most kScatterColumns + 2 * halo
        const uint32_t wx0 = windowed && chunk > P.halo ? chunk - P.halo : 0u;
        const uint32_t wcolumns = windowed ? min(chunk_last + P.halo, T - 1u) - wx0 + 1u : 0u;
        if (windowed) {
            if (chunk != px0) __syncthreads();  // the window of the previous chunk has been read
            for (uint32_t r = wave; r < wrows; r += kScatterThreads / 64u) {
                const uint16_t* row = tile + uint64_t(wy0 + r) * T + wx0;
                for (uint32_t i = lane; i < wcolumns; i += 64u) window[r][i] = row[i];
            }
            __syncthreads();
        }
        const uint32_t px = chunk + lane;
        const bool in_row = px <= chunk_last;
        const uint32_t i = px - b;
        for (uint32_t y = y_begin + wave; y <= y_end; y += kScatterThreads / 64u) {
            const uint32_t py = b + y;
            uint32_t code = kNone;  // (a lane beyond the row counts nowhere)
            if (in_row) {
                const uint32_t raw = windowed ? uint32_t(window[py - wy0][px - wx0]) : uint32_t(tile[uint64_t(py) * T + px]);
                code = kNoData;
                if (raw != 0u) {
                    const Cell cell = cell_of(P, t, i, y);
                    const TapSplit sp = tap_split(tp, cell.uv);
                    // ONE window test per cell: the columns and rows its taps touch, after the clamp (first[a][0] <= [1] <= [2])
                    const uint32_t lo_x = texel_clamp(sp.first[0][0], T), hi_x = texel_clamp(sp.first[0][2] + 1, T);
                    const uint32_t lo_y = texel_clamp(sp.first[1][0], T), hi_y = texel_clamp(sp.first[1][2] + 1, T);
                    float v;
                    F3 s = {0.0f, 0.0f, 1.0f};
                    bool data;
                    if (lo_x >= wx0 && hi_x - wx0 < wcolumns && lo_y >= wy0 && hi_y - wy0 < wrows) {
                        auto fetch = [&](uint32_t x, uint32_t yy) -> uint32_t { return window[yy - wy0][x - wx0]; };
                        data = centre_tap(tp, sp, fetch, v);
                        if (data) s = tile_normal(tp, P.nm, dist, sp, fetch);
                    } else {  // a tap outside the window (or no window): the layer in HBM
                        auto fetch = [&](uint32_t x, uint32_t yy) -> uint32_t { return tile[uint64_t(yy) * T + x]; };
                        data = centre_tap(tp, sp, fetch, v);
                        if (data) s = tile_normal(tp, P.nm, dist, sp, fetch);
                    }
                    if (data) {
                        const float h = P.nm.min_height + (P.nm.max_height - P.nm.min_height) * v;
                        const uint32_t mask_texel = mask ? mask[uint64_t(py) * T + px] : 0u;
                        code = select_rule(P, rules, h, s.z, mask_texel, unit(draw(cell.key, 0u)));
                    }
                }
                out[uint64_t(y) * c + i] = uint8_t(code);
            }
            no_data += uint32_t(__builtin_popcountll(__builtin_amdgcn_ballot_w64(code == kNoData)));
#pragma unroll
            for (uint32_t k = 0; k < BT_SCATTER_MAX_RULES; k++) {
                if (k >= P.rule_count) break;
                placed[k] += uint32_t(__builtin_popcountll(__builtin_amdgcn_ballot_w64(code == k)));
            }
        }
    }
    // ONE record per block, through LDS
    if (lane == 0u) {
#pragma unroll
        for (uint32_t k = 0; k < BT_SCATTER_MAX_RULES; k++) wave_words[wave][k] = placed[k];
        wave_words[wave][BT_SCATTER_MAX_RULES] = no_data;
    }
    __syncthreads();
    if (threadIdx.x < kBlockWords) {
        uint32_t sum = 0u;
        for (uint32_t w = 0; w < kScatterThreads / 64u; w++) sum += wave_words[w][threadIdx.x];
        block_words[(uint64_t(blockIdx.x) * gridDim.y + blockIdx.y) * kBlockWords + threadIdx.x] = sum;
    }
}

// blocks: those of the chunk, tile by tile; first: the entries of the chunk's tiles
__global__ __launch_bounds__(kScanThreads) void scatter_scan_kernel(const uint32_t* __restrict__ block_words, uint32_t blocks, uint32_t blocks_per_tile,
                                                                    uint64_t* __restrict__ block_offsets, uint64_t* __restrict__ first, ScatterState* state) {
    __shared__ uint32_t wave_sum[kScanThreads / 64u];
    __shared__ uint64_t wave_totals[kScanThreads / 64u][kBlockWords];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t running = state->total;  // (read by every thread before the first barrier, written behind the last)
    uint64_t mine[kBlockWords] = {};  // this thread's blocks, word by word
    for (uint32_t base = 0; base < blocks; base += kScanItems) {
        const uint32_t block = base + threadIdx.x;
        uint32_t n = 0u;
        if (block < blocks) {
#pragma unroll
            for (uint32_t k = 0; k < kBlockWords; k++) {
                const uint32_t w = block_words[uint64_t(block) * kBlockWords + k];
                mine[k] += w;
                if (k < BT_SCATTER_MAX_RULES) n += w;
            }
        }
        uint32_t inclusive = n;  // over the wave
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t below = __shfl_up(inclusive, d);
            if (lane >= d) inclusive += below;
        }
        if (lane == 63u) wave_sum[wave] = inclusive;
        __syncthreads();
        uint32_t before = 0u, trip = 0u;
        for (uint32_t w = 0; w < kScanThreads / 64u; w++) {
            const uint32_t s = wave_sum[w];
            if (w < wave) before += s;
            trip += s;
        }
        if (block < blocks) {
            const uint64_t offset = running + before + (inclusive - n);
            block_offsets[block] = offset;
            if (block % blocks_per_tile == 0u) first[block / blocks_per_tile] = offset;
        }
        running += trip;
        __syncthreads();  // wave_sum has been read
    }
#pragma unroll
    for (uint32_t k = 0; k < kBlockWords; k++) {
        uint64_t v = mine[k];
#pragma unroll
        for (uint32_t d = 32u; d >= 1u; d >>= 1) v += __shfl_xor(v, d);
        if (lane == 0u) wave_totals[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < kBlockWords) {
        uint64_t sum = 0u;
        for (uint32_t w = 0; w < kScanThreads / 64u; w++) sum += wave_totals[w][threadIdx.x];
        if (threadIdx.x < BT_SCATTER_MAX_RULES) state->per_rule[threadIdx.x] += sum;
        else state->no_data += sum;
    }
    if (threadIdx.x == 0u) state->total = running;
}

// step 7 for a placing cell
__device__ __forceinline__ bt_scatter_instance instance_of(const ScatterParams& P, const model::Model& M, const bt_scatter_rule& r, const ScatterTile& t, const uint16_t* __restrict__ tile, const NormalTaps& tp,
                                                           float dist, uint32_t i, uint32_t j, uint32_t rule) {
    using namespace model;
    const uint32_t T = P.m.texture_size;
    const Cell cell = cell_of(P, t, i, j);
    const TapSplit sp = tap_split(tp, cell.uv);
    auto fetch = [&](uint32_t x, uint32_t yy) -> uint32_t { return tile[uint64_t(yy) * T + x]; };
    float v;
    (void)centre_tap(tp, sp, fetch, v);
    const float h = P.nm.min_height + (P.nm.max_height - P.nm.min_height) * v;
    const F3 s = tile_normal(tp, P.nm, dist, sp, fetch);
    const double tiles_per_side = double(1u << t.lod);
    const Coordinate co = {t.side, {(double(t.x) + double(cell.uv[0])) / tiles_per_side, (double(t.y) + double(cell.uv[1])) / tiles_per_side}};
    const V3 local = coordinate_local_position(co, M);
    const V3 p = position_local_to_world(M, local, double(h));  // == coordinate_world_position(co, model, h)
    // WORLD NORMAL steps 2 - 4 with the unit local of the position and the tile's side as the face
    F3 W = {s.x, s.z, s.y};
    if (is_spherical(M)) {
        const V3 vn = normalize3({local.x / M.scale.x, local.y / M.scale.y, local.z / M.scale.z});
        const F3 N = norm3f({float(vn.x), float(vn.y), float(vn.z)});
        const uint32_t pair = t.side >> 1;  // FACE_UP (attachments.wgsl:55-62)
        const F3 face_up = {pair == 2u ? -1.0f : 0.0f, pair == 0u ? 1.0f : 0.0f, pair == 1u ? -1.0f : 0.0f};
        const F3 tan = cross3f(face_up, N);
        const F3 bit = cross3f(N, tan);
        W = {(tan.x * s.x + bit.x * s.y) + N.x * s.z, (tan.y * s.x + bit.y * s.y) + N.y * s.z, (tan.z * s.x + bit.z * s.y) + N.z * s.z};
    }
    const F3 n = norm3f(W);
    bt_scatter_instance inst;
    inst.position[0] = p.x, inst.position[1] = p.y, inst.position[2] = p.z;
    inst.normal[0] = n.x, inst.normal[1] = n.y, inst.normal[2] = n.z;
    inst.scale = r.scale_lo + (r.scale_hi - r.scale_lo) * unit(draw(cell.key, 3u));
    inst.yaw = 6.2831855f * unit(draw(cell.key, 4u));
    inst.rule = rule;
    inst.cell[0] = cell.gx, inst.cell[1] = cell.gy;
    return inst;
}

// list: the call's device list of list_cap records; block_offsets: of the chunk's blocks, as the scan left them
__global__ __launch_bounds__(kScatterThreads) void scatter_emit_kernel(ScatterParams P, model::Model M, const bt_scatter_rule* __restrict__ rules,
                                                                       const ScatterTile* __restrict__ tiles, const uint8_t* __restrict__ codes,
                                                                       const uint64_t* __restrict__ block_offsets, bt_scatter_instance* __restrict__ list,
                                                                       uint64_t list_cap) {
    __shared__ uint32_t row_count[kScatterRows];
    const uint64_t base = block_offsets[uint64_t(blockIdx.x) * gridDim.y + blockIdx.y];
    if (base >= list_cap) return;  // (the whole workgroup: nothing of this block fits, and no barrier is skipped by a part of it)
    const ScatterTile t = tiles[blockIdx.x];
    const uint32_t T = P.m.texture_size, c = P.m.center_size;
    const uint32_t y_begin = blockIdx.y * kScatterRows;
    const uint32_t rows = min(kScatterRows, c - y_begin);
    const uint16_t* __restrict__ tile = P.heights + uint64_t(t.layer) * T * T;
    const uint8_t* __restrict__ in = codes + uint64_t(blockIdx.x) * c * c + uint64_t(y_begin) * c;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    // the placing cells of each row of the block
    for (uint32_t r = wave; r < rows; r += kScatterThreads / 64u) {
        uint32_t n = 0u;
        for (uint32_t i0 = 0; i0 < c; i0 += kScatterColumns) {
            const uint32_t i = i0 + lane;
            const bool placing = i < c && in[uint64_t(r) * c + i] < kNoData;
            n += uint32_t(__builtin_popcountll(__builtin_amdgcn_ballot_w64(placing)));
        }
        if (lane == 0u) row_count[r] = n;
    }
    __syncthreads();
    const NormalTaps tp = normal_taps(P.m);
    const float dist = normal_dist(P.m, P.nm, t.lod);
    for (uint32_t r = wave; r < rows; r += kScatterThreads / 64u) {
        uint64_t next = base;  // the rank of the row's next placing cell
        for (uint32_t q = 0; q < r; q++) next += row_count[q];
        for (uint32_t i0 = 0; i0 < c; i0 += kScatterColumns) {
            const uint32_t i = i0 + lane;
            const uint32_t code = i < c ? uint32_t(in[uint64_t(r) * c + i]) : kNone;
            const bool placing = code < kNoData;
            const uint64_t ballot = __builtin_amdgcn_ballot_w64(placing);
            const uint64_t rank = next + __builtin_amdgcn_mbcnt_hi(uint32_t(ballot >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(ballot), 0u));
            next += uint32_t(__builtin_popcountll(ballot));
            if (placing && rank < list_cap) list[rank] = instance_of(P, M, rules[code], t, tile, tp, dist, i, y_begin + r, code);
        }
    }
}

}  // namespace

bt_status scatter_run(bt_ctx* ctx, const ScatterJob& job, const std::vector<ScatterTile>& tiles, bt_scatter_instance* out, uint64_t cap, uint64_t* out_first,
                      bt_scatter_stats* stats) {
    const char* who = "bt_atlas_scatter_instances";
    const uint64_t count = tiles.size();
    const uint32_t c = job.meta.center_size;
    const uint64_t tile_cells = uint64_t(c) * c;
    const uint32_t blocks_per_tile = (c + kScatterRows - 1u) / kScatterRows;
    const uint64_t chunk = std::min<uint64_t>({count, kScatterChunkTiles, std::max<uint64_t>(1u, kScatterChunkCells / tile_cells)});
    const uint64_t list_cap = std::min<uint64_t>(cap, count * tile_cells);
    // the scratch: the state, the rules, the tile list, the firsts; then one chunk's block records, block offsets and cell bytes; then the list
    const uint64_t rules_at = align256(sizeof(ScatterState)), tiles_at = rules_at + align256(sizeof(bt_scatter_rule) * BT_SCATTER_MAX_RULES);
    const uint64_t first_at = tiles_at + align256(count * sizeof(ScatterTile));
    const uint64_t words_at = first_at + align256(count * sizeof(uint64_t));
    const uint64_t offsets_at = words_at + align256(chunk * blocks_per_tile * kBlockWords * sizeof(uint32_t));
    const uint64_t codes_at = offsets_at + align256(chunk * blocks_per_tile * sizeof(uint64_t));
    const uint64_t list_at = codes_at + align256(chunk * tile_cells);
    BT_HIP(hipSetDevice(ctx->device));
    if (bt_status st = ctx->scatter.reserve(ctx, list_at + list_cap * sizeof(bt_scatter_instance))) return st;
    uint8_t* dev = (uint8_t*)ctx->scatter.dev;
    ScatterState* state = (ScatterState*)dev;
    const ScatterTile* tiles_dev = (const ScatterTile*)(dev + tiles_at);
    const model::Model model = model::make_model(*job.model);
    ScatterParams P{};
    P.m = job.meta;
    P.nm = {model.min_height, model.max_height, normal_side_length(model)};
    P.heights = (const uint16_t*)job.heights;  // a read: no layer is marked written
    P.mask = (const uint32_t*)job.mask;
    P.halo = splat_reach(job.meta), P.rule_count = job.rule_count, P.seed = job.seed, P.jitter = job.jitter;
    const bt_scatter_rule* rules_dev = (const bt_scatter_rule*)(dev + rules_at);
    hipStream_t s = ctx->stream;
    uint32_t launches = 0;
    ScatterState totals{};
    hipError_t e = hipMemsetAsync(state, 0, sizeof(ScatterState), s);
    if (e == hipSuccess) e = hipMemcpyAsync(dev + rules_at, job.rules, job.rule_count * sizeof(bt_scatter_rule), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(dev + tiles_at, tiles.data(), count * sizeof(ScatterTile), hipMemcpyHostToDevice, s);
    for (uint64_t begin = 0; begin < count && e == hipSuccess; begin += chunk) {
        const uint32_t n = uint32_t(std::min<uint64_t>(chunk, count - begin));
        const dim3 grid(n, blocks_per_tile);
        scatter_decide_kernel<<<grid, kScatterThreads, 0, s>>>(P, rules_dev, tiles_dev + begin, dev + codes_at, (uint32_t*)(dev + words_at));
        scatter_scan_kernel<<<1, kScanThreads, 0, s>>>((const uint32_t*)(dev + words_at), n * blocks_per_tile, blocks_per_tile, (uint64_t*)(dev + offsets_at),
                                                       (uint64_t*)(dev + first_at) + begin, state);
        launches += 2u;
        if (list_cap) {
            scatter_emit_kernel<<<grid, kScatterThreads, 0, s>>>(P, model, rules_dev, tiles_dev + begin, dev + codes_at, (const uint64_t*)(dev + offsets_at),
                                                                 (bt_scatter_instance*)(dev + list_at), list_cap);
            launches++;
        }
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&totals, state, sizeof(ScatterState), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    const uint64_t written = std::min<uint64_t>(totals.total, cap);
    // the list in one piece, up to cap
    if (e == hipSuccess && written) e = hipMemcpyAsync(out, dev + list_at, written * sizeof(bt_scatter_instance), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && out_first) e = hipMemcpyAsync(out_first, dev + first_at, count * sizeof(uint64_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(s);
        return hip_fail(e, who);
    }
    if (out_first) out_first[count] = totals.total;
    stats->total = totals.total, stats->written = written;
    stats->cells = count * tile_cells, stats->cells_no_data = totals.no_data;
    for (uint32_t k = 0; k < BT_SCATTER_MAX_RULES; k++) stats->per_rule[k] = totals.per_rule[k];
    stats->launches = launches;
    return BT_OK;
}

}  // namespace bt

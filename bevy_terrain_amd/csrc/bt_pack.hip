// Packed tiles on the device (the format: PACKED TILES in the header; the host half: bt_pack.cpp).
//
// One wave owns one strip of one tile, and a wave64 ballot is exactly one bit plane of a group of 64 values.
//   measure  a strip's residuals -> group widths -> the strip's payload bytes (one word per strip)
//   scan     one wave: the exclusive sum of the strip sizes in 64 bits -> where every stream and every strip's payload begins
//   emit     the residuals again: w ballots per group, lane k keeps word k, ONE 8 w-byte store per group; the width bytes leave in
//            64-byte rows, the header with strip 0, the padding with the last strip
//   decode   lanes < w load the group's words, every lane gathers its bits and un-zigzags, a wave scan runs along the row with a carry
//            from the previous group, and the value of the row above (this wave wrote it) is added: one row segment per store
// No atomics, nothing depends on the schedule.  The encoder visits the groups in stream order (y, plane, group), so a strip's offsets
// are running sums of wave-uniform widths.
#include "bt_internal.hpp"

namespace bt {
namespace {

constexpr uint32_t kStripRows = BT_PACK_STRIP_ROWS;

template <bool kRgba>
__device__ inline uint32_t plane_value(const uint8_t* tile, uint32_t T, uint32_t x, uint32_t y, uint32_t c) {
    const uint64_t texel = uint64_t(y) * T + x;
    return kRgba ? uint32_t(tile[texel * 4u + c]) : uint32_t(reinterpret_cast<const uint16_t*>(tile)[texel]);
}

// the zigzagged residual of lane `lane` of group g of plane c of row y; carry: the row difference of the previous group's last lane
template <bool kRgba>
__device__ inline uint32_t group_z(const uint8_t* tile, uint32_t T, uint32_t y, uint32_t y0, uint32_t c, uint32_t g, uint32_t lane, uint32_t& carry) {
    constexpr uint32_t mask = kRgba ? 0xFFu : 0xFFFFu, half = (mask + 1u) >> 1;
    const uint32_t x = g * 64u + lane;
    const bool real = x < T;
    uint32_t d = 0;
    if (real) {
        d = plane_value<kRgba>(tile, T, x, y, c);
        if (y > y0) d -= plane_value<kRgba>(tile, T, x, y - 1u, c);
        d &= mask;
    }
    uint32_t left = __shfl_up(d, 1);
    if (lane == 0) left = carry;
    carry = __builtin_amdgcn_readlane(d, 63);
    const uint32_t r = (d - left) & mask;
    const uint32_t z = (r & half) ? ((mask + 1u - r) * 2u - 1u) : 2u * r;
    return real ? z : 0u;
}

// the bit planes of a group: returns w; lane k < w keeps word k in `mine`
template <bool kRgba>
__device__ inline uint32_t group_words(uint32_t z, uint32_t lane, uint64_t& mine) {
    constexpr uint32_t bits = kRgba ? 8u : 16u;
    uint32_t w = 0;
    mine = 0;
#pragma unroll
    for (uint32_t k = 0; k < bits; k++) {
        const uint64_t word = __builtin_amdgcn_ballot_w64(((z >> k) & 1u) != 0u);
        if (word != 0ull) w = k + 1u;
        if (lane == k) mine = word;
    }
    return w;
}

template <bool kRgba>
__global__ __launch_bounds__(64) void pack_measure_kernel(PackShape s, const uint8_t* level0, PackTiles tiles, uint32_t* strip_bytes) {
    const uint32_t q = blockIdx.x / s.strips, strip = blockIdx.x % s.strips, lane = threadIdx.x;
    const uint8_t* tile = level0 + s.tile_bytes * tiles.layers[q];
    const uint32_t y0 = strip * kStripRows, y1 = min(s.T, y0 + kStripRows);
    uint32_t words = 0;
    for (uint32_t y = y0; y < y1; y++)
        for (uint32_t c = 0; c < s.planes; c++) {
            uint32_t carry = 0;
            for (uint32_t g = 0; g < s.gpr; g++) {
                const uint32_t z = group_z<kRgba>(tile, s.T, y, y0, c, g, lane, carry);
                uint64_t mine;
                words += group_words<kRgba>(z, lane, mine);
            }
        }
    if (lane == 0) strip_bytes[blockIdx.x] = words * 8u;
}

__global__ __launch_bounds__(64) void pack_scan_kernel(PackShape s, uint32_t count, const uint32_t* strip_bytes, uint64_t* starts, uint64_t* strip_off) {
    const uint32_t lane = threadIdx.x, n = count * s.strips;
    uint64_t running = 0;
    for (uint32_t i = 0; i < n; i += 64u) {
        const uint32_t j = i + lane;
        const uint64_t v = j < n ? uint64_t(strip_bytes[j]) : 0ull;
        uint64_t incl = v;
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint64_t below = __shfl_up(incl, d);
            if (lane >= d) incl += below;
        }
        const uint64_t excl = running + incl - v;
        if (j < n) {
            const uint32_t q = j / s.strips;
            strip_off[j] = uint64_t(q + 1u) * s.head + excl;
            if (j % s.strips == 0) starts[q] = uint64_t(q) * s.head + excl;
        }
        running += __shfl(incl, 63);
    }
    if (lane == 0) starts[count] = uint64_t(count) * s.head + running;
}

template <bool kRgba>
__global__ __launch_bounds__(64) void pack_emit_kernel(PackShape s, uint32_t format, const uint8_t* level0, PackTiles tiles, const uint64_t* starts,
                                                       const uint64_t* strip_off, uint8_t* out) {
    const uint32_t q = blockIdx.x / s.strips, strip = blockIdx.x % s.strips, lane = threadIdx.x;
    const uint8_t* tile = level0 + s.tile_bytes * tiles.layers[q];
    const uint32_t y0 = strip * kStripRows, y1 = min(s.T, y0 + kStripRows);
    uint8_t* stream = out + starts[q];
    uint8_t* widths = stream + 16u + uint64_t(y0) * s.planes * s.gpr;  // this strip's width bytes
    uint64_t* payload = reinterpret_cast<uint64_t*>(out + strip_off[blockIdx.x]);
    uint32_t n = 0, keep = 0;
    uint64_t cursor = 0;  // words
    for (uint32_t y = y0; y < y1; y++)
        for (uint32_t c = 0; c < s.planes; c++) {
            uint32_t carry = 0;
            for (uint32_t g = 0; g < s.gpr; g++) {
                const uint32_t z = group_z<kRgba>(tile, s.T, y, y0, c, g, lane, carry);
                uint64_t mine;
                const uint32_t w = group_words<kRgba>(z, lane, mine);
                if (lane < w) payload[cursor + lane] = mine;
                cursor += w;
                if (lane == (n & 63u)) keep = w;
                n++;
                if ((n & 63u) == 0) widths[n - 64u + lane] = uint8_t(keep);
            }
        }
    if (lane < (n & 63u)) widths[(n & ~63u) + lane] = uint8_t(keep);
    if (strip == 0 && lane == 0) {
        uint64_t* header = reinterpret_cast<uint64_t*>(stream);
        header[0] = 0x31505442ull | (uint64_t(format & 0xFFu) << 32) | (uint64_t(kStripRows) << 40) | (uint64_t(s.T & 0xFFFFu) << 48);  // 'B' 'T' 'P' '1'
        header[1] = (starts[q + 1u] - starts[q] - s.head) & 0xFFFFFFFFull;
    }
    if (strip == s.strips - 1u && lane < s.head - 16u - s.W) stream[16u + s.W + lane] = 0;
}

template <bool kRgba>
__global__ __launch_bounds__(64) void pack_decode_kernel(PackShape s, uint8_t* level0, PackTiles tiles, const uint8_t* packed, const uint64_t* starts,
                                                         const uint64_t* strip_off) {
    constexpr uint32_t mask = kRgba ? 0xFFu : 0xFFFFu;
    const uint32_t q = blockIdx.x / s.strips, strip = blockIdx.x % s.strips, lane = threadIdx.x;
    uint8_t* tile = level0 + s.tile_bytes * tiles.layers[q];
    const uint32_t y0 = strip * kStripRows, y1 = min(s.T, y0 + kStripRows);
    const uint32_t groups = (y1 - y0) * s.planes * s.gpr;
    const uint8_t* widths = packed + starts[q] + 16u + uint64_t(y0) * s.planes * s.gpr;
    const uint64_t* payload = reinterpret_cast<const uint64_t*>(packed + strip_off[blockIdx.x]);
    uint32_t n = 0, batch = 0;
    uint64_t cursor = 0;  // words
    for (uint32_t y = y0; y < y1; y++)
        for (uint32_t c = 0; c < s.planes; c++) {
            uint32_t carry = 0;
            for (uint32_t g = 0; g < s.gpr; g++) {
                if ((n & 63u) == 0) batch = n + lane < groups ? uint32_t(widths[n + lane]) : 0u;  // the next 64 widths, one per lane
                const uint32_t w = __builtin_amdgcn_readlane(batch, n & 63u);
                n++;
                const uint64_t word = lane < w ? payload[cursor + lane] : 0ull;
                cursor += w;
                const uint32_t lo = uint32_t(word), hi = uint32_t(word >> 32);
                uint32_t z = 0;
                for (uint32_t k = 0; k < w; k++) {
                    const uint32_t half = lane < 32u ? __builtin_amdgcn_readlane(lo, k) : __builtin_amdgcn_readlane(hi, k);
                    z |= ((half >> (lane & 31u)) & 1u) << k;
                }
                uint32_t r = (z >> 1) ^ (0u - (z & 1u));
                for (uint32_t d = 1; d < 64u; d <<= 1) {
                    const uint32_t below = __shfl_up(r, d);
                    if (lane >= d) r += below;
                }
                r = (r + carry) & mask;
                carry = __builtin_amdgcn_readlane(r, 63);
                const uint32_t x = g * 64u + lane;
                if (x < s.T) {
                    if (y > y0) r = (r + plane_value<kRgba>(tile, s.T, x, y - 1u, c)) & mask;  // the row above: this lane stored it
                    const uint64_t texel = uint64_t(y) * s.T + x;
                    if (kRgba)
                        tile[texel * 4u + c] = uint8_t(r);
                    else
                        reinterpret_cast<uint16_t*>(tile)[texel] = uint16_t(r);
                }
            }
        }
}

}  // namespace

bt_status launch_pack_measure(hipStream_t stream, uint32_t format, const PackShape& s, const void* level0, const PackTiles& tiles, uint32_t* strip_bytes) {
    if (!tiles.count) return BT_OK;
    const uint32_t grid = tiles.count * s.strips;
    if (format == BT_FORMAT_R16)
        pack_measure_kernel<false><<<grid, 64, 0, stream>>>(s, static_cast<const uint8_t*>(level0), tiles, strip_bytes);
    else
        pack_measure_kernel<true><<<grid, 64, 0, stream>>>(s, static_cast<const uint8_t*>(level0), tiles, strip_bytes);
    return launched("pack_measure_kernel");
}

bt_status launch_pack_scan(hipStream_t stream, const PackShape& s, uint32_t count, const uint32_t* strip_bytes, uint64_t* starts, uint64_t* strip_off) {
    pack_scan_kernel<<<1, 64, 0, stream>>>(s, count, strip_bytes, starts, strip_off);
    return launched("pack_scan_kernel");
}

bt_status launch_pack_emit(hipStream_t stream, uint32_t format, const PackShape& s, const void* level0, const PackTiles& tiles, const uint64_t* starts,
                           const uint64_t* strip_off, uint8_t* out) {
    if (!tiles.count) return BT_OK;
    const uint32_t grid = tiles.count * s.strips;
    if (format == BT_FORMAT_R16)
        pack_emit_kernel<false><<<grid, 64, 0, stream>>>(s, format, static_cast<const uint8_t*>(level0), tiles, starts, strip_off, out);
    else
        pack_emit_kernel<true><<<grid, 64, 0, stream>>>(s, format, static_cast<const uint8_t*>(level0), tiles, starts, strip_off, out);
    return launched("pack_emit_kernel");
}

bt_status launch_pack_decode(hipStream_t stream, uint32_t format, const PackShape& s, void* level0, const PackTiles& tiles, const uint8_t* packed,
                             const uint64_t* starts, const uint64_t* strip_off) {
    if (!tiles.count) return BT_OK;
    const uint32_t grid = tiles.count * s.strips;
    if (format == BT_FORMAT_R16)
        pack_decode_kernel<false><<<grid, 64, 0, stream>>>(s, static_cast<uint8_t*>(level0), tiles, packed, starts, strip_off);
    else
        pack_decode_kernel<true><<<grid, 64, 0, stream>>>(s, static_cast<uint8_t*>(level0), tiles, packed, starts, strip_off);
    return launched("pack_decode_kernel");
}

}  // namespace bt

// TileCoordinate (coordinate.rs): children, neighbours across cube faces, parent and name of a tile, and the bincode varints of a tile
// list (formats/mod.rs).  Index arithmetic only: no device call.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "bt_internal.hpp"

namespace bt {

// coordinate.rs:9-16: for each side: itself, then the side behind its -x, -y, +x, +y edge.
static const uint32_t kNeighbouringSides[6][5] = {
    {0, 4, 2, 1, 5}, {1, 0, 2, 3, 5}, {2, 0, 4, 3, 1}, {3, 2, 4, 5, 1}, {4, 2, 0, 5, 3}, {5, 4, 0, 1, 3},
};

// coordinate.rs:18-53: how a tile position on `side` maps onto `other` (per output axis).
enum Axis : uint8_t { kZero, kLast, kS, kT };
static const Axis kEven[6][2] = {{kS, kT}, {kZero, kT}, {kZero, kS}, {kT, kS}, {kT, kZero}, {kS, kZero}};
static const Axis kOdd[6][2] = {{kS, kT}, {kS, kLast}, {kT, kLast}, {kT, kS}, {kLast, kS}, {kLast, kT}};

void tile_children(bt_tile_coordinate c, bt_tile_coordinate out[4]) {
    for (uint32_t i = 0; i < 4; i++) out[i] = {c.side, c.lod + 1, (c.x << 1) + (i & 1u), (c.y << 1) + (i >> 1)};
}

static bt_tile_coordinate neighbour_at(bt_tile_coordinate c, int nx, int ny, bool spherical) {
    const bt_tile_coordinate invalid = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    if (c.lod > 30u || (spherical && c.side >= 6u)) return invalid;  // (not a tile: TileCoordinate::INVALID and the like have no neighbours)
    const int n = int(1u << c.lod);
    const bool out_x = nx < 0 || nx >= n, out_y = ny < 0 || ny >= n;
    if (!spherical) {
        if (out_x || out_y) return invalid;
        return {c.side, c.lod, uint32_t(nx), uint32_t(ny)};
    }
    if (out_x && out_y) return invalid;  // cube corner: no diagonal neighbour (coordinate.rs:231-239)
    const int edge = nx < 0 ? 1 : ny < 0 ? 2 : nx >= n ? 3 : ny >= n ? 4 : 0;
    const uint32_t s = uint32_t(std::clamp(nx, 0, n - 1)), t = uint32_t(std::clamp(ny, 0, n - 1));
    const uint32_t other = kNeighbouringSides[c.side][edge];
    const Axis* info = (c.side % 2 == 0 ? kEven : kOdd)[(6 + other - c.side) % 6];
    uint32_t xy[2];
    for (int k = 0; k < 2; k++)
        xy[k] = info[k] == kZero ? 0u : info[k] == kLast ? uint32_t(n - 1) : info[k] == kS ? s : t;
    return {other, c.lod, xy[0], xy[1]};
}

void tile_neighbours(bt_tile_coordinate c, bool spherical, bt_tile_coordinate out[8]) {
    for (int i = 0; i < 8; i++) out[i] = neighbour_at(c, int(c.x) + kNeighbourOffsets[i][0], int(c.y) + kNeighbourOffsets[i][1], spherical);
}

}  // namespace bt

using namespace bt;

// ------------------------------------------------------------------ bincode varints (formats/mod.rs)

static uint64_t put_varint(uint64_t v, uint8_t* out, uint64_t pos, uint64_t cap) {
    uint8_t tmp[9];
    uint32_t n = 1;
    if (v < 251) {
        tmp[0] = uint8_t(v);
    } else {
        const uint32_t bytes = v < (1ull << 16) ? 2 : v < (1ull << 32) ? 4 : 8;
        tmp[0] = bytes == 2 ? 251 : bytes == 4 ? 252 : 253;
        for (uint32_t k = 0; k < bytes; k++) tmp[1 + k] = uint8_t(v >> (8 * k));
        n = 1 + bytes;
    }
    if (out && pos + n <= cap) memcpy(out + pos, tmp, n);
    return pos + n;
}

static bool get_varint(const uint8_t* in, uint64_t n, uint64_t& pos, uint64_t& v) {
    if (pos >= n) return false;
    const uint8_t tag = in[pos++];
    if (tag < 251) {
        v = tag;
        return true;
    }
    const uint32_t bytes = tag == 251 ? 2 : tag == 252 ? 4 : tag == 253 ? 8 : 0;
    if (!bytes || pos + bytes > n) return false;
    v = 0;
    for (uint32_t k = 0; k < bytes; k++) v |= uint64_t(in[pos + k]) << (8 * k);
    pos += bytes;
    return true;
}

extern "C" {

void bt_tile_children(bt_tile_coordinate c, bt_tile_coordinate out[4]) {
    if (out) tile_children(c, out);
}
void bt_tile_neighbours(bt_tile_coordinate c, uint32_t spherical, bt_tile_coordinate out[8]) {
    if (out) tile_neighbours(c, spherical != 0, out);
}
bt_tile_coordinate bt_tile_parent(bt_tile_coordinate c) { return {c.side, c.lod - 1u, c.x >> 1, c.y >> 1}; }
int32_t bt_tile_name(bt_tile_coordinate c, char* buf, size_t cap) {
    return snprintf(buf, cap, "%u_%u_%u_%u", c.side, c.lod, c.x, c.y);
}

uint64_t bt_tc_encode(const bt_tile_coordinate* tiles, uint32_t count, uint8_t* out, uint64_t cap) {
    uint64_t pos = put_varint(count, out, 0, cap);
    for (uint32_t i = 0; i < count; i++) {
        pos = put_varint(tiles[i].side, out, pos, cap);
        pos = put_varint(tiles[i].lod, out, pos, cap);
        pos = put_varint(tiles[i].x, out, pos, cap);
        pos = put_varint(tiles[i].y, out, pos, cap);
    }
    return pos;
}

int64_t bt_tc_decode(const uint8_t* data, uint64_t bytes, bt_tile_coordinate* tiles, uint32_t cap) {
    uint64_t pos = 0, len = 0;
    if (!data || !get_varint(data, bytes, pos, len)) return -1;
    for (uint64_t i = 0; i < len; i++) {
        uint64_t v[4];
        for (int k = 0; k < 4; k++)
            if (!get_varint(data, bytes, pos, v[k]) || v[k] > 0xFFFFFFFFull) return -1;
        if (tiles && i < cap) tiles[i] = {uint32_t(v[0]), uint32_t(v[1]), uint32_t(v[2]), uint32_t(v[3])};
    }
    return int64_t(len);
}

}  // extern "C"

// SPHERE CONTACT (include/bevy_terrain_amd.h, "terrain collision"): sphere_contact, the closest ground point of one sphere, which the
// contact kernel and the sweep kernel (bt_collide.hip) both call.  The ground point G(q) is made of ray_frame and sample_surface, the
// functions ray_eval is made of, so a contact agrees with bt_tile_tree_sample_attachment and bt_tile_tree_raycast bit for bit.
//
// A wave evaluates one sphere: every argument but `lane` is wave-uniform, so is every branch, and all 64 lanes reach every cross-lane
// operation.  A round is one G(q) per lane; its winner is found by a butterfly (__shfl_xor, six steps) over the 64-bit pattern of d2,
// which orders non-negative doubles as the doubles order; a NaN takes the pattern of +inf, which never beats best.D2 either.  The
// lowest lane holding the minimum is the winner (a ballot), and x, y, the point and the height are broadcast from it.
#pragma once

#include "bt_raycast_device.hpp"

namespace bt {

#if defined(__HIPCC__)

struct GroundPoint {
    model::V3 g;
    float h;
};

// G(q) and h_q of step 4
__device__ __forceinline__ GroundPoint ground_point(const Ground& G, model::V3 local) {
    using namespace model;
    float value[4];
    sample_ground(G, position_local_to_world(G.P.model, local, G.approximate_height), value);
    const float h = height_of_value(G.P.model, value[0]);
    return {position_local_to_world(G.P.model, local, double(h)), h};
}

__device__ __forceinline__ model::V3 cross3(model::V3 a, model::V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ model::V3 sub3(model::V3 a, model::V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }

// the smallest d2 of the wave (a NaN counts as +inf) and the lowest lane that holds it
__device__ __forceinline__ double wave_min_key(double d2, uint32_t& winner) {
    unsigned long long key = d2 != d2 ? 0x7FF0000000000000ull : (unsigned long long)__double_as_longlong(d2);
#pragma unroll
    for (int mask = 1; mask < 64; mask <<= 1) {
        const unsigned long long other = __shfl_xor(key, mask);
        key = other < key ? other : key;
    }
    const unsigned long long mine = d2 != d2 ? 0x7FF0000000000000ull : (unsigned long long)__double_as_longlong(d2);
    winner = uint32_t(__ffsll(__ballot(mine == key))) - 1u;  // (every lane holds the minimum now: at least one bit)
    return __longlong_as_double((long long)key);
}

__device__ __forceinline__ bt_sphere_contact sphere_contact(const Ground& G, model::V3 c, double r, uint32_t refine_rounds, uint32_t lane) {
    using namespace model;
    bt_sphere_contact out{};
    if (!(finite(c.x) && finite(c.y) && finite(c.z) && finite(r)) || r < 0.0) {
        out.status = BT_CONTACT_INVALID;
        return out;
    }
    const Model& model = G.P.model;
    const RayFrame frame = ray_frame(model, c);
    const V3& n = frame.n;
    const double a = dot3(sub3(c, frame.ground0), n);
    if (G.skip_above && a - r > G.ceiling) {
        out.status = BT_CONTACT_FAR;
        return out;
    }
    const GroundPoint foot = ground_point(G, frame.local);
    const double f = a - double(foot.h);
    if (f <= 0.0) {
        out.status = BT_CONTACT_BELOW;
        out.distance = f;
        out.depth = r - f;
        out.point[0] = foot.g.x, out.point[1] = foot.g.y, out.point[2] = foot.g.z;
        out.normal[0] = n.x, out.normal[1] = n.y, out.normal[2] = n.z;
        out.height = foot.h;
        return out;
    }
    V3 e1 = {1.0, 0.0, 0.0}, e2 = {0.0, 0.0, 1.0};
    if (is_spherical(model)) {
        const double ax = fabs(n.x), ay = fabs(n.y), az = fabs(n.z);
        uint32_t k = 0;
        double least = ax;
        if (ay < least) k = 1, least = ay;
        if (az < least) k = 2;
        const V3 u = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
        e1 = normalize3(cross3(u, n));
        e2 = cross3(n, e1);
    }
    const V3 d0 = sub3(foot.g, c);
    double best_d2 = dot3(d0, d0), ox = 0.0, oy = 0.0, w = r;
    uint32_t candidate = 0;
    V3 point = foot.g;
    float height = foot.h;
    const double sx = (2.0 * double(lane & 7u) - 7.0) / 7.0, sy = (2.0 * double(lane >> 3) - 7.0) / 7.0;
    for (uint32_t round = 0; round <= refine_rounds; round++) {
        const double x = ox + w * sx, y = oy + w * sy;
        const V3 q = {c.x + (x * e1.x + y * e2.x), c.y + (x * e1.y + y * e2.y), c.z + (x * e1.z + y * e2.z)};
        const GroundPoint s = ground_point(G, ray_frame(model, q).local);
        const V3 d = sub3(s.g, c);
        uint32_t winner;
        const double least = wave_min_key(dot3(d, d), winner);
        // the broadcasts are unconditional: no cross-lane operation sits inside a branch
        const double wx = __shfl(x, int(winner)), wy = __shfl(y, int(winner));
        const V3 wg = {__shfl(s.g.x, int(winner)), __shfl(s.g.y, int(winner)), __shfl(s.g.z, int(winner))};
        const float wh = __shfl(s.h, int(winner));
        if (least < best_d2) {  // (uniform: `least` is the same in every lane)
            best_d2 = least;
            candidate = 64u * round + winner + 1u;
            ox = wx;
            oy = wy;
            point = wg;
            height = wh;
        }
        w = w * (2.0 / 7.0);
    }
    const double distance = sqrt(best_d2);
    out.status = distance < r ? BT_CONTACT_TOUCHING : BT_CONTACT_NONE;
    out.candidate = candidate;
    out.distance = distance;
    out.depth = r - distance;
    out.point[0] = point.x, out.point[1] = point.y, out.point[2] = point.z;
    if (distance > 0.0) {
        const double inv = 1.0 / distance;
        out.normal[0] = (c.x - point.x) * inv, out.normal[1] = (c.y - point.y) * inv, out.normal[2] = (c.z - point.z) * inv;
    } else {
        out.normal[0] = n.x, out.normal[1] = n.y, out.normal[2] = n.z;
    }
    out.height = height;
    return out;
}

#endif  // __HIPCC__

}  // namespace bt

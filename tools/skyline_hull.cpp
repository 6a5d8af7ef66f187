// The host baseline of tools/skyline_bench.py: the SKYLINE section of include/bevy_terrain_amd.h computed sequentially, one thread, by the
// header's hull reading: every digital line walked against its direction with the upper convex hull of the cells walked so far as a stack,
// the strict pop test (a collinear entry stays: the nearest cell on a tie).  Integers throughout.
#include <cstdint>
#include <cstdlib>
#include <vector>

namespace {

int64_t floor_div(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

struct Entry {
    int32_t u, z;
};

}  // namespace

// z: width * height u16, row-major.  directions: count x {dx, dy, sun_num, sun_den} as int64.  steps (u16) and rise (i32): count planes of
// width * height; mask (u64) and count_out (u8): one plane each.  Returns the sum of the steps planes.
extern "C" uint64_t skyline_hull(const uint16_t* z, uint32_t width, uint32_t height, const int64_t* directions, uint32_t count, uint16_t* steps, int32_t* rise, uint64_t* mask,
                                 uint8_t* count_out) {
    const uint64_t cells = uint64_t(width) * height;
    for (uint64_t i = 0; i < cells; i++) mask[i] = 0u, count_out[i] = 0u;
    uint64_t sum = 0;
    std::vector<int64_t> off;
    std::vector<Entry> stack;
    for (uint32_t k = 0; k < count; k++) {
        const int64_t dx = directions[4u * k], dy = directions[4u * k + 1u], num = directions[4u * k + 2u], den = directions[4u * k + 3u];
        const bool x_major = std::llabs(dx) >= std::llabs(dy);
        const int64_t major_d = x_major ? dx : dy, minor_d = x_major ? dy : dx;
        const int64_t n = std::llabs(major_d), s = major_d > 0 ? 1 : -1, m = minor_d * s;
        const int64_t L = x_major ? width : height, M = x_major ? height : width;
        off.resize(size_t(L));
        int64_t lowest = 0, highest = 0;
        for (int64_t u = 0; u < L; u++) {
            off[size_t(u)] = floor_div(2 * u * m + n, 2 * n);
            lowest = off[size_t(u)] < lowest ? off[size_t(u)] : lowest, highest = off[size_t(u)] > highest ? off[size_t(u)] : highest;
        }
        uint16_t* steps_k = steps + k * cells;
        int32_t* rise_k = rise + k * cells;
        for (int64_t j = -highest; j <= M - 1 - lowest; j++) {
            stack.clear();
            for (int64_t w = 0; w < L; w++) {
                const int64_t u = s > 0 ? L - 1 - w : w, v = j + off[size_t(u)];
                if (v < 0 || v >= M) continue;
                const uint64_t cell = x_major ? uint64_t(v) * width + uint64_t(u) : uint64_t(u) * width + uint64_t(v);
                const int64_t za = z[cell];
                while (stack.size() >= 2u) {
                    const Entry &p = stack[stack.size() - 1u], &q = stack[stack.size() - 2u];
                    const int64_t t_p = std::llabs(p.u - u), t_q = std::llabs(q.u - u);
                    if (!((q.z - za) * t_p > (p.z - za) * t_q)) break;
                    stack.pop_back();
                }
                int64_t t = 0, up = 0;
                if (!stack.empty()) t = std::llabs(stack.back().u - u), up = stack.back().z - za;
                steps_k[cell] = uint16_t(t), rise_k[cell] = int32_t(up);
                sum += uint64_t(t);
                if (up * den <= t * num) mask[cell] |= uint64_t(1) << k, count_out[cell]++;
                stack.push_back(Entry{int32_t(u), int32_t(za)});
            }
        }
    }
    return sum;
}

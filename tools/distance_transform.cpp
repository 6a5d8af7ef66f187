// The host baseline of tools/distance_bench.py: the DISTANCE section of include/bevy_terrain_amd.h computed sequentially, one thread, by the
// separable reading: r per column in two sweeps, then per row the lower envelope of the parabolas (x - i)^2 + (y - r(i, y))^2 by a stack
// scan.  The tie rule is the header's: the envelope is taken of the triples (distance, r, i) in lexicographic order, which is the order of
// parabolas lifted by an infinitesimal multiple of their index r * width + i, so the scan stays exact.  Integers throughout.
#include <cstdint>
#include <vector>

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kNoRow = 0xFFFFu;

struct Row {
    const uint16_t* r;
    int64_t y;
    int64_t g2(int64_t i) const { return (y - r[i]) * (y - r[i]); }
    int64_t f(int64_t x, int64_t i) const { return (x - i) * (x - i) + g2(i); }
    // is column j (> i) preferred to column i at x
    bool later_wins(int64_t x, int64_t i, int64_t j) const {
        const int64_t a = f(x, i), b = f(x, j);
        return b < a || (b == a && r[j] < r[i]);
    }
    // the largest x at which column i is preferred to column j (> i); floor of a signed quotient
    int64_t sep(int64_t i, int64_t j) const {
        const int64_t n = j * j - i * i + g2(j) - g2(i), d = 2 * (j - i);
        int64_t q = n / d;
        if (n % d != 0 && n < 0) q--;
        if (n % d == 0 && r[j] < r[i]) q--;  // a tie at x = q that column j takes
        return q;
    }
};

}  // namespace

// seed: width * height bytes, non-zero = seed.  dist2, nearest: width * height u32.  Returns the number of seeds.
extern "C" uint64_t distance_transform(const uint8_t* seed, uint32_t width, uint32_t height, uint32_t* dist2, uint32_t* nearest) {
    const uint64_t cells = uint64_t(width) * height;
    std::vector<uint16_t> r(cells, uint16_t(kNoRow));
    uint64_t seeds = 0;
    for (uint32_t x = 0; x < width; x++) {
        uint32_t above = kNoRow;
        for (uint32_t y = 0; y < height; y++) {
            if (seed[uint64_t(y) * width + x]) above = y, seeds++;
            r[uint64_t(y) * width + x] = uint16_t(above);
        }
        uint32_t below = kNoRow;
        for (uint32_t y = height; y-- > 0u;) {
            if (seed[uint64_t(y) * width + x]) below = y;
            const uint32_t up = r[uint64_t(y) * width + x];
            if (below != kNoRow && (up == kNoRow || below - y < y - up)) r[uint64_t(y) * width + x] = uint16_t(below);  // the upper one on a tie
        }
    }
    std::vector<int64_t> s(width), t(width);
    for (uint32_t y = 0; y < height; y++) {
        const Row row{r.data() + uint64_t(y) * width, int64_t(y)};
        uint32_t* d_out = dist2 + uint64_t(y) * width;
        uint32_t* n_out = nearest + uint64_t(y) * width;
        int64_t q = -1;
        for (int64_t u = 0; u < int64_t(width); u++) {
            if (row.r[u] == kNoRow) continue;
            while (q >= 0 && row.later_wins(t[q], s[q], u)) q--;
            if (q < 0) {
                q = 0, s[0] = u, t[0] = 0;
            } else {
                const int64_t from = 1 + row.sep(s[q], u);
                if (from < int64_t(width)) q++, s[q] = u, t[q] = from;
            }
        }
        if (q < 0) {
            for (uint32_t x = 0; x < width; x++) d_out[x] = kNone, n_out[x] = kNone;
            continue;
        }
        for (int64_t x = int64_t(width) - 1; x >= 0; x--) {
            d_out[x] = uint32_t(row.f(x, s[q]));
            n_out[x] = uint32_t(row.r[s[q]]) * width + uint32_t(s[q]);
            if (x == t[q]) q--;
        }
    }
    return seeds;
}

// The host baseline of tools/drainage_bench.py: the DRAINAGE section of include/bevy_terrain_amd.h computed sequentially, one thread.
// W by priority-flood (std::priority_queue from the outlets upwards), F by a breadth-first search from the drain cells, the directions by
// the header's rule, A by peeling the forest from its leaves (donor counts).  Returns the outflow (the sum of A over the outlets).
#include <cstdint>
#include <functional>
#include <queue>
#include <vector>

namespace {
const int kDx[8] = {1, 1, 0, -1, -1, -1, 0, 1}, kDy[8] = {0, 1, 1, 1, 0, -1, -1, -1};
}

extern "C" uint32_t drainage_flood(const uint16_t* raw, const uint8_t* mask, const uint8_t* weight, uint32_t w, uint32_t h, uint16_t* W, uint32_t* F, uint8_t* dir, uint32_t* A) {
    const uint64_t cells = uint64_t(w) * h;
    std::vector<uint8_t> kind(cells);  // 0 void, 1 active, 2 outlet
    auto active = [&](int64_t x, int64_t y) { return x >= 0 && y >= 0 && x < int64_t(w) && y < int64_t(h) && raw[y * w + x] != 0 && !(mask && mask[y * w + x]); };
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) {
            const uint64_t i = uint64_t(y) * w + x;
            if (!active(x, y)) continue;
            kind[i] = 1;
            for (int k = 0; k < 8; k++)
                if (!active(int64_t(x) + kDx[k], int64_t(y) + kDy[k])) kind[i] = 2;
        }
    // W: cells leave the heap in ascending level; a cell first reached from level L gets max(z, L)
    constexpr uint32_t kUnset = 0xFFFFFFFFu;
    std::vector<uint32_t> level(cells, kUnset);
    std::priority_queue<uint64_t, std::vector<uint64_t>, std::greater<uint64_t>> heap;
    for (uint64_t i = 0; i < cells; i++)
        if (kind[i] == 2) level[i] = raw[i], heap.push(uint64_t(raw[i]) << 32 | i);
    while (!heap.empty()) {
        const uint64_t top = heap.top();
        heap.pop();
        const uint32_t i = uint32_t(top), l = uint32_t(top >> 32), x = i % w, y = i / w;
        for (int k = 0; k < 8; k++) {
            const int64_t nx = int64_t(x) + kDx[k], ny = int64_t(y) + kDy[k];
            if (nx < 0 || ny < 0 || nx >= int64_t(w) || ny >= int64_t(h)) continue;
            const uint64_t n = uint64_t(ny) * w + uint64_t(nx);
            if (!kind[n] || level[n] != kUnset) continue;
            level[n] = raw[n] > l ? raw[n] : l;
            heap.push(uint64_t(level[n]) << 32 | n);
        }
    }
    for (uint64_t i = 0; i < cells; i++) W[i] = kind[i] ? uint16_t(level[i]) : uint16_t(0);
    // F: breadth-first from the drain cells through neighbours of equal W
    std::vector<uint32_t> queue;
    queue.reserve(cells);
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) {
            const uint64_t i = uint64_t(y) * w + x;
            F[i] = kind[i] ? kUnset : 0u;
            if (!kind[i]) continue;
            bool drain = kind[i] == 2;
            for (int k = 0; k < 8 && !drain; k++) {
                const uint64_t n = uint64_t(int64_t(y) + kDy[k]) * w + uint64_t(int64_t(x) + kDx[k]);  // not an outlet: every neighbour is inside and active
                drain = W[n] < W[i];
            }
            if (drain) F[i] = 0, queue.push_back(uint32_t(i));
        }
    for (size_t head = 0; head < queue.size(); head++) {
        const uint32_t i = queue[head], x = i % w, y = i / w;
        for (int k = 0; k < 8; k++) {
            const int64_t nx = int64_t(x) + kDx[k], ny = int64_t(y) + kDy[k];
            if (nx < 0 || ny < 0 || nx >= int64_t(w) || ny >= int64_t(h)) continue;
            const uint64_t n = uint64_t(ny) * w + uint64_t(nx);
            if (kind[n] && F[n] == kUnset && W[n] == W[i]) F[n] = F[i] + 1u, queue.push_back(uint32_t(n));
        }
    }
    // the directions, and how many cells give to each
    std::vector<uint8_t> donors(cells);
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) {
            const uint64_t i = uint64_t(y) * w + x;
            A[i] = kind[i] ? (weight ? weight[i] : 1u) : 0u;
            dir[i] = kind[i] == 0 ? 255 : 8;
            if (kind[i] != 1) continue;
            uint64_t best = 0;
            int steepest = -1, flat = -1;
            for (int k = 7; k >= 0; k--) {
                const uint64_t n = uint64_t(int64_t(y) + kDy[k]) * w + uint64_t(int64_t(x) + kDx[k]);
                if (W[n] < W[i]) {
                    const uint64_t d = uint64_t(W[i] - W[n]), score = d * d * ((k & 1) ? 1u : 2u);
                    if (score >= best) best = score, steepest = k;
                } else if (W[n] == W[i] && F[i] != 0u && F[n] == F[i] - 1u) {
                    flat = k;
                }
            }
            const int k = steepest >= 0 ? steepest : flat;
            dir[i] = uint8_t(k);
            donors[uint64_t(int64_t(y) + kDy[k]) * w + uint64_t(int64_t(x) + kDx[k])]++;
        }
    // A: a cell gives once all its donors have given
    queue.clear();
    for (uint64_t i = 0; i < cells; i++)
        if (kind[i] && !donors[i]) queue.push_back(uint32_t(i));
    uint32_t outflow = 0;
    for (size_t head = 0; head < queue.size(); head++) {
        const uint32_t i = queue[head];
        if (dir[i] == 8) {
            outflow += A[i];
            continue;
        }
        const uint32_t n = uint32_t(int64_t(i) + int64_t(kDy[dir[i]]) * int64_t(w) + kDx[dir[i]]);
        A[n] += A[i];
        if (--donors[n] == 0) queue.push_back(n);
    }
    return outflow;
}

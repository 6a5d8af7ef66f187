// The host baseline of tools/viewshed_bench.py: the VIEWSHED section of include/bevy_terrain_amd.h computed sequentially, one thread.
// Observer by observer and target by target, each line walked from the observer with q and r advanced by a DDA in 64-bit integers (no
// division in the sample loop, as on the device, so the comparison is of like with like), the largest S_j / j kept by cross-multiplication,
// one ceiling per line.  Returns the number of line samples (the sum of n - 1 over the used observers and their covered active targets).
#include <cstdint>
#include <cstdlib>

struct Observer {
    uint32_t x, y, eye_height, radius;
};

extern "C" uint64_t viewshed_lines(const uint16_t* raw, uint32_t w, uint32_t h, const Observer* observers, uint32_t observer_count, uint32_t target_height, uint32_t* clearance,
                                   uint8_t* count, uint64_t* mask) {
    const uint64_t cells = uint64_t(w) * h;
    for (uint64_t i = 0; i < cells; i++) clearance[i] = 0xFFFFFFFFu, count[i] = 0, mask[i] = 0;
    uint64_t samples = 0;
    for (uint32_t o = 0; o < observer_count; o++) {
        const Observer& ob = observers[o];
        const int64_t zo = raw[uint64_t(ob.y) * w + ob.x];
        if (zo == 0) continue;  // skipped
        const int64_t E = zo + ob.eye_height;
        for (uint32_t ty = 0; ty < h; ty++)
            for (uint32_t tx = 0; tx < w; tx++) {
                const uint64_t i = uint64_t(ty) * w + tx;
                const int64_t zt = raw[i];
                if (zt == 0) continue;
                const int64_t dx = int64_t(tx) - ob.x, dy = int64_t(ty) - ob.y;
                if (ob.radius != 0 && uint64_t(dx * dx + dy * dy) > uint64_t(ob.radius) * ob.radius) continue;
                const bool x_major = std::llabs(dx) >= std::llabs(dy);
                const int64_t n = x_major ? std::llabs(dx) : std::llabs(dy), m = x_major ? dy : dx;
                const int64_t major_step = x_major ? (dx < 0 ? -1 : 1) : (dy < 0 ? -int64_t(w) : int64_t(w)), minor_step = x_major ? int64_t(w) : 1;
                int64_t C = 0;
                if (n > 1) {
                    int64_t at = int64_t(ob.y) * w + ob.x, r = 0, Sb = 0, jb = 0;
                    for (int64_t j = 1; j < n; j++) {
                        at += major_step;
                        r += m;
                        if (r >= n) r -= n, at += minor_step;
                        if (r < 0) r += n, at -= minor_step;
                        const int64_t za = raw[at], zb = r ? raw[at + minor_step] : 0;
                        const int64_t S = za * (n - r) + zb * r - E * n;
                        if (jb == 0 || S * jb > Sb * j) Sb = S, jb = j;
                    }
                    const int64_t M = Sb >= 0 ? (Sb + jb - 1) / jb : -((-Sb) / jb);  // the ceiling, towards +inf
                    C = E + M - zt;
                    if (C < 0) C = 0;
                    samples += uint64_t(n - 1);
                }
                if (uint32_t(C) < clearance[i]) clearance[i] = uint32_t(C);
                if (C <= int64_t(target_height)) count[i]++, mask[i] |= uint64_t(1) << o;
            }
    }
    return samples;
}

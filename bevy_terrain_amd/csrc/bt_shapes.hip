// bt_atlas_rasterize_shapes: the raster kernel.  The host half is in bt_edit.cpp (the call, for the write-back) and bt_shapes.cpp (the
// rules, the boxes, the records); the definition is the SHAPES section of include/bevy_terrain_amd.h.
//
// shapes_raster_kernel   ONE launch.  A workgroup of 256 lanes owns a block of kBlockW x kBlockH = 64 x 16 cells of U; wave v of it owns
//                        the rows 4 v .. 4 v + 3 and lane l of the wave column l, so a lane has four cells of one column, one below the
//                        other.  Their running value, count, last and winding number stay in registers across the whole list.
//                        The records (the shapes whose box is not empty, in list order) are read uniformly; one whose box misses the
//                        block is skipped by the whole workgroup.  The vertices of an entry pass through LDS kChunk edges at a time: the
//                        chunk holds kChunk + 1 vertices, the last being the end of its last edge (index taken modulo the entry's vertex
//                        count), so an edge that spans two chunks and the closing edge are edges like any other.  A wave sorts the chunk's
//                        edges 64 at a time, a lane to an edge, into those that can touch its cells and the rest, and walks the set bits
//                        of the ballot alone; for such an edge every lane reads the same LDS address (a broadcast) and the vertex is made
//                        a scalar, so what is left to decide is a scalar branch:
//                          polygon   a horizontal edge, or one whose y-range misses the wave's four rows: skipped; one wholly at or left
//                                    of the block's first column: skipped (it never meets a row strictly right of P); one wholly right of
//                                    the block's last column: counted by its y-range alone; otherwise the cross product, formed once for
//                                    the lane's first cell and stepped by 256 (b.x - a.x) per row.
//                          stroke    a segment whose box grown by r misses the wave's cells: skipped; otherwise the three-case test, the
//                                    128-bit comparison as two high / low product pairs.
//                        None of the skips changes a result: each only omits terms that are zero by the definition.
//                        The texels are folded in place (one lane reads and writes a cell), the planes written with ordinary stores; the
//                        two counts are integer sums, folded per workgroup and added atomically, which does not depend on the order.
#include "bt_internal.hpp"

namespace bt {

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kWave = 64;
constexpr uint32_t kChunk = BT_SHAPES_CHUNK;
constexpr uint32_t kBlockW = BT_SHAPES_BLOCK_W, kBlockH = BT_SHAPES_BLOCK_H;
constexpr uint32_t kRows = kBlockH / (kThreads / kWave);  // cells of a lane
static_assert(kBlockW == kWave && kRows == 4u && kChunk >= 1u, "a wave to 64 columns of four rows");

__device__ __forceinline__ int32_t uniform(int32_t v) { return __builtin_amdgcn_readfirstlane(v); }

// the sum of v over a workgroup, in thread 0; slot: four words of LDS of this fold's own
__device__ __forceinline__ unsigned long long group_sum(unsigned long long v, unsigned long long* slot) {
    for (int off = int(kWave) / 2; off > 0; off >>= 1) v += __shfl_down(v, off);
    if (threadIdx.x % kWave == 0u) slot[threadIdx.x / kWave] = v;
    __syncthreads();
    if (threadIdx.x != 0u) return 0u;
    for (uint32_t k = 1; k < kThreads / kWave; k++) v += slot[k];
    return v;
}

__device__ __forceinline__ uint32_t fold_value(uint32_t v, uint32_t op, uint32_t value, bool wide) {
    if (!wide && v == 0u) return 0u;  // no data stays no data
    int32_t r = int32_t(v);
    switch (op) {
        case BT_SHAPE_SET: r = int32_t(value); break;
        case BT_SHAPE_MAX: r = max(r, int32_t(value)); break;
        case BT_SHAPE_MIN: r = min(r, int32_t(value)); break;
        case BT_SHAPE_ADD: r = r + int32_t(value); break;
        default: r = r - int32_t(value); break;  // BT_SHAPE_SUB
    }
    return uint32_t(wide ? min(max(r, 0), 255) : min(max(r, 1), 65535));
}

__global__ __launch_bounds__(kThreads) void shapes_raster_kernel(ShapesJob job) {
    __shared__ bt_shape_vertex verts[kChunk + 1u];
    __shared__ unsigned long long slots[2][kThreads / kWave];
    const uint32_t uw = uint32_t(job.u.x_hi) - job.u.x_lo + 1u, uh = uint32_t(job.u.y_hi) - job.u.y_lo + 1u;
    const uint32_t lane = threadIdx.x % kWave, wave = uint32_t(uniform(int32_t(threadIdx.x / kWave)));
    const uint32_t ux = blockIdx.x * kBlockW + lane, uy0 = blockIdx.y * kBlockH + wave * kRows;  // in U
    // the block in cells of the window, for the shapes' boxes
    const uint32_t block_x_lo = job.u.x_lo + blockIdx.x * kBlockW, block_x_hi = min(block_x_lo + kBlockW - 1u, uint32_t(job.u.x_hi));
    const uint32_t block_y_lo = job.u.y_lo + blockIdx.y * kBlockH, block_y_hi = min(block_y_lo + kBlockH - 1u, uint32_t(job.u.y_hi));
    // the sample points: the lane's column and first row; the range of the wave's
    const int32_t px = int32_t(256u * (job.u.x_lo + ux)), py0 = int32_t(256u * (job.u.y_lo + uy0));
    const int32_t wx_lo = int32_t(256u * block_x_lo), wx_hi = int32_t(256u * block_x_hi);
    const int32_t wy_lo = int32_t(256u * (job.u.y_lo + uy0)), wy_hi = wy_lo + int32_t(256u * (kRows - 1u));

    bool valid[kRows];
    uint32_t old_texel[kRows], value[kRows], count[kRows], last[kRows];
    for (uint32_t j = 0; j < kRows; j++) {
        valid[j] = ux < uw && uy0 + j < uh;
        const uint32_t i = (uy0 + j) * uw + ux;
        old_texel[j] = !valid[j] ? 0u : job.wide ? ((const uint32_t*)job.texels)[i] : uint32_t(((const uint16_t*)job.texels)[i]);
        value[j] = job.wide ? (old_texel[j] >> job.shift) & 0xFFu : old_texel[j];
        count[j] = 0u, last[j] = BT_SHAPES_NONE;
    }

    for (uint32_t s = 0; s < job.record_count; s++) {
        const ShapeRecord& rec = job.records[s];
        if (rec.box.x_lo > block_x_hi || rec.box.x_hi < block_x_lo || rec.box.y_lo > block_y_hi || rec.box.y_hi < block_y_lo) continue;
        const bool polygon = rec.kind == BT_SHAPE_POLYGON;
        const int32_t r = int32_t(rec.half_width);
        const uint64_t r2 = uint64_t(rec.half_width) * rec.half_width;
        int32_t acc[kRows] = {0, 0, 0, 0};  // polygon: the winding number; stroke: non-zero once a segment covers the cell
        for (uint32_t e = rec.first_entry; e < rec.first_entry + rec.entry_count; e++) {
            const uint32_t first = job.entries[e].first_vertex, n = job.entries[e].vertex_count;
            // edge i runs from vertex i to vertex (i + 1) mod n: n of them on a contour and a closed stroke (one vertex: the degenerate
            // segment), n - 1 on an open one
            const uint32_t edges = polygon || (rec.flags & BT_SHAPE_CLOSED) ? n : max(n - 1u, 1u);
            for (uint32_t c0 = 0; c0 < edges; c0 += kChunk) {
                const uint32_t chunk = min(kChunk, edges - c0);
                __syncthreads();  // the chunk before has been read
                for (uint32_t t = threadIdx.x; t <= chunk; t += kThreads) {
                    uint32_t i = c0 + t;  // <= edges <= n
                    if (i >= n) i -= n;
                    verts[t] = job.vertices[first + i];
                }
                __syncthreads();
                // the wave sorts the chunk's edges 64 at a time, a lane to an edge: which of them can touch its cells at all?
                for (uint32_t g0 = 0; g0 < chunk; g0 += kWave) {
                    bool touches = false;
                    if (g0 + lane < chunk) {
                        const bt_shape_vertex a = verts[g0 + lane], b = verts[g0 + lane + 1u];
                        if (polygon)  // not horizontal, its y-range holds one of the wave's rows, and it is not wholly at or left of the first column
                            touches = a.y != b.y && max(a.y, b.y) > wy_lo && min(a.y, b.y) <= wy_hi && max(a.x, b.x) > wx_lo;
                        else
                            touches = !(max(a.x, b.x) + r < wx_lo || min(a.x, b.x) - r > wx_hi || max(a.y, b.y) + r < wy_lo || min(a.y, b.y) - r > wy_hi);
                    }
                    for (uint64_t todo = __ballot(touches); todo != 0u; todo &= todo - 1u) {
                        const uint32_t i = g0 + uint32_t(__ffsll((unsigned long long)todo)) - 1u;
                        const int32_t ax = uniform(verts[i].x), ay = uniform(verts[i].y), bx = uniform(verts[i + 1u].x), by = uniform(verts[i + 1u].y);
                        const int32_t dx = bx - ax, dy = by - ay;
                        if (polygon) {
                            const int32_t y_lo = min(ay, by), y_hi = max(ay, by);  // counts for y_lo <= P.y < y_hi
                            const int32_t dir = dy > 0 ? 1 : -1;
                            if (min(ax, bx) > wx_hi) {
                                for (uint32_t j = 0; j < kRows; j++) {
                                    const int32_t py = py0 + int32_t(256u * j);
                                    acc[j] += y_lo <= py && py < y_hi ? dir : 0;
                                }
                                continue;
                            }
                            int64_t c = int64_t(dx) * (py0 - ay) - int64_t(dy) * (px - ax);
                            for (uint32_t j = 0; j < kRows; j++) {
                                const int32_t py = py0 + int32_t(256u * j);
                                const bool crosses = dir > 0 ? c > 0 : c < 0;
                                acc[j] += y_lo <= py && py < y_hi && crosses ? dir : 0;
                                c += 256 * int64_t(dx);
                            }
                        } else {
                            const int64_t L = int64_t(dx) * dx + int64_t(dy) * dy;
                            const uint64_t rhs_hi = __umul64hi(r2, uint64_t(L)), rhs_lo = r2 * uint64_t(L);
                            const int32_t ex = px - ax, fx = px - bx;
                            for (uint32_t j = 0; j < kRows; j++) {
                                const int32_t py = py0 + int32_t(256u * j);
                                const int32_t ey = py - ay, fy = py - by;
                                const int64_t t = int64_t(ex) * dx + int64_t(ey) * dy;
                                bool hit;
                                if (L == 0 || t <= 0) {
                                    hit = uint64_t(int64_t(ex) * ex + int64_t(ey) * ey) <= r2;
                                } else if (t >= L) {
                                    hit = uint64_t(int64_t(fx) * fx + int64_t(fy) * fy) <= r2;
                                } else {
                                    const int64_t c = int64_t(dx) * ey - int64_t(dy) * ex;
                                    const uint64_t u = uint64_t(c < 0 ? -c : c);
                                    const uint64_t lhs_hi = __umul64hi(u, u), lhs_lo = u * u;
                                    hit = lhs_hi < rhs_hi || (lhs_hi == rhs_hi && lhs_lo <= rhs_lo);
                                }
                                acc[j] |= int32_t(hit);
                            }
                        }
                    }
                }
            }
        }
        for (uint32_t j = 0; j < kRows; j++) {
            const bool covered = polygon && !(rec.flags & BT_SHAPE_NONZERO) ? (acc[j] & 1) != 0 : acc[j] != 0;
            if (!covered) continue;
            count[j] = min(count[j] + 1u, 255u);
            last[j] = rec.k;
            value[j] = fold_value(value[j], rec.op, rec.value, job.wide != 0u);
        }
    }

    unsigned long long covered = 0u, written = 0u;
    for (uint32_t j = 0; j < kRows; j++) {
        if (!valid[j]) continue;
        const uint32_t i = (uy0 + j) * uw + ux;
        const uint32_t texel = job.wide ? (old_texel[j] & ~(0xFFu << job.shift)) | (value[j] << job.shift) : value[j];
        if (job.wide)
            ((uint32_t*)job.texels)[i] = texel;
        else
            ((uint16_t*)job.texels)[i] = uint16_t(texel);
        job.count[i] = uint8_t(count[j]);
        job.last[i] = uint16_t(last[j]);
        covered += count[j] != 0u;
        written += texel != old_texel[j];
    }
    covered = group_sum(covered, slots[0]), written = group_sum(written, slots[1]);
    if (threadIdx.x != 0u) return;
    if (covered) atomicAdd(&job.counts->covered, covered);
    if (written) atomicAdd(&job.counts->written, written);
}

}  // namespace

bt_status launch_shapes_raster(hipStream_t stream, const ShapesJob& job) {
    const uint32_t uw = uint32_t(job.u.x_hi) - job.u.x_lo + 1u, uh = uint32_t(job.u.y_hi) - job.u.y_lo + 1u;
    shapes_raster_kernel<<<dim3((uw + kBlockW - 1u) / kBlockW, (uh + kBlockH - 1u) / kBlockH), kThreads, 0, stream>>>(job);
    return launched("shapes_raster_kernel");
}

}  // namespace bt

"""Sequential model of bt_atlas_drainage: the DRAINAGE section of include/bevy_terrain_amd.h, stated on its own.

TEST INFRASTRUCTURE ONLY.  Imports neither the product nor the oracle.  On purpose another algorithm than the device's relaxations: the
filled level by priority-flood (heapq, from the outlets upwards), the flat distance by a breadth-first search from the drain cells, the
directions by the header's rule in Python integers (no width to overflow), the accumulation by one pass in descending (W, F) order.  A
window is raw (h, w) uint16 (0 = no data; texels of tiles the atlas does not hold arrive as 0, as bt_atlas_read_region delivers them) plus
an optional (h, w) void mask and an optional (h, w) uint8 weight plane."""
import heapq
from collections import deque

import numpy as np

NEIGHBOURS = [(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)]
OUTLET, VOID = 8, 255
MAX_CELLS = 1 << 22
STATS = ("cells", "voids", "outlets", "tiles_missing", "filled", "flats", "max_flat_distance", "max_accumulation", "outflow")
SCHEDULE = ("sweeps_fill", "sweeps_flat", "sweeps_accumulate", "launches")  # the fields of bt_drainage_stats that describe the schedule


def void_cells(raw, void=None):
    out = np.asarray(raw) == 0
    if void is not None:
        out = out | (np.asarray(void) != 0)
    return out


def drainage(raw, void=None, weight=None):
    """-> (W (h, w) uint16, F (h, w) uint32, direction (h, w) uint8, A (h, w) uint32, stats without tiles_missing and the schedule)"""
    raw = np.asarray(raw)
    h, w = raw.shape
    is_void = void_cells(raw, void)
    z = [[0 if is_void[y, x] else int(raw[y, x]) for x in range(w)] for y in range(h)]
    active = [[not is_void[y, x] for x in range(w)] for y in range(h)]

    def neighbours(x, y):
        """(k, nx, ny) of the neighbours that are inside and active"""
        for k, (dx, dy) in enumerate(NEIGHBOURS):
            nx, ny = x + dx, y + dy
            if 0 <= nx < w and 0 <= ny < h and active[ny][nx]:
                yield k, nx, ny

    cells = [(x, y) for y in range(h) for x in range(w) if active[y][x]]
    outlet = {(x, y) for x, y in cells if sum(1 for _ in neighbours(x, y)) < 8}

    # W: priority-flood.  Cells leave the heap in ascending level; a cell first reached from a cell of level L gets max(z, L)
    W = [[None] * w for _ in range(h)]
    heap = [(z[y][x], y, x) for x, y in outlet]
    heapq.heapify(heap)
    for x, y in outlet:
        W[y][x] = z[y][x]
    while heap:
        level, y, x = heapq.heappop(heap)
        for _, nx, ny in neighbours(x, y):
            if W[ny][nx] is None:
                W[ny][nx] = max(z[ny][nx], level)
                heapq.heappush(heap, (W[ny][nx], ny, nx))
    assert all(W[y][x] is not None for x, y in cells), "an active cell no outlet reaches"

    # F: breadth-first from the drain cells through neighbours of equal W
    F = [[None] * w for _ in range(h)]
    queue = deque()
    for x, y in cells:
        if (x, y) in outlet or any(W[ny][nx] < W[y][x] for _, nx, ny in neighbours(x, y)):
            F[y][x] = 0
            queue.append((x, y))
    while queue:
        x, y = queue.popleft()
        for _, nx, ny in neighbours(x, y):
            if F[ny][nx] is None and W[ny][nx] == W[y][x]:
                F[ny][nx] = F[y][x] + 1
                queue.append((nx, ny))
    assert all(F[y][x] is not None for x, y in cells), "an active cell of a flat no drain cell reaches"

    # the direction plane
    direction = np.full((h, w), VOID, dtype=np.uint8)
    receiver = {}
    for x, y in cells:
        if (x, y) in outlet:
            direction[y, x] = OUTLET
            continue
        best = None
        for k, nx, ny in neighbours(x, y):
            d = W[y][x] - W[ny][nx]
            if d > 0:
                score = d * d * (1 if k & 1 else 2)
                if best is None or score > best[0]:
                    best = (score, k, nx, ny)
        if best is None:
            best = next((0, k, nx, ny) for k, nx, ny in neighbours(x, y) if W[ny][nx] == W[y][x] and F[ny][nx] == F[y][x] - 1)
        direction[y, x] = best[1]
        receiver[(x, y)] = (best[2], best[3])

    # A: every cell hands its sum to its receiver, the highest (W, F) first, so a cell is complete before it gives
    A = [[0] * w for _ in range(h)]
    for x, y in cells:
        A[y][x] = 1 if weight is None else int(weight[y][x])
    for x, y in sorted(cells, key=lambda c: (-W[c[1]][c[0]], -F[c[1]][c[0]])):
        if (x, y) in receiver:
            rx, ry = receiver[(x, y)]
            A[ry][rx] += A[y][x]

    plane = lambda rows, dtype: np.array([[0 if v is None else v for v in row] for row in rows], dtype=np.int64).astype(dtype).reshape(h, w)
    Wp, Fp, Ap = plane(W, np.uint16), plane(F, np.uint32), plane(A, np.uint32)
    stats = dict(cells=h * w, voids=h * w - len(cells), outlets=len(outlet), filled=sum(1 for x, y in cells if W[y][x] > z[y][x]),
                 flats=sum(1 for x, y in cells if F[y][x] > 0), max_flat_distance=max((F[y][x] for x, y in cells), default=0),
                 max_accumulation=max((A[y][x] for x, y in cells), default=0), outflow=sum(A[y][x] for x, y in outlet))
    return Wp, Fp, direction, Ap, stats


def receivers(direction):
    """{(x, y): (rx, ry)} of the cells whose direction is a k"""
    h, w = direction.shape
    out = {}
    for y in range(h):
        for x in range(w):
            k = int(direction[y, x])
            if k < 8:
                out[(x, y)] = (x + NEIGHBOURS[k][0], y + NEIGHBOURS[k][1])
    return out


def chain_length(direction, start):
    """cells on the way from start = (x, y) downstream to its outlet, both included"""
    x, y = start
    n = 1
    while direction[y, x] < 8:
        dx, dy = NEIGHBOURS[int(direction[y, x])]
        x, y, n = x + dx, y + dy, n + 1
        assert n <= direction.size
    assert direction[y, x] == OUTLET
    return n

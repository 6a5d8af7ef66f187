"""numpy + heapq model of bt_atlas_path_field and bt_path_trace: the PATH FIELD section of include/bevy_terrain_amd.h, stated on its own.

TEST INFRASTRUCTURE ONLY.  Imports neither the product nor the oracle.  Every float is np.float32 and every written operation of the
header is one numpy operation on float32 operands, so each is rounded once to binary32.  A window is raw (h, w) uint16 (0 = no data;
texels of tiles the atlas does not hold arrive as 0, as bt_atlas_read_region delivers them) plus an optional (h, w) mask; a cost is a dict
with the fields of bt_path_cost; goals are (x, y, cost0)."""
import heapq

import numpy as np

F = np.float32
INF = F(np.inf)
NEIGHBOURS = [(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)]
GOAL, UNREACHABLE, BLOCKED = 8, 254, 255
MAX_CELLS, MAX_GOALS = 1 << 22, 4096

COST_DEFAULT = dict(min_height=0.0, max_height=1.0, cell_size=1.0, max_grade=np.inf, grade_weight=0.0, climb_weight=0.0, descend_weight=0.0)


def cost(**fields):
    out = dict(COST_DEFAULT)
    out.update(fields)
    return out


def blocked_cells(raw, mask=None):
    blocked = np.asarray(raw) == 0
    if mask is not None:
        blocked = blocked | (np.asarray(mask) != 0)
    return blocked


def heights(raw, c):
    """h = min_height + (max_height - min_height) * (f32(raw) / 65535.0f)"""
    lo, hi = F(c["min_height"]), F(c["max_height"])
    return lo + (hi - lo) * (np.asarray(raw).astype(F) / F(65535.0))


def shifted(plane, dx, dy, fill):
    """out[y, x] = plane[y + dy, x + dx], `fill` where that lies outside"""
    h, w = plane.shape
    out = np.full_like(plane, fill)
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    out[yd, xd] = plane[ys, xs]
    return out


def edge_weights(raw, mask, c, reached=None):
    """W (8, h, w) float32: W[k][y, x] = w((x, y) -> neighbour k), +inf where the edge does not exist.  reached: counts what removed an edge"""
    blocked = blocked_cells(raw, mask)
    hgt = heights(raw, c)
    cell = F(c["cell_size"])
    diag = cell * F(1.41421356)
    gw, cw, dw, mg = F(c["grade_weight"]), F(c["climb_weight"]), F(c["descend_weight"]), F(c["max_grade"])
    W = np.empty((8,) + hgt.shape, dtype=F)
    with np.errstate(invalid="ignore", over="ignore"):
        for k, (dx, dy) in enumerate(NEIGHBOURS):
            run = diag if k & 1 else cell
            free_b = ~shifted(blocked, dx, dy, True)
            hb = shifted(hgt, dx, dy, F(0))
            rise = hb - hgt
            g = np.abs(rise) / run
            grade_ok = g <= mg  # a NaN fails
            up = np.where(rise > 0, rise, F(0))
            down = np.where(rise < 0, -rise, F(0))
            w = ((run * (F(1.0) + gw * g)) + cw * up) + dw * down
            exists = ~blocked & free_b
            if k & 1:
                corner_ok = ~shifted(blocked, dx, 0, True) & ~shifted(blocked, 0, dy, True)
                if reached is not None:
                    reached["corner_cut"] = reached.get("corner_cut", 0) + int((exists & grade_ok & ~corner_ok).sum())
                exists = exists & corner_ok
            if reached is not None:
                reached["grade_cut"] = reached.get("grade_cut", 0) + int((exists & ~grade_ok).sum())
            W[k] = np.where(exists & grade_ok, w, INF).astype(F)
    return W


def usable_goals(raw, mask, goals):
    """{(x, y): the smallest cost0 among the goal entries on that free cell}, the number of entries on blocked cells"""
    blocked = blocked_cells(raw, mask)
    best, on_blocked = {}, 0
    for g in goals:
        x, y, c0 = int(g[0]), int(g[1]), F(g[2] if len(g) > 2 else 0.0)
        if blocked[y, x]:
            on_blocked += 1
            continue
        if (x, y) not in best or c0 < best[(x, y)]:
            best[(x, y)] = c0
    return best, on_blocked


def dijkstra(W, goal_costs):
    """D (h, w) float32: the minimum over paths of the left fold of rounded adds, by Dijkstra's algorithm on the reversed edges"""
    _, h, w = W.shape
    D = np.full((h, w), INF, dtype=F)
    heap = []
    for (x, y), c0 in goal_costs.items():
        D[y, x] = c0
        heap.append((float(c0), x, y))
    heapq.heapify(heap)
    while heap:
        d, x, y = heapq.heappop(heap)
        if d > float(D[y, x]):
            continue
        db = D[y, x]
        # every cell a that has (x, y) as its neighbour k: a = (x, y) - offset k
        for k, (dx, dy) in enumerate(NEIGHBOURS):
            ax, ay = x - dx, y - dy
            if ax < 0 or ay < 0 or ax >= w or ay >= h:
                continue
            cand = db + W[k, ay, ax]  # float32 + float32: one rounding
            if cand < D[ay, ax]:
                D[ay, ax] = cand
                heapq.heappush(heap, (float(cand), ax, ay))
    return D


def jacobi(W, goal_costs, max_iterations=None):
    """the same field by whole-grid relaxation from +inf: X <- min(X, min_k (X(b_k) + W[k])) until nothing moves.  Returns (D, iterations)"""
    _, h, w = W.shape
    D = np.full((h, w), INF, dtype=F)
    for (x, y), c0 in goal_costs.items():
        D[y, x] = c0
    limit = h * w if max_iterations is None else max_iterations
    for it in range(limit + 1):
        new = D.copy()
        with np.errstate(invalid="ignore"):
            for k, (dx, dy) in enumerate(NEIGHBOURS):
                cand = shifted(D, dx, dy, INF) + W[k]
                new = np.where(cand < new, cand, new)
        if np.array_equal(new.view(np.uint32), D.view(np.uint32)):
            return D, it
        D = new
    raise AssertionError("no fixed point")


def next_plane(raw, mask, W, D, goal_costs):
    blocked = blocked_cells(raw, mask)
    h, w = D.shape
    out = np.full((h, w), UNREACHABLE, dtype=np.uint8)
    found = np.isinf(D)
    with np.errstate(invalid="ignore"):
        for k in range(7, -1, -1):  # descending: the smallest matching k stays
            dx, dy = NEIGHBOURS[k]
            match = ~np.isinf(D) & ((shifted(D, dx, dy, INF) + W[k]) == D)
            out[match] = k
            found |= match
    for (x, y), c0 in goal_costs.items():
        if c0 == D[y, x]:
            out[y, x] = GOAL
            found[y, x] = True
    out[np.isinf(D)] = UNREACHABLE
    out[blocked] = BLOCKED
    assert found.all(), "a finite D that no neighbour and no goal explains"
    return out


def field(raw, mask, c, goals, reached=None):
    """(D float32 (h, w), next uint8 (h, w), stats without sweeps and launches) of the header's definition"""
    raw = np.asarray(raw)
    W = edge_weights(raw, mask, c, reached)
    goal_costs, on_blocked = usable_goals(raw, mask, goals)
    D = dijkstra(W, goal_costs)
    nxt = next_plane(raw, mask, W, D, goal_costs)
    stats = dict(cells=int(raw.size), blocked=int(blocked_cells(raw, mask).sum()), reachable=int((~np.isinf(D)).sum()), goals_used=len(goals) - on_blocked,
                 goals_blocked=on_blocked)
    if reached is not None:
        reached["unreachable"] = int((np.isinf(D) & ~blocked_cells(raw, mask)).sum())
        reached["dominated_goals"] = sum(1 for g in goals if not blocked_cells(raw, mask)[int(g[1]), int(g[0])] and F(g[2] if len(g) > 2 else 0.0) > D[int(g[1]), int(g[0])])
    return D, nxt, stats


TRACE_OK, TRACE_BLOCKED, TRACE_UNREACHABLE, TRACE_LOOP = "ok", "blocked", "unreachable", "loop"


def trace(nxt, start):
    """bt_path_trace: ([(x, y), ...] start and goal included, status)"""
    h, w = nxt.shape
    x, y = int(start[0]), int(start[1])
    cells = []
    for step in range(h * w + 1):
        cells.append((x, y))
        n = int(nxt[y, x])
        if n == GOAL:
            return cells, TRACE_OK
        if step == 0 and n in (BLOCKED, UNREACHABLE):
            return cells, TRACE_BLOCKED if n == BLOCKED else TRACE_UNREACHABLE
        if n > 7 or step == h * w:
            break
        nx, ny = x + NEIGHBOURS[n][0], y + NEIGHBOURS[n][1]
        if nx < 0 or ny < 0 or nx >= w or ny >= h:
            break
        x, y = nx, ny
    return cells, TRACE_LOOP


def fold_along(raw, c, cells, cost0):
    """the left fold of w along a traced route, from its goal back to its start, each weight formed by the header's formula with float32
    scalars (no plane of weights): what D(start) must equal bit for bit"""
    hgt = heights(raw, c)
    cell = F(c["cell_size"])
    diag = cell * F(1.41421356)
    v = F(cost0)
    for (ax, ay), (bx, by) in reversed(list(zip(cells[:-1], cells[1:]))):
        run = diag if (ax != bx and ay != by) else cell
        rise = hgt[by, bx] - hgt[ay, ax]
        g = np.abs(rise) / run
        up = rise if rise > 0 else F(0)
        down = -rise if rise < 0 else F(0)
        v = v + (((run * (F(1.0) + F(c["grade_weight"]) * g)) + F(c["climb_weight"]) * up) + F(c["descend_weight"]) * down)
    return v

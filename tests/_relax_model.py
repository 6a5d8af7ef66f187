"""Schedule model of the block relaxation: relax_kernel<Rule> and relax_sweeps of csrc/bt_relax.hpp, emulated sweep by sweep in numpy.

TEST INFRASTRUCTURE ONLY.  Imports nothing of the product.  What it emulates is the PROTOCOL, not the fields: blocks of 32 x 32 cells
with a one-cell halo staged at the moment a block runs, at most 64 rounds a block, the write-back of the changed cells, the nine flag bits
in the other flag map, the count of blocks that flagged anything, and the host's batches of 4, 8, 16, then 32 sweeps.  The four rules
(path, fill, flat, accumulate) are restated on the staged tile; the planes that the calls build around their relaxations (the heights and
goals of the path field; z and the initial W, the seed of F, the directions and the initial A of drainage) are restated here or handed in
from the sequential models.

What concurrent workgroups may read is bracketed by the ORDERS: blocks run one after the other in ascending, descending or a seeded random
order, each staging the planes as they stand (the most a block can see of its neighbours' work in the same sweep), or "stale": every block
stages the planes as they stood when the sweep began (the least).  Rounds inside a block are Jacobi: every cell reads the tile of the round
before.  The device's rounds are in place and can only be faster, so a sweep count from here is an upper-ish figure: good for choosing
scenes, never an expected value.

The switches weaken THE MODEL, never a kernel: `drop` leaves out flag bits, `own_block_only` flags only the goal's own block, and
`halo_corners=False` leaves the four corner cells of the halo at the rule's outside words."""
import numpy as np

BLOCK, TILE, ROUNDS = 32, 34, 64
BATCH_FIRST, BATCH_MAX = 4, 32
NONE = np.uint32(0xFFFFFFFF)
NEIGHBOURS = [(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)]
OUTLET, VOID = 8, 255

# name: (bit, dx, dy) of the block the bit flags.  INITIAL is the model's own: "flagged by the caller", in the log only
BITS = {"left": (1, -1, 0), "right": (2, 1, 0), "up": (4, 0, -1), "down": (8, 0, 1), "up_left": (16, -1, -1), "up_right": (32, 1, -1), "down_left": (64, -1, 1),
        "down_right": (128, 1, 1), "self": (256, 0, 0)}
CARDINAL, DIAGONAL = ("left", "right", "up", "down"), ("up_left", "up_right", "down_left", "down_right")
INITIAL = 512
ORDERS = ("ascending", "descending", "random", "stale")

F32 = np.float32
INF_BITS, NAN_BITS = np.uint32(0x7F800000), np.uint32(0x7FC00000)


def nb(tile, k):
    """the 32 x 32 view of neighbour k of every cell of the block, on a staged 34 x 34 tile"""
    dx, dy = NEIGHBOURS[k]
    return tile[1 + dy:1 + dy + BLOCK, 1 + dx:1 + dx + BLOCK]


def own(tile):
    return tile[1:1 + BLOCK, 1:1 + BLOCK]


# ---------------------------------------------------------------------------------------------- the rules, on uint32 words

class FillRule:
    """X = max(z, min over neighbours), descending.  a = z (0: void or outside), x = X (NONE on void cells and outside)"""
    outside_a, outside_x = np.uint32(0), NONE

    def cell(self, ta):
        return own(ta)

    def step(self, ta, tx, a):
        x = own(tx)
        m = nb(tx, 0)
        for k in range(1, 8):
            m = np.minimum(m, nb(tx, k))
        return np.where(a == 0, x, np.minimum(x, np.maximum(a, m)))


class FlatRule:
    """X = 1 + min over the neighbours of equal W, descending.  a = the final W (NONE: void or outside), x = F (NONE: not reached)"""
    outside_a, outside_x = NONE, NONE

    def cell(self, ta):
        return own(ta)

    def step(self, ta, tx, a):
        x = own(tx)
        m = np.full((BLOCK, BLOCK), NONE, np.uint32)
        for k in range(8):
            m = np.minimum(m, np.where(nb(ta, k) == a, nb(tx, k), NONE))
        return np.where((a == NONE) | (x == 0) | (m == NONE), x, np.minimum(x, m + np.uint32(1)))


class AccumulateRule:
    """X = w + the sum over the neighbours that point at the cell, ascending.  a = direction | w << 8, x = A; the sum wraps at 32 bits"""
    outside_a, outside_x = np.uint32(VOID), NONE

    def cell(self, ta):
        return own(ta)

    def step(self, ta, tx, a):
        total = a >> np.uint32(8)
        for k in range(8):
            total = total + np.where((nb(ta, k) & np.uint32(255)) == np.uint32((k + 4) & 7), nb(tx, k), np.uint32(0))
        return np.where((a & np.uint32(255)) == np.uint32(VOID), own(tx), total)


class PathRule:
    """D = min(D, min over neighbours of D + w), descending.  a = the bits of the height (NaN: blocked or outside), x = the bits of D.
    The cell's state is its eight weights, formed once from the staged heights, float32 with one rounding per written operation"""
    outside_a, outside_x = NAN_BITS, INF_BITS

    def __init__(self, cost):
        self.cell_size = F32(cost["cell_size"])
        self.diag = self.cell_size * F32(1.41421356)
        self.max_grade, self.gw, self.cw, self.dw = (F32(cost[f]) for f in ("max_grade", "grade_weight", "climb_weight", "descend_weight"))

    def cell(self, ta):
        h = ta.view(F32)
        ha = own(h)
        w = np.empty((8, BLOCK, BLOCK), F32)
        with np.errstate(invalid="ignore", over="ignore"):
            for k, (dx, dy) in enumerate(NEIGHBOURS):
                run = self.diag if k & 1 else self.cell_size
                rise = nb(h, k) - ha
                g = np.abs(rise) / run
                ok = g <= self.max_grade  # a NaN height on either side fails
                up, down = np.where(rise > 0, rise, F32(0)), np.where(rise < 0, -rise, F32(0))
                wk = ((run * (F32(1) + self.gw * g)) + self.cw * up) + self.dw * down
                if k & 1:  # no corner cutting: both cells beside the diagonal are free
                    hx, hy = h[1:1 + BLOCK, 1 + dx:1 + dx + BLOCK], h[1 + dy:1 + dy + BLOCK, 1:1 + BLOCK]
                    ok = ok & ~np.isnan(hx) & ~np.isnan(hy)
                w[k] = np.where(ok, wk, F32(np.inf))
        return w

    def step(self, ta, tx, w):
        d = tx.view(F32)
        best = own(d)
        with np.errstate(invalid="ignore"):
            for k in range(8):
                cand = nb(d, k) + w[k]
                best = np.where(cand < best, cand, best)
        return np.ascontiguousarray(best, F32).view(np.uint32)


# ---------------------------------------------------------------------------------------------- the skeleton

class Result:
    """x: the final plane of words (h, w) uint32; sweeps: how many the host launched (whole batches); quiet: the first sweep, counted from
    1, that flagged nothing (what a host that looked after every sweep would have launched); converged; log: per sweep {(bx, by): the OR
    of the bits that flagged the block, each bit as its sender set it (INITIAL: the caller)}; limited: {(sweep, bx, by)} of the blocks that
    stopped at the round limit; changed: per sweep the number of cells written back"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def relax(rule, a, x, flags, order="ascending", seed=0, drop=(), halo_corners=True, rounds=ROUNDS):
    """one call's sweeps.  a, x: (h, w) planes of words; flags: (blocks_y, blocks_x) the caller's initial flags; drop: names of BITS
    that are never set"""
    assert order in ORDERS
    a, x = np.asarray(a, np.uint32), np.asarray(x, np.uint32)
    h, w = a.shape
    by_n, bx_n = (h + BLOCK - 1) // BLOCK, (w + BLOCK - 1) // BLOCK
    assert np.shape(flags) == (by_n, bx_n)
    drop_mask = sum(BITS[name][0] for name in drop)
    # the planes with the outside words around them, out to whole blocks plus the halo: a tile is a slice
    A = np.full((by_n * BLOCK + 2, bx_n * BLOCK + 2), rule.outside_a, np.uint32)
    X = np.full(A.shape, rule.outside_x, np.uint32)
    A[1:h + 1, 1:w + 1], X[1:h + 1, 1:w + 1] = a, x
    inside = np.zeros(A.shape, bool)
    inside[1:h + 1, 1:w + 1] = True
    rng = np.random.default_rng(seed)
    active = {(bx, by): INITIAL for by in range(by_n) for bx in range(bx_n) if flags[by][bx]}
    log, limited, changed_cells = [], set(), []

    def one_sweep(sweep):
        nonlocal active
        log.append(dict(active))
        blocks = sorted(active, key=lambda b: (b[1], b[0]))
        if order == "descending":
            blocks.reverse()
        elif order == "random":
            blocks = [blocks[i] for i in rng.permutation(len(blocks))]
        source = X.copy() if order == "stale" else X
        activate, marked, written = {}, 0, 0
        for bx, by in blocks:
            ys, xs = slice(by * BLOCK, by * BLOCK + TILE), slice(bx * BLOCK, bx * BLOCK + TILE)
            ta, tx = A[ys, xs].copy(), source[ys, xs].copy()
            if not halo_corners:
                for cy, cx in ((0, 0), (0, TILE - 1), (TILE - 1, 0), (TILE - 1, TILE - 1)):
                    ta[cy, cx], tx[cy, cx] = rule.outside_a, rule.outside_x
            x_in = own(tx).copy()
            cell = rule.cell(ta)
            more = True
            for _ in range(rounds):
                new = rule.step(ta, tx, cell)
                more = bool((new != own(tx)).any())
                if not more:
                    break
                tx[1:1 + BLOCK, 1:1 + BLOCK] = new
            moved = own(tx) != x_in
            assert not moved[~inside[ys, xs][1:1 + BLOCK, 1:1 + BLOCK]].any(), "a rule moved a cell outside the window"
            X[ys, xs][1:1 + BLOCK, 1:1 + BLOCK][moved] = own(tx)[moved]
            written += int(moved.sum())
            l, r, u, d = moved[:, 0].any(), moved[:, -1].any(), moved[0, :].any(), moved[-1, :].any()
            mask = (1 if l else 0) | (2 if r else 0) | (4 if u else 0) | (8 if d else 0) | (16 if moved[0, 0] else 0) | (32 if moved[0, -1] else 0) | \
                   (64 if moved[-1, 0] else 0) | (128 if moved[-1, -1] else 0) | (256 if more else 0)
            if more:
                limited.add((sweep, bx, by))
            mask &= ~drop_mask
            flagged = False
            for bit, dx, dy in BITS.values():
                nx, ny = bx + dx, by + dy
                if mask & bit and 0 <= nx < bx_n and 0 <= ny < by_n:
                    activate[(nx, ny)] = activate.get((nx, ny), 0) | bit
                    flagged = True
            marked += flagged
        active = activate
        changed_cells.append(written)
        return marked

    cells = h * w
    sweeps, batch, converged, quiet = 0, BATCH_FIRST, False, None
    while not converged and sweeps < cells:
        marked = 0
        for _ in range(min(batch, cells - sweeps)):
            marked = one_sweep(sweeps) if active else 0
            sweeps += 1
            if marked == 0 and quiet is None:
                quiet = sweeps
        converged = marked == 0
        batch = min(2 * batch, BATCH_MAX)
    return Result(x=X[1:h + 1, 1:w + 1].copy(), sweeps=sweeps, quiet=quiet, converged=converged, log=log, limited=limited, changed=changed_cells)


# ---------------------------------------------------------------------------------------------- the planes around the relaxations

def shifted(plane, dx, dy, fill):
    """out[y, x] = plane[y + dy, x + dx], `fill` where that lies outside"""
    h, w = plane.shape
    out = np.full_like(plane, fill)
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    out[yd, xd] = plane[ys, xs]
    return out


def all_blocks(shape):
    return np.ones(((shape[0] + BLOCK - 1) // BLOCK, (shape[1] + BLOCK - 1) // BLOCK), bool)


def void_cells(raw, void=None):
    out = np.asarray(raw) == 0
    return out | (np.asarray(void) != 0) if void is not None else out


def fill(raw, void=None, **kw):
    """drain_prepare_kernel, then the fill -> (W (h, w) uint16, Result)"""
    is_void = void_cells(raw, void)
    outlet = np.zeros(is_void.shape, bool)
    for dx, dy in NEIGHBOURS:
        outlet |= shifted(is_void, dx, dy, True)
    z = np.where(is_void, 0, raw).astype(np.uint32)
    x0 = np.where(is_void, NONE, np.where(outlet, z, np.uint32(65535))).astype(np.uint32)
    res = relax(FillRule(), z, x0, all_blocks(z.shape), **kw)
    return np.where(is_void, 0, res.x).astype(np.uint16), res


def flat(raw, void, W, **kw):
    """drain_flat_seed_kernel on the final W, then the flat distance -> (F (h, w) uint32, Result)"""
    is_void = void_cells(raw, void)
    a = np.where(is_void, NONE, W).astype(np.uint32)
    drain = np.zeros(is_void.shape, bool)
    for dx, dy in NEIGHBOURS:
        drain |= shifted(is_void, dx, dy, True) | (shifted(a, dx, dy, NONE) < a)  # an outlet, or a lower neighbour (a void one is NONE: never lower)
    x0 = np.where(is_void | ~drain, NONE, np.uint32(0)).astype(np.uint32)
    res = relax(FlatRule(), a, x0, all_blocks(a.shape), **kw)
    return np.where(is_void, 0, res.x).astype(np.uint32), res


def accumulate(direction, weight=None, **kw):
    """the words drain_direction_kernel leaves (the direction plane is the caller's), then the accumulation -> (A (h, w) uint32, Result)"""
    direction = np.asarray(direction)
    is_void = direction == VOID
    wt = np.ones(direction.shape, np.uint32) if weight is None else np.asarray(weight).astype(np.uint32)
    a = direction.astype(np.uint32) | wt << np.uint32(8)  # (a void cell's weight is in its word too, and never read)
    res = relax(AccumulateRule(), a, np.where(is_void, np.uint32(0), wt), all_blocks(a.shape), **kw)
    return res.x, res


def path(raw, mask, cost, goals, own_block_only=False, **kw):
    """path_prepare_kernel, then the path field -> (D (h, w) float32, Result)"""
    raw = np.asarray(raw)
    blocked = void_cells(raw, mask)
    lo, hi = F32(cost["min_height"]), F32(cost["max_height"])
    hgt = np.where(blocked, F32(np.nan), lo + (hi - lo) * (raw.astype(F32) / F32(65535.0))).astype(F32)
    D = np.full(raw.shape, np.inf, F32)
    flags = ~all_blocks(raw.shape)
    for g in goals:
        gx, gy, c0 = int(g[0]), int(g[1]), F32(g[2] if len(g) > 2 else 0.0) + F32(0.0)
        if blocked[gy, gx]:
            continue
        D[gy, gx] = min(D[gy, gx], c0)
        bx, by = gx // BLOCK, gy // BLOCK
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if (dx or dy) and own_block_only:
                    continue
                if 0 <= bx + dx < flags.shape[1] and 0 <= by + dy < flags.shape[0]:
                    flags[by + dy, bx + dx] = True
    res = relax(PathRule(cost), hgt.view(np.uint32), D.view(np.uint32), flags, **kw)
    return res.x.view(F32), res

"""The scenes of bt_atlas_drainage shared by tests/test_drain_model.py (no GPU: every scene reaches what it is named for, on the model alone)
and tests/test_gpu_drain.py (the device against the model).

TEST INFRASTRUCTURE ONLY.  The atlases are those of tests/_splat_cases.py (attachment 1 = H, the R16 heights, with its planted no-data
texels): T = 16 and 72, planar, `partial` (tiles missing) and a cube.  A scene is a window of H, optionally a void mask and a weight plane,
and optionally a `plant`: a function from the window's texels as the jobs left them to the texels the scene wants, which the GPU test writes
over the whole window with write_region before the call (so planted scenes share one atlas per spec, kept apart from the one the
unplanted scenes read).  Without a GPU the window's texels come from the CPU oracle's state of the same jobs through the model of
bt_atlas_read_region.  No window exceeds 96 x 96."""
import functools

import numpy as np

import _drain_model as M
import _paint_model as PM
import _splat_cases as SC

ROUNDS = 64  # kRelaxRounds: rounds of one block in one sweep, at most
BLOCK = 32


def Scene(spec, rect, plant=None, void=None, weight=None, side=0, lod=None, reach=()):
    """rect (x0, y0, w, h) in mosaic texels; plant: raw (h, w) uint16 -> texels (h, w) uint16 (finest LOD only); void / weight: (h, w) uint8
    or None; reach: names of scene_reaches() that must hold"""
    assert rect[2] <= 96 and rect[3] <= 96 and (plant is None or lod is None)
    return dict(spec=spec, rect=rect, plant=plant, void=void, weight=weight, side=side, lod=lod, reach=set(reach))


def random_bytes(h, w, seed, share=None):
    """share: a 0 / 1 mask with that share of ones; None: bytes 0..255"""
    rng = np.random.default_rng(seed)
    return (rng.random((h, w)) < share).astype(np.uint8) if share is not None else rng.integers(0, 256, (h, w)).astype(np.uint8)


# ---------------------------------------------------------------------------------------------- plants

def quantised(raw):
    """three levels: large flats and many ties; no-data texels stay"""
    q = (raw.astype(np.int64) * 3 // 65536 + 1) * 20000
    return np.where(raw == 0, 0, q).astype(np.uint16)


def random_void(share, seed):
    def plant(raw):
        return np.where(random_bytes(*raw.shape, seed, share) != 0, 0, raw).astype(np.uint16)
    return plant


def chebyshev(h, w, cx, cy):
    y, x = np.mgrid[0:h, 0:w]
    return np.maximum(np.abs(x - cx), np.abs(y - cy))


def bowl(island):
    """70 x 70: a bowl around the corner of four blocks (its pit: cells 31..32 in both axes), z = 10000 + 300 r with r the Chebyshev distance
    from (31.5, 31.5).  The lowest way out is a level trench at 15000 along y = 40 from x = 40 to the window's edge at (69, 40), in the block
    (2, 1): the lake (r <= 16.5: cells 15..48) fills to 15000 across the four blocks and spills in a fifth.  island: a crater on an island in
    the lake, r < 5.5 at 16000 + 100 r inside a wall (r = 5.5) of 18000 with a notch of 17000 at (37, 31): a lake at 17000 that spills into
    the one at 15000"""
    def plant(raw):
        r = chebyshev(70, 70, 31.5, 31.5)
        z = 10000 + 300 * r
        z[:, 69] = 50000
        z[40, 40:70] = 15000
        if island:
            z = np.where(r < 5.5, 16000 + 100 * r, z)
            z[r == 5.5] = 18000
            z[31, 37] = 17000
        return z.astype(np.uint16)
    return plant


def plateau(hole):
    def plant(raw):
        z = np.full((70, 70), 30000, np.uint16)
        if hole:
            z[35, 35] = 0
        return z
    return plant


def serpentine_channel(n):
    """(n, n) bool: a channel one cell wide along the odd rows 1..n - 3 (x = 1..n - 2), joined alternately at x = n - 2 and x = 1.  Row 1 is
    walked from the left; where n = 32 the last row, 29, is walked from the left too and ends at (30, 29)"""
    c = np.zeros((n, n), bool)
    for i, y in enumerate(range(1, n - 2, 2)):
        c[y, 1:n - 1] = True
        if y + 1 < n - 2:
            c[y + 1, n - 2 if i % 2 == 0 else 1] = True
    return c


def banded_channel():
    """(96, 96) bool, nine blocks: three bands, one per column of blocks (x = 1..30, 33..62, 65..94), each a serpentine over the odd rows
    1..93 with rows of 30 cells; the first band is walked downwards from (1, 1), the second upwards, the third downwards again, joined by
    (31..32, 93) and (63..64, 1).  4372 cells, 68 times ROUNDS; some 470 of them in every block, which the walk enters once, through an
    edge: leftwards never, rightwards twice, downwards four times, upwards twice.  Rows as wide as the window would let a sweep that runs
    its blocks one after the other carry the news through three blocks; rows of one block do not"""
    c = np.zeros((96, 96), bool)
    for band in range(3):
        x0, x1 = 32 * band + 1, 32 * band + 30
        rows = list(range(1, 94, 2))[::-1 if band % 2 else 1]
        for i, y in enumerate(rows):
            c[y, x0:x1 + 1] = True
            if i + 1 < len(rows):
                c[(y + rows[i + 1]) // 2, x1 if i % 2 == 0 else x0] = True
        if band < 2:
            c[rows[-1], x1 + 1:x1 + 3] = True
    return c


def serpentine(n):
    """n x n: ridges of 60000, a level channel of 1000 inside a ring of ridge (the window's edge) whose one gap is (0, 1).  n = 32, one
    block: serpentine_channel, some 460 cells to walk, seven times ROUNDS.  n = 96: banded_channel"""
    def plant(raw):
        c = serpentine_channel(n) if n == 32 else banded_channel()
        c[1, 0] = True
        return np.where(c, 1000, 60000).astype(np.uint16)
    return plant


# the bit a block sets for the neighbour block at (dx, dy), by name (tests/_relax_model.BITS)
BIT_NAMES = {(-1, 0): "left", (1, 0): "right", (0, -1): "up", (0, 1): "down", (-1, -1): "up_left", (1, -1): "up_right", (-1, 1): "down_left", (1, 1): "down_right"}
CROSSINGS = {  # name: (kind, mirrored in x, mirrored in y): the bit the serpentine's block sets when the news leaves it
    "down_right": ("corner", False, False), "down_left": ("corner", True, False), "up_right": ("corner", False, True), "up_left": ("corner", True, True),
    "right": ("right", False, False), "left": ("right", True, False), "down": ("down", False, False), "up": ("down", False, True),
}


def crossing_channel(bit, far_open=False):
    """(64, 64) bool, four blocks: the serpentine of one block (serpentine_channel(32), more than 4 x ROUNDS cells) in block (0, 0), a tail
    to the block's border, ONE step into the next block, and a straight channel there that ends one cell short of the window's edge, or on
    it (far_open).  The channel is connected by cardinal steps but for the corner's one diagonal step.
      corner: tail (30, 30), (31, 30), (31, 31); the step to (32, 32); then row 32: only a corner cell of block (0, 0) touches block (1, 1)
      right:  tail (31, 29); the step to (32, 29); then row 29
      down:   tail (30, 30), (30, 31); the step to (30, 32); then column 30
    and mirrored in x and / or y for the other bits (the serpentine stays one of rows, which lanes walk in lockstep)"""
    kind, mirror_x, mirror_y = CROSSINGS[bit]
    c = np.zeros((64, 64), bool)
    c[:32, :32] = serpentine_channel(32)
    end = 64 if far_open else 63
    if kind == "corner":
        c[30, 30] = c[30, 31] = c[31, 31] = True
        c[32, 32:end] = True
    elif kind == "right":
        c[29, 31:end] = True
    else:
        c[30:end, 30] = True
    return c[::-1 if mirror_y else 1, ::-1 if mirror_x else 1]


def crossing(bit, upstream):
    """64 x 64: ridges of 60000 around crossing_channel(bit) at 1000.  upstream False: the one outlet of the channel is the gap beside the
    serpentine's first cell, so the level and the flat distance walk the serpentine for more than four sweeps and then step into a block
    that went quiet long before.  upstream True: the outlet is the far channel's end on the window's edge, so the sums walk that way"""
    def plant(raw):
        c = crossing_channel(bit, far_open=upstream).copy()
        if not upstream:
            _, mirror_x, mirror_y = CROSSINGS[bit]
            c[62 if mirror_y else 1, 63 if mirror_x else 0] = True
        return np.where(c, 1000, 60000).astype(np.uint16)
    return plant


# drops (cardinal a, diagonal b) of the centre of a 3 x 3: Pell pairs, b^2 - 2 a^2 = -1 or +1 by turns, so the scores 2 a^2 and b^2 differ by
# one; the last five overflow 32 bits in one score or both.  The issue's last pair names b = 65535, which no window holds: heights are
# 1..65535, so the largest drop is 65534, as the header says of the score; (46341, 65534) is that case (2 a^2 >= 2^32 > b^2)
SCORE_PAIRS = [(5, 7), (12, 17), (29, 41), (169, 239), (985, 1393), (5741, 8119), (33461, 47321), (46341, 65534)]


def score_window(a, b, turn):
    """5 x 5: a ring of outlets at height 1 around a 3 x 3 of 65535 whose centre has the cardinal neighbour k = 2 turn at 65535 - a and the
    diagonal neighbour k = 2 turn + 3 at 65535 - b: every W equals its z"""
    def plant(raw):
        z = np.full((5, 5), 1, np.uint16)
        z[1:4, 1:4] = 65535
        for k, drop in ((2 * turn, a), ((2 * turn + 3) % 8, b)):
            dx, dy = M.NEIGHBOURS[k]
            z[2 + dy, 2 + dx] = 65535 - drop
        return z
    return plant


def funnel(raw):
    """66 x 66: a ring of 60000 (the window's edge: outlets that receive nothing) with one gap of 100 at (0, 33), and inside it
    1000 + 100 d with d the Chebyshev distance from the gap: every inner cell has a lower inner neighbour or the gap, so all 64 x 64 of
    them drain through the gap"""
    z = 1000 + 100 * chebyshev(66, 66, 0, 33)
    z[0, :] = z[65, :] = z[:, 0] = z[:, 65] = 60000
    z[33, 0] = 100
    return z.astype(np.uint16)


# ---------------------------------------------------------------------------------------------- the scenes

SCENES = {
    "one_cell": Scene("planar_b2", (13, 15, 1, 1)),
    "one_row": Scene("planar_b2", (5, 7, 7, 1)),
    "one_column": Scene("planar_b2", (7, 5, 1, 7)),
    # pits in four blocks
    "bowl": Scene("planar_72", (70, 71, 70, 70), plant=bowl(False), reach={"lake_in_four_blocks", "spill_in_a_fifth"}),
    "bowl_with_island_lake": Scene("planar_72", (70, 71, 70, 70), plant=bowl(True), reach={"lake_in_four_blocks", "spill_in_a_fifth", "two_lake_levels"}),
    "plateau": Scene("planar_72", (70, 71, 70, 70), plant=plateau(False), reach={"flat_34"}),
    "plateau_with_a_hole": Scene("planar_72", (70, 71, 70, 70), plant=plateau(True), reach={"outlet_inside"}),
    "serpentine": Scene("planar_72", (75, 77, 32, 32), plant=serpentine(32), reach={"long_chain", "long_flat"}),
    # void cells
    "random_void": Scene("planar_72", (70, 71, 50, 45), plant=random_void(0.3, 5), reach={"planted_zeros"}),
    "missing_tiles": Scene("partial", (0, 0, 48, 48), reach={"tiles_missing"}),
    "void_mask": Scene("planar_b2", (27, 36, 13, 11), void=random_bytes(11, 13, 6, 0.3), reach={"mask_only"}),
    "all_three_voids": Scene("partial", (0, 0, 48, 48), void=random_bytes(48, 48, 7, 0.3), reach={"tiles_missing", "planted_zeros", "mask_and_zeros"}),
    # weights
    "funnel_255": Scene("planar_72", (70, 71, 66, 66), plant=funnel, weight=np.full((66, 66), 255, np.uint8), reach={"one_outlet_takes_all"}),
    "weights_zero": Scene("planar_72", (3, 5, 40, 33), weight=np.zeros((33, 40), np.uint8)),
    "weights_random": Scene("planar_72", (3, 5, 40, 33), weight=random_bytes(33, 40, 8)),
    # placement: another side of a cube, a LOD below the top (the mosaic of lod 1 is 136 across), origins that are no tile's
    "cube_side": Scene("cube_3", (5, 3, 40, 37), side=4),
    "lod_below_the_top": Scene("planar_72", (5, 6, 60, 50), lod=1),
}
SIZES = []  # widths around the block size against heights 33 and 65, on the jobs' heights and quantised to three levels
for _w in (31, 32, 33, 63, 64, 65):
    for _h in (33, 65):
        SCENES[f"w{_w}_h{_h}"] = Scene("planar_72", (3, 5, _w, _h))
        SCENES[f"w{_w}_h{_h}_quantised"] = Scene("planar_72", (3, 5, _w, _h), plant=quantised, reach={"big_flats"})
        SIZES += [f"w{_w}_h{_h}", f"w{_w}_h{_h}_quantised"]
# the protocol of the block relaxation (tests/_relax_model.py, tests/test_relax_model.py): a crossing per flag bit, in both roles, and the
# long walk into the host loop's steady batch
CROSSING_SCENES = []  # every corner in both roles; of the edges those that no other scene already needs (test_relax_model.py names which does)
for _bit, _roles in (("down_right", (False, True)), ("down_left", (False, True)), ("up_right", (False, True)), ("up_left", (False, True)), ("left", (False, True)),
                     ("right", (True,)), ("up", (True,))):
    for _upstream in _roles:
        _name = f"crossing_{_bit}_upstream" if _upstream else f"crossing_{_bit}"
        SCENES[_name] = Scene("planar_72", (70, 71, 64, 64), plant=crossing(_bit, _upstream), reach={"long_chain", "long_flat", ("late_sum_" if _upstream else "late_level_") + _bit})
        CROSSING_SCENES.append(_name)
SCENES["long_walk"] = Scene("planar_72", (151, 69, 96, 96), plant=serpentine(96), reach={"long_chain", "long_flat", "walk_of_56_sweeps"})
SCORES = []
for _i, (_a, _b) in enumerate(SCORE_PAIRS):
    SCENES[f"score_{_a}_{_b}"] = Scene("planar_b2", (19, 21, 5, 5), plant=score_window(_a, _b, _i % 4), reach={"scores_one_apart_or_past_32_bits"})
    SCORES.append(f"score_{_a}_{_b}")


def geometry(scene):
    spec = SC.SPECS[scene["spec"]]
    lod = spec["lods"] - 1 if scene["lod"] is None else scene["lod"]
    return spec, lod


@functools.lru_cache(maxsize=None)
def window(name):
    """the scene's raw texels (h, w) uint16 and the number of tiles of the window the atlas does not hold, without a GPU"""
    scene = SCENES[name]
    spec, lod = geometry(scene)
    tiles = SC.oracle_state(scene["spec"])[0]
    x0, y0, w, h = scene["rect"]
    raw, missing = PM.read_region(tiles, lod, scene["side"], x0, y0, w, h, spec["b"])
    if scene["plant"] is not None:
        raw = scene["plant"](raw)
        assert raw.shape == (h, w) and raw.dtype == np.uint16
    return raw, missing


@functools.lru_cache(maxsize=None)
def expected(name):
    """(raw, W, F, direction, A, stats) of the model: computed once, shared, not to be written to"""
    scene = SCENES[name]
    raw, missing = window(name)
    W, F, direction, A, stats = M.drainage(raw, scene["void"], scene["weight"])
    stats["tiles_missing"] = missing
    for plane in (raw, W, F, direction, A):
        plane.setflags(write=False)
    return raw, W, F, direction, A, stats


def scene_reaches(name):
    """what a scene's planes reach, by name"""
    scene = SCENES[name]
    raw, W, F, direction, A, stats = expected(name)
    h, w = raw.shape
    void = scene["void"]
    lake = (W > raw) & (direction != M.VOID)
    blocks = lambda cells: {(int(x) // BLOCK, int(y) // BLOCK) for y, x in np.argwhere(cells)}
    out = {"tiles_missing": stats["tiles_missing"] > 0, "flat_34": stats["max_flat_distance"] == 34 and stats["flats"] == 68 * 68}
    # a no-data texel with data to its left and right lies in no missing tile: a tile is 12 texels wide
    out["planted_zeros"] = bool(((raw[:, 1:-1] == 0) & (raw[:, :-2] != 0) & (raw[:, 2:] != 0)).any()) if w > 2 else False
    out["mask_only"] = void is not None and void.any() and not (raw == 0).any()
    out["mask_and_zeros"] = void is not None and bool((void != 0)[raw != 0].any()) and bool((raw == 0).any())
    out["big_flats"] = stats["max_flat_distance"] >= 3 and stats["flats"] > stats["cells"] // 4
    out["outlet_inside"] = h > 40 and w > 40 and direction[34, 34] == M.OUTLET and stats["outlets"] == 4 * 69 + 8
    if lake.any():
        big = lake & (W == 15000)
        out["lake_in_four_blocks"] = blocks(big) == {(0, 0), (1, 0), (0, 1), (1, 1)}
        # the trench's end: the outlet the big lake leaves by, in block (2, 1)
        out["spill_in_a_fifth"] = w == 70 and direction[40, 69] == M.OUTLET and W[40, 69] == 15000 and A[40, 69] > int(big.sum())
        out["two_lake_levels"] = bool((lake & (W == 17000)).any()) and bool(big.any())
    start = np.unravel_index(np.argmax(F), F.shape)
    out["long_flat"] = stats["max_flat_distance"] > 4 * ROUNDS
    out["long_chain"] = direction[start] != M.VOID and M.chain_length(direction, (int(start[1]), int(start[0]))) > 4 * ROUNDS
    out["walk_of_56_sweeps"] = out["long_chain"] and min(stats["max_flat_distance"], M.chain_length(direction, (int(start[1]), int(start[0])))) > 56 * ROUNDS
    # a step of the flow from one block into another, late: the level and the flat distance come UP the flow, out of the receiver's block
    # (F counts the cells they walked), the sums go DOWN it, out of the donor's block (A counts at least the cells they were summed over)
    for (x, y), (rx, ry) in M.receivers(direction).items():
        step = (x // BLOCK - rx // BLOCK, y // BLOCK - ry // BLOCK)
        if step != (0, 0) and W[y, x] == W[ry, rx]:
            if F[y, x] > 4 * ROUNDS:
                out["late_level_" + BIT_NAMES[step]] = True
            if A[y, x] > 4 * ROUNDS and M.chain_length(direction, (x, y)) <= BLOCK + 2:
                out["late_sum_" + BIT_NAMES[(-step[0], -step[1])]] = True
    inner = (h - 2) * (w - 2)
    out["one_outlet_takes_all"] = scene["weight"] is not None and stats["max_accumulation"] == 255 * (inner + 1) and bool((np.sort(A[direction == M.OUTLET])[:-1] == 255).all())
    if name.startswith("score_"):
        a, b = (int(v) for v in name.split("_")[1:])
        k_card, k_diag = [k for k in range(8) if raw[2 + M.NEIGHBOURS[k][1], 2 + M.NEIGHBOURS[k][0]] != 65535]
        if k_card & 1:
            k_card, k_diag = k_diag, k_card
        out["scores_one_apart_or_past_32_bits"] = (abs(2 * a * a - b * b) == 1 or 2 * a * a >= 1 << 32) and direction[2, 2] == (k_card if 2 * a * a > b * b else k_diag) \
            and bool((W == raw).all())
    return out

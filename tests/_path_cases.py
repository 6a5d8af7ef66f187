"""The scenes of bt_atlas_path_field shared by tests/test_path_model.py (no GPU: every scene reaches what it is named for, on the model
alone) and tests/test_gpu_path.py (the device against the model).

TEST INFRASTRUCTURE ONLY.  The atlases are those of tests/_splat_cases.py (attachment 1 = H, the R16 heights, with its planted no-data
texels): T = 16 and 72, planar, `partial` (tiles missing) and a cube.  A scene is a window of H, a cost, goals, optionally a host mask and
`plants`: rectangles of walls (zeros) or of whole texels written over the window with write_region before the call.  Without a GPU the window's
texels come from the CPU oracle's state of the same jobs through the model of bt_atlas_read_region."""
import functools

import numpy as np

import _drain_cases as DC
import _paint_model as PM
import _path_model as M
import _splat_cases as SC

F = np.float32
INF = np.inf
SPAN = dict(min_height=SC.LO, max_height=SC.HI)
# a texel of the T = 16 mosaic (48 across a face of 1000) and of the T = 72 mosaic (272 across)
CELL_16, CELL_72 = 1000.0 / 48.0, 1000.0 / 272.0

WALK = dict(SPAN, grade_weight=2.0, climb_weight=3.0, descend_weight=0.5)


def serpentine(n):
    """(n, n) bool walls: every odd row is a wall with one gap, alternately at the right and the left end"""
    wall = np.zeros((n, n), dtype=bool)
    for i, y in enumerate(range(1, n, 2)):
        wall[y, :] = True
        wall[y, n - 1 if i % 2 == 0 else 0] = False
    return wall


def boxed_pocket(h, w, x, y):
    """a mask that walls the 3 x 3 cells around (x, y) in: the cell is free and cannot be reached"""
    mask = np.zeros((h, w), dtype=np.uint8)
    mask[y - 1:y + 2, x - 1:x + 2] = 1
    mask[y, x] = 0
    return mask


def random_mask(h, w, share, seed, keep=()):
    mask = (np.random.default_rng(seed).random((h, w)) < share).astype(np.uint8)
    for x, y in keep:
        mask[y, x] = 0
    return mask


def Scene(spec, rect, cost, goals, mask=None, plants=(), side=0, lod=None, reach=()):
    """rect (x0, y0, w, h) in mosaic texels; goals (x, y, cost0) in cells of the window; mask: (h, w) uint8 or None; plants: [(x, y, array)]
    in CELLS OF THE WINDOW, a bool array of walls or a uint16 array of whole texels; reach: names of counters of _path_model.field /
    scene_reaches() that must be >= 1"""
    return dict(spec=spec, rect=rect, cost=M.cost(**cost), goals=list(goals), mask=mask, plants=list(plants), side=side, lod=lod, reach=set(reach))


# The protocol of the block relaxation (tests/_relax_model.py, tests/test_relax_model.py).  A corridor is free cells of one height (raw
# 1000) between walls; a pillar is a free cell of raw 65535, some 490 above the corridor over a cell of 3.7: with max_grade 1.5 no step
# onto it or off it passes, cardinal or diagonal, so it is never reached and carries nothing, but it lets the diagonal step beside it pass
# the no-corner-cutting test
FLOOR, PILLAR = 1000, 65535
PILLARS = dict(WALK, cell_size=CELL_72, max_grade=1.5)


def corridor(channel, pillars=()):
    """whole texels: walls but for the channel's cells (FLOOR) and the pillars (x, y)"""
    texels = np.where(channel, FLOOR, 0).astype(np.uint16)
    for x, y in pillars:
        assert texels[y, x] == 0
        texels[y, x] = PILLAR
    return texels


def crossing(bit):
    """64 x 64, _drain_cases.crossing_channel as a corridor: the goal on the serpentine's first cell, more than 4 x ROUNDS cells to the
    block's border, one step into the next block.  At a corner that step is diagonal, and the two cells beside it, one in each of the
    cardinal blocks, are pillars; everything else on the two block borders is wall.  -> (texels, the goal)"""
    kind, mirror_x, mirror_y = DC.CROSSINGS[bit]
    flip = lambda x, y: (63 - x if mirror_x else x, 63 - y if mirror_y else y)
    pillars = [flip(32, 31), flip(31, 32)] if kind == "corner" else []
    return corridor(DC.crossing_channel(bit), pillars), flip(1, 1) + (0.0,)


def goal_in_a_corner():
    """40 x 40: the goal on (31, 31), the last cell of block (0, 0), whose three neighbours there are walls; pillars on (32, 31) and
    (31, 32); a corridor along row 32 of block (1, 1): the only way on from the goal is the diagonal block"""
    c = np.zeros((40, 40), bool)
    c[31, 31] = True
    c[32, 32:39] = True
    return corridor(c, [(32, 31), (31, 32)]), (31, 31, 0.0)


def goal_on_an_edge():
    """40 x 40: the goal on (31, 10), on the right edge of block (0, 0), whose five neighbours there are walls; a corridor along row 10 of
    block (1, 0): the only way on is the cardinal block"""
    c = np.zeros((40, 40), bool)
    c[10, 31:39] = True
    return corridor(c), (31, 10, 0.0)


# three goals of different cost0: a plain one, one beside it that it dominates, one on a planted no-data texel (window (3, 5, ...) of the
# T = 72 mosaic: the hole block of _splat_cases.HOLES at mosaic (14..17, 5..8) is cells (11..14, 0..3))
THREE_GOALS = [(20, 20, 0.5), (21, 20, 1000.0), (12, 2, 0.0)]

SCENES = {
    "one_cell": Scene("planar_b2", (13, 15, 1, 1), dict(SPAN, cell_size=CELL_16), [(0, 0, 2.0)]),
    "one_row": Scene("planar_b2", (5, 7, 40, 1), dict(WALK, cell_size=CELL_16), [(3, 0, 0.0)]),
    "one_column": Scene("planar_b2", (7, 5, 1, 40), dict(WALK, cell_size=CELL_16), [(0, 36, 1.0)]),
    "w31": Scene("planar_72", (3, 5, 31, 40), dict(WALK, cell_size=CELL_72, max_grade=1.5), THREE_GOALS, reach={"dominated_goals", "goals_blocked", "corner_cut", "grade_cut"}),
    "w32": Scene("planar_72", (3, 5, 32, 40), dict(WALK, cell_size=CELL_72, max_grade=1.5), THREE_GOALS, reach={"dominated_goals", "goals_blocked", "corner_cut"}),
    "w33": Scene("planar_72", (3, 5, 33, 40), dict(WALK, cell_size=CELL_72, max_grade=1.5), THREE_GOALS, reach={"dominated_goals", "goals_blocked", "corner_cut"}),
    "w65": Scene("planar_72", (3, 5, 65, 40), dict(WALK, cell_size=CELL_72, max_grade=1.5), THREE_GOALS + [(64, 39, 7.0)],
                 reach={"dominated_goals", "goals_blocked", "corner_cut", "grade_cut", "several_blocks"}),
    # all weights zero and no grade limit: pure distance; the route from (32, 32) to the goal at (20, 20) leaves its block through the corner
    "pure_distance_through_a_block_corner": Scene("planar_72", (3, 5, 65, 40), dict(SPAN, cell_size=CELL_72), [(20, 20, 0.0)], reach={"block_corner", "corner_cut"}),
    "grade_unlimited": Scene("planar_72", (69, 70, 50, 45), dict(WALK, cell_size=CELL_72, max_grade=INF), [(5, 40, 0.0), (44, 3, 2.5)]),
    "grade_tight": Scene("planar_72", (69, 70, 50, 45), dict(WALK, cell_size=CELL_72, max_grade=0.6), [(5, 40, 0.0), (44, 3, 2.5)], reach={"grade_cut"}),
    # the whole face of the atlas whose job covered (0.3, 0.3) .. (0.9, 0.9) only: tiles the atlas does not hold are blocked
    "missing_tiles": Scene("partial", (0, 0, 48, 48), dict(WALK, cell_size=CELL_16), [(24, 24, 0.0), (2, 2, 0.0)], reach={"tiles_missing", "goals_blocked"}),
    "missing_tiles_odd_window": Scene("partial", (7, 9, 35, 31), dict(WALK, cell_size=CELL_16, max_grade=2.0), [(20, 18, 0.0)], reach={"tiles_missing"}),
    # a window without a no-data texel: the host mask is the only source of blocked cells, and walls one cell in
    "mask_alone": Scene("planar_b2", (27, 36, 13, 11), dict(WALK, cell_size=CELL_16), [(1, 1, 0.0)], mask=boxed_pocket(11, 13, 8, 6), reach={"mask_only", "unreachable"}),
    "mask_and_holes": Scene("planar_b2", (1, 2, 45, 44), dict(WALK, cell_size=CELL_16), [(40, 40, 0.0), (3, 3, 4.0)],
                            mask=random_mask(44, 45, 0.15, 3, keep=[(40, 40), (3, 3)]) | boxed_pocket(44, 45, 30, 8), reach={"unreachable", "corner_cut", "holes_and_mask"}),
    # the 96 x 96 serpentine maze over four tiles of the T = 72 mosaic, at an odd origin: its route is thousands of cells long, the path
    # field's long walk into the host loop's steady batch
    "maze": Scene("planar_72", (151, 69, 96, 96), dict(WALK, cell_size=CELL_72), [(0, 0, 0.0), (50, 0, 5000.0), (3, 1, 0.0)],
                  plants=[(0, 0, serpentine(96))], reach={"corner_cut", "long_route", "route_of_56_sweeps", "goals_blocked", "dominated_goals", "several_blocks"}),
    "cube_face": Scene("cube_3", (5, 3, 40, 37), dict(WALK, cell_size=CELL_16, max_grade=3.0), [(30, 30, 0.0), (2, 33, 1.0)], side=4, reach={"corner_cut"}),
}
WIDTHS = ["w31", "w32", "w33", "w65"]
CROSSING_SCENES = []  # every corner; of the edges the one the maze does not need (its route never enters a block upwards)
for _bit in ("down_right", "down_left", "up_right", "up_left", "up"):
    _texels, _goal = crossing(_bit)
    SCENES[f"crossing_{_bit}"] = Scene("planar_72", (70, 71, 64, 64), PILLARS, [_goal], plants=[(0, 0, _texels)], reach={f"late_step_{_bit}"} |
                                       ({"unreachable", "grade_cut", "pillars_beside_a_block_corner"} if _bit != "up" else set()))
    CROSSING_SCENES.append(f"crossing_{_bit}")
for _name, (_texels, _goal), _reach in (("goal_in_a_corner", goal_in_a_corner(), "goal_leaves_by_the_corner"), ("goal_on_an_edge", goal_on_an_edge(), "goal_leaves_by_the_edge")):
    SCENES[_name] = Scene("planar_72", (70, 71, 40, 40), PILLARS, [_goal], plants=[(0, 0, _texels)], reach={_reach})


def geometry(scene):
    spec = SC.SPECS[scene["spec"]]
    lod = spec["lods"] - 1 if scene["lod"] is None else scene["lod"]
    return spec, lod


def planted(raw, scene):
    """the window's texels after the scene's plants: where a bool plant is True (a wall) the texel becomes 0; a uint16 plant replaces the
    texels"""
    raw = raw.copy()
    for x, y, plant in scene["plants"]:
        part = raw[y:y + plant.shape[0], x:x + plant.shape[1]]
        if plant.dtype == bool:
            part[plant] = 0
        else:
            part[...] = plant
    return raw


@functools.lru_cache(maxsize=None)
def window(name):
    """the scene's raw texels (h, w) uint16 and the number of tiles of the window the atlas does not hold, without a GPU"""
    scene = SCENES[name]
    spec, lod = geometry(scene)
    tiles = SC.oracle_state(scene["spec"])[0]
    x0, y0, w, h = scene["rect"]
    raw, missing = PM.read_region(tiles, lod, scene["side"], x0, y0, w, h, spec["b"])
    return planted(raw, scene), missing


@functools.lru_cache(maxsize=None)
def expected(name):
    """(raw, D, next, stats, reached) of the model: computed once, shared, not to be written to"""
    scene = SCENES[name]
    raw, missing = window(name)
    reached = {}
    D, nxt, stats = M.field(raw, scene["mask"], scene["cost"], scene["goals"], reached)
    stats["tiles_missing"] = missing
    reached.update(scene_reaches(scene, raw, D, nxt, stats))
    for plane in (raw, D, nxt):
        plane.setflags(write=False)
    return raw, D, nxt, stats, reached


def scene_reaches(scene, raw, D, nxt, stats):
    """counters of what a scene's shape reaches beyond those of _path_model.field"""
    h, w = raw.shape
    out = dict(goals_blocked=stats["goals_blocked"], tiles_missing=stats["tiles_missing"], several_blocks=int(w > 32 or h > 32))
    mask = scene["mask"]
    out["mask_only"] = int(mask is not None and mask.any() and not (raw == 0).any())
    out["holes_and_mask"] = int(mask is not None and mask.any() and (raw == 0).any())
    out["block_corner"] = int(w > 32 and h > 32 and nxt[32, 32] == 5)  # (32, 32) steps to (31, 31): across the corner of four blocks
    start = np.unravel_index(np.argmax(np.where(np.isinf(D), -1.0, D)), D.shape)
    cells, status = M.trace(nxt, (start[1], start[0]))
    out["long_route"] = int(status == M.TRACE_OK and len(cells) >= 2000)
    out["route_of_56_sweeps"] = int(status == M.TRACE_OK and len(cells) > 56 * DC.ROUNDS)
    # a step of a route from one block into another, late: the field comes up the route, out of the block of the cell stepped to, after
    # as many cells as the cost counts (a corridor of one height: a cell_size each, or more)
    late = F(4 * DC.ROUNDS) * F(scene["cost"]["cell_size"]) * F(1.41421356)
    for y, x in np.argwhere((nxt < 8) & (D > late)):
        dx, dy = M.NEIGHBOURS[int(nxt[y, x])]
        step = (int(x) // DC.BLOCK - int(x + dx) // DC.BLOCK, int(y) // DC.BLOCK - int(y + dy) // DC.BLOCK)
        if step != (0, 0):
            out["late_step_" + DC.BIT_NAMES[step]] = out.get("late_step_" + DC.BIT_NAMES[step], 0) + 1
    free = (raw != 0) if mask is None else (raw != 0) & (mask == 0)
    pillar = free & np.isinf(D)
    out["pillars_beside_a_block_corner"] = int(h > 32 and w > 32 and ((pillar[31, 32] and pillar[32, 31] and nxt[31, 31] < 8 and nxt[32, 32] < 8) or
                                                                      (pillar[31, 31] and pillar[32, 32] and nxt[31, 32] < 8 and nxt[32, 31] < 8)))
    # a goal that is the only reached cell of its block, and the cells that step onto it
    out["goal_leaves_by_the_corner"] = out["goal_leaves_by_the_edge"] = 0
    for gy, gx in np.argwhere(nxt == M.GOAL):
        bx, by = int(gx) // DC.BLOCK, int(gy) // DC.BLOCK
        if np.isfinite(D[by * DC.BLOCK:(by + 1) * DC.BLOCK, bx * DC.BLOCK:(bx + 1) * DC.BLOCK]).sum() != 1:
            continue
        steps = set()
        for k, (dx, dy) in enumerate(M.NEIGHBOURS):
            nx, ny = int(gx) - dx, int(gy) - dy
            if 0 <= nx < w and 0 <= ny < h and nxt[ny, nx] == k:
                steps.add((abs(nx // DC.BLOCK - bx), abs(ny // DC.BLOCK - by)))
        out["goal_leaves_by_the_corner"] += int(steps == {(1, 1)})
        out["goal_leaves_by_the_edge"] += int(steps == {(1, 0)} or steps == {(0, 1)})
    return out


def farthest(D):
    """(x, y) of the reachable cell with the largest cost"""
    y, x = np.unravel_index(np.argmax(np.where(np.isinf(D), -1.0, D)), D.shape)
    return int(x), int(y)

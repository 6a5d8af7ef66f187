"""The scenes of bt_atlas_path_field shared by tests/test_path_model.py (no GPU: every scene reaches what it is named for, on the model
alone) and tests/test_gpu_path.py (the device against the model).

TEST INFRASTRUCTURE ONLY.  The atlases are those of tests/_splat_cases.py (attachment 1 = H, the R16 heights, with its planted no-data
texels): T = 16 and 72, planar, `partial` (tiles missing) and a cube.  A scene is a window of H, a cost, goals, optionally a host mask and
`plants`: rectangles of texels written over the window with write_region before the call (zeros are walls).  Without a GPU the window's
texels come from the CPU oracle's state of the same jobs through the model of bt_atlas_read_region."""
import functools

import numpy as np

import _paint_model as PM
import _path_model as M
import _splat_cases as SC

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
    """rect (x0, y0, w, h) in mosaic texels; goals (x, y, cost0) in cells of the window; mask: (h, w) uint8 or None; plants: [(x, y, texels)]
    in CELLS OF THE WINDOW; reach: names of counters of _path_model.field / scene_reaches() that must be >= 1"""
    return dict(spec=spec, rect=rect, cost=M.cost(**cost), goals=list(goals), mask=mask, plants=list(plants), side=side, lod=lod, reach=set(reach))


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
    # the 96 x 96 serpentine maze over four tiles of the T = 72 mosaic, at an odd origin: its route is thousands of cells long
    "maze": Scene("planar_72", (151, 69, 96, 96), dict(WALK, cell_size=CELL_72), [(0, 0, 0.0), (50, 0, 5000.0), (3, 1, 0.0)],
                  plants=[(0, 0, serpentine(96))], reach={"corner_cut", "long_route", "goals_blocked", "dominated_goals", "several_blocks"}),
    "cube_face": Scene("cube_3", (5, 3, 40, 37), dict(WALK, cell_size=CELL_16, max_grade=3.0), [(30, 30, 0.0), (2, 33, 1.0)], side=4, reach={"corner_cut"}),
}
WIDTHS = ["w31", "w32", "w33", "w65"]


def geometry(scene):
    spec = SC.SPECS[scene["spec"]]
    lod = spec["lods"] - 1 if scene["lod"] is None else scene["lod"]
    return spec, lod


def planted(raw, scene):
    """the window's texels after the scene's plants: where a plant's array is True (a wall) the texel becomes 0"""
    raw = raw.copy()
    for x, y, walls in scene["plants"]:
        part = raw[y:y + walls.shape[0], x:x + walls.shape[1]]
        part[walls] = 0
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
    return out


def farthest(D):
    """(x, y) of the reachable cell with the largest cost"""
    y, x = np.unravel_index(np.argmax(np.where(np.isinf(D), -1.0, D)), D.shape)
    return int(x), int(y)

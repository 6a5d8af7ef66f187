"""The scenes of bt_atlas_rasterize_shapes shared by tests/test_shapes_model.py (no GPU: every scene reaches what it is named for, on the
model alone) and tests/test_gpu_shapes.py (the device against the model).

TEST INFRASTRUCTURE ONLY.  The atlases are those of tests/_splat_cases.py (attachment 0 = G, Rgba8; attachment 1 = H, the R16 heights with
its planted no-data texels).  A scene is a window of one attachment and a list of shapes in the model's form (tests/_shapes_model.py:
integers in 1/256 cell).  No window exceeds 200 x 100 cells."""
import math

import numpy as np

import _shapes_model as M
from _splat_cases import G, H
from bevy_terrain_amd import _ffi

CHUNK = _ffi.SHAPES_CHUNK                                    # edges of a chunk of vertices in LDS
BLOCK_W, BLOCK_H = _ffi.SHAPES_BLOCK_W, _ffi.SHAPES_BLOCK_H  # cells of a workgroup's block
AT = (3, 5)  # where most windows lie in the mosaic of planar_72 (272 across): across the tile edges at 68


def Scene(rect, shapes, spec="planar_72", attachment=G, channel=0, side=0, lod=None, reach=()):
    w, h = rect[2:]
    assert w <= 200 and h <= 100
    return dict(rect=rect, shapes=shapes, spec=spec, attachment=attachment, channel=channel, side=side, lod=lod, reach=set(reach))


def cells(*points):
    """points in whole cells -> 1/256 cell"""
    return [(256 * x, 256 * y) for x, y in points]


def square(a, b, clockwise=False):
    """the axis-aligned square with corners on the sample points (a, a) and (b, b)"""
    ring = cells((a, a), (b, a), (b, b), (a, b))
    return ring[::-1] if clockwise else ring


def pentagram(cx=2560, cy=2560, radius=2400):
    return [(round(cx + radius * math.cos(math.radians(-90 + 144 * k))), round(cy + radius * math.sin(math.radians(-90 + 144 * k)))) for k in range(5)]


def ring(n, cx, cy, rx, ry, phase=0.0):
    """n vertices around an ellipse, counter-clockwise in (x, y)"""
    return [(round(cx + rx * math.cos(phase + 2 * math.pi * k / n)), round(cy + ry * math.sin(phase + 2 * math.pi * k / n))) for k in range(n)]


def everything(w, h, **kw):
    """a polygon larger than the window on every side"""
    return M.polygon([(-700, -900), (256 * w + 500, -300), (256 * w + 900, 256 * h + 400), (-300, 256 * h + 1000)], **kw)


LONG_SEGMENT = M.stroke([(-(1 << 23), -(1 << 23) + 777), (1 << 23, 1 << 23)], 5 * 256, value=9)
STRADDLE = ring(2 * CHUNK + 3, 256 * 30, 256 * 20, 256 * 27.3, 256 * 17.6, 0.1)
HOLE_OUTER, HOLE_INNER = cells((2, 2), (20, 3), (21, 16), (3, 17)), cells((8, 6), (14, 7), (13, 12), (7, 11))

SCENES = {
    # degenerate windows
    "one_cell": Scene((13, 15, 1, 1), [M.polygon([(-100, -100), (300, -100), (-100, 300)], value=7), M.stroke([(0, 0)], 0, op=M.ADD, value=3)], reach={"all_covered"}),
    "one_cell_missed": Scene((13, 15, 1, 1), [M.polygon([(-100, -120), (300, -100), (300, 300)], value=7)], reach={"box_but_nothing_covered"}),
    "one_row": Scene((5, 27, 9, 1), [M.stroke(cells((1, 0), (7, 0)), 0, value=5), M.polygon(cells((3, -2), (6, -2), (6, 2), (3, 2)), op=M.ADD, value=2)]),
    "one_column": Scene((27, 25, 1, 9), [M.stroke(cells((0, 1), (0, 6)), 100, value=5), M.polygon(cells((-2, 3), (2, 3), (2, 8), (-2, 8)), op=M.ADD, value=2)]),
    # the boundary rules
    "square_ccw": Scene((*AT, 10, 10), [M.polygon(square(2, 6), value=9)], reach={"square_2_to_5"}),
    "square_cw": Scene((*AT, 10, 10), [M.polygon(square(2, 6, clockwise=True), value=9)], reach={"square_2_to_5"}),
    "vertex_on_a_sample_row": Scene((*AT, 12, 12), [M.polygon(cells((1, 5), (6, 1), (10, 5), (6, 9)), value=9), M.polygon(cells((1, 5), (6, 9), (10, 5), (6, 1)), nonzero=True, op=M.ADD, value=1)]),
    "horizontal_edge_on_a_sample_row": Scene((*AT, 12, 10), [M.polygon(cells((1, 3), (9, 3), (7, 7), (3, 7)), value=9), M.polygon([(300, 768), (2000, 768), (1000, 2000)], op=M.ADD, value=1)]),
    "pentagram_even_odd": Scene((*AT, 21, 21), [M.polygon(pentagram(), value=9)], reach={"covers_65"}),
    "pentagram_nonzero": Scene((*AT, 21, 21), [M.polygon(pentagram(), nonzero=True, value=9)], reach={"covers_95"}),
    "line_45": Scene((*AT, 21, 21), [M.stroke(cells((0, 0), (10, 10)), 0, value=9)], reach={"covers_11"}),
    "line_half": Scene((*AT, 21, 21), [M.stroke(cells((0, 0), (20, 10)), 0, value=9)], reach={"covers_11"}),
    "three_four_five": Scene((*AT, 24, 20), [M.stroke(cells((2, 2), (10, 8)), 5 * 256, value=9)], reach={"distance_5_in"}),
    "three_four_five_less_one": Scene((*AT, 24, 20), [M.stroke(cells((2, 2), (10, 8)), 5 * 256 - 1, value=9)], reach={"distance_5_out"}),
    # a polygon with a hole, both orientations, both fill rules
    **{f"hole_{o}_{i}_{'nonzero' if nz else 'even_odd'}": Scene((*AT, 24, 20), [M.polygon([HOLE_OUTER[::-1] if o == "cw" else HOLE_OUTER, HOLE_INNER[::-1] if i == "cw" else HOLE_INNER],
                                                                                          nonzero=nz, value=9)], reach={"hole_open" if not nz or o != i else "hole_filled"})
       for o in ("cw", "ccw") for i in ("cw", "ccw") for nz in (False, True)},
    # the window against the shapes
    "larger_than_the_window": Scene((*AT, 40, 30), [everything(40, 30, value=9)], reach={"all_covered"}),
    "all_outside": Scene((*AT, 40, 30), [M.polygon(cells((-9, -9), (-2, -9), (-2, -1)), value=9), M.stroke(cells((45, 3), (60, 40)), 3 * 256, value=9),
                                         M.stroke([(40 * 256 - 1 + 300, 5 * 256)], 300, value=9)], reach={"u_empty"}),
    "partly_outside": Scene((*AT, 40, 30), [M.polygon(cells((-9, -9), (12, -3), (5, 11)), value=9), M.stroke(cells((30, 25), (60, 40)), 3 * 256, op=M.ADD, value=9),
                                            M.polygon(cells((-9, 40), (-2, 40), (-2, 50)), value=9)], reach={"one_culled"}),
    # the chunks of vertices: a contour of 2 * CHUNK + 3 vertices, and strokes whose last segment is the chunk's last and the next one's first
    "chunk_straddle": Scene((*AT, 60, 40), [M.polygon(STRADDLE, value=9), M.stroke(STRADDLE[:CHUNK + 1], 90, op=M.ADD, value=1), M.stroke(STRADDLE[:CHUNK + 2], 90, op=M.ADD, value=1),
                                            M.stroke(STRADDLE[:CHUNK], 90, closed=True, op=M.ADD, value=1)], reach={"straddles"}),
    "long_segment": Scene((*AT, 64, 64), [LONG_SEGMENT], reach={"covers_845"}),
    "duplicates_disc_closed": Scene((*AT, 30, 24), [M.polygon(cells((2, 2), (2, 2), (12, 3), (12, 3), (12, 3), (6, 12), (2, 2)), value=9), M.stroke(cells((20, 5), (20, 5), (25, 9), (25, 9)), 400, op=M.ADD, value=1),
                                                    M.stroke(cells((8, 17)), 3 * 256 + 17, op=M.ADD, value=1), M.stroke(cells((15, 12), (27, 14), (20, 22)), 200, closed=True, op=M.ADD, value=1),
                                                    M.stroke(cells((3, 20), (9, 22)), 128, closed=True, op=M.ADD, value=1)]),
    # sizes about the kernel's block: every cell is covered, so U is the window
    **{f"block_{w}x{h}": Scene((*AT, w, h), [everything(w, h, value=9), M.stroke([(-500, 300), (256 * w + 100, 256 * h - 400)], 333, op=M.ADD, value=3),
                                             M.polygon(ring(9, 128 * w, 128 * h, 100 * w, 100 * h), op=M.ADD, value=1)], reach={"all_covered"})
       for w, h in ((BLOCK_W - 1, BLOCK_H - 1), (BLOCK_W, BLOCK_H), (BLOCK_W + 1, BLOCK_H + 1), (2 * BLOCK_W + 1, BLOCK_H - 1), (BLOCK_W - 1, 4 * BLOCK_H + 1), (200, 100))},
    # order matters
    "set_then_add": Scene((*AT, 20, 16), [M.polygon(square(2, 12), value=40), M.polygon(square(6, 15), op=M.ADD, value=5)]),
    "add_then_set": Scene((*AT, 20, 16), [M.polygon(square(6, 15), op=M.ADD, value=5), M.polygon(square(2, 12), value=40)]),
    "count_saturates": Scene((*AT, 16, 12), [M.stroke(cells((5, 5), (9, 7)), 300, op=M.ADD, value=0) for _ in range(300)], reach={"under_300"}),
    "max_shapes": Scene((*AT, 80, 60), [M.stroke([(256 * (k % 80) + 7 * (k % 5), 256 * (k // 80) + 3 * (k % 7))], 90 + k % 200, op=M.ADD, value=1) for k in range(M.MAX_SHAPES)],
                        reach={"max_shapes"}),
    # other layers
    "r16_holes": Scene((10, 2, 20, 12), [M.polygon(cells((1, 1), (18, 2), (17, 10), (2, 9)), value=30000), M.stroke(cells((0, 5), (19, 6)), 256, op=M.SUB, value=65535)], spec="planar_b2",
                       attachment=H),
    "missing_tiles": Scene((0, 0, 48, 40), [M.polygon(cells((1, 1), (45, 2), (40, 38), (2, 30)), op=M.ADD, value=77), M.stroke(cells((0, 20), (47, 22)), 500, value=3)], spec="partial", channel=2),
    "missing_tiles_r16": Scene((0, 0, 48, 40), [M.polygon(cells((1, 1), (45, 2), (40, 38), (2, 30)), op=M.ADD, value=77)], spec="partial", attachment=H),
    "cube_side": Scene((8, 3, 40, 37), [M.polygon([ring(12, 5000, 4500, 4800, 4300), ring(5, 5000, 4500, 2000, 1500)[::-1]], nonzero=True, op=M.MAX, value=200), M.stroke(cells((0, 0), (39, 36)), 300, op=M.MIN, value=20)],
                       spec="cube_3", side=4, channel=1),
    "lod_below_the_top": Scene((5, 6, 60, 50), [M.polygon(ring(40, 7000, 6000, 6500, 5500), op=M.SUB, value=90), M.stroke(cells((3, 3), (50, 45), (55, 10)), 700, op=M.ADD, value=120)], lod=1, channel=3),
}
# every op in both formats; each Rgba8 channel
for _name, _op in (("set", M.SET), ("max", M.MAX), ("min", M.MIN), ("add", M.ADD), ("sub", M.SUB)):
    for _ai, _values in ((G, (0, 100, 255)), (H, (0, 1, 33000, 65535))):
        SCENES[f"op_{_name}_{'g' if _ai == G else 'h'}"] = Scene((60, 62, 30, 24), [M.polygon(ring(7, 1500 + 1200 * i, 2800, 1300, 2500), op=_op, value=v) for i, v in enumerate(_values)],
                                                                attachment=_ai, channel=1 if _ai == G else 0)
OPS = [n for n in SCENES if n.startswith("op_")]
for _c in range(4):
    SCENES[f"channel_{_c}"] = Scene((60, 62, 30, 24), [M.polygon(ring(7, 3800, 2800, 3300, 2500), op=M.ADD, value=90), M.stroke(cells((2, 2), (27, 20)), 300, value=_c)], channel=_c)
HOLES = [n for n in SCENES if n.startswith("hole_")]
BLOCKS = [n for n in SCENES if n.startswith("block_")]


def covers(name):
    """the cells each shape of a scene covers: a list of (h, w) bool planes, by the model"""
    scene = SCENES[name]
    w, h = scene["rect"][2:]
    return [M.cover(s, w, h) for s in scene["shapes"]]


def scene_reaches(name):
    scene = SCENES[name]
    w, h = scene["rect"][2:]
    shapes = scene["shapes"]
    planes = covers(name)
    total = sum(p.astype(int) for p in planes)
    boxes = [M.box(s, w, h) for s in shapes]
    out = {"all_covered": bool((total > 0).all()), "u_empty": M.union(boxes) == M.EMPTY and len(shapes) > 1,
           "one_culled": sum(b == M.EMPTY for b in boxes) == 1 and M.union(boxes) != M.EMPTY,
           "box_but_nothing_covered": M.union(boxes) != M.EMPTY and not total.any(),
           "covers_65": int(planes[0].sum()) == 65, "covers_95": int(planes[0].sum()) == 95, "covers_11": int(planes[0].sum()) == 11, "covers_845": int(planes[0].sum()) == 845,
           "under_300": int(total.max()) == 300, "max_shapes": len(shapes) == M.MAX_SHAPES and int(total.max()) > 1}
    ys, xs = np.nonzero(planes[0])
    out["square_2_to_5"] = planes[0].sum() == 16 and (xs.min(), xs.max(), ys.min(), ys.max()) == (2, 5, 2, 5)
    if name.startswith("three_four_five"):
        # (13, 12) lies (3, 4) from the end (10, 8); (3, 9) lies 5 from the middle (6, 5) at right angles, along (-3, 4)
        out["distance_5_in"] = bool(planes[0][12, 13]) and bool(planes[0][9, 3])
        out["distance_5_out"] = not planes[0][12, 13] and not planes[0][9, 3] and bool(planes[0][12, 12])
    if name.startswith("hole_"):
        out["hole_open"] = bool(planes[0][4, 5]) and not planes[0][9, 10]
        out["hole_filled"] = bool(planes[0][4, 5]) and bool(planes[0][9, 10])
    if name == "chunk_straddle":
        out["straddles"] = len(shapes[0]["contours"][0]) == 2 * CHUNK + 3 and [len(s["points"]) for s in shapes[1:]] == [CHUNK + 1, CHUNK + 2, CHUNK]
    return out

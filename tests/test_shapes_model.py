"""The model of bt_atlas_rasterize_shapes (tests/_shapes_model.py) without a GPU: against a second restatement of the rules (a scanline
fill with fractions for polygons, fractions.Fraction distances for strokes), against answers worked by hand, and bt_shapes_check through
ctypes against the model's validator and boxes, rule by rule; and every scene of tests/_shapes_cases.py reaches what it is named for."""
import ctypes as C
import pathlib
import re
from fractions import Fraction

import numpy as np
import pytest

import _shapes_cases as SC
import _shapes_model as M
import bevy_terrain_amd as bt
from bevy_terrain_amd import _ffi

ROOT = pathlib.Path(__file__).resolve().parent.parent


# ---------------------------------------------------------------------------------------------- the second restatement

def scanline_cover(contours, nonzero, width, height):
    """per sample row, the exact x at which every edge that spans the row (half-open in y) meets it, as a fraction; the winding number of
    a sample point is the sum of the directions of the crossings strictly to its right"""
    out = np.zeros((height, width), bool)
    for cy in range(height):
        y = 256 * cy
        crossings = []
        for c in contours:
            for (ax, ay), (bx, by) in zip(c, c[1:] + c[:1]):
                if ay == by or not (min(ay, by) <= y < max(ay, by)):
                    continue
                crossings.append((Fraction(ax) + Fraction(bx - ax) * Fraction(y - ay, by - ay), 1 if by > ay else -1))
        for cx in range(width):
            w = sum(d for x, d in crossings if x > 256 * cx)
            out[cy, cx] = w != 0 if nonzero else w % 2 == 1
    return out


def fraction_stroke_cover(points, r, closed, width, height):
    """the squared distance from the sample point to the nearest point of each segment, as a fraction"""
    out = np.zeros((height, width), bool)
    for cy in range(height):
        for cx in range(width):
            p = (256 * cx, 256 * cy)
            for a, b in M.segments(points, closed):
                d = (b[0] - a[0], b[1] - a[1])
                L = d[0] * d[0] + d[1] * d[1]
                t = Fraction(0) if L == 0 else min(Fraction(1), max(Fraction(0), Fraction((p[0] - a[0]) * d[0] + (p[1] - a[1]) * d[1], L)))
                q = (a[0] + t * d[0], a[1] + t * d[1])
                if (p[0] - q[0]) ** 2 + (p[1] - q[1]) ** 2 <= r * r:
                    out[cy, cx] = True
                    break
    return out


def restated(shape, w, h):
    if "contours" in shape:
        return scanline_cover(shape["contours"], shape["nonzero"], w, h)
    return fraction_stroke_cover(shape["points"], shape["r"], shape["closed"], w, h)


def random_shapes(rng, w, h, n, snap=False):
    """snap: vertices on sample points and half cells, so that points on edges and vertices are common"""
    def point():
        x, y = rng.integers(-3 * 256, (w + 3) * 256), rng.integers(-3 * 256, (h + 3) * 256)
        return (int(x) // 128 * 128, int(y) // 128 * 128) if snap else (int(x), int(y))
    shapes = []
    for _ in range(n):
        op, value = int(rng.integers(0, 5)), int(rng.integers(0, 256))
        if rng.integers(2):
            shapes.append(M.polygon([[point() for _ in range(rng.integers(3, 8))] for _ in range(rng.integers(1, 3))], bool(rng.integers(2)), op, value))
        else:
            r = int(rng.integers(0, 4)) * 128 if snap else int(rng.integers(0, 700))
            shapes.append(M.stroke([point() for _ in range(rng.integers(1, 5))], r, bool(rng.integers(2)), op, value))
    return shapes


@pytest.mark.parametrize("snap", [False, True])
def test_model_against_the_second_restatement_on_random_lists(snap):
    rng = np.random.default_rng(11 + snap)
    for _ in range(12):
        w, h = (int(v) for v in rng.integers(1, 14, 2))
        for s in random_shapes(rng, w, h, 4, snap):
            assert np.array_equal(M.cover(s, w, h), restated(s, w, h)), s


@pytest.mark.parametrize("name", ["square_ccw", "square_cw", "vertex_on_a_sample_row", "horizontal_edge_on_a_sample_row", "pentagram_even_odd", "pentagram_nonzero", "line_45",
                                  "line_half", "three_four_five", "three_four_five_less_one", "duplicates_disc_closed", "one_row", "one_column", "one_cell", *SC.HOLES])
def test_model_against_the_second_restatement_on_the_boundary_scenes(name):
    w, h = SC.SCENES[name]["rect"][2:]
    for s, plane in zip(SC.SCENES[name]["shapes"], SC.covers(name)):
        assert np.array_equal(plane, restated(s, w, h)), (name, s)


def test_nothing_outside_its_box_is_covered():
    rng = np.random.default_rng(3)
    seen_empty = 0
    for _ in range(40):
        w, h = (int(v) for v in rng.integers(1, 20, 2))
        for s in random_shapes(rng, w, h, 3, bool(rng.integers(2))):
            full = M.cover(s, w, h) if "contours" in s else M.stroke_cover(s["points"], s["r"], s["closed"], w, h)
            b = M.box(s, w, h)
            inside = np.zeros((h, w), bool)
            if b != M.EMPTY:
                inside[b[1]:b[3] + 1, b[0]:b[2] + 1] = True
            seen_empty += b == M.EMPTY
            assert not (full & ~inside).any(), (s, b)
    assert seen_empty > 0


# ---------------------------------------------------------------------------------------------- worked by hand

def test_the_square_on_sample_points_covers_2_to_5_either_way_round():
    for clockwise in (False, True):
        for nonzero in (False, True):
            plane = M.cover(M.polygon(SC.square(2, 6, clockwise), nonzero), 10, 10)
            assert np.array_equal(np.argwhere(plane), [[y, x] for y in range(2, 6) for x in range(2, 6)])


def test_reversing_a_contour_negates_the_winding_number_and_a_horizontal_edge_never_counts():
    star = SC.pentagram()
    assert np.array_equal(M.winding([star], 21, 21), -M.winding([star[::-1]], 21, 21)) and abs(M.winding([star], 21, 21)).max() == 2
    flat = SC.cells((1, 3), (9, 3), (7, 7), (3, 7))
    w = M.winding([flat], 12, 10)
    assert (w[3, 1:9] != 0).all() and not w[7].any() and not w[2].any()  # the upper edge's row is in (a.y <= P.y), the lower edge's is not (P.y < b.y)


def test_pentagram_counts():
    assert int(M.cover(M.polygon(SC.pentagram()), 21, 21).sum()) == 65 and int(M.cover(M.polygon(SC.pentagram(), nonzero=True), 21, 21).sum()) == 95


def test_zero_width_strokes_cover_the_sample_points_on_the_segment():
    plane = M.cover(M.stroke(SC.cells((0, 0), (10, 10)), 0), 21, 21)
    assert np.array_equal(np.argwhere(plane), [[k, k] for k in range(11)])
    plane = M.cover(M.stroke(SC.cells((0, 0), (20, 10)), 0), 21, 21)
    assert np.array_equal(np.argwhere(plane), [[k, 2 * k] for k in range(11)])


def test_three_four_five():
    at5 = M.cover(M.stroke(SC.cells((2, 2), (10, 8)), 5 * 256), 24, 20)
    less = M.cover(M.stroke(SC.cells((2, 2), (10, 8)), 5 * 256 - 1), 24, 20)
    exactly = [(13, 12), (14, 11), (3, 9), (9, 1), (7, 12)]  # (3, 4) and (4, 3) from the end; 5 at right angles from (6, 5), from (6, 5) the other way and from (10, 8)
    assert all(at5[y, x] and not less[y, x] for x, y in exactly) and not (less & ~at5).any() and int(at5.sum()) > int(less.sum())


def test_fold_rules():
    texels = np.array([[0, 1, 100, 65535]], np.uint16)
    whole = lambda **kw: [SC.everything(4, 1, **kw)]
    assert M.raster(texels, whole(op=M.SET, value=0))[2].tolist() == [[0, 1, 1, 1]]
    assert M.raster(texels, whole(op=M.SUB, value=65535))[2].tolist() == [[0, 1, 1, 1]]
    assert M.raster(texels, whole(op=M.ADD, value=65535))[2].tolist() == [[0, 65535, 65535, 65535]]
    assert M.raster(texels, whole(op=M.MAX, value=200))[2].tolist() == [[0, 200, 200, 65535]] and M.raster(texels, whole(op=M.MIN, value=50))[2].tolist() == [[0, 1, 50, 50]]
    rgba = np.array([[[0, 10, 20, 30], [250, 251, 252, 253]]], np.uint8)
    count, last, out, stats = M.raster(rgba, [SC.everything(2, 1, op=M.ADD, value=10), SC.everything(2, 1, op=M.SUB, value=15)], channel=2)
    assert out.tolist() == [[[0, 10, 15, 30], [250, 251, 240, 253]]] and count.tolist() == [[2, 2]] and last.tolist() == [[1, 1]] and stats["written"] == 2
    assert M.raster(rgba, [SC.everything(2, 1, op=M.SET, value=0)], channel=0)[2][:, :, 0].tolist() == [[0, 0]]  # no hole rule
    a = M.raster(rgba, SC.SCENES["set_then_add"]["shapes"][:0] + [SC.everything(2, 1, value=40), SC.everything(2, 1, op=M.ADD, value=5)])[2]
    b = M.raster(rgba, [SC.everything(2, 1, op=M.ADD, value=5), SC.everything(2, 1, value=40)])[2]
    assert a[:, :, 0].tolist() == [[45, 45]] and b[:, :, 0].tolist() == [[40, 40]]


# ---------------------------------------------------------------------------------------------- the scenes' reach

@pytest.mark.parametrize("name", sorted(SC.SCENES))
def test_every_scene_reaches_what_it_is_named_for(name):
    reaches = SC.scene_reaches(name)
    missing = [r for r in SC.SCENES[name]["reach"] if not reaches.get(r)]
    assert not missing, (name, missing)
    vertices, entries = M.pack(SC.SCENES[name]["shapes"])
    assert M.validate(vertices, entries, *SC.SCENES[name]["rect"][2:])[0] is None


def test_the_chunk_straddling_contour_and_the_block_sizes():
    assert len(SC.STRADDLE) == 2 * SC.CHUNK + 3
    sizes = {SC.SCENES[n]["rect"][2:] for n in SC.BLOCKS}
    assert {(SC.BLOCK_W - 1, SC.BLOCK_H - 1), (SC.BLOCK_W, SC.BLOCK_H), (SC.BLOCK_W + 1, SC.BLOCK_H + 1)} <= sizes
    # the contour's box straddles blocks too, so its chunks are walked by several workgroups
    b = M.box(SC.SCENES["chunk_straddle"]["shapes"][0], 60, 40)
    assert b[3] - b[1] + 1 > SC.BLOCK_H


def test_the_long_segment_needs_128_bits():
    s = SC.LONG_SEGMENT
    exact = M.stroke_cover(s["points"], s["r"], False, 64, 64)
    wrapped = M.stroke_cover(s["points"], s["r"], False, 64, 64, wrap64=True)
    assert int(exact.sum()) == 845 and int((exact != wrapped).sum()) > 2000
    assert np.array_equal(exact[:12, :12], fraction_stroke_cover(s["points"], s["r"], False, 12, 12))


def test_count_saturation_scene():
    total = sum(p.astype(int) for p in SC.covers("count_saturates"))
    assert total.max() == 300
    count, last, _, stats = M.raster(np.zeros((12, 16, 4), np.uint8), SC.SCENES["count_saturates"]["shapes"])
    assert count.max() == 255 and set(np.unique(last)) == {299, M.NONE} and stats["covered"] == int((total > 0).sum())


# ---------------------------------------------------------------------------------------------- bt_shapes_check

def check(vertices, entries, w, h, boxes=True):
    """(status, boxes or None, shapes, bad entry) of bt_shapes_check; the outputs start patterned"""
    vertices, entries = np.ascontiguousarray(vertices, dtype=np.int32), np.ascontiguousarray(entries, dtype=np.uint32)
    out = np.full((max(len(entries), 1), 4), 7, np.uint16)
    count, bad = C.c_uint32(7), C.c_uint32(7)
    rc = _ffi.lib().bt_shapes_check(vertices.ctypes.data_as(C.POINTER(_ffi.ShapeVertexC)), len(vertices), entries.ctypes.data_as(C.POINTER(_ffi.ShapeC)), len(entries), w, h,
                                    out.ctypes.data_as(C.POINTER(_ffi.ShapeBoxC)) if boxes else None, C.byref(count), C.byref(bad))
    return rc, out, count.value, bad.value


@pytest.mark.parametrize("name", sorted(SC.SCENES))
def test_check_gives_the_models_boxes_on_the_scenes(name):
    scene = SC.SCENES[name]
    w, h = scene["rect"][2:]
    vertices, entries = M.pack(scene["shapes"])
    rc, boxes, count, bad = check(vertices, entries, w, h)
    assert (rc, count, bad) == (0, len(scene["shapes"]), M.NO_ENTRY)
    assert boxes[:count].tolist() == [list(M.box(s, w, h)) for s in scene["shapes"]]
    assert M.unpack(vertices, entries) == scene["shapes"]


def test_check_boxes_on_random_lists_and_without_a_window():
    rng = np.random.default_rng(9)
    for _ in range(60):
        w, h = (int(v) for v in rng.integers(1, 40, 2))
        shapes = random_shapes(rng, w, h, 5, bool(rng.integers(2)))
        rc, boxes, count, _ = check(*M.pack(shapes), w, h)
        assert rc == 0 and boxes[:count].tolist() == [list(M.box(s, w, h)) for s in shapes]
    # the division is mathematical: a vertex one unit before a sample point, one unit past it, and r that just reaches
    for x, r, want in ((-1, 0, M.EMPTY), (-1, 1, (0, 0, 0, 0)), (0, 0, (0, 0, 0, 0)), (1, 0, M.EMPTY), (257, 1, (1, 0, 1, 0)), (-257, 256, M.EMPTY), (-256, 256, (0, 0, 0, 0)),
                       (256 * 9 + 1, 0, M.EMPTY), (256 * 9 + 1, 1, (9, 0, 9, 0)), (256 * 10, 255, M.EMPTY), (256 * 10, 256, (9, 0, 9, 0))):
        s = M.stroke([(x, 0)], r)
        assert M.box(s, 10, 1) == want and check(*M.pack([s]), 10, 1)[1][0].tolist() == list(want), (x, r)
    s = [M.stroke([(0, 0)], 5)]
    assert check(*M.pack(s), 0, 5)[1][0].tolist() == list(M.EMPTY) and check(*M.pack(s), 5, 0)[1][0].tolist() == list(M.EMPTY)
    assert check(*M.pack(s), 5, 5, boxes=False)[::2] == (0, 1)
    L = _ffi.lib()
    assert L.bt_shapes_check(None, 0, None, 0, 4, 4, None, None, None) == 0 and L.bt_shapes_check(None, 1, None, 1, 4, 4, None, None, None) == -1


def test_check_refuses_rule_by_rule():
    good = [M.polygon([SC.square(1, 5), SC.square(2, 4)], nonzero=True, op=M.ADD, value=3), M.stroke(SC.cells((1, 1), (3, 3)), 100, closed=True)]
    vertices, entries = M.pack(good)
    assert check(vertices, entries, 8, 8)[0] == 0 and M.validate(vertices, entries, 8, 8) == (None, M.NO_ENTRY, 2)
    KIND, FLAGS, FIRST, COUNT, R, OP, VALUE, PAD = range(8)

    def broken(entry, field, value, vertex=None):
        v, e = vertices.copy(), entries.copy()
        e[entry, field] = value
        if vertex is not None:
            v[vertex[0]] = vertex[1:]
        return v, e

    cases = [broken(0, KIND, 2), broken(2, KIND, 0xFFFFFFFF), broken(0, FLAGS, M.NONZERO | M.MORE | M.CLOSED), broken(2, FLAGS, M.NONZERO), broken(2, FLAGS, M.MORE), broken(1, FLAGS, 8 | M.NONZERO),
             broken(1, OP, 5), broken(2, VALUE, 65536), broken(1, PAD, 1), broken(0, R, 1), broken(2, R, M.MAX_HALF_WIDTH + 1), broken(0, COUNT, 2), broken(2, COUNT, 0),
             broken(2, COUNT, 3), broken(2, FIRST, 0xFFFFFFFF), broken(0, KIND, 0, vertex=(5, M.MAX_COORD + 1, 0)), broken(0, KIND, 0, vertex=(9, 0, -M.MAX_COORD - 1)),
             # the run: the second contour differs in op, in value, in NONZERO; MORE on the last entry; a stroke after MORE
             broken(1, OP, M.SET), broken(1, VALUE, 4), broken(1, FLAGS, 0), broken(1, FLAGS, M.NONZERO | M.MORE), broken(1, KIND, M.STROKE)]
    for v, e in cases:
        rule, entry, _ = M.validate(v, e, 8, 8)
        rc, boxes, count, bad = check(v, e, 8, 8)
        assert rule is not None and (rc, count, bad) == (-1, 0, entry) and (boxes == 7).all(), (rule, entry, bad)
        assert f"entry {entry}".encode() in _ffi.lib().bt_last_error()
    # the largest accepted values
    for v, e in (broken(2, R, M.MAX_HALF_WIDTH), broken(2, VALUE, 65535), broken(0, KIND, 0, vertex=(5, M.MAX_COORD, -M.MAX_COORD))):
        assert check(v, e, 8, 8)[0] == 0 and M.validate(v, e, 8, 8)[0] is None
    # the limits of the list and the window
    one = M.pack([M.stroke([(0, 0)], 0)])
    many = np.repeat(one[1], M.MAX_SHAPES + 1, axis=0)
    assert check(one[0], many, 8, 8)[::3] == (-1, M.MAX_SHAPES) and M.validate(one[0], many, 8, 8)[:2] == ("shapes", M.MAX_SHAPES)
    assert check(one[0], many[:M.MAX_SHAPES], 8, 8)[::2] == (0, M.MAX_SHAPES)
    tri = M.pack([M.polygon(SC.cells((0, 0), (2, 0), (0, 2)))])
    contours = np.repeat(tri[1], M.MAX_ENTRIES + 1, axis=0)
    contours[:, 1] = M.MORE
    contours[-1, 1] = 0
    assert check(tri[0], contours, 8, 8)[::3] == (-1, M.NO_ENTRY) and M.validate(tri[0], contours, 8, 8)[:2] == ("entries", M.NO_ENTRY)
    contours = contours[1:]
    assert check(tri[0], contours, 8, 8)[::2] == (0, 1) and M.validate(tri[0], contours, 8, 8) == (None, M.NO_ENTRY, 1)  # one polygon of 65536 contours
    assert check(np.zeros((M.MAX_VERTICES + 1, 2), np.int32), one[1], 8, 8)[::3] == (-1, M.NO_ENTRY) and check(np.zeros((M.MAX_VERTICES, 2), np.int32), one[1], 8, 8)[0] == 0
    for w, h, ok in ((8193, 1, False), (1, 8193, False), (8192, 512, True), (8192, 513, False), (2049, 2048, False), (2048, 2048, True)):
        assert (check(*one, w, h)[0] == 0) == ok == (M.validate(*one, w, h)[0] is None), (w, h)


# ---------------------------------------------------------------------------------------------- the mirror

def test_the_mirror_has_the_headers_constants_and_symbols():
    header = (ROOT / "include" / "bevy_terrain_amd.h").read_text()

    def define(name):
        return int(re.search(rf"^#define {name} (\w+)$", header, flags=re.M).group(1).rstrip("u"), 0)

    assert define("BT_SHAPES_NONE") == _ffi.SHAPES_NONE == M.NONE and define("BT_SHAPES_NO_ENTRY") == _ffi.SHAPES_NO_ENTRY == M.NO_ENTRY
    assert define("BT_SHAPES_MAX_SHAPES") == _ffi.SHAPES_MAX_SHAPES == M.MAX_SHAPES and define("BT_SHAPES_MAX_ENTRIES") == _ffi.SHAPES_MAX_ENTRIES == M.MAX_ENTRIES
    assert define("BT_SHAPES_MAX_SIDE") == _ffi.SHAPES_MAX_SIDE == M.MAX_SIDE and define("BT_SHAPES_CHUNK") == _ffi.SHAPES_CHUNK
    assert define("BT_SHAPES_BLOCK_W") == _ffi.SHAPES_BLOCK_W and define("BT_SHAPES_BLOCK_H") == _ffi.SHAPES_BLOCK_H
    assert "#define BT_SHAPES_MAX_VERTICES (1u << 20)" in header and _ffi.SHAPES_MAX_VERTICES == M.MAX_VERTICES == 1 << 20
    assert "#define BT_SHAPES_MAX_COORD (1 << 23)" in header and _ffi.SHAPES_MAX_COORD == M.MAX_COORD == 1 << 23
    assert "#define BT_SHAPES_MAX_HALF_WIDTH (1u << 20)" in header and _ffi.SHAPES_MAX_HALF_WIDTH == M.MAX_HALF_WIDTH == 1 << 20
    assert "#define BT_SHAPES_MAX_CELLS (1u << 22)" in header and _ffi.SHAPES_MAX_CELLS == M.MAX_CELLS == 1 << 22
    assert "enum { BT_SHAPE_POLYGON = 0, BT_SHAPE_STROKE = 1 };" in header and (_ffi.SHAPE_POLYGON, _ffi.SHAPE_STROKE) == (M.POLYGON, M.STROKE) == (0, 1)
    assert "enum { BT_SHAPE_NONZERO = 1, BT_SHAPE_CLOSED = 2, BT_SHAPE_MORE = 4 };" in header
    assert (_ffi.SHAPE_NONZERO, _ffi.SHAPE_CLOSED, _ffi.SHAPE_MORE) == (M.NONZERO, M.CLOSED, M.MORE) == (1, 2, 4)
    assert "enum { BT_SHAPE_SET = 0, BT_SHAPE_MAX = 1, BT_SHAPE_MIN = 2, BT_SHAPE_ADD = 3, BT_SHAPE_SUB = 4 };" in header
    assert (_ffi.SHAPE_SET, _ffi.SHAPE_MAX, _ffi.SHAPE_MIN, _ffi.SHAPE_ADD, _ffi.SHAPE_SUB) == (M.SET, M.MAX, M.MIN, M.ADD, M.SUB) == (0, 1, 2, 3, 4)
    assert "enum { BT_SHAPES_DRY_RUN = 1 };" in header and _ffi.SHAPES_DRY_RUN == 1
    for struct, ctype in (("bt_shape_vertex", _ffi.ShapeVertexC), ("bt_shape", _ffi.ShapeC), ("bt_shape_box", _ffi.ShapeBoxC), ("bt_shapes_stats", _ffi.ShapesStatsC)):
        stated = int(re.search(rf"\}} {struct}; /\* (\d+) bytes \*/", header).group(1))
        assert stated == C.sizeof(ctype) and stated % 8 == 0, struct
    assert C.sizeof(_ffi.ShapeC) == 32
    for name in ("bt_shapes_check", "bt_atlas_rasterize_shapes"):
        assert name in _ffi.header_symbols() and name in _ffi.PROTOTYPES
    assert _ffi.header_abi_version() == 6


def test_pack_shapes_rounds_once_to_the_nearest_256th():
    shapes = [dict(polygon=[[(0.0, 0.0), (2.0, 0.001), (1.0, 1.997)], [(0.5, 0.25), (1.0, 0.25), (0.75, 0.5)]], nonzero=True, op="add", value=7),
              dict(stroke=[(-1.0, 3.00195), (1 / 512, -1 / 512)], half_width=1.5, closed=True, op="min", value=2)]
    vertices, entries = bt.TileAtlas.pack_shapes(shapes)
    assert vertices.tolist() == [[0, 0], [512, 0], [256, 511], [128, 64], [256, 64], [192, 128], [-256, 768], [1, 0]]  # a half goes up: 0.5 -> 1, -0.5 -> 0
    assert entries.tolist() == [[M.POLYGON, M.NONZERO | M.MORE, 0, 3, 0, M.ADD, 7, 0], [M.POLYGON, M.NONZERO, 3, 3, 0, M.ADD, 7, 0], [M.STROKE, M.CLOSED, 6, 2, 384, M.MIN, 2, 0]]
    fixed = bt.TileAtlas.pack_shapes([dict(stroke=[(5, -7)], half_width=3)], fixed=True)
    assert fixed[0].tolist() == [[5, -7]] and fixed[1][0, 4] == 3
    boxes, count = bt.TileAtlas.check_shapes(vertices, entries, 4, 4)
    assert count == 2 and boxes.tolist() == [list(M.box(s, 4, 4)) for s in M.unpack(vertices, entries)]
    with pytest.raises(_ffi.BtError):
        bt.TileAtlas.check_shapes(vertices, entries[:1], 4, 4)  # MORE on the last entry

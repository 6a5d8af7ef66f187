"""The cases of bt_atlas_splat_from_height shared by tests/test_splat_model.py (no GPU: every case reaches the branch it is named for, on states
the CPU oracle makes from the same jobs) and tests/test_gpu_splat.py (the device against the model).

TEST INFRASTRUCTURE ONLY.  An atlas has two attachments of one texture and border size: 0 is G, the Rgba8 target (so the helpers of
tests/test_gpu_edit.py, which look at attachment 0, check the target), 1 is H, the R16 heights.  Both are filled by preprocessing jobs (G from
a random raster: the call must overwrite something), then no-data texels are planted in H with write_region, since a job resamples its
source: a block, a single texel, a column piece."""
import functools
import math

import numpy as np

import _cases as K
import _edit_model as EM
import _oracle as O
import _splat_model as SM
from bevy_terrain_amd import SplatRule as R
from bevy_terrain_amd import TerrainModel
from test_gpu_edit import RGBA8, R16, cube_faces, source_r16

INF = math.inf
G, H = 0, 1  # attachment indices
LO, HI = -50.0, 450.0  # the models' height range: a span of 500 over a face of 1000 (texels of ~20 at the finest LOD of the small shapes)

PLANAR = (TerrainModel.planar((0.0, 0.0, 0.0), 1000.0, LO, HI), O.make_model("planar", (0, 0, 0), 1000.0, 0.0, LO, HI))
SPHERE = (TerrainModel.sphere((0.0, 0.0, 0.0), 1000.0, LO, HI), O.make_model("spherical", (0, 0, 0), 1000.0, 0.0, LO, HI))

# no-data texels planted in H on every side, (y0, x0, h, w) in mosaic texels of the finest LOD: inside the smallest mosaic used (24 x 24)
HOLES = [(5, 14, 4, 4), (20, 3, 1, 1), (12, 21, 6, 1)]

SPECS = {
    "planar_b2": dict(kind="planar", T=16, b=2, lods=3, n=64),
    "planar_b1": dict(kind="planar", T=16, b=1, lods=3, n=64),
    "planar_72": dict(kind="planar", T=72, b=2, lods=3, n=272),
    "planar_136": dict(kind="planar", T=136, b=3, lods=3, n=520),
    "cube_2": dict(kind="cube", T=16, b=2, lods=2, n=40),
    "cube_3": dict(kind="cube", T=16, b=2, lods=3, n=40),
    "partial": dict(kind="planar", T=16, b=2, lods=3, n=64, extent=dict(top_left=(0.3, 0.3), bottom_right=(0.9, 0.9))),
    "no_lod0": dict(kind="planar", T=16, b=2, lods=3, n=64, lod_range=range(1, 3)),
}


def models(spec):
    return SPHERE if spec["kind"] == "cube" else PLANAR


def heights_source(spec):
    return source_r16(spec["n"])


def target_source(spec):
    return K.random_raster(RGBA8, spec["n"], spec["n"], seed=8)


def target_faces(spec):
    return [K.random_raster(RGBA8, spec["n"], spec["n"], seed=100 + s) for s in range(6)]


def hole_rects(spec):
    """HOLES as (side, x0, y0, zeros) for write_region on H"""
    return [(side, x, y, np.zeros((h, w), np.uint16)) for side in range(6 if spec["kind"] == "cube" else 1) for y, x, h, w in HOLES]


@functools.lru_cache(maxsize=None)
def oracle_state(spec_name):
    """the state the device atlas of test_gpu_splat.py starts from, made by the CPU oracle and the model of write_region:
    ({coord: H tile}, {coord: G tile})"""
    spec = SPECS[spec_name]
    T, b, lods, cube = spec["T"], spec["b"], spec["lods"], spec["kind"] == "cube"
    atlas = O.OracleAtlas(lods, 128, cube, [(T, b, 1, RGBA8), (T, b, 1, R16)])
    atlas.clear_attachment(G).clear_attachment(H)
    if cube:
        atlas.preprocess_spherical(G, target_faces(spec), (0, lods)).preprocess_spherical(H, cube_faces(spec["n"]), (0, lods)).run(4)
    else:
        levels = spec.get("lod_range") or range(0, lods)
        extent = spec.get("extent", {})
        atlas.preprocess_tile(G, target_source(spec), (levels.start, levels.stop), **extent)
        atlas.preprocess_tile(H, heights_source(spec), (levels.start, levels.stop), **extent).run(4)
    g = {coord: atlas.tile(G, i) for coord, i in atlas.tiles()}
    h = {coord: atlas.tile(H, i) for coord, i in atlas.tiles()}
    for side, x, y, zeros in hole_rects(spec):
        h = EM.write_region(h, lods - 1, side, x, y, zeros, b)
    return EM.propagate(h, b, cube), g


# ---------------------------------------------------------------------------------------------- the rule sets (world heights; slopes in degrees)

WATER, SAND, GRASS, FOREST, ROCK, SNOW = (0.1, 0.3, 0.7), (0.8, 0.75, 0.5), (0.3, 0.6, 0.2), (0.1, 0.4, 0.15), (0.5, 0.45, 0.4), (1.0, 1.0, 1.0)

RULES = {
    # one rule without limits: every data texel is its colour
    "one": ("colour", [R(colour=GRASS)]),
    # four weight rules; above 300 only the fourth (the alpha byte) reaches: r = g = b = 0 and the zero rule sets r
    "weights_alpha_dominant": ("weights", [R(height=(-INF, 150.0), height_fade=40.0), R(height=(150.0, 260.0), height_fade=40.0, weight=2.0),
                                           R(slope=(25.0, 90.0), slope_fade=0.05, height=(-INF, 280.0), weight=0.5), R(height=(300.0, INF), weight=3.0)]),
    # eight colour rules by height and slope, all with fades: most texels mix several
    "colour_eight": ("colour", [R(height=(-INF, 110.0), height_fade=20.0, colour=WATER), R(height=(110.0, 140.0), height_fade=15.0, colour=SAND),
                                R(height=(140.0, 230.0), height_fade=30.0, slope=(0.0, 30.0), slope_fade=0.05, colour=GRASS),
                                R(height=(180.0, 260.0), height_fade=30.0, slope=(10.0, 40.0), slope_fade=0.05, colour=FOREST, weight=0.75),
                                R(height=(230.0, 330.0), height_fade=30.0, colour=ROCK), R(slope=(40.0, 90.0), slope_fade=0.1, colour=(0.35, 0.3, 0.3), weight=4.0),
                                R(height=(300.0, INF), height_fade=25.0, slope=(0.0, 50.0), slope_fade=0.1, colour=SNOW, weight=2.0),
                                R(height=(200.0, 210.0), colour=(2.0, -1.0, 0.5), weight=0.25)]),
    # hard bands (fade 0) with infinite bounds: a partition of the heights, and a hard slope limit on top
    "hard_bands": ("colour", [R(height=(-INF, 200.0), colour=WATER), R(height=(200.0, INF), colour=ROCK), R(slope=(35.0, 90.0), colour=SNOW, weight=8.0)]),
    # bands that leave the heights between 170 and 230 and the flat ground above to nobody: the fallback
    "leaves_some_to_fallback": ("weights", [R(height=(-INF, 160.0), height_fade=10.0), R(height=(240.0, INF), height_fade=10.0, slope=(20.0, 90.0), slope_fade=0.02)]),
    # black rules only: every reached data texel would be (0, 0, 0, 255) in colour mode, and a black fallback likewise: the zero rule both ways
    "black": ("colour", [R(height=(-INF, 220.0), height_fade=5.0, colour=(0.0, 0.0, 0.0))]),
}
FALLBACK = {"leaves_some_to_fallback": (9, 8, 7, 6), "black": (0, 0, 0, 77)}


def Call(rules, rect=None, lod=None, side=0, reach=()):
    """one bt_atlas_splat_from_height call: rules: a name of RULES; rect (x0, y0, w, h) in mosaic texels of `lod` (None: the whole face);
    reach: names of _splat_model.splat_texels' counters that must be >= 1, or of shape_reaches()"""
    return dict(rules=rules, rect=rect, lod=lod, side=side, reach=set(reach))


WHOLE_72 = {"second_row_block", "second_column_chunk", "second_lane_trip_of_the_staging"}

CASES = {
    # T = 16, b = 2 (c = 12) and b = 1 (c = 14), lod_count 3: mosaics of 48 and 56
    "whole_face": ("planar_b2", [Call("colour_eight", reach={"holes", "mixed", "partial"})]),
    "one_texel": ("planar_b2", [Call("one", rect=(13, 15, 1, 1))]),
    "odd_origin_over_four_tiles": ("planar_b2", [Call("colour_eight", rect=(7, 9, 11, 9), reach={"mixed"})]),
    "ends_mid_tile": ("planar_b2", [Call("hard_bands", rect=(0, 0, 17, 21), reach={"holes"})]),
    "one_rule": ("planar_b2", [Call("one", reach={"holes"})]),
    "weights_and_the_zero_rule": ("planar_b2", [Call("weights_alpha_dominant", reach={"zero_rule", "mixed", "partial", "holes"})]),
    "hard_bands_infinite_bounds": ("planar_b2", [Call("hard_bands", reach={"mixed", "holes"})]),
    "fallback": ("planar_b2", [Call("leaves_some_to_fallback", reach={"fallback", "partial", "holes"})]),
    "black_and_the_zero_rule": ("planar_b2", [Call("black", reach={"zero_rule", "fallback", "holes"})]),
    "hole_block_texel_and_straddling_taps": ("planar_b2", [Call("colour_eight", rect=(12, 3, 8, 8), reach={"holes", "taps_straddle_a_hole"}),
                                                           Call("weights_alpha_dominant", rect=(2, 19, 3, 3), reach={"holes", "taps_straddle_a_hole"})]),
    "odd_border": ("planar_b1", [Call("colour_eight", reach={"holes", "mixed"}), Call("hard_bands", rect=(9, 11, 11, 9)), Call("one", rect=(15, 17, 1, 1)),
                                 Call("weights_alpha_dominant", rect=(0, 0, 19, 33), reach={"holes"})]),
    # T = 72, b = 2 (c = 68): rows past one lane trip, a second row block, a second column chunk of the LDS window with its halo
    "beyond_one_block": ("planar_72", [Call("colour_eight", reach=WHOLE_72 | {"holes", "mixed"}),
                                       # texels 1 .. 66 of tile (1, 1): an odd origin, a second column chunk of two texels and five row blocks
                                       Call("weights_alpha_dominant", rect=(69, 69, 66, 66), reach={"second_row_block", "second_column_chunk"})]),
    # T = 136, b = 3 (c = 130): three column chunks, an odd border
    "t136_b3": ("planar_136", [Call("colour_eight", rect=(120, 125, 150, 40), reach={"second_row_block", "second_column_chunk", "mixed"})]),
    # the cube at T = 16: texels on edges of an even and an odd side and at a corner, whose taps read cross-face aprons
    "cube_lod_count_2": ("cube_2", [Call("colour_eight", side=0, rect=(0, 5, 3, 14), reach={"face_edge"}),
                                    Call("weights_alpha_dominant", side=3, rect=(18, 0, 6, 6), reach={"face_edge", "face_corner"}),
                                    Call("hard_bands", side=4, reach={"face_edge", "face_corner", "holes"}),
                                    Call("one", side=1, lod=0, rect=(0, 0, 12, 12))]),
    "cube_lod_count_3": ("cube_3", [Call("colour_eight", side=2, rect=(40, 0, 8, 30), reach={"face_edge", "face_corner"}),
                                    Call("leaves_some_to_fallback", side=5, reach={"face_edge", "face_corner", "holes"}),
                                    Call("hard_bands", side=1, lod=1, rect=(0, 3, 24, 20), reach={"face_edge"})]),
    # the plan
    "missing_tiles": ("partial", [Call("colour_eight"), Call("hard_bands", rect=(7, 9, 10, 9))]),
    "missing_parent": ("no_lod0", [Call("colour_eight", rect=(19, 19, 10, 10))]),
    "below_the_finest_lod": ("planar_b2", [Call("colour_eight", lod=1, rect=(5, 6, 14, 13), reach={"mixed"})]),
}
SMALL = ["whole_face", "one_texel", "odd_origin_over_four_tiles", "ends_mid_tile", "one_rule", "weights_and_the_zero_rule", "hard_bands_infinite_bounds", "fallback",
         "black_and_the_zero_rule", "hole_block_texel_and_straddling_taps"]


def call_arguments(spec, call):
    """(lod, side, rect, mode, rules, fallback) of a call on an atlas of `spec`"""
    c = spec["T"] - 2 * spec["b"]
    lod = spec["lods"] - 1 if call["lod"] is None else call["lod"]
    rect = (0, 0, c << lod, c << lod) if call["rect"] is None else call["rect"]
    mode, rules = RULES[call["rules"]]
    return lod, call["side"], rect, mode, rules, FALLBACK.get(call["rules"], (0, 0, 0, 255))


def shape_reaches(spec, call, h_tiles):
    """names of what a call's rectangle reaches on an atlas that holds h_tiles (the kernel's constants: 16 rows per workgroup, 64 columns
    per chunk, 64 lanes)"""
    T, b = spec["T"], spec["b"]
    c = T - 2 * b
    lod, side, (x0, y0, w, h), _, _, _ = call_arguments(spec, call)
    halo = T // (2 * c) + 2
    names = set()
    n = c << lod
    for coord in SM.rect_tiles(lod, side, (x0, y0, w, h), c):
        if coord not in h_tiles:
            continue
        ox, oy = coord[2] * c, coord[3] * c
        xa, xb, ya, yb = max(x0, ox) - ox, min(x0 + w, ox + c) - ox, max(y0, oy) - oy, min(y0 + h, oy + c) - oy  # [xa, xb) x [ya, yb) in the tile
        if yb - ya > 16:
            names.add("second_row_block")
        if xb - xa > 64:
            names.add("second_column_chunk")
        if min(xb - xa, 64) + 2 * halo > 64:
            names.add("second_lane_trip_of_the_staging")
        on_x, on_y = (ox + xa == 0) or (ox + xb == n), (oy + ya == 0) or (oy + yb == n)
        if spec["kind"] == "cube" and (on_x or on_y):
            names.add("face_edge")
        if spec["kind"] == "cube" and ((ox + xa == 0 or ox + xb == n) and (oy + ya == 0 or oy + yb == n)):
            names.add("face_corner")
        # a data texel of the rectangle within one texel of a no-data texel: its taps interpolate the hole's zeros
        tile = h_tiles[coord]
        data = tile != 0
        near = np.zeros_like(data)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                near |= ~np.roll(np.roll(data, dy, axis=0), dx, axis=1)
        part = (slice(b + ya, b + yb), slice(b + xa, b + xb))
        if (data[part] & near[part]).any():
            names.add("taps_straddle_a_hole")
    return names


def model_call(h_tiles, g_tiles, spec, call, reached=None):
    """the model's target tiles after one call: the rules on the tiles of its LOD, then F over the LODs up to it"""
    lod, side, rect, mode, rules, fallback = call_arguments(spec, call)
    coarse = {k: v for k, v in g_tiles.items() if k[1] <= lod}
    derived = SM.apply_splat(h_tiles, coarse, models(spec)[1], lod, side, rect, mode, rules, fallback, spec["b"], reached)
    out = dict(g_tiles)
    out.update(EM.propagate(derived, spec["b"], spec["kind"] == "cube"))
    return out


def assert_reached(name, n, spec, call, h_tiles, reached):
    counters = {"holes", "fallback", "zero_rule", "mixed", "partial"}
    for want in call["reach"] & counters:
        assert reached.get(want, 0) >= 1, (name, n, want, reached)
    shapes = call["reach"] - counters
    assert shapes <= shape_reaches(spec, call, h_tiles), (name, n, sorted(shapes - shape_reaches(spec, call, h_tiles)))

"""The numpy model of bt_atlas_splat_from_height (tests/_splat_model.py) held to the SPLAT section of include/bevy_terrain_amd.h, without a GPU:
against a per-texel restatement of the header's lines in plain Python, against closed forms, against the normal bake's model; then the
cases of tests/test_gpu_splat.py on states the CPU oracle makes from the same jobs: each reaches the branch it is named for; and the new
entry point through the C ABI: the symbol and every refusal that needs no device."""
import ctypes as C
import math

import numpy as np
import pytest

import _edit_model as EM
import _normal_model as NM
import _oracle as O
import _splat_cases as SC
import _splat_model as SM
from _splat_cases import R
from bevy_terrain_amd import _ffi

F = np.float32
U = 2.0 ** -24  # the unit roundoff of binary32
INF, NAN = math.inf, math.nan
MODEL = O.make_model("planar", (0, 0, 0), 1000.0, 0.0, -50.0, 450.0)


# ---------------------------------------------------------------------------------------------- 1. the header's lines, texel by texel

def restated_texel(raw, sz, model, mode, rules, fallback):
    """steps 1, 2, 4 - 7 of SPLAT for ONE texel in np.float32 scalars, written from the header (s.z is step 3's, not restated)"""
    if raw == 0:
        return (0, 0, 0, 0)

    def clamp01(t):
        return (F(1) if t > F(1) else t) if t > F(0) else F(0)

    def sm(t):
        return (t * t) * (F(3.0) - F(2.0) * t)

    def band(x, lo, hi, fade):
        if fade > 0:
            r = clamp01((x - (lo - fade)) / fade)
            q = clamp01(((hi + fade) - x) / fade)
        else:
            r = F(1) if x >= lo else F(0)
            q = F(1) if x <= hi else F(0)
        return sm(r) * sm(q)

    def enc8(v):
        return int(np.floor(F(0.5) + F(255.0) * clamp01(v)))

    with np.errstate(all="ignore"):
        v = F(raw) / F(65535.0)
        h = F(model.min_height) + (F(model.max_height) - F(model.min_height)) * v
        steep = F(1.0) - F(sz)
        w, total = [], None
        for rule in rules:
            lo, hi = rule.steep()
            wk = (F(rule.weight) * band(h, F(rule.height[0]), F(rule.height[1]), F(rule.height_fade))) * band(steep, F(lo), F(hi), F(rule.slope_fade))
            total = wk if total is None else total + wk
            w.append(wk)
        if total > 0:
            if mode == "weights":
                out = [enc8(wk / total) for wk in w] + [0] * (4 - len(w))
            else:
                out = []
                for ch in range(3):
                    acc = None
                    for rule, wk in zip(rules, w):
                        term = wk * F(rule.colour[ch])
                        acc = term if acc is None else acc + term
                    out.append(enc8(acc / total))
                out.append(255)
        else:
            out = [int(b) for b in fallback]
    if out[0] == 0 and out[1] == 0 and out[2] == 0:
        out[0] = 1
    return tuple(out)


def rough_tile(T, seed, holes=True):
    """a tile whose heights span most of the range and whose slopes span flat to steep, with a no-data block and texel"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:T, 0:T]
    tile = (9000 + 2600 * x + 300 * y * (y > T // 2) + rng.integers(0, 4000, (T, T))).astype(np.uint16)
    tile[:, T // 2:] = tile[:, T // 2:] // 32 + 30000  # a flat half
    if holes:
        tile[4:6, 5:8] = 0
        tile[T - 4, 3] = 0
    return tile


@pytest.mark.parametrize("rules", list(SC.RULES))
def test_model_equals_the_header_restated_per_texel(rules):
    """both modes, fade 0 and > 0, infinite bounds: the rule sets of the GPU cases on a tile that reaches holes, several rules at once, the
    fallback and the zero rule"""
    mode, rule_list = SC.RULES[rules]
    fallback = SC.FALLBACK.get(rules, (0, 0, 0, 255))
    T, b, lod = 16, 2, 2
    c = T - 2 * b
    seen = {}
    for seed in (1, 2):
        tile = rough_tile(T, seed)
        h, steep = SM.height_and_steep(MODEL, tile, b, lod)
        raw = tile[b:-b, b:-b]
        got = SM.splat_texels(raw, h, steep, mode, rule_list, fallback, seen)
        sz = SM.tile_s(MODEL, tile, b, lod)[2].reshape(c, c)
        for j in range(c):
            for i in range(c):
                assert tuple(int(v) for v in got[j, i]) == restated_texel(int(raw[j, i]), sz[j, i], MODEL, mode, rule_list, fallback), (seed, i, j)
    assert seen["holes"] >= 1 and seen["data"] > seen["holes"]
    assert steep.max() > 0.3 and steep.min() < 0.02, "the tile is all flat or all steep"


def test_the_rule_sets_reach_every_branch_of_the_restatement():
    """over the sets: a partial weight, several rules on one texel, the fallback, the zero rule, holes"""
    seen = {}
    for rules, (mode, rule_list) in SC.RULES.items():
        tile = rough_tile(16, 1)
        h, steep = SM.height_and_steep(MODEL, tile, 2, 2)
        SM.splat_texels(tile[2:-2, 2:-2], h, steep, mode, rule_list, SC.FALLBACK.get(rules, (0, 0, 0, 255)), seen)
    assert all(seen[name] >= 1 for name in ("holes", "fallback", "zero_rule", "mixed", "partial")), seen


# ---------------------------------------------------------------------------------------------- 2. closed forms

@pytest.mark.parametrize("T,b,exact", [(16, 1, True), (32, 2, True), (16, 2, False), (72, 2, False)])
def test_constant_heights_are_flat(T, b, exact):
    """equal texels: both differences are 0 and s.z = dist * (1 / sqrt(dist * dist)).  sqrt(dist * dist) is dist in binary32, and
    dist * fl(1 / dist) is 1 + e with |e| <= 2^-24 before its rounding, which gives 1 or 1 - 2^-24: steep is 0 or 2^-24 for any dist, and
    0 exactly for the shapes test_normal_model.py checks s = (0, 0, 1) on (a face of 1000: the same dist).  h is one value."""
    for value in (1, 1000, 65535):
        for lod in range(4):
            h, steep = SM.height_and_steep(MODEL, np.full((T, T), value, np.uint16), b, lod)
            assert steep.dtype == np.float32 and ((steep == 0.0) | (steep == F(2.0 ** -24))).all()
            if exact:
                assert (steep == 0.0).all(), (value, lod)
            assert (h == F(-50.0) + (F(450.0) - F(-50.0)) * (F(value) / F(65535.0))).all()


@pytest.mark.parametrize("T,b,lod,k", [(16, 2, 2, 2000), (16, 1, 0, 300), (32, 2, 1, 1500)])
def test_linear_ramp_has_the_steepness_of_its_gradient(T, b, lod, k):
    """heights 1000 + k * column: every tap pair differs by k * (T / c) texels' worth, so s.z = dist / hypot(dx, dist) and steep = 1 - s.z.
    The bound is test_normal_model.py's for s.z (5.3 spacings of the largest height over the gradient's length + 4 u) plus one rounding of
    the subtraction from 1 (u)."""
    c = T - 2 * b
    tile = np.broadcast_to((1000 + k * np.arange(T, dtype=np.int64)).astype(np.uint16), (T, T)).copy()
    h, steep = SM.height_and_steep(MODEL, tile, b, lod)
    span = 500.0
    dx = span * k * (T / c) / 65535.0
    dist = (1000.0 / 2.0) / (c * 2.0 ** lod)
    g = np.hypot(dx, dist)
    tol = 5.3 * float(np.spacing(F(span * float(tile.max()) / 65535.0 + 50.0))) / g + 4.0 * U + U
    found = np.abs(steep.astype(np.float64) - (1.0 - dist / g)).max()
    print(f"steep {1.0 - dist / g:.6f}, tol {tol / U:.1f} u, found {found / U:.2f} u")
    assert found <= tol and 1.0 - dist / g > 1e-3
    assert np.abs(h.astype(np.float64) - (-50.0 + span * tile[b:-b, b:-b] / 65535.0)).max() <= 500.0 * 2 * U


def test_complementary_ramps_share_the_whole():
    """rule A: height <= a fading out over f; rule B: height >= a + f fading in over f.  Between a and a + f, with t = (x - a) / f, A's band
    is sm(1 - t) and B's sm(t), and sm(t) + sm(1 - t) = 1: the two bytes are enc8 of two numbers that sum to 1 up to rounding: 255 +- 1."""
    a, f = 100.0, 200.0
    rules = [R(height=(-INF, a), height_fade=f), R(height=(a + f, INF), height_fade=f)]
    raw = np.arange(1, 65536, 7, dtype=np.uint16)
    h = (F(-50.0) + F(500.0) * (raw.astype(np.float32) / F(65535.0))).astype(np.float32)
    out = SM.splat_texels(raw, h, np.zeros(raw.shape, np.float32), "weights", rules, (0, 0, 0, 0))
    inside = (h > a) & (h < a + f)
    total = out[..., 0].astype(int) + out[..., 1].astype(int)
    assert inside.sum() > 1000 and (np.abs(total[inside] - 255) <= 1).all()
    assert (out[..., 0][inside] > 0).any() and (out[..., 1][inside] > 0).any() and (out[..., 2:] == 0).all()
    assert (out[h <= a][:, :2] == (255, 0)).all() and (out[h >= a + f][:, :2] == (0, 255)).all()
    # monotonic: A's share falls with the height
    assert (np.diff(out[..., 0].astype(int)) <= 0).all()


def test_fallback_zero_rule_and_holes():
    raw = np.array([0, 30000, 30000, 60000, 0], np.uint16)
    h = np.array([100.0, 100.0, 300.0, 300.0, 300.0], np.float32)
    steep = np.zeros(5, np.float32)
    rules = [R(height=(50.0, 150.0), colour=(0.5, 0.25, 1.0))]
    seen = {}
    out = SM.splat_texels(raw, h, steep, "colour", rules, (9, 8, 7, 6), seen)
    assert out.tolist() == [[0, 0, 0, 0], [128, 64, 255, 255], [9, 8, 7, 6], [9, 8, 7, 6], [0, 0, 0, 0]]  # a hole in, a hole out; a texel no rule reaches: the fallback
    assert seen["holes"] == 2 and seen["fallback"] == 2 and seen["zero_rule"] == 0
    # the zero rule: a black colour, a black fallback, and a weights map whose first three bytes are 0
    out = SM.splat_texels(raw, h, steep, "colour", [R(height=(50.0, 150.0))], (0, 0, 0, 200), seen)
    assert out.tolist() == [[0, 0, 0, 0], [1, 0, 0, 255], [1, 0, 0, 200], [1, 0, 0, 200], [0, 0, 0, 0]] and seen["zero_rule"] == 3
    four = [R(height=(-INF, 0.0)), R(height=(-INF, 0.0)), R(height=(-INF, 0.0)), R(height=(50.0, INF))]
    out = SM.splat_texels(raw, h, steep, "weights", four, (0, 0, 0, 0))
    assert out.tolist() == [[0, 0, 0, 0], [1, 0, 0, 255], [1, 0, 0, 255], [1, 0, 0, 255], [0, 0, 0, 0]]
    # a NaN steepness reaches no band, hard or faded
    nan = np.full(5, np.nan, np.float32)
    for fade in (0.0, 0.1):
        out = SM.splat_texels(raw, h, nan, "colour", [R(colour=(1.0, 1.0, 1.0), slope=(10.0, 80.0), slope_fade=fade)], (9, 8, 7, 6))
        assert (out[[1, 2, 3]] == (9, 8, 7, 6)).all()


def test_slope_limits_in_degrees():
    assert R().steep() == (-INF, INF) and R(slope=(0.0, 90.0)).steep() == (-INF, INF)
    lo, hi = R(slope=(30.0, 60.0)).steep()
    assert lo == float(F(1.0 - math.cos(math.radians(30.0)))) and hi == float(F(0.5))
    c = R(height=(1.0, 2.0), slope=(30.0, 60.0), height_fade=3.0, slope_fade=0.25, weight=5.0, colour=(0.1, 0.2, 0.3))._c()
    assert C.sizeof(c) == 48 and (c.height_lo, c.height_hi, c.height_fade, c.steep_fade, c.weight) == (1.0, 2.0, 3.0, 0.25, 5.0)
    assert c.steep_lo == lo and c.steep_hi == hi and list(c.colour) == [float(F(0.1)), float(F(0.2)), float(F(0.3))]


# ---------------------------------------------------------------------------------------------- 3. s is the normal bake's

@pytest.mark.parametrize("T,b", [(16, 2), (16, 1)])
def test_s_encodes_to_the_normal_map(T, b):
    c = T - 2 * b
    for lod in (0, 2):
        tile = rough_tile(T, 3)
        s = SM.tile_s(MODEL, tile, b, lod)
        baked = NM.tile_normal_map(MODEL, tile, b, lod)
        data = tile[b:-b, b:-b] != 0
        for k in range(3):
            assert np.array_equal(NM.enc(s[k]).reshape(c, c)[data], baked[..., k][data])
        assert data.sum() < c * c


# ---------------------------------------------------------------------------------------------- 4. the GPU cases reach their branches

@pytest.mark.parametrize("name", list(SC.CASES))
def test_cases_reach_their_branches(name):
    spec_name, calls = SC.CASES[name]
    spec = SC.SPECS[spec_name]
    b = spec["b"]
    h_tiles, g_tiles = SC.oracle_state(spec_name)
    assert set(h_tiles) == set(g_tiles)
    fine = spec["lods"] - 1
    assert any((t[b:-b, b:-b] == 0).any() for k, t in h_tiles.items() if k[1] == fine), "no no-data texel was planted"
    for n, call in enumerate(calls):
        reached = {}
        after = SC.model_call(h_tiles, g_tiles, spec, call, reached)
        SC.assert_reached(name, n, spec, call, h_tiles, reached)
        assert reached.get("data", 0) >= 1, (name, n, "the rectangle holds no data texel of an existing tile")
        changed_texels = sum(int((g_tiles[k][b:-b, b:-b] != after[k][b:-b, b:-b]).any(axis=-1).sum()) for k in g_tiles)
        assert changed_texels >= 1, (name, n, "the call changes nothing")
        g_tiles = after


def test_shape_names_of_the_big_cases():
    spec = SC.SPECS["planar_72"]
    h_tiles = {(0, 2, x, y): np.ones((72, 72), np.uint16) for x in range(4) for y in range(4)}
    assert SC.shape_reaches(spec, SC.Call("one"), h_tiles) >= SC.WHOLE_72
    assert not SC.shape_reaches(spec, SC.Call("one", rect=(0, 0, 16, 16)), h_tiles) & {"second_row_block", "second_column_chunk"}


# ---------------------------------------------------------------------------------------------- 5. the C ABI without a device

BT_ERR_INVALID_ARGUMENT = -1


def rule_c(**fields):
    values = dict(height_lo=-INF, height_hi=INF, height_fade=0.0, steep_lo=-INF, steep_hi=INF, steep_fade=0.0, weight=1.0, colour=(0.5, 0.5, 0.5))
    values.update(fields)
    colour = values.pop("colour")
    return _ffi.SplatRuleC(colour=(C.c_float * 3)(*colour), **values)


BAD_RULES = {
    "height_lo nan": (dict(height_lo=NAN), "NaN"), "height_hi nan": (dict(height_hi=NAN), "NaN"), "steep_lo nan": (dict(steep_lo=NAN), "NaN"),
    "steep_hi nan": (dict(steep_hi=NAN), "NaN"), "height_fade nan": (dict(height_fade=NAN), "fade"), "steep_fade nan": (dict(steep_fade=NAN), "fade"),
    "weight nan": (dict(weight=NAN), "weight"), "height lo > hi": (dict(height_lo=2.0, height_hi=1.0), "lo > hi"),
    "steep lo > hi": (dict(steep_lo=0.5, steep_hi=0.25), "lo > hi"), "height_fade negative": (dict(height_fade=-1.0), "fade"),
    "height_fade inf": (dict(height_fade=INF), "fade"), "steep_fade negative": (dict(steep_fade=-0.5), "fade"), "steep_fade inf": (dict(steep_fade=INF), "fade"),
    "weight negative": (dict(weight=-1.0), "weight"), "weight inf": (dict(weight=INF), "weight"),
}


def test_symbol_and_the_refusals_that_need_no_device():
    """the entry point exists in the header, the binding and the library; with a NULL atlas every refusal that is decided before the atlas is
    looked at names its reason, and valid arguments get as far as the NULL atlas; stats are zeroed by every refused call"""
    assert "bt_atlas_splat_from_height" in _ffi.header_symbols() and "bt_atlas_splat_from_height" in _ffi.PROTOTYPES
    L = _ffi.lib()
    model = _ffi.TerrainModelC(kind=0, a=1000.0, min_height=0.0, max_height=100.0)
    good = (_ffi.SplatRuleC * 8)(*[rule_c() for _ in range(8)])
    fallback = (C.c_uint8 * 4)(1, 2, 3, 4)
    few = (_ffi.TileCoordinateC * 2)()

    def call(model=C.byref(model), mode=_ffi.SPLAT_COLOUR, rules=good, count=1, fallback=fallback, changed=None, cap=0, why=None):
        stats = _ffi.EditStatsC(*([7] * 8))
        status = L.bt_atlas_splat_from_height(None, 0, 1, model, 0, 0, 0, 0, 4, 4, mode, rules, count, fallback, changed, cap, C.byref(stats))
        assert status == BT_ERR_INVALID_ARGUMENT, (why, status)
        assert not any(getattr(stats, name) for name, _ in _ffi.EditStatsC._fields_), "stats are not zeroed"
        text = L.bt_last_error().decode()
        assert text.startswith("bt_atlas_splat_from_height: ") and why in text, (why, text)

    call(why="NULL atlas")
    call(count=8, why="NULL atlas")
    call(mode=_ffi.SPLAT_WEIGHTS, count=4, why="NULL atlas")
    call(changed=few, cap=2, why="NULL atlas")
    call(model=None, why="NULL model")
    call(rules=None, why="NULL rules")
    call(fallback=None, why="NULL fallback")
    call(cap=2, why="NULL changed")
    call(mode=2, why="mode 2")
    call(count=0, why="0 rules")
    call(count=9, why="9 rules")
    call(mode=_ffi.SPLAT_WEIGHTS, count=5, why="5 rules")
    for name, (fields, why) in BAD_RULES.items():
        for mode in (_ffi.SPLAT_COLOUR, _ffi.SPLAT_WEIGHTS):
            call(mode=mode, rules=(_ffi.SplatRuleC * 2)(rule_c(), rule_c(**fields)), count=2, why="rule 1: ")
            assert why in L.bt_last_error().decode(), (name, L.bt_last_error().decode())
    call(rules=(_ffi.SplatRuleC * 1)(rule_c(colour=(0.5, INF, 0.5))), why="colour")
    call(rules=(_ffi.SplatRuleC * 1)(rule_c(colour=(NAN, 0.5, 0.5))), why="colour")
    call(mode=_ffi.SPLAT_WEIGHTS, rules=(_ffi.SplatRuleC * 1)(rule_c(colour=(NAN, 0.5, 0.5))), why="colour")  # a NaN anywhere
    call(mode=_ffi.SPLAT_WEIGHTS, rules=(_ffi.SplatRuleC * 1)(rule_c(colour=(0.5, INF, 0.5))), why="NULL atlas")  # weights mode does not read the colour
    call(rules=(_ffi.SplatRuleC * 1)(rule_c(height_lo=-INF, height_hi=-INF, steep_lo=INF, steep_hi=INF)), why="NULL atlas")  # lo == hi, infinite: legal
    call(model=C.byref(_ffi.TerrainModelC(kind=3, a=1000.0)), why="model")
    call(model=C.byref(_ffi.TerrainModelC(kind=0, a=0.0)), why="model")

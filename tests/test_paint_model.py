"""tests/_paint_model.py against the definitions in include/bevy_terrain_amd.h (PAINT, bt_atlas_read_region), without a GPU: the
vectorised model is held against a per-texel scalar restatement of the header's lines, then its fixed points, the hole rules, the order of
the stamps, and read_region against _edit_model.write_region.  The two entry points are called with a NULL atlas through ctypes."""
import ctypes as C
import itertools

import numpy as np
import pytest

import _edit_model as EM
import _paint_model as PM
from bevy_terrain_amd import PaintStamp as P
from bevy_terrain_amd import _ffi

F32 = np.float32
BT_ERR_INVALID_ARGUMENT = -1


def scalar_stamp(u, gx, gy, s):
    """the header's PAINT section for one texel, one np.float32 operation per written operation; u: four ints"""
    u = [int(v) for v in u]
    if u[0] | u[1] | u[2] == 0:
        return u
    dx = F32(gx) - F32(s.center[0])
    dy = F32(gy) - F32(s.center[1])
    d2 = F32(dx * dx) + F32(dy * dy)
    r2 = F32(s.radius) * F32(s.radius)
    if not d2 < r2:
        return u
    if s.falloff == "hard":
        w = F32(1)
    else:
        q = F32(d2 / r2)
        sm = F32(F32(1) - q)
        w = F32(sm * sm)
    a = F32(F32(s.opacity) * w)
    mask = s.channel_mask()
    out = list(u)
    for k in range(4):
        if not (mask >> k) & 1:
            continue
        c = F32(F32(u[k]) / F32(255))
        colour = F32(s.color[k])
        if s.mode == "blend":
            cn = F32(c + F32(F32(colour - c) * a))
        else:
            cn = F32(c + F32(colour * a))
        clamped = min(max(cn, F32(0)), F32(1))
        out[k] = int(np.floor(F32(F32(0.5) + F32(F32(255) * clamped))))
    if out[0] | out[1] | out[2] == 0:
        for k in range(3):
            if (mask >> k) & 1:
                out[k] = 1
    return out


def random_texels(rng, h, w):
    """texels with many small and saturated bytes (the zero rule and the clamp are reached) and some without data"""
    t = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
    small = rng.random((h, w)) < 0.3
    t[small] = rng.integers(0, 3, size=(int(small.sum()), 4), dtype=np.uint8)
    t[rng.random((h, w)) < 0.1, :3] = 0
    return t


@pytest.mark.parametrize("mode,falloff", list(itertools.product(["blend", "add"], ["smooth", "hard"])))
def test_model_is_the_scalar_restatement(mode, falloff):
    rng = np.random.default_rng(5)
    h, w = 9, 11
    gy, gx = np.mgrid[0:h, 0:w]
    gx, gy = gx + 37, gy + 101
    zero_rule = 0
    for mask in range(1, 16):
        t = random_texels(rng, h, w)
        for colour, opacity in [((0.9, 0.2, 0.4, 1.0), 0.7), ((-0.3, 0.0, 1.6, -1.0), 1.0), (tuple(rng.random(4).tolist()), 0.37)]:
            s = P((41.3, 105.6), 5.25, colour, opacity=opacity, mode=mode, falloff=falloff, channels=mask)
            reached = {}
            got = PM.paint_texels(t, gx, gy, s, reached)
            want = np.array([[scalar_stamp(t[y, x], gx[y, x], gy[y, x], s) for x in range(w)] for y in range(h)], dtype=np.uint8)
            assert np.array_equal(got, want), (mask, colour, np.argwhere(got != want)[:3].tolist())
            assert 0 < reached["under_disc"] < h * w and reached["holes_under_disc"] > 0
            zero_rule += reached["zero_rule"]
            unselected = [k for k in range(4) if not (mask >> k) & 1]
            assert np.array_equal(got[..., unselected], t[..., unselected])
    assert zero_rule > 0, "the zero rule was never reached"


def field(n=24, seed=2):
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 256, size=(n, n, 4), dtype=np.uint8)
    t[..., 0] |= 1
    gy, gx = np.mgrid[0:n, 0:n]
    return t, gx, gy


def test_blend_towards_the_own_colour_changes_nothing():
    """c + (c - c) * a == c, and floor(0.5 + 255 * (f32(v) / 255)) == v for every byte v"""
    every = np.arange(256, dtype=np.uint8)
    assert np.array_equal(np.floor(F32(0.5) + F32(255) * (every.astype(F32) / F32(255))).astype(np.uint8), every)
    gy, gx = np.mgrid[0:16, 0:16]
    for v in (1, 2, 77, 128, 254, 255):
        t = np.full((16, 16, 4), v, np.uint8)
        colour = tuple([float(F32(v) / F32(255))] * 4)
        for falloff, opacity in (("smooth", 0.6), ("hard", 1.0), ("smooth", 1.0)):
            assert np.array_equal(PM.paint_texels(t, gx, gy, P((7.5, 8.0), 6.0, colour, opacity=opacity, falloff=falloff), None), t)


def test_full_hard_blend_gives_the_colour_exactly():
    t, gx, gy = field()
    for v in (1, 3, 100, 200, 255):
        s = P((11.5, 12.0), 7.0, tuple([float(F32(v) / F32(255))] * 4), opacity=1.0, falloff="hard")
        got = PM.paint_texels(t, gx, gy, s)
        disc = (gx - 11.5) ** 2 + (gy - 12.0) ** 2 < 49.0
        assert (got[disc] == v).all() and np.array_equal(got[~disc], t[~disc]) and 100 < disc.sum() < t.shape[0] * t.shape[1]


def test_hole_rules():
    t, gx, gy = field()
    t[3:7, 5:9, :3] = 0
    t[3:7, 5:9, 3] = 200  # rgb == 0 and alpha != 0: no data
    t[15, 15] = 0
    holes = (t[..., :3] == 0).all(axis=-1)
    stamps = [P((8.0, 6.0), 9.0, (0.0, 0.0, 0.0, 0.0), falloff="hard"), P((12.0, 12.0), 30.0, (-1.0, -1.0, -1.0, -1.0), mode="add", opacity=0.9),
              P((12.0, 12.0), 30.0, (0.0, 0.0, 0.0, 0.5), channels="a"), P((14.0, 14.0), 6.0, (-2.0, 0.0, 0.0, 0.0), mode="add", channels="r"),
              P((6.0, 6.0), 5.0, (0.0, 0.0, 0.0, 0.0), channels="gb", falloff="hard")]
    u, reached = t, {}
    for s in stamps:
        v = PM.paint_texels(u, gx, gy, s, reached)
        assert np.array_equal(v[holes], t[holes]), "a texel without data was touched"
        assert np.array_equal((v[..., :3] == 0).all(axis=-1), holes), "a stamp made or filled a hole"
        if s.channel_mask() == 8:
            assert np.array_equal(v[..., :3], u[..., :3]) and not np.array_equal(v[..., 3], u[..., 3]), "an alpha-only mask"
        u = v
    assert reached["zero_rule"] > 100 and reached["holes_under_disc"] >= 17
    # the zero rule sets exactly the channels of the mask among r, g, b
    one = np.array([[[1, 0, 0, 9]]], np.uint8)
    zero = np.zeros((1, 1), np.int64)
    assert PM.paint_texels(one, zero, zero, P((0.0, 0.0), 1.0, (0.0,) * 4, falloff="hard", channels="ra")).tolist() == [[[1, 0, 0, 0]]]
    assert PM.paint_texels(one, zero, zero, P((0.0, 0.0), 1.0, (0.0,) * 4, falloff="hard", channels="rgb")).tolist() == [[[1, 1, 1, 9]]]
    assert PM.paint_texels(one, zero, zero, P((0.0, 0.0), 1.0, (0.0,) * 4, falloff="hard", channels="g")).tolist() == [[[1, 0, 0, 9]]]


def test_stamps_apply_in_list_order():
    T, b = 16, 2
    rng = np.random.default_rng(4)
    tiles = {(0, 1, x, y): rng.integers(1, 256, size=(T, T, 4), dtype=np.uint8) for x in range(2) for y in range(2)}
    tiles[(0, 0, 0, 0)] = rng.integers(1, 256, size=(T, T, 4), dtype=np.uint8)
    tiles[(1, 1, 0, 0)] = rng.integers(1, 256, size=(T, T, 4), dtype=np.uint8)
    s1, s2 = P((11.0, 12.0), 6.0, (1.0, 0.0, 0.5, 1.0), opacity=0.8), P((13.0, 11.0), 5.0, (0.5, 0.5, -0.5, 0.0), mode="add", falloff="hard")
    ab, ba = PM.apply_paint(tiles, 1, [s1, s2], b), PM.apply_paint(tiles, 1, [s2, s1], b)
    assert any(not np.array_equal(ab[k], ba[k]) for k in tiles)
    one_by_one = PM.apply_paint(PM.apply_paint(tiles, 1, [s1], b), 1, [s2], b)
    assert all(np.array_equal(ab[k], one_by_one[k]) for k in tiles)
    # only the centre texels of the tiles of the LOD and of the stamp's side move
    for k in tiles:
        if k[0] != 0 or k[1] != 1:
            assert np.array_equal(ab[k], tiles[k])
        else:
            apron = np.ones((T, T), bool)
            apron[b:-b, b:-b] = False
            assert np.array_equal(ab[k][apron], tiles[k][apron])
    assert not np.array_equal(ab[(0, 1, 0, 0)], tiles[(0, 1, 0, 0)]) and not np.array_equal(ab[(0, 1, 1, 1)], tiles[(0, 1, 1, 1)])


@pytest.mark.parametrize("fmt", ["r16", "rgba8"])
def test_read_region_model_inverts_the_write_region_model(fmt):
    T, b, lod = 16, 2, 2
    c = T - 2 * b
    rng = np.random.default_rng(9)

    def tile():
        return rng.integers(1, 65536, size=(T, T), dtype=np.uint16) if fmt == "r16" else rng.integers(1, 256, size=(T, T, 4), dtype=np.uint8)

    held = [(x, y) for x in range(4) for y in range(4) if (x, y) not in ((0, 0), (2, 1), (3, 3))]
    tiles = {(0, lod, x, y): tile() for x, y in held}
    tiles[(0, 1, 0, 0)] = tile()
    tiles[(1, lod, 0, 0)] = tile()
    n = 4 * c
    for x0, y0, w, h in [(0, 0, n, n), (c - 5, c - 3, 11, 9), (1, 2, 3, 4), (2 * c + 1, c + 1, c - 2, 3), (n - 1, n - 1, 1, 1), (5, 5, 0, 3)]:
        texels = (rng.integers(1, 65536, size=(h, w), dtype=np.uint16) if fmt == "r16" else rng.integers(1, 256, size=(h, w, 4), dtype=np.uint8))
        written = EM.write_region(tiles, lod, 0, x0, y0, texels, b)
        got, missing = PM.read_region(written, lod, 0, x0, y0, w, h, b)
        gy, gx = np.mgrid[y0:y0 + h, x0:x0 + w]
        over_held = np.zeros((h, w), bool)
        for x, y in held:
            over_held |= (gx // c == x) & (gy // c == y)
        assert np.array_equal(got[over_held], texels[over_held]) and not got[~over_held].any()
        absent = {(int(x), int(y)) for x, y in zip((gx // c).ravel(), (gy // c).ravel())} - set(held)
        assert missing == len(absent)
        # texels outside the rectangle, other LODs and other sides are as they were: the read of the unwritten state differs only inside
        before, _ = PM.read_region(tiles, lod, 0, 0, 0, n, n, b)
        after, _ = PM.read_region(written, lod, 0, 0, 0, n, n, b)
        outside = np.ones((n, n), bool)
        outside[y0:y0 + h, x0:x0 + w] = False
        assert np.array_equal(before[outside], after[outside])
    absent, missing = PM.read_region(tiles, lod, 0, 0, 0, c, c, b)
    assert missing == 1 and not absent.any() and absent.shape[:2] == (c, c)
    assert np.array_equal(PM.read_region(tiles, 1, 0, 0, 0, c, c, b)[0], tiles[(0, 1, 0, 0)][b:-b, b:-b])
    assert np.array_equal(PM.read_region(tiles, lod, 1, 3, 2, 4, 5, b)[0], tiles[(1, lod, 0, 0)][b + 2:b + 7, b + 3:b + 7])


def test_binding_and_null_atlas():
    for name in ("bt_atlas_paint", "bt_atlas_read_region"):
        assert name in _ffi.header_symbols() and name in _ffi.PROTOTYPES, name
    assert C.sizeof(_ffi.PaintStampC) == 48 and (_ffi.PAINT_BLEND, _ffi.PAINT_ADD) == (0, 1)
    assert P((1.0, 2.0), 3.0, (0.1, 0.2, 0.3, 0.4), channels="ga").channel_mask() == 10 and P((1.0, 2.0), 3.0, (0.0,) * 4, channels=(0, 2)).channel_mask() == 5
    c = P((1.0, 2.0), 3.0, (0.25, 0.5, 0.75, 1.0), opacity=0.5, mode="add", falloff="hard", channels="b", side=4)._c()
    assert (c.side, c.mode, c.falloff, c.channel_mask, list(c.center), c.radius, c.opacity, list(c.color)) == (4, 1, 1, 4, [1.0, 2.0], 3.0, 0.5, [0.25, 0.5, 0.75, 1.0])
    L = _ffi.lib()
    one = (_ffi.PaintStampC * 1)(P((5.0, 5.0), 2.0, (0.5,) * 4)._c())
    stats = _ffi.EditStatsC(1, 2, 3, 4, 5, 6, 7, 8)
    assert L.bt_atlas_paint(None, 0, 0, one, 1, None, 0, C.byref(stats)) == BT_ERR_INVALID_ARGUMENT
    assert b"NULL atlas" in L.bt_last_error() and not any(getattr(stats, f) for f, _ in _ffi.EditStatsC._fields_)
    assert L.bt_atlas_paint(None, 0, 0, None, 0, None, 0, None) == BT_ERR_INVALID_ARGUMENT
    buf = (C.c_uint8 * 64)()
    missing = C.c_uint32(5)
    assert L.bt_atlas_read_region(None, 0, 0, 0, 0, 0, 4, 4, buf, 0, C.byref(missing)) == BT_ERR_INVALID_ARGUMENT
    assert b"NULL atlas" in L.bt_last_error() and missing.value == 0 and not any(buf)
    assert L.bt_atlas_read_region(None, 0, 0, 0, 0, 0, 0, 0, None, 0, None) == BT_ERR_INVALID_ARGUMENT
    # what can be refused without the atlas is refused without it, as by the other brushes
    bad = (_ffi.PaintStampC * 1)(P((5.0, 5.0), 2.0, (0.5,) * 4, channels=0)._c())
    assert L.bt_atlas_paint(None, 0, 0, bad, 1, None, 0, None) == BT_ERR_INVALID_ARGUMENT and b"channel_mask" in L.bt_last_error()

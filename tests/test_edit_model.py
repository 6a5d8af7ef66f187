"""CPU checks of in-place editing: the numpy model (tests/_edit_model.py) pinned against the committed goldens (outputs of the reference's
own WGSL), the brush arithmetic against answers worked by hand, and the three entry points' export and argument checks (no GPU: what can
be refused before any device work is).  The GPU comparisons are in test_gpu_edit.py."""
import ctypes as C
import os
from collections import namedtuple

import numpy as np
import pytest

import _edit_model as EM
import _oracle as O
from bevy_terrain_amd import _ffi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BT_ERR_INVALID_ARGUMENT = -1
Stamp = namedtuple("Stamp", "center radius amount mode falloff side", defaults=("add", "smooth", 0))

# planar_r16_t24_overlay is left out: its second dataset re-splits, re-downsamples and re-stitches only ITS OWN tiles (preprocessor.rs:298-312
# queues tasks for the tiles of the dataset's rectangle), so the aprons of the first dataset's tiles next to the overlay still mirror the
# centres from before the overlay: that golden's state is not F of its primary centres, by the reference's own behaviour.
PINNED = ["planar_r16_t16", "planar_r16_t32_subrect", "planar_rgba8_t16", "planar_rgba8_t32_b3", "cube_r16_t16", "cube_rgba8_t16"]


def golden_tiles(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    fmt, T, b, lods = (int(v) for v in g["params"])
    return {tuple(int(v) for v in row[:4]): g["tiles"][k] for k, row in enumerate(g["coords"])}, b, name.startswith("cube")


@pytest.mark.parametrize("name", PINNED)
def test_propagate_reproduces_the_golden(name):
    """F applied to the golden's own tiles gives every golden tile back byte for byte: derived centres, aprons, cube seams"""
    tiles, b, cube = golden_tiles(name)
    got = EM.propagate(tiles, b, cube)
    bad = [k for k in tiles if not np.array_equal(got[k], tiles[k])]
    assert not bad, (name, len(bad), len(tiles), bad[:4])
    assert any(any(k in tiles for k in O.children(c)) for c in tiles), "no derived tile: the pin would be empty"


def test_propagate_notices_a_stale_ancestor_and_a_stale_apron():
    """the pin has teeth: a changed primary texel moves its ancestors and the aprons that mirror it"""
    tiles, b, cube = golden_tiles("planar_r16_t16")
    finest = max(k[1] for k in tiles)
    coord = (0, finest, 1, 1)
    edited = {k: v.copy() for k, v in tiles.items()}
    edited[coord][b, b] ^= 0x4000  # the tile's top-left centre texel: mirrored by three neighbours' aprons
    got = EM.propagate(edited, b, cube)
    differing = {k for k in tiles if not np.array_equal(got[k], tiles[k])}
    assert {coord, (0, finest - 1, 0, 0), (0, finest, 0, 0), (0, finest, 1, 0), (0, finest, 0, 1)} <= differing
    assert differing <= EM.allowed_changed(tiles, {coord}, cube)


def field(value=0x8000, n=9):
    return np.full((n, n), value, np.uint16), *np.mgrid[0:n, 0:n][::-1]


def test_brush_known_answers_smooth_radius_two():
    """constant 0x8000, radius 2 at the integer centre (4, 4), ADD 0.25: w = 1 at d2 = 0, (1 - 1/4)^2 = 0.5625 at d2 = 1, 0.25 at d2 = 2, and
    d2 = 4 is not < r2.  h = 32768/65535; t' = floor(0.5 + 65535 * (h + 0.25 * w))"""
    t, gx, gy = field()
    out = EM.stamp_texels(t, gx, gy, Stamp((4.0, 4.0), 2.0, 0.25))
    assert out[4, 4] == 49152 and out[4, 5] == out[3, 4] == 41984 and out[3, 3] == out[5, 5] == 36864  # 32768 + 16384 / 9216 / 4096 (+- rounding: exact here)
    assert out[4, 6] == out[2, 4] == out[4, 2] == 0x8000 and out[0, 0] == 0x8000
    assert (out != 0x8000).sum() == 9
    # the weights themselves, in float32
    assert np.float32(1) - np.float32(1) / np.float32(4) == np.float32(0.75) and np.float32(0.75) * np.float32(0.75) == np.float32(0.5625)


def test_brush_flatten_hard_lands_on_the_target_and_zeros_stay():
    t, gx, gy = field()
    t[4, 5] = 0
    for target in (0.0, 0.25, 1.0, 12345 / 65535):
        out = EM.stamp_texels(t, gx, gy, Stamp((4.0, 4.0), 3.0, target, "flatten", "hard"))
        want = max(1, int(np.floor(0.5 + 65535 * np.float32(target))))
        assert out[4, 4] == want and out[4, 5] == 0 and out[4, 7] == 0x8000, (target, out[4, 4], want)
    # SMOOTH at the centre has w = 1 too
    assert EM.stamp_texels(t, gx, gy, Stamp((4.0, 4.0), 3.0, 0.25, "flatten"))[4, 4] == 16384


def test_brush_never_produces_zero_and_saturates():
    t, gx, gy = field(3)
    out = EM.stamp_texels(t, gx, gy, Stamp((4.0, 4.0), 2.0, -1.0, "add", "hard"))
    assert out[4, 4] == 1 and out[0, 0] == 3  # clamp(h') = 0 -> floor(0.5) = 0 -> max(1, .)
    out = EM.stamp_texels(t, gx, gy, Stamp((4.0, 4.0), 2.0, 0.4 / 65535 - 3 / 65535, "add", "hard"))
    assert out[4, 4] == 1  # a result below 0.5 / 65535
    out = EM.stamp_texels(field(65000)[0], gx, gy, Stamp((4.0, 4.0), 2.0, 0.5, "add", "hard"))
    assert out[4, 4] == 65535


def test_stamp_order_matters():
    tiles = {(0, 0, 0, 0): np.full((12, 12), 0x8000, np.uint16)}
    add, flat = Stamp((4.0, 4.0), 3.0, 0.25, "add", "hard"), Stamp((4.0, 4.0), 3.0, 0.125, "flatten", "hard")
    a = EM.apply_stamps(tiles, 0, [add, flat], 2)[(0, 0, 0, 0)]
    f = EM.apply_stamps(tiles, 0, [flat, add], 2)[(0, 0, 0, 0)]
    assert a[6, 6] == 8192 and f[6, 6] == 8192 + 16384  # centre texel (4, 4) is tile texel (6, 6) with b = 2
    assert a[0, 0] == f[0, 0] == 0x8000  # aprons are not the brush's
    # a stamp of another side does nothing
    assert np.array_equal(EM.apply_stamps(tiles, 0, [add._replace(side=3)], 2)[(0, 0, 0, 0)], tiles[(0, 0, 0, 0)])


def test_write_region_model_crosses_tiles_and_skips_absent_ones():
    tiles = {(0, 1, 0, 0): np.ones((8, 8), np.uint16), (0, 1, 1, 1): np.ones((8, 8), np.uint16)}  # c = 4, b = 2; (1, 0) and (0, 1) absent
    texels = np.arange(100, 136, dtype=np.uint16).reshape(6, 6)
    texels[2, 2] = 0
    out = EM.write_region(tiles, 1, 0, 1, 1, texels, 2)
    assert np.array_equal(out[(0, 1, 0, 0)][3:6, 3:6], texels[0:3, 0:3]) and out[(0, 1, 0, 0)][2, 2] == 1
    assert np.array_equal(out[(0, 1, 1, 1)][2:5, 2:5], texels[3:6, 3:6]) and out[(0, 1, 1, 1)][5, 5] == 1
    assert EM.region_tiles(1, 0, 1, 1, 6, 6, 4) == {(0, 1, 0, 0), (0, 1, 1, 0), (0, 1, 0, 1), (0, 1, 1, 1)}


def test_symbols_are_declared_and_bound():
    for name in ("bt_atlas_edit_height", "bt_atlas_write_region", "bt_atlas_save_tiles"):
        assert name in _ffi.header_symbols() and name in _ffi.PROTOTYPES, name
    assert C.sizeof(_ffi.EditStampC) == 32 and C.sizeof(_ffi.EditStatsC) == 32
    assert (_ffi.EDIT_ADD, _ffi.EDIT_FLATTEN, _ffi.EDIT_FALLOFF_SMOOTH, _ffi.EDIT_FALLOFF_HARD, _ffi.EDIT_MAX_STAMPS) == (0, 1, 0, 1, 256)


def stamp_c(side=0, mode=0, falloff=0, center=(1.0, 1.0), radius=1.0, amount=0.1):
    return _ffi.EditStampC(side, mode, falloff, 0, (C.c_float * 2)(*center), radius, amount)


def test_null_handles_are_refused():
    L = _ffi.lib()
    one = (_ffi.EditStampC * 1)(stamp_c())
    stats = _ffi.EditStatsC()
    assert L.bt_atlas_edit_height(None, 0, 0, one, 1, None, 0, C.byref(stats)) == BT_ERR_INVALID_ARGUMENT
    assert b"NULL atlas" in L.bt_last_error()
    assert L.bt_atlas_edit_height(None, 0, 0, None, 0, None, 0, None) == BT_ERR_INVALID_ARGUMENT
    texels = (C.c_uint16 * 4)()
    assert L.bt_atlas_write_region(None, 0, 0, 0, 0, 0, 2, 2, texels, 0, None, 0, None) == BT_ERR_INVALID_ARGUMENT
    assert b"NULL atlas" in L.bt_last_error()
    assert L.bt_atlas_save_tiles(None, 0, b"/nonexistent", None, 0) == BT_ERR_INVALID_ARGUMENT
    assert b"NULL atlas" in L.bt_last_error()


@pytest.mark.parametrize("why,make", [
    (b"side", lambda: [stamp_c(side=6)]),
    (b"mode", lambda: [stamp_c(mode=2)]),
    (b"falloff", lambda: [stamp_c(falloff=2)]),
    (b"center", lambda: [stamp_c(center=(float("nan"), 0.0))]),
    (b"center", lambda: [stamp_c(center=(0.0, float("inf")))]),
    (b"radius", lambda: [stamp_c(radius=0.0)]),
    (b"radius", lambda: [stamp_c(radius=-1.0)]),
    (b"radius", lambda: [stamp_c(radius=float("inf"))]),
    (b"radius", lambda: [stamp_c(radius=float("nan"))]),
    (b"amount", lambda: [stamp_c(amount=float("nan"))]),
    (b"stamp 1", lambda: [stamp_c(), stamp_c(radius=0.0)]),
    (b"at most 256", lambda: [stamp_c()] * 257),
])
def test_stamps_are_checked_before_any_device_work(why, make):
    """the stamp list is validated before the atlas is looked at: the refusal names the stamp's fault, not the NULL atlas"""
    L = _ffi.lib()
    stamps = make()
    arr = (_ffi.EditStampC * len(stamps))(*stamps)
    assert L.bt_atlas_edit_height(None, 0, 0, arr, len(stamps), None, 0, None) == BT_ERR_INVALID_ARGUMENT
    assert why in L.bt_last_error() and b"NULL atlas" not in L.bt_last_error(), L.bt_last_error()


def test_null_stamps_and_null_changed_are_refused():
    L = _ffi.lib()
    assert L.bt_atlas_edit_height(None, 0, 0, None, 1, None, 0, None) == BT_ERR_INVALID_ARGUMENT and b"NULL stamps" in L.bt_last_error()
    one = (_ffi.EditStampC * 1)(stamp_c())
    assert L.bt_atlas_edit_height(None, 0, 0, one, 1, None, 4, None) == BT_ERR_INVALID_ARGUMENT and b"changed" in L.bt_last_error()

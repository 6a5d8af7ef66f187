"""CPU checks of the smoothing brush (bt_atlas_smooth_height): the numpy model (tests/_smooth_model.py) against a second, per-texel
statement of the definition; the fixed points the header names; the snapshot property (an in-place pass gives other bytes); and the entry
point's export and argument checks (no GPU: everything that is refused before any device work).  The GPU comparisons are in
test_gpu_smooth.py."""
import ctypes as C

import numpy as np
import pytest

import _smooth_model as SM
from _smooth_model import Stamp
from bevy_terrain_amd import _ffi

F32 = np.float32
BT_ERR_INVALID_ARGUMENT = -1


def holed_tile(T=24, seed=3, holes=0.15):
    """a random layer, apron included, with single-texel holes and a block of them"""
    rng = np.random.default_rng(seed)
    tile = rng.integers(1, 65536, size=(T, T), dtype=np.uint16)
    tile[rng.random((T, T)) < holes] = 0
    tile[9:14, 3:9] = 0
    return tile


def texel_by_definition(S, b, k, i, j, gx, gy, stamps, side):
    """steps 1 - 3 of the header for ONE centre texel: a plain loop, an integer sum, np.float32 scalars"""
    px, py = b + i, b + j
    t0 = int(S[py][px])
    if t0 == 0:
        return 0
    total, n = 0, 0
    for dy in range(-k, k + 1):
        for dx in range(-k, k + 1):
            v = int(S[py + dy][px + dx])
            total += v
            n += 1 if v != 0 else 0
    m = F32(total) / (F32(65535) * F32(n))
    t = t0
    for s in stamps:
        if s.side != side:
            continue
        dx = F32(gx) - F32(s.center[0])
        dy = F32(gy) - F32(s.center[1])
        d2 = (dx * dx) + (dy * dy)
        r2 = F32(s.radius) * F32(s.radius)
        if not d2 < r2:
            continue
        if s.falloff == "hard":
            w = F32(1)
        else:
            q = d2 / r2
            sm = F32(1) - q
            w = sm * sm
        a = F32(s.strength) * w
        h = F32(t) / F32(65535)
        hn = h + (m - h) * a
        cl = F32(0) if hn < 0 else (F32(1) if hn > 1 else hn)
        t = max(1, int(np.floor(F32(0.5) + F32(65535) * cl)))
        assert all(isinstance(v, np.float32) for v in (m, d2, r2, w, a, h, hn, cl)), "an operation left binary32"
    return t


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_model_equals_the_definition_texel_by_texel(k):
    T, b = 24, 4
    c = T - 2 * b
    coord = (2, 1, 1, 0)  # mosaic origin (16, 0) on side 2
    tile = holed_tile(T, seed=3 + k)
    stamps = [Stamp((24.25, 7.5), 9.0, 0.75, side=2), Stamp((20.0, 4.0), 5.5, 1.0, "hard", side=2), Stamp((24.0, 8.0), 30.0, 0.5, side=3),
              Stamp((27.0, 11.0), 6.0, 0.3, "smooth", side=2)]
    out = SM.apply_smooth({coord: tile}, 1, stamps, b, k)[coord]
    want = tile.copy()
    for j in range(c):
        for i in range(c):
            want[b + j, b + i] = texel_by_definition(tile.tolist(), b, k, i, j, c + i, j, stamps, 2)
    assert np.array_equal(out, want), np.argwhere(out != want)[:4]
    centre = tile[b:-b, b:-b]
    assert (out != tile).sum() > c * c // 2 and np.array_equal(out == 0, tile == 0) and (centre == 0).sum() > 20
    aprons = np.ones((T, T), bool)
    aprons[b:-b, b:-b] = False
    assert np.array_equal(out[aprons], tile[aprons]), "the model wrote an apron texel"
    # the stamp of side 3 did nothing: without it the result is the same
    assert np.array_equal(SM.apply_smooth({coord: tile}, 1, [s for s in stamps if s.side == 2], b, k)[coord], out)


def whole(T, stamp_radius=100.0, **kw):
    return [Stamp((T / 2.0, T / 2.0), stamp_radius, **kw)]


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_fixed_points(k):
    """a constant field, a linear ramp (sum = n * t, so m == h bit for bit), an isolated data texel (n = 1); holes neither filled nor made"""
    T, b = 28, 4
    key = (0, 0, 0, 0)
    y, x = np.mgrid[0:T, 0:T]
    for name, tile in {
        "constant": np.full((T, T), 0x1234, np.uint16),
        "ramp": (1000 + 37 * x + 1501 * y).astype(np.uint16),
        "ramp_down": (60000 - 901 * x - 3 * y).astype(np.uint16),
    }.items():
        for stamps in (whole(T, strength=1.0, falloff="hard"), whole(T, strength=0.625), [Stamp((9.3, 11.1), 6.0, 0.9), Stamp((12.0, 8.0), 7.0, 1.0, "hard")]):
            out = SM.apply_smooth({key: tile}, 0, stamps, b, k)[key]
            assert np.array_equal(out, tile), (name, k, np.argwhere(out != tile)[:3])
    m, n = SM.box_mean((1000 + 37 * x + 1501 * y).astype(np.uint16), b, k)
    assert (n == (2 * k + 1) ** 2).all() and np.array_equal(m, (1000 + 37 * x + 1501 * y)[b:-b, b:-b].astype(F32) / F32(65535))
    lone = np.zeros((T, T), np.uint16)
    lone[b + 7, b + 9] = 40000
    out = SM.apply_smooth({key: lone}, 0, whole(T, strength=1.0, falloff="hard"), b, k)[key]
    assert np.array_equal(out, lone)
    holed = holed_tile(T, seed=11)
    out = SM.apply_smooth({key: holed}, 0, whole(T, strength=1.0, falloff="hard"), b, k)[key]
    assert np.array_equal(out == 0, holed == 0) and (out != holed).any()


def test_known_answer_hard_strength_one():
    """a spike of 65535 in a field of 6553 (k = 1, b = 1): the spike's box is 8 * 6553 + 65535 = 117959 over 9 texels"""
    tile = np.full((7, 7), 6553, np.uint16)
    tile[3, 3] = 65535
    key = (0, 0, 0, 0)
    out = SM.apply_smooth({key: tile}, 0, [Stamp((2.0, 2.0), 1.5, 1.0, "hard")], 1, 1)[key]  # centre texel (2, 2) is layer pixel (3, 3)
    want = int(np.floor(F32(0.5) + F32(65535) * (F32(117959) / (F32(65535) * F32(9)))))
    assert out[3, 3] == want == 13107 and out[3, 4] == out[2, 2] == 13107  # d2 = 1 and 2 are < 2.25; every such box holds the spike
    assert out[3, 5] == 6553 and out[1, 1] == 6553  # d2 = 4: outside the stamp
    half = SM.apply_smooth({key: tile}, 0, [Stamp((2.0, 2.0), 1.5, 0.5, "hard")], 1, 1)[key]
    h, m = F32(65535) / F32(65535), F32(117959) / (F32(65535) * F32(9))
    assert half[3, 3] == int(np.floor(F32(0.5) + F32(65535) * (h + (m - h) * F32(0.5))))


@pytest.mark.parametrize("k", [1, 2])
def test_in_place_application_gives_other_bytes(k):
    """the snapshot property is observable: a pass that reads what it has written differs on most texels of random data"""
    T, b = 24, 2
    key = (0, 0, 0, 0)
    tile = holed_tile(T, seed=21, holes=0.02)
    stamps = whole(T, strength=1.0, falloff="hard")
    model = SM.apply_smooth({key: tile}, 0, stamps, b, k)[key]
    in_place = SM.apply_smooth_in_place({key: tile}, 0, stamps, b, k)[key]
    centre = (slice(b, T - b), slice(b, T - b))
    differing = (model[centre] != in_place[centre]).sum() / float((tile[centre] != 0).sum())
    assert differing > 0.5, differing
    assert np.array_equal(model[b, b:b + 1], in_place[b, b:b + 1]), "the first texel of the pass has read nothing written"


def test_one_call_of_two_stamps_is_not_two_calls():
    T, b, k = 24, 2, 2
    key = (0, 0, 0, 0)
    tile = holed_tile(T, seed=5, holes=0.02)
    s1, s2 = Stamp((8.0, 9.0), 6.0, 1.0, "hard"), Stamp((11.0, 10.0), 6.0, 0.5, "hard")
    one = SM.apply_smooth({key: tile}, 0, [s1, s2], b, k)[key]
    two = SM.apply_smooth(SM.apply_smooth({key: tile}, 0, [s1], b, k), 0, [s2], b, k)[key]
    assert (one != two).sum() > 20


# ---------------------------------------------------------------------------------------------- the C ABI, without a device

def test_symbol_is_declared_and_bound():
    assert "bt_atlas_smooth_height" in _ffi.header_symbols() and "bt_atlas_smooth_height" in _ffi.PROTOTYPES
    assert C.sizeof(_ffi.SmoothStampC) == 24 and _ffi.SMOOTH_MAX_KERNEL == 4
    assert _ffi.header_abi_version() == 6 == _ffi.lib().bt_abi_version()


def stamp_c(side=0, falloff=0, center=(1.0, 1.0), radius=1.0, strength=0.5):
    return _ffi.SmoothStampC(side, falloff, (C.c_float * 2)(*center), radius, strength)


def dirty_stats():
    stats = _ffi.EditStatsC()
    C.memset(C.byref(stats), 0xAB, C.sizeof(stats))
    return stats


def zeroed(stats):
    return not any(getattr(stats, name) for name, _ in _ffi.EditStatsC._fields_)


def test_null_atlas_stamps_and_changed_are_refused():
    L = _ffi.lib()
    one = (_ffi.SmoothStampC * 1)(stamp_c())
    stats = dirty_stats()
    assert L.bt_atlas_smooth_height(None, 0, 0, 1, one, 1, None, 0, C.byref(stats)) == BT_ERR_INVALID_ARGUMENT
    assert b"NULL atlas" in L.bt_last_error() and zeroed(stats)
    assert L.bt_atlas_smooth_height(None, 0, 0, 1, None, 0, None, 0, None) == BT_ERR_INVALID_ARGUMENT and b"NULL atlas" in L.bt_last_error()
    stats = dirty_stats()
    assert L.bt_atlas_smooth_height(None, 0, 0, 1, None, 1, None, 0, C.byref(stats)) == BT_ERR_INVALID_ARGUMENT
    assert b"NULL stamps" in L.bt_last_error() and zeroed(stats)
    stats = dirty_stats()
    assert L.bt_atlas_smooth_height(None, 0, 0, 1, one, 1, None, 4, C.byref(stats)) == BT_ERR_INVALID_ARGUMENT
    assert b"changed" in L.bt_last_error() and zeroed(stats)


@pytest.mark.parametrize("why,k,make", [
    (b"at most 256", 1, lambda: [stamp_c()] * 257),
    (b"kernel_radius 0", 0, lambda: [stamp_c()]),
    (b"kernel_radius 5", 5, lambda: [stamp_c()]),
    (b"strength", 1, lambda: [stamp_c(strength=0.0)]),
    (b"strength", 1, lambda: [stamp_c(strength=1.5)]),
    (b"strength", 1, lambda: [stamp_c(strength=float("nan"))]),
    (b"strength", 2, lambda: [stamp_c(strength=-0.5)]),
    (b"falloff", 1, lambda: [stamp_c(falloff=2)]),
    (b"side", 1, lambda: [stamp_c(side=6)]),
    (b"center", 1, lambda: [stamp_c(center=(float("nan"), 0.0))]),
    (b"radius", 1, lambda: [stamp_c(radius=0.0)]),
    (b"radius", 1, lambda: [stamp_c(radius=float("inf"))]),
    (b"stamp 1", 1, lambda: [stamp_c(), stamp_c(strength=2.0)]),
])
def test_arguments_are_checked_before_any_device_work(why, k, make):
    """refused without an atlas: the refusal names the argument's fault, not the NULL atlas, and stats come back zeroed"""
    L = _ffi.lib()
    stamps = make()
    arr = (_ffi.SmoothStampC * len(stamps))(*stamps)
    stats = dirty_stats()
    assert L.bt_atlas_smooth_height(None, 0, 0, k, arr, len(stamps), None, 0, C.byref(stats)) == BT_ERR_INVALID_ARGUMENT
    assert why in L.bt_last_error() and b"NULL atlas" not in L.bt_last_error(), L.bt_last_error()
    assert zeroed(stats)


def test_strength_one_is_accepted():
    """the interval is (0, 1]: strength 1 passes the stamp checks (the refusal that follows is the NULL atlas)"""
    L = _ffi.lib()
    arr = (_ffi.SmoothStampC * 1)(stamp_c(strength=1.0))
    assert L.bt_atlas_smooth_height(None, 0, 0, 4, arr, 1, None, 0, None) == BT_ERR_INVALID_ARGUMENT and b"NULL atlas" in L.bt_last_error()

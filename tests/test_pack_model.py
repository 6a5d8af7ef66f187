"""The packed tile format without a GPU: the numpy model (tests/_pack_model.py) against a scalar restatement and two streams worked by
hand, its round trip and bound on every case of tests/_pack_cases.py, what each case reaches, and the library's two device-free entry
points (bt_packed_tile_bound, bt_packed_tile_check) against the model."""
import numpy as np
import pytest

import _pack_cases as PC
import _pack_model as M
import bevy_terrain_amd as bt
from bevy_terrain_amd import _ffi

R16, RGBA8 = M.FORMAT_R16, M.FORMAT_RGBA8
BT_ERR_INVALID_ARGUMENT, BT_ERR_IO, BT_ERR_UNSUPPORTED = -1, -4, -5
FMT = {R16: bt.AttachmentFormat.R16, RGBA8: bt.AttachmentFormat.Rgba8}
NAMES = PC.names()


def words(*values):
    return b"".join(int(v).to_bytes(8, "little") for v in values)


def test_r16_stream_by_hand():
    """T = 3, one strip, one group per row.  Row differences 1 2 4 / 0 1 0 / -1 -3 -4, residuals 1 1 2 / 0 1 -1 / -1 -2 -1, zigzag
    2 2 4 / 0 2 1 / 1 3 1, widths 3 2 2; the bit planes of row 0 are 000, 011, 100"""
    tile = np.array([[1, 2, 4], [1, 3, 4], [0, 0, 0]], np.uint16)
    want = b"BTP1" + bytes([1, 32, 3, 0]) + (56).to_bytes(4, "little") + bytes(4) + bytes([3, 2, 2]) + bytes(5) + words(0, 3, 4, 4, 2, 7, 2)
    assert M.encode(tile) == want and M.encode_scalar(tile) == want
    assert np.array_equal(M.decode(want), tile) and M.check(want) == (R16, 3)
    assert bt.packed_tile_check(want) == (bt.AttachmentFormat.R16, 3)


def test_rgba8_stream_by_hand():
    """T = 2: planes 10 12 / 10 13, 0 0 / 1 1, 255 255 / 0 0 and 7 7 / 7 7.  Zigzag per plane: 20 4 / 0 2, 0 0 / 2 0, 1 0 / 2 0 (255 is -1,
    0 - 255 is 1) and 14 0 / 0 0; the widths in (y, plane) order are 5 0 1 4 and 2 2 2 0"""
    tile = np.array([[[10, 0, 255, 7], [12, 0, 255, 7]], [[10, 1, 0, 7], [13, 1, 0, 7]]], np.uint8)
    payload = words(0, 0, 3, 0, 1) + words(1) + words(0, 1, 1, 1) + words(0, 2) + words(0, 1) + words(0, 1)
    want = b"BTP1" + bytes([0, 32, 2, 0]) + (128).to_bytes(4, "little") + bytes(4) + bytes([5, 0, 1, 4, 2, 2, 2, 0]) + payload
    assert M.encode(tile) == want and M.encode_scalar(tile) == want
    assert np.array_equal(M.decode(want), tile) and M.check(want) == (RGBA8, 2)
    assert bt.packed_tile_check(want) == (bt.AttachmentFormat.Rgba8, 2)


@pytest.mark.parametrize("fmt,T", [(R16, 1), (RGBA8, 1), (R16, 5), (RGBA8, 7), (R16, 33), (RGBA8, 34), (R16, 66)])
def test_model_against_the_scalar_restatement(fmt, T):
    for kind in ("noise", "smooth", "spikes", "checker"):
        tile = PC.tile(kind, fmt, T)
        assert M.encode(tile) == M.encode_scalar(tile), (kind, fmt, T)


@pytest.mark.parametrize("kind,fmt,T", NAMES)
def test_round_trip_bound_and_check(kind, fmt, T):
    tile, data = PC.tile(kind, fmt, T), PC.stream(kind, fmt, T)
    assert M.check(data) == (fmt, T)
    back = M.decode(data)
    assert back.dtype == tile.dtype and np.array_equal(back, tile)
    assert len(data) <= M.bound(fmt, T) and len(data) % 8 == 0
    assert bt.packed_tile_bound(FMT[fmt], T) == M.bound(fmt, T)
    assert bt.packed_tile_check(data) == (FMT[fmt], T)
    if T <= 136:  # an accepted stream that is not the canonical one decodes to the same tile
        loose = PC.loosened(kind, fmt, T)
        assert (loose != data or kind != "smooth") and np.array_equal(M.decode(loose), tile)
        assert bt.packed_tile_check(loose) == (FMT[fmt], T)


@pytest.mark.parametrize("fmt,T", PC.SHAPES + [PC.BIG] + PC.EVERY_WIDTH + [(R16, 1), (RGBA8, 1), (R16, 65535), (RGBA8, 65535)])
def test_bound(fmt, T):
    planes, b, gpr, strips, W, head = M.shape(fmt, T)
    raw = T * T * planes * b // 8
    assert M.bound(fmt, T) == 16 + M.pad8(W) + 8 * b * W and M.bound(fmt, T) >= raw + W + 16  # (a group is 64 lanes wide, the dead ones included)
    if T % 64 == 0:  # the raw size plus one byte per 64 values plus at most 23
        assert raw + W + 16 <= M.bound(fmt, T) <= raw + W + 23
    assert bt.packed_tile_bound(FMT[fmt], T) == M.bound(fmt, T)
    if T <= 136:  # reached exactly by the tile whose every residual is the most negative one, and by nothing more
        assert len(PC.stream("most_negative", fmt, T)) == M.bound(fmt, T)


def test_bound_refusals():
    out = _ffi.C.c_uint64(7)
    L = _ffi.lib()
    assert L.bt_packed_tile_bound(1, 512, None) == BT_ERR_INVALID_ARGUMENT
    for fmt, T, status in ((1, 0, BT_ERR_INVALID_ARGUMENT), (1, 65536, BT_ERR_INVALID_ARGUMENT), (2, 64, BT_ERR_INVALID_ARGUMENT), (3, 64, BT_ERR_UNSUPPORTED),
                           (5, 64, BT_ERR_UNSUPPORTED)):
        assert L.bt_packed_tile_bound(fmt, T, _ffi.C.byref(out)) == status and out.value == 0, (fmt, T)


def test_what_the_cases_reach():
    """widths, partial groups and strips: the reach the GPU tests rely on"""
    for fmt, T in PC.SHAPES + [PC.BIG]:
        planes, b, gpr, strips, W, head = M.shape(fmt, T)
        assert PC.widths_of(PC.stream("zeros", fmt, T)).max() == 0 and len(PC.stream("zeros", fmt, T)) == head if (fmt, T) != PC.BIG else True
    shapes = {T: M.shape(R16, T) for T in (24, 64, 72, 136, 512)}
    assert [(shapes[T][2], shapes[T][3], T % 64, T % 32) for T in (24, 64, 72, 136, 512)] == [(1, 1, 24, 24), (1, 2, 0, 0), (2, 3, 8, 8), (3, 5, 8, 8), (8, 16, 0, 0)]
    for fmt, T in PC.SHAPES:
        planes, b, gpr, strips, W, head = M.shape(fmt, T)
        w = PC.widths_of(PC.stream("constant", fmt, T))
        assert (w[::32, :, 0] > 0).all() and w[1::32].max() == 0  # only the first texel of a strip differs from what it predicts
        w = PC.widths_of(PC.stream("inclined", fmt, T))
        rows = np.arange(T) % 32 != 0
        assert (w[rows][:, :, 1:] == 0).all() and (w[rows][:, :, 0] <= 7).all() and w[0].max() > 0
        assert (PC.widths_of(PC.stream("most_negative", fmt, T)) == b).all()
        w = PC.widths_of(PC.stream("noise", fmt, T))
        assert (w == b).mean() > 0.9, "uniform noise takes the raw escape"
        w = PC.widths_of(PC.stream("checker", fmt, T))
        assert 1 <= w.min() and w.max() <= 3  # differences of +-(2^b - 1) wrap around to -+1: every residual is small
        w = PC.widths_of(PC.stream("spikes", fmt, T))
        assert w[1, 0, gpr - 1] == b and w[T - 1, planes - 1, (T // 2) // 64] == b and (w == 0).sum() >= w.size - 6
        w = PC.widths_of(PC.stream("smooth", fmt, T))
        assert 0 < w[rows].max() < b and len(np.unique(w)) >= 3
    for fmt, T in PC.EVERY_WIDTH:
        planes, b, gpr, strips, W, head = M.shape(fmt, T)
        w = PC.widths_of(PC.stream("every_width", fmt, T))
        assert gpr == b + 1 and list(w[3, 0]) == list(range(b + 1))
        if planes > 1:
            assert list(w[3, 1]) == list(range(b, -1, -1))
    for T in (24, 72, 136):
        w = PC.widths_of(PC.stream("four_widths", RGBA8, T))
        assert list(w[0, :, 0]) == [1, 3, 5, 8] and w[1].max() == 0 and list(w[2, :, 0]) == [1, 3, 5, 8]


def test_strip_offsets_are_prefix_sums():
    for kind, fmt, T in (("smooth", R16, 136), ("noise", RGBA8, 72), ("zeros", R16, 24)):
        data = PC.stream(kind, fmt, T)
        planes, b, gpr, strips, W, head = M.shape(fmt, T)
        w = PC.widths_of(data).astype(np.int64)
        assert M.strip_offsets(data) == [head + 8 * int(w[:32 * s].sum()) for s in range(strips)]


@pytest.mark.parametrize("name,data,rule", PC.invalid_streams(), ids=[n for n, _, _ in PC.invalid_streams()])
def test_check_rejects(name, data, rule):
    with pytest.raises(M.PackError) as e:
        M.check(data)
    assert e.value.rule == rule
    fmt, T = _ffi.C.c_uint32(77), _ffi.C.c_uint32(77)
    status = _ffi.lib().bt_packed_tile_check(_ffi.C.c_char_p(data), len(data), _ffi.C.byref(fmt), _ffi.C.byref(T))
    assert status == (BT_ERR_UNSUPPORTED if name == "strip rows 16" else BT_ERR_IO), name
    text = _ffi.lib().bt_last_error().decode()
    said = {"size": "at least 16", "magic": "magic", "format": "format", "strip rows": "strips of", "texture_size": "texture_size 0", "bytes 12-15": "bytes 12-15",
            "width": "width", "padding": "padding", "payload field": "payload field", "total size": "bytes"}[rule]
    assert said in text, (name, text)
    with pytest.raises(_ffi.BtError):
        bt.packed_tile_check(data)


def test_check_agrees_with_the_model_on_mutated_streams():
    """one byte changed, bytes cut off or appended, anywhere in a valid stream: the validator accepts exactly what the model accepts,
    and names the same format and size when it does"""
    rng = np.random.default_rng(11)
    L = _ffi.lib()
    accepted = 0
    for kind, fmt, T in (("smooth", R16, 27), ("spikes", RGBA8, 24), ("zeros", R16, 72), ("noise", RGBA8, 5)):
        good = PC.stream(kind, fmt, T)
        for trial in range(150):
            bad = bytearray(good)
            how = trial % 3
            if how == 0:
                at = int(rng.integers(0, min(len(bad), 16 + M.shape(fmt, T)[5]))) if trial % 2 else int(rng.integers(0, len(bad)))
                bad[at] = int(rng.integers(0, 256)) if trial % 4 else min(bad[at] + 1, 255)
            elif how == 1:
                bad = bad[:int(rng.integers(0, len(bad) + 1))]
            else:
                bad += bytes(int(rng.integers(1, 17)))
            bad = bytes(bad)
            try:
                want = M.check(bad)
            except M.PackError:
                want = None
            f, t = _ffi.C.c_uint32(), _ffi.C.c_uint32()
            status = L.bt_packed_tile_check(_ffi.C.c_char_p(bad) if bad else _ffi.C.c_char_p(b"\0"), len(bad), _ffi.C.byref(f), _ffi.C.byref(t))
            assert (status == 0) == (want is not None), (kind, trial, status, want)
            if want is not None:
                assert (f.value, t.value) == want
                accepted += 1
    assert accepted > 20  # (a payload byte may change freely: the stream stays valid and decodes to another tile)


def test_check_unsupported_headers_and_null():
    good = bytearray(PC.stream("smooth", R16, 27))
    L = _ffi.lib()
    for fmt in (3, 5):  # formats the configuration knows and nothing processes
        bad = bytes(good[:4]) + bytes([fmt]) + bytes(good[5:])
        assert L.bt_packed_tile_check(_ffi.C.c_char_p(bad), len(bad), None, None) == BT_ERR_UNSUPPORTED
    assert L.bt_packed_tile_check(None, 16, None, None) == BT_ERR_INVALID_ARGUMENT
    assert L.bt_packed_tile_check(_ffi.C.c_char_p(bytes(good)), len(good), None, None) == 0

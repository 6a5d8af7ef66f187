"""The packed tile format (PACKED TILES in include/bevy_terrain_amd.h) in numpy: an encoder, a decoder and a checker written from the
definition's text, and a scalar restatement of the encoder for tiny tiles.  The library's second implementation: the device's bytes
must equal encode(), whatever decode() accepts the device must decode to the same tile, and check() names the rule the validator
names.  A tile is (T, T) uint16 for R16 and (T, T, 4) uint8 for Rgba8."""
import numpy as np

FORMAT_RGBA8, FORMAT_R16 = 0, 1
STRIP = 32
MAGIC = b"BTP1"


class PackError(ValueError):
    def __init__(self, rule, message=""):
        super().__init__(f"{rule}: {message}" if message else rule)
        self.rule = rule


def pad8(n):
    return (n + 7) & ~7


def shape(fmt, T):
    """planes, b, gpr, strips, W, head"""
    planes, b = (1, 16) if fmt == FORMAT_R16 else (4, 8)
    gpr = (T + 63) // 64
    W = planes * T * gpr
    return planes, b, gpr, (T + STRIP - 1) // STRIP, W, 16 + pad8(W)


def bound(fmt, T):
    planes, b, gpr, strips, W, head = shape(fmt, T)
    return head + 8 * b * W


def format_of(tile):
    return FORMAT_R16 if tile.ndim == 2 else FORMAT_RGBA8


def to_planes(tile):
    """(planes, T, T) int64"""
    return tile.astype(np.int64)[None] if tile.ndim == 2 else np.moveaxis(tile.astype(np.int64), 2, 0)


def from_planes(planes, fmt):
    return planes[0].astype(np.uint16) if fmt == FORMAT_R16 else np.ascontiguousarray(np.moveaxis(planes, 0, 2)).astype(np.uint8)


def residuals(planes, b):
    """r = v(x, y) - v(x-1, y) - v(x, y-1) + v(x-1, y-1) mod 2^b, terms left of the tile or above the strip's first row being 0"""
    up = np.zeros_like(planes)
    up[:, 1:] = planes[:, :-1]
    up[:, ::STRIP] = 0
    d = planes - up
    left = np.zeros_like(d)
    left[:, :, 1:] = d[:, :, :-1]
    return (d - left) % (1 << b)


def from_residuals(r, b):
    """the inverse: a prefix sum along the rows, then down the columns of each strip"""
    d = np.cumsum(r, axis=2) % (1 << b)
    out = np.empty_like(d)
    for y0 in range(0, d.shape[1], STRIP):
        out[:, y0:y0 + STRIP] = np.cumsum(d[:, y0:y0 + STRIP], axis=1) % (1 << b)
    return out


def zigzag(r, b):
    s = np.where(r >= (1 << (b - 1)), r - (1 << b), r)
    return np.where(s >= 0, 2 * s, -2 * s - 1)


def unzigzag(z, b):
    s = np.where(z & 1, -((z + 1) >> 1), z >> 1)
    return s % (1 << b)


def bit_length(a):
    out = np.zeros(a.shape, np.int64)
    a = a.copy()
    while a.any():
        out += a != 0
        a >>= 1
    return out


def group_z(tile):
    """Z[y, c, g, lane]: the zigzagged residuals in stream order, the dead lanes 0"""
    fmt, T = format_of(tile), tile.shape[0]
    planes, b, gpr, *_ = shape(fmt, T)
    z = zigzag(residuals(to_planes(tile), b), b)  # (planes, T, T)
    padded = np.zeros((planes, T, gpr * 64), np.int64)
    padded[:, :, :T] = z
    return np.ascontiguousarray(np.moveaxis(padded.reshape(planes, T, gpr, 64), 0, 1))


def minimal_widths(tile):
    """the width byte of every group, in stream order"""
    return bit_length(group_z(tile).max(axis=3)).reshape(-1)


def header(fmt, T, payload, strip=STRIP):
    return MAGIC + bytes([fmt, strip]) + int(T).to_bytes(2, "little") + int(payload).to_bytes(4, "little") + bytes(4)


def encode(tile, widths=None, dead_bits=None):
    """The stream of a tile.  widths: the width bytes to use (each at least the minimal one) in place of the minimal ones; dead_bits: a
    numpy Generator whose bits fill the dead lanes of the last group of every row (an accepted stream, not the canonical one)."""
    fmt, T = format_of(tile), tile.shape[0]
    planes, b, gpr, strips, W, head = shape(fmt, T)
    Z = group_z(tile).reshape(W, 64).astype(np.uint64)
    least = bit_length(Z.max(axis=1).astype(np.int64))
    widths = least if widths is None else np.asarray(widths, np.int64)
    assert widths.shape == (W,) and (widths >= least).all() and (widths <= b).all()
    lanes = np.arange(64, dtype=np.uint64)
    words = np.zeros((W, b), np.uint64)
    for k in range(b):
        words[:, k] = np.bitwise_or.reduce(((Z >> np.uint64(k)) & np.uint64(1)) << lanes, axis=1)
    if dead_bits is not None and T % 64:
        dead = np.uint64(((1 << 64) - 1) ^ ((1 << (T % 64)) - 1))
        last = np.arange(W) % gpr == gpr - 1
        garbage = dead_bits.integers(0, 1 << 64, size=(W, b), dtype=np.uint64) & dead
        words[last] |= garbage[last]
    keep = np.arange(b)[None, :] < widths[:, None]
    payload = words[keep].astype("<u8").tobytes()
    return header(fmt, T, len(payload)) + widths.astype(np.uint8).tobytes() + bytes(head - 16 - W) + payload


def check(data):
    """(fmt, T) of a valid stream; PackError naming the first violated rule, in the order of the definition's list"""
    data = bytes(data)
    if len(data) < 16:
        raise PackError("size")
    if data[:4] != MAGIC:
        raise PackError("magic")
    fmt, strip, T = data[4], data[5], int.from_bytes(data[6:8], "little")
    payload = int.from_bytes(data[8:12], "little")
    if fmt not in (FORMAT_R16, FORMAT_RGBA8):
        raise PackError("format")
    if strip != STRIP:
        raise PackError("strip rows")
    if T < 1:
        raise PackError("texture_size")
    if any(data[12:16]):
        raise PackError("bytes 12-15")
    planes, b, gpr, strips, W, head = shape(fmt, T)
    if len(data) < head:
        raise PackError("total size", "the widths are cut short")
    widths = np.frombuffer(data, np.uint8, W, 16)
    if (widths > b).any():
        raise PackError("width")
    if any(data[16 + W:head]):
        raise PackError("padding")
    if payload != 8 * int(widths.sum(dtype=np.int64)):
        raise PackError("payload field")
    if len(data) != head + payload:
        raise PackError("total size")
    return fmt, T


def decode(data):
    """the tile of an accepted stream (any w <= b; the dead lanes' bits are ignored)"""
    fmt, T = check(data)
    planes, b, gpr, strips, W, head = shape(fmt, T)
    widths = np.frombuffer(data, np.uint8, W, 16).astype(np.int64)
    payload = np.frombuffer(data, "<u8", int(widths.sum()), head).astype(np.uint64)
    words = np.zeros((W, b), np.uint64)
    words[np.arange(b)[None, :] < widths[:, None]] = payload
    lanes = np.arange(64, dtype=np.uint64)
    Z = np.zeros((W, 64), np.int64)
    for k in range(b):
        Z |= (((words[:, k, None] >> lanes) & np.uint64(1)).astype(np.int64)) << k
    z = np.moveaxis(Z.reshape(T, planes, gpr * 64), 1, 0)[:, :, :T]
    return from_planes(from_residuals(unzigzag(z, b), b), fmt)


def strip_offsets(data):
    """where every strip's payload begins, from the stream's first byte"""
    fmt, T = check(data)
    planes, b, gpr, strips, W, head = shape(fmt, T)
    widths = np.frombuffer(data, np.uint8, W, 16).astype(np.int64)
    before = np.concatenate([[0], np.cumsum(widths)])
    return [head + 8 * int(before[min(s * STRIP * planes * gpr, W)]) for s in range(strips)]


def encode_scalar(tile):
    """encode() restated texel by texel, for tiny tiles"""
    fmt, T = format_of(tile), tile.shape[0]
    planes, b, gpr, strips, W, head = shape(fmt, T)
    mod = 1 << b

    def v(c, x, y, y0):
        if x < 0 or y < y0:
            return 0
        return int(tile[y, x]) if fmt == FORMAT_R16 else int(tile[y, x, c])

    widths, payload = [], b""
    for y in range(T):
        y0 = y - y % STRIP
        for c in range(planes):
            for g in range(gpr):
                zs = []
                for lane in range(64):
                    x = g * 64 + lane
                    if x >= T:
                        zs.append(0)
                        continue
                    r = (v(c, x, y, y0) - v(c, x - 1, y, y0) - v(c, x, y - 1, y0) + v(c, x - 1, y - 1, y0)) % mod
                    s = r - mod if r >= mod // 2 else r
                    zs.append(2 * s if s >= 0 else -2 * s - 1)
                w = max(zs).bit_length()
                widths.append(w)
                for k in range(w):
                    payload += sum(((z >> k) & 1) << lane for lane, z in enumerate(zs)).to_bytes(8, "little")
    return header(fmt, T, len(payload)) + bytes(widths) + bytes(head - 16 - W) + payload

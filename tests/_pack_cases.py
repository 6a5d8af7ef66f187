"""The tiles of the packed tile tests (tests/_pack_model.py is the format).  A case is a function of (format, T) that returns one tile;
several are made from a chosen residual plane pushed through the model's decoder.  names() lists the (kind, format, T) cases; what each
kind reaches (widths, partial groups, strips) is asserted by test_pack_model.py."""
import functools

import numpy as np

import _pack_model as M

R16, RGBA8 = M.FORMAT_R16, M.FORMAT_RGBA8
SHAPES = [(R16, 24), (RGBA8, 24), (R16, 64), (R16, 72), (RGBA8, 72), (R16, 136), (RGBA8, 136)]
BIG = (R16, 512)
# one row that holds a group of every width 0 .. b needs b + 1 groups: T = 64 (b + 1)
EVERY_WIDTH = [(R16, 64 * 17), (RGBA8, 64 * 9)]


def _dims(fmt, T):
    planes, b, *_ = M.shape(fmt, T)
    return planes, b


def _from_z(fmt, T, z):
    """the tile whose zigzagged residuals are z: (planes, T, T)"""
    planes, b = _dims(fmt, T)
    return M.from_planes(M.from_residuals(M.unzigzag(z.astype(np.int64), b), b), fmt)


def zeros(fmt, T):
    planes, b = _dims(fmt, T)
    return _from_z(fmt, T, np.zeros((planes, T, T), np.int64))


def constant(fmt, T):
    tile = zeros(fmt, T)
    tile[...] = 201 if fmt == RGBA8 else 40961
    return tile


def inclined(fmt, T):
    """a plane: residuals are zero beyond the first row and column of each strip"""
    planes, b = _dims(fmt, T)
    y, x = np.mgrid[0:T, 0:T]
    v = np.stack([(7 + (3 + c) * x + (5 + 2 * c) * y) % (1 << b) for c in range(planes)])
    return M.from_planes(v, fmt)


def checker(fmt, T):
    """0 / all ones: every difference wraps around"""
    planes, b = _dims(fmt, T)
    y, x = np.mgrid[0:T, 0:T]
    v = np.stack([((x + y + c) & 1) * ((1 << b) - 1) for c in range(planes)])
    return M.from_planes(v, fmt)


def noise(fmt, T):
    planes, b = _dims(fmt, T)
    rng = np.random.default_rng(1000 * T + fmt)
    return M.from_planes(rng.integers(0, 1 << b, size=(planes, T, T)), fmt)


def most_negative(fmt, T):
    """every residual is -2^(b-1): z all ones"""
    planes, b = _dims(fmt, T)
    return _from_z(fmt, T, np.full((planes, T, T), (1 << b) - 1, np.int64))


def spikes(fmt, T):
    """one spike in the last real lane of the last group (row 1), one in the last row of the last strip"""
    planes, b = _dims(fmt, T)
    z = np.zeros((planes, T, T), np.int64)
    z[0, 1 % T, T - 1] = (1 << b) - 1
    z[planes - 1, T - 1, T // 2] = 1 << (b - 1)
    return _from_z(fmt, T, z)


def every_width(fmt, T):
    """row 3: group g of plane 0 has one value of bit length g, for g = 0 .. b (T = 64 (b + 1)); the other planes run the other way"""
    planes, b = _dims(fmt, T)
    z = np.zeros((planes, T, T), np.int64)
    for c in range(planes):
        for g in range(min(b + 1, (T + 63) // 64)):
            w = g if c % 2 == 0 else b - g
            if w and g * 64 + 5 < T:
                z[c, 3 % T, g * 64 + 5] = (1 << w) - 1 if g % 2 else 1 << (w - 1)
    return _from_z(fmt, T, z)


def four_widths(fmt, T):
    """Rgba8: the four planes of one group have the widths 1, 3, 5 and 8, on every second row"""
    assert fmt == RGBA8
    z = np.zeros((4, T, T), np.int64)
    for c, w in enumerate((1, 3, 5, 8)):
        z[c, ::2, (7 * c + 2) % T] = 1 << (w - 1)
    return _from_z(fmt, T, z)


def smooth(fmt, T):
    """a gentle surface with a little noise: mixed small widths, the usual case"""
    planes, b = _dims(fmt, T)
    rng = np.random.default_rng(77 * T + fmt)
    y, x = np.mgrid[0:T, 0:T]
    v = np.stack([((1 << (b - 1)) + (1 << (b - 3)) * (np.sin(x / (9.0 + c)) + np.cos(y / (13.0 - c)))).astype(np.int64) + rng.integers(0, 3, size=(T, T))
                  for c in range(planes)])
    return M.from_planes(v % (1 << b), fmt)


KINDS = {"zeros": zeros, "constant": constant, "inclined": inclined, "checker": checker, "noise": noise, "most_negative": most_negative,
         "spikes": spikes, "every_width": every_width, "smooth": smooth}


def names():
    out = [(kind, fmt, T) for fmt, T in SHAPES for kind in KINDS]
    out += [("four_widths", RGBA8, T) for T in (24, 72, 136)]
    out += [("every_width", fmt, T) for fmt, T in EVERY_WIDTH]
    out += [(kind, *BIG) for kind in ("smooth", "noise", "spikes")]
    return out


@functools.lru_cache(maxsize=None)
def tile(kind, fmt, T):
    t = four_widths(fmt, T) if kind == "four_widths" else KINDS[kind](fmt, T)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def stream(kind, fmt, T):
    """the model's encoding, computed once"""
    return M.encode(tile(kind, fmt, T))


def widths_of(data):
    fmt, T = M.check(data)
    planes, b, gpr, strips, W, head = M.shape(fmt, T)
    return np.frombuffer(data, np.uint8, W, 16).reshape(T, planes, gpr)


def loosened(kind, fmt, T, seed=5):
    """an accepted stream of the same tile that is not the canonical one: widths raised at random, garbage in the dead lanes' bits"""
    t = tile(kind, fmt, T)
    planes, b = _dims(fmt, T)
    rng = np.random.default_rng(seed)
    least = M.minimal_widths(t)
    widths = np.minimum(b, least + rng.integers(0, 4, size=least.shape) * (rng.random(least.shape) < 0.5))
    return M.encode(t, widths=widths, dead_bits=rng)


def invalid_streams():
    """(name, stream, rule): one violation each, made from a valid R16 stream of T = 27 (27 width bytes, 5 of padding)"""
    good = bytearray(stream("smooth", R16, 27))
    planes, b, gpr, strips, W, head = M.shape(R16, 27)
    out = [("truncated by one byte", bytes(good[:-1]), "total size"), ("one byte too long", bytes(good) + b"\0", "total size")]

    def patched(at, value):
        bad = bytearray(good)
        bad[at] = value
        return bytes(bad)

    out.append(("bad magic", patched(3, ord("2")), "magic"))
    out.append(("strip rows 16", patched(5, 16), "strip rows"))
    widths = np.frombuffer(bytes(good), np.uint8, W, 16)
    slack = int(np.argmax(widths < b))
    assert widths[slack] < b
    out.append(("a width of b + 1", patched(16 + slack, b + 1), "width"))
    assert head - 16 - W > 0
    out.append(("a non-zero pad byte", patched(head - 1, 1), "padding"))
    out.append(("a wrong payload field", patched(8, (good[8] + 8) & 0xFF), "payload field"))
    zero_T = bytearray(good)
    zero_T[6:8] = b"\0\0"
    out.append(("T = 0", bytes(zero_T), "texture_size"))
    out.append(("bytes 12-15", patched(13, 1), "bytes 12-15"))
    out.append(("an unknown format", patched(4, 9), "format"))
    out.append(("shorter than a header", bytes(good[:15]), "size"))
    return out

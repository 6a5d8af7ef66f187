"""examples/rivers.py on a tiny atlas: it finds lakes and rivers, follows one river to an outlet, prints the counts, and --ppm draws them"""
import re

import numpy as np
import pytest

from test_gpu_render_examples import run

pytestmark = pytest.mark.gpu


def test_the_example_finds_lakes_and_rivers_and_draws_them(tmp_path):
    picture = str(tmp_path / "rivers.ppm")
    out = run("rivers.py", "--texture-size", "32", "--lods", "3", "--threshold", "60", "--ppm", picture)
    size = 28 * 4
    head = re.search(r"drainage of a (\d+) x \1 mosaic: (\d+) outlets, (\d+) void cells, (\d+) launches \((\d+) fill, (\d+) flat and (\d+) accumulation sweeps\)", out)
    assert head, out
    n, outlets, voids, launches, fill, flat, accumulate = (int(v) for v in head.groups())
    assert n == size and outlets >= 4 * (size - 1) and voids == 0 and launches == 5 + fill + flat + accumulate and min(fill, flat, accumulate) >= 1, out
    counts = re.search(r"lake texels: (\d+) \(the deepest (\d+) raw units, flat distances up to (\d+)\); river texels at 60 cells or more: (\d+); "
                       r"the largest accumulation is (\d+) of (\d+) cells", out)
    assert counts, out
    lakes, deepest, _, rivers, largest, total = (int(v) for v in counts.groups())
    assert 0 < lakes < size * size and deepest > 0 and 0 < rivers < size * size and 60 <= largest <= total == size * size, out
    river = re.search(r"the river from the summit: (\d+) cells, ok, it leaves at \((\d+), (\d+)\) with (\d+) cells drained", out)
    assert river and int(river.group(1)) >= 1 and int(river.group(4)) >= int(river.group(1)), out  # every cell on the way drains through the end
    data = open(picture, "rb").read()
    header = b"P6\n%d %d\n255\n" % (size, size)
    assert data.startswith(header) and len(data) == len(header) + size * size * 3
    rgb = np.frombuffer(data[len(header):], np.uint8).reshape(size, size, 3)
    for colour, count in (((40, 90, 200), lakes), ((90, 170, 255), rivers)):
        drawn = int((rgb == np.array(colour, np.uint8)).all(axis=2).sum())
        assert 0 < drawn <= count, (colour, drawn, count)  # the traced river is drawn over some of them
    assert int((rgb == np.array((255, 60, 40), np.uint8)).all(axis=2).sum()) == int(river.group(1))

"""examples/sun_hours.py on a tiny atlas: the mask and the count it saves are the model's for its suns, the baked byte is the model's, no tree
stands on a cell that no sun of the day reaches (the byte is 0 there, so the probability is 0), and --ppm draws the trees"""
import re

import numpy as np
import pytest

import _skyline_model as M
from test_gpu_render_examples import run

pytestmark = pytest.mark.gpu


def test_no_tree_stands_where_the_sun_never_shines(tmp_path):
    picture, saved = str(tmp_path / "sun_hours.ppm"), str(tmp_path / "sun_hours.npz")
    out = run("sun_hours.py", "--texture-size", "32", "--lods", "3", "--suns", "12", "--max-elevation", "6", "--ppm", picture, "--save", saved)
    size = 28 * 4
    made = np.load(saved)
    heights, directions, trees, byte, count = made["heights"], made["directions"], made["trees"], made["byte"], made["count"]
    assert heights.shape == (size, size) and directions.shape == (12, 4) and (directions[:, 3] == 4096).all() and (directions[:, 2] > 0).all()
    assert directions[0, 0] > 0 and directions[-1, 0] < 0 and (directions[:, 1] > 0).all()  # from +x over +y to -x
    _, _, mask, want, stats = M.skyline(heights, directions)
    assert np.array_equal(made["mask"], mask) and np.array_equal(count, want)
    dark = count == 0
    assert np.array_equal(byte, M.bake_plane(want, 12)) and not byte[dark].any() and (byte == 255).any()
    assert 0 < dark.sum() < size * size // 2, int(dark.sum())
    assert len(trees) > 100 and not dark[trees[:, 1], trees[:, 0]].any() and byte[trees[:, 1], trees[:, 0]].min() > 0
    assert (byte[trees[:, 1], trees[:, 0]] < 255).any()  # some stand in half shade
    head = re.search(r"skyline of a (\d+) x \1 mosaic: (\d+) suns over (\d+) lines, the farthest horizon (\d+) steps away, (\d+) launches", out)
    assert head and [int(v) for v in head.groups()] == [size, 12, stats["lines"], stats["max_steps"], M.launches(size, size, 12, bake=True)], out
    cells = re.search(r"cells: (\d+), without any sun: (\d+), with every sun: (\d+)", out)
    assert cells and [int(v) for v in cells.groups()] == [size * size, int(dark.sum()), int((want == 12).sum())], out
    counts = re.search(r"trees: (\d+), on a cell without sun: (\d+), on a cell with every sun: (\d+)", out)
    assert counts and [int(v) for v in counts.groups()] == [len(trees), 0, int((want[trees[:, 1], trees[:, 0]] == 12).sum())], out
    data = open(picture, "rb").read()
    header = b"P6\n%d %d\n255\n" % (size, size)
    assert data.startswith(header) and len(data) == len(header) + size * size * 3
    rgb = np.frombuffer(data[len(header):], np.uint8).reshape(size, size, 3)
    assert int((rgb == np.array((10, 60, 20), np.uint8)).all(axis=2).sum()) == len(np.unique(trees, axis=0))

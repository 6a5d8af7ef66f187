"""examples/setback.py on a tiny atlas: the distances it saves are the model's on its rivers, the baked byte is the model's, no tree stands
on a river cell (the byte is 0 there, so the probability is 0), and --ppm draws rivers and trees"""
import re

import numpy as np
import pytest

import _distance_model as M
from test_gpu_render_examples import run

pytestmark = pytest.mark.gpu


def test_no_tree_stands_on_a_river(tmp_path):
    picture, saved = str(tmp_path / "setback.ppm"), str(tmp_path / "setback.npz")
    out = run("setback.py", "--texture-size", "32", "--lods", "3", "--threshold", "40", "--reach", "6", "--ppm", picture, "--save", saved)
    size = 28 * 4
    made = np.load(saved)
    rivers, trees, byte = made["rivers"], made["trees"], made["byte"]
    assert rivers.shape == (size, size) and 0 < rivers.sum() < size * size // 4
    dist2, nearest, stats = M.field(rivers)
    assert np.array_equal(made["dist2"], dist2) and np.array_equal(made["nearest"], nearest)
    assert np.array_equal(byte, M.bake_plane(dist2, 6)) and not byte[rivers].any() and (byte == 255).any()
    assert len(trees) > 100 and not rivers[trees[:, 1], trees[:, 0]].any()
    assert byte[trees[:, 1], trees[:, 0]].min() > 0 and (byte[trees[:, 1], trees[:, 0]] < 255).any()  # some stand on the graded bank
    head = re.search(r"distance field of a (\d+) x \1 mosaic: (\d+) river cells at 40 cells or more, the farthest cell is (\d+) away squared, (\d+) launches", out)
    assert head and [int(v) for v in head.groups()] == [size, stats["seeds"], stats["max_dist2"], 7], out
    counts = re.search(r"trees: (\d+), on a river cell: (\d+), within 6 cells of a river: (\d+)", out)
    assert counts and [int(v) for v in counts.groups()] == [len(trees), 0, int((byte[trees[:, 1], trees[:, 0]] < 255).sum())], out
    data = open(picture, "rb").read()
    header = b"P6\n%d %d\n255\n" % (size, size)
    assert data.startswith(header) and len(data) == len(header) + size * size * 3
    rgb = np.frombuffer(data[len(header):], np.uint8).reshape(size, size, 3)
    assert (rgb[rivers] == np.array((90, 170, 255), np.uint8)).all() and int((rgb == np.array((10, 60, 20), np.uint8)).all(axis=2).sum()) == len(np.unique(trees, axis=0))

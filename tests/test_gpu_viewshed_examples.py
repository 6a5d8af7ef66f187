"""examples/viewshed.py on a tiny atlas: it prints what two watchtowers see, the counts equal the model's on the same terrain, and --ppm
draws the seen cells"""
import os
import re
import sys

import numpy as np
import pytest

import _viewshed_model as M
from test_gpu_render_examples import ROOT, run

pytestmark = pytest.mark.gpu


def test_the_example_counts_what_the_model_counts_and_draws_it(tmp_path):
    picture, saved = str(tmp_path / "viewshed.ppm"), str(tmp_path / "heights.npy")
    out = run("viewshed.py", "--texture-size", "32", "--lods", "3", "--eye-height", "300", "--target-height", "20", "--ppm", picture, "--heights", saved)
    size = 28 * 4
    heights = np.load(saved)
    assert heights.shape == (size, size) and heights.dtype == np.uint16
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import viewshed as example  # its choice of towers, from the heights alone
    finally:
        sys.path.pop(0)
    observers = example.towers(heights, 300)
    assert observers[1][3] == size // 3 and observers[0][3] == 0
    clearance, count, mask, stats = M.viewshed(heights, observers, 20)
    head = re.search(r"viewshed of a (\d+) x \1 mosaic from 2 towers at \((\d+), (\d+)\) and \((\d+), (\d+)\): (\d+) line samples in (\d+) launches", out)
    assert head, out
    n, x0, y0, x1, y1, samples, launches = (int(v) for v in head.groups())
    assert n == size and [(x0, y0), (x1, y1)] == [o[:2] for o in observers] and samples == stats["samples"] and launches == 5, out
    counts = re.search(r"covered cells: (\d+); cells on which a target of 20 is seen: (\d+) \(by the first tower (\d+), by the second (\d+), by both (\d+)\); "
                       r"the tallest mast needed: (\d+)", out)
    assert counts, out
    want = (stats["covered"], stats["visible"], int((mask & np.uint64(1) != 0).sum()), int((mask & np.uint64(2) != 0).sum()), int((count == 2).sum()), stats["max_clearance"])
    assert tuple(int(v) for v in counts.groups()) == want, (out, want)
    assert 0 < want[4] <= min(want[2], want[3]) and want[1] < want[0] == size * size, want  # both towers see some cells, and not every cell is seen
    for x, y, c, k in re.findall(r"cell \((\d+), (\d+)\): height \d+, seen from (\d+) above the ground, by (\d+) towers", out):
        assert int(clearance[int(y), int(x)]) == int(c) and int(count[int(y), int(x)]) == int(k), (x, y, out)
    assert len(re.findall(r"cell \(\d+, \d+\): height \d+, ", out)) == 3, out
    data = open(picture, "rb").read()
    header = b"P6\n%d %d\n255\n" % (size, size)
    assert data.startswith(header) and len(data) == len(header) + size * size * 3
    rgb = np.frombuffer(data[len(header):], np.uint8).reshape(size, size, 3)
    assert int((rgb == np.array(example.TOWER, np.uint8)).all(axis=2).sum()) >= 2 * 4  # the two towers, each 3 x 3 but for the map's edge

"""examples/lakes.py on a tiny atlas: it labels the lakes, prints the five largest, removes the puddles from the mask layer with the bake
(and asserts itself that no lake of --min-area cells or more lost a cell), and --ppm draws every lake in its own colour"""
import re

import numpy as np
import pytest

from test_gpu_render_examples import run

pytestmark = pytest.mark.gpu


def test_the_example_labels_the_lakes_and_removes_the_puddles(tmp_path):
    picture = str(tmp_path / "lakes.ppm")
    out = run("lakes.py", "--texture-size", "32", "--lods", "3", "--min-area", "6", "--ppm", picture)
    size = 28 * 4
    head = re.search(r"lakes of a (\d+) x \1 mosaic: (\d+) lakes of (\d+) water cells in (\d+) launches; the largest has (\d+) cells and starts at cell (\d+)", out)
    assert head, out
    n, lakes, water, launches, largest, first = (int(v) for v in head.groups())
    assert n == size and 0 < lakes <= water < size * size and launches == 7 and 0 < largest <= water and first < size * size, out
    listed = re.findall(r"  lake (\d+): (\d+) cells, x (\d+)\.\.(\d+), y (\d+)\.\.(\d+), mean height ([\d.]+) raw units \((\d+)\.\.(\d+)\), shore (\d+) edges", out)
    assert len(listed) == min(5, lakes), out
    areas = [int(row[1]) for row in listed]
    assert areas == sorted(areas, reverse=True) and areas[0] == largest
    for _, area, xa, xb, ya, yb, mean, lo, hi, edges in listed:
        assert int(area) <= (int(xb) - int(xa) + 1) * (int(yb) - int(ya) + 1) and int(lo) <= float(mean) <= int(hi) and 4 <= int(edges) <= 4 * int(area), out
    tail = re.search(r"puddles below 6 cells: (\d+) lakes, (\d+) cells removed from the mask layer in (\d+) launches and (\d+) of the edit, (\d+) tiles changed; "
                     r"(\d+) water cells stay", out)
    assert tail, out
    puddles, removed, bake_launches, edit_launches, changed, stay = (int(v) for v in tail.groups())
    assert 0 < puddles < lakes and puddles <= removed <= 5 * puddles and bake_launches == 8 and edit_launches > 0 and changed > 0 and stay == water - removed, out
    data = open(picture, "rb").read()
    header = b"P6\n%d %d\n255\n" % (size, size)
    assert data.startswith(header) and len(data) == len(header) + size * size * 3
    rgb = np.frombuffer(data[len(header):], np.uint8).reshape(size, size, 3)
    assert int((rgb == np.array((255, 0, 255), np.uint8)).all(axis=2).sum()) == removed

"""examples/erosion.py on a tiny atlas: it erodes, changes texels inside its window only, prints the count, and --ppm draws before and after
side by side"""
import re

import numpy as np
import pytest

from test_gpu_render_examples import run

pytestmark = pytest.mark.gpu


def test_the_example_erodes_its_window_and_draws_before_and_after(tmp_path):
    picture = str(tmp_path / "before_after.ppm")
    out = run("erosion.py", "--texture-size", "32", "--lods", "3", "--steps", "40", "--ppm", picture)
    size = 28 * 4
    window = size - size // 4
    head = re.search(r"eroded a window of (\d+) x (\d+) cells at \((\d+), (\d+)\) of a (\d+) x \5 mosaic: (\d+) steps, (\d+) simulation launches, (\d+) launches of the write-back, "
                     r"(\d+) tiles changed", out)
    assert head and [int(v) for v in head.groups()[:7]] == [window, window, (size - window) // 2, (size - window) // 2, size, 40, 42], out
    assert int(head.group(8)) == 4 and int(head.group(9)) == 21, out  # the region launch, two downsample launches, the stitch launch; every tile of the atlas
    texels = re.search(r"texels changed: (\d+) of (\d+) in the window, (\d+) outside it; the largest change is ([0-9.]+) of 400 height units", out)
    assert texels and int(texels.group(2)) == window * window and int(texels.group(3)) == 0, out
    assert window * window // 4 < int(texels.group(1)) < window * window and 0.0 < float(texels.group(4)) < 100.0, out  # the weight plane's rim keeps its texels
    left = re.search(r"water left: (\S+), sediment in suspension: (\S+)", out)
    assert left and float(left.group(1).rstrip(",")) > 0.0 and np.isfinite(float(left.group(2))), out
    data = open(picture, "rb").read()
    width = 2 * size + 2
    header = b"P6\n%d %d\n255\n" % (width, size)
    assert data.startswith(header) and len(data) == len(header) + width * size * 3
    rgb = np.frombuffer(data[len(header):], np.uint8).reshape(size, width, 3)
    assert (rgb[:, size:size + 2] == 255).all() and not np.array_equal(rgb[:, :size], rgb[:, size + 2:])
    edge = (size - window) // 2
    assert np.array_equal(rgb[:edge - 1, :size], rgb[:edge - 1, size + 2:]), "the picture differs outside the window"

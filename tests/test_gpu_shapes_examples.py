"""examples/roads.py on a tiny atlas: the planes it saves are the model's for its shapes, the mask byte is 255 exactly on them, no tree
stands on a road or in the lake, the lake's floor is level, and --ppm draws roads, lake and trees"""
import re

import numpy as np
import pytest

import _shapes_model as M
from test_gpu_render_examples import run

pytestmark = pytest.mark.gpu


def test_no_tree_stands_on_a_road_or_in_the_lake(tmp_path):
    picture, saved = str(tmp_path / "roads.ppm"), str(tmp_path / "roads.npz")
    out = run("roads.py", "--texture-size", "32", "--lods", "3", "--reach", "4", "--ppm", picture, "--save", saved)
    size = 28 * 4
    made = np.load(saved)
    shapes = M.unpack(made["vertices"], made["entries"])
    assert M.validate(made["vertices"], made["entries"], size, size) == (None, M.NO_ENTRY, 4) and "contours" in shapes[-1] and len(shapes[-1]["contours"]) == 2
    count, last, texels, stats = M.raster(np.zeros((size, size, 4), np.uint8), shapes)
    assert np.array_equal(made["count"], count) and np.array_equal(made["last"], last)
    covered, lake, trees = count > 0, made["lake"], made["trees"]
    assert np.array_equal(lake, last == 3) and 0 < lake.sum() < covered.sum() < size * size // 3
    assert np.array_equal(made["mask"][:, :, 0], texels[:, :, 0]) and np.array_equal(made["mask"][:, :, 0] == 255, covered)
    assert not made["mask"][:, :, 1][covered].any() and (made["mask"][:, :, 1] == 255).any()
    assert len(trees) > 100 and not covered[trees[:, 1], trees[:, 0]].any()
    assert len(np.unique(made["heights"][lake])) == 1 and len(np.unique(made["heights"][~lake])) > 100
    head = re.search(r"shapes into a (\d+) x \1 mosaic: (\d+) shapes, (\d+) culled, (\d+) cells covered, (\d+) texels written, (\d+) launches", out)
    assert head and [int(v) for v in head.groups()] == [size, 4, 0, stats["covered"], stats["written"], 2], out
    levelled = re.search(r"lake: (\d+) cells levelled to (\d+)", out)
    assert levelled and [int(v) for v in levelled.groups()] == [int(lake.sum()), int(made["heights"][lake][0])], out
    counts = re.search(r"trees: (\d+), on a road or in the lake: (\d+), within 4 cells of one: (\d+)", out)
    assert counts and [int(v) for v in counts.groups()][:2] == [len(trees), 0], out
    data = open(picture, "rb").read()
    header = b"P6\n%d %d\n255\n" % (size, size)
    assert data.startswith(header) and len(data) == len(header) + size * size * 3
    rgb = np.frombuffer(data[len(header):], np.uint8).reshape(size, size, 3)
    assert (rgb[lake] == np.array((90, 170, 255), np.uint8)).all() and (rgb[covered & ~lake] == np.array((70, 70, 70), np.uint8)).all()
    assert int((rgb == np.array((10, 60, 20), np.uint8)).all(axis=2).sum()) == len(np.unique(trees, axis=0))

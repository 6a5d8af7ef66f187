"""examples/minimal.py --render --shadows under a low sun (--sun): the same picture as without --shadows, but for ground pixels in shadow,
which keep only the ambient light and so are darker; nothing is brighter, and the sky does not change"""
import re

import numpy as np
import pytest

from test_gpu_render_examples import run

pytestmark = pytest.mark.gpu


def read_ppm(path):
    data = open(path, "rb").read()
    header = b"P6\n640 360\n255\n"
    assert data.startswith(header) and len(data) == len(header) + 640 * 360 * 3
    return np.frombuffer(data[len(header):], np.uint8).reshape(360, 640, 3)


def test_the_planar_example_casts_shadows(tmp_path):
    assets, plain, shadowed = str(tmp_path / "assets"), str(tmp_path / "view.ppm"), str(tmp_path / "shadowed.ppm")
    run("preprocess_planar.py", "--assets", assets, "--size", "1024")
    sun = ("--sun", "0.75", "0.3", "0.6")  # 17 degrees over the horizon
    before = run("minimal.py", "--assets", assets, "--frames", "24", "--render", plain, *sun)
    after = run("minimal.py", "--assets", assets, "--frames", "24", "--render", shadowed, "--shadows", *sun)
    assert "sun shadows" not in before and f"rendered 640 x 360 to {shadowed}" in after, after
    occluded, ground = (int(v) for v in re.search(r"sun shadows: (\d+) of (\d+) ground pixels are in shadow", after).groups())
    a, b = read_ppm(plain), read_ppm(shadowed)
    sky = (a == (120, 170, 230)).all(axis=2)
    assert np.array_equal(a[sky], b[sky]) and (~sky).sum() == ground
    assert (b <= a).all()  # a shadow only takes light away
    darker = (b < a).any(axis=2)
    # an occluded pixel is darker unless it faced away from the sun already (or its grey rounds to the same byte): some are, none else is
    assert 0 < darker.sum() <= occluded < ground, (int(darker.sum()), occluded, ground)
    assert darker.sum() >= ground // 100, (int(darker.sum()), ground)

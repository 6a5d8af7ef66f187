"""examples/minimal.py --render: the example writes the last frame's view, ray-cast on the GPU, as a binary PPM that holds sky and ground"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(script, *args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", script)] + list(args), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (script, p.stdout[-1500:], p.stderr[-1500:])
    return p.stdout


def test_the_planar_example_writes_its_view(tmp_path):
    assets, picture = str(tmp_path / "assets"), str(tmp_path / "view.ppm")
    run("preprocess_planar.py", "--assets", assets, "--size", "1024")
    out = run("minimal.py", "--assets", assets, "--frames", "24", "--render", picture)
    assert f"rendered 640 x 360 to {picture}" in out, out
    data = open(picture, "rb").read()
    header = b"P6\n640 360\n255\n"
    assert data.startswith(header) and len(data) == len(header) + 640 * 360 * 3
    pixels = np.frombuffer(data[len(header):], np.uint8).reshape(360, 640, 3)
    sky = (pixels == (120, 170, 230)).all(axis=2)
    assert sky.sum() >= 640 * 360 // 20 and (~sky).sum() >= 640 * 360 // 4, (int(sky.sum()), int((~sky).sum()))
    ground = pixels[~sky]
    assert (ground[:, 0] == ground[:, 1]).all() and (ground[:, 1] == ground[:, 2]).all() and len(set(ground[:, 0].tolist())) >= 16  # lit greys

"""examples/packed_tiles.py on a tiny terrain: both sizes per LOD are those of the files it wrote, every packed file is the model's
encoding of its raw twin, and the run ends with its equality assertion"""
import os
import re

import numpy as np
import pytest

import _pack_model as M
from test_gpu_render_examples import run

pytestmark = pytest.mark.gpu


def test_the_example_prints_both_sizes_and_its_files_are_the_models(tmp_path):
    assets = str(tmp_path / "assets")
    out = run("packed_tiles.py", "--assets", assets, "--size", "256", "--texture-size", "72", "--lods", "2")
    assert re.search(r"loaded the packed files into a fresh atlas: 30 layers and mip levels equal", out), out  # 5 tiles, 2 attachments, 3 levels
    for name, dtype, shape in (("height", np.uint16, (72, 72)), ("albedo", np.uint8, (72, 72, 4))):
        directory = os.path.join(assets, "terrains/packed/data", name)
        files = sorted(os.listdir(directory))
        assert len(files) == 10 and sum(f.endswith(".btp") for f in files) == 5
        raw = packed = 0
        for f in files:
            if f.endswith(".bin"):
                tile = np.fromfile(os.path.join(directory, f), dtype).reshape(shape)
                stream = open(os.path.join(directory, f[:-4] + ".btp"), "rb").read()
                assert stream == M.encode(tile), (name, f)
                raw, packed = raw + tile.nbytes, packed + len(stream)
        block = out[out.index(name + " ("):]
        total = re.search(r"all  : raw\s+(\d+) bytes, packed\s+(\d+) bytes, ratio ([0-9.]+)", block)
        assert total and [int(total.group(1)), int(total.group(2))] == [raw, packed] and abs(float(total.group(3)) - raw / packed) < 1e-3, out
        assert len(re.findall(r"lod \d: raw", block.split("all  :")[0])) == 2

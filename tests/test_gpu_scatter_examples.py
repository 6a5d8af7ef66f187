"""examples/vegetation.py at a small size: what it prints of its instances is what the numpy model (tests/_scatter_model.py) derives from
the state the example itself made (its heights and its splat map, downloaded), and its instances are the model's byte for byte."""
import importlib.util
import os
import re

import numpy as np
import pytest

import _oracle as O
import _scatter_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_vegetation_example_prints_the_models_counts(capsys, tmp_path):
    spec = importlib.util.spec_from_file_location("vegetation", os.path.join(ROOT, "examples", "vegetation.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    ppm = tmp_path / "vegetation.ppm"
    made = example.main(["--texture-size", "16", "--lods", "3", "--seed", "11", "--ppm", str(ppm)])
    printed = capsys.readouterr().out
    counts = re.search(r"per rule: trees (\d+) rocks (\d+)", printed)
    totals = re.search(r"scattered (\d+) tiles: (\d+) cells, (\d+) without data, (\d+) instances", printed)
    assert counts and totals, printed
    atlas, b = made.tile_atlas, example.BORDER_SIZE
    index = {(t.side, t.lod, t.x, t.y): i for t, i in atlas.tiles()}
    h_data, m_data = atlas.download_tiles(example.HEIGHT, 0, atlas.atlas_size), atlas.download_tiles(example.SPLAT, 0, atlas.atlas_size)
    model = O.make_model("planar", (0, 0, 0), example.TERRAIN_SIZE, 0.0, example.MIN_HEIGHT, example.MAX_HEIGHT)
    coords = [(t.side, t.lod, t.x, t.y) for t in made.coords]
    assert len(coords) == 16
    want, first, stats = M.scatter(model, {k: h_data[i] for k, i in index.items()}, b, coords, example.SCATTER_RULES, seed=11, jitter=1.0,
                                   mask_tiles={k: m_data[i] for k, i in index.items()})
    assert [int(v) for v in counts.groups()] == stats["per_rule"][:2]
    assert [int(v) for v in totals.groups()] == [16, stats["cells"], stats["cells_no_data"], stats["total"]]
    assert stats["per_rule"][example.TREES] >= 1 and stats["per_rule"][example.ROCKS] >= 1, "the example places nothing of a rule: the comparison would be empty"
    assert made.instances.tobytes() == want.tobytes() and np.array_equal(made.first, first)
    # the picture: the splat map's size, a dot where an instance is
    image = example.picture(made)
    assert image.shape == (made.size, made.size, 4) and os.path.getsize(ppm) > 3 * made.size * made.size
    trees = made.instances["cell"][made.instances["rule"] == example.TREES]
    assert (image[trees[:, 1], trees[:, 0], :3] == np.array(example.DOTS[example.TREES], np.uint8)).all()

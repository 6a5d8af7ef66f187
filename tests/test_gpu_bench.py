"""bench.py as it is run for every change: a plain run times the headline steps and nothing else, and --dump-outputs writes
what the last timed step left in the atlas — checked here against the oracle's run of the same 16k job."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _cases as K
import _oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_times_the_headline_and_dumps_the_last_step(tmp_path):
    import bevy_terrain_amd as bt

    out = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2", "--dump-outputs", str(out)]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 4 and line["warmup"] == 2 and line["ms_per_step"] > 0
    assert line["unit"] == "tiles/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["value"] == pytest.approx(1365 / (line["ms_per_step"] / 1e3), rel=1e-12)
    # the side measurements belong to --full
    assert not {"roofline", "end_to_end", "cpu_baseline"} & set(line)
    assert line["config"]["ms_per_step_two_in_flight"] is None and not {"workloads", "tiling_prepass"} & set(line["config"])

    arrays = {f[:-len(".npy")]: np.load(out / f) for f in os.listdir(out)}
    assert set(arrays) == {"tile_coords", "tile_sums", "tile_sample", "tile_sample_coords"}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64e6
    coords, sums, sample, sample_coords = (arrays[k] for k in ("tile_coords", "tile_sums", "tile_sample", "tile_sample_coords"))
    assert coords.shape == (1365, 5) and sums.shape == (1365,) and sample.shape == (len(sample_coords), 512, 512) and len(sample_coords) > 0

    device = bt.Device(0)
    ptr = device.synth_fbm_r16(16384, 16384, 42)
    src = device.download(ptr, (16384, 16384), np.uint16)
    device.free(ptr)
    oracle = K.oracle_planar(src, 6, 512, 2, O.FORMAT_R16, atlas_size=2048, threads=O.usable_cores())
    assert [tuple(int(v) for v in row) for row in coords] == [c + (i,) for c, i in oracle.tiles()]
    assert all(sums[r] == float(oracle.tile(0, i).sum(dtype=np.uint64)) for r, (_, i) in enumerate(oracle.tiles()))
    for row, tile in zip(sample_coords, sample):
        assert np.array_equal(tile, oracle.tile(0, int(row[4])).astype(np.float32)), row

"""The kept scratch of the tile tree's queries (bt::Scratch of the context: grown on demand, kept until bt_ctx_trim) when a call outgrows it:
bt_tile_tree_raycast, bt_tile_tree_sample_normal and bt_tile_tree_render on ONE context, in that order and with no trim in between, each as
small call -> a call large enough to replace the buffer -> the small call again.  The small calls agree to the bit, the large call's
leading results are the small call's (its leading inputs are the small batch), bt_ctx_trim then gives back at least the three large
buffers (sizes from the documented layouts), a second trim nothing, and the small calls come out the same after it."""
import ctypes as C

import numpy as np
import pytest

import bevy_terrain_amd as bt
from bevy_terrain_amd import _ffi
from test_gpu_raycast import Streamed, make_rays

pytestmark = pytest.mark.gpu
SMALL, LARGE = 32, 4096
PLANES = ("t", "status", "normal", "rgba")


def same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def test_queries_outgrow_their_scratch_and_trim_gives_it_back(tmp_path):
    device = bt.Device(0)
    s = Streamed(device, tmp_path, "planar")  # test_gpu_raycast.py's smallest terrain
    rng = np.random.default_rng(11)

    # the inputs: each large batch begins with the small one
    few, many = make_rays(s.omodel, s.view, SMALL, seed=1), make_rays(s.omodel, s.view, LARGE - SMALL, seed=2)
    rays_small, rays_large = few, tuple(np.concatenate([a, b]) for a, b in zip(few, many))
    centre = np.array([float(s.omodel.position[i]) for i in range(3)])
    positions_large = centre + np.column_stack([rng.uniform(-480.0, 480.0, LARGE), rng.uniform(0.0, 300.0, LARGE), rng.uniform(-480.0, 480.0, LARGE)])
    positions_small = positions_large[:SMALL]
    # straight down onto the terrain; every term of a pixel's origin is exact in binary64, and pixel (x, y), x, y < 8, of the 64 x 64 camera
    # starts where pixel (x, y) of the 8 x 8 camera does: origin + 7 right - 7 up, right and up times 8
    origin, right, up = np.array([10.0, 400.0, 3.0]), np.array([32.0, 0.0, 0.0]), np.array([0.0, 0.0, -32.0])
    camera_small = bt.RenderCamera(origin, (0.0, -1.0, 0.0), right, up, 8, 8, 0.0, 512.0, orthographic=True)
    camera_large = bt.RenderCamera(origin + 7.0 * right - 7.0 * up, (0.0, -1.0, 0.0), 8.0 * right, 8.0 * up, 64, 64, 0.0, 512.0, orthographic=True)
    small_origins, large_origins = bt.render_rays(camera_small)[0].reshape(8, 8, 3), bt.render_rays(camera_large)[0].reshape(64, 64, 3)
    assert same(small_origins, large_origins[:8, :8])

    def raycast(rays):
        return s.tree.raycast(0, *rays, steps=64, refine_rounds=1)

    def render(camera):
        return s.tree.render(camera, steps=64, refine_rounds=1)

    # 1. raycast
    hits = raycast(rays_small)
    hits_large = raycast(rays_large)
    assert len(set(hits["status"])) >= 2  # (not one answer for every ray)
    assert same(hits_large[:SMALL], hits) and same(raycast(rays_small), hits)
    # 2. sample_normal
    normals = s.tree.sample_normal(0, positions_small)
    normals_large = s.tree.sample_normal(0, positions_large)
    assert len(np.unique(normals[0], axis=0)) > SMALL // 2
    assert all(same(l[:SMALL], n) for l, n in zip(normals_large, normals))
    assert all(same(a, n) for a, n in zip(s.tree.sample_normal(0, positions_small), normals))
    # 3. render
    picture = render(camera_small)
    picture_large = render(camera_large)
    assert picture["stats"]["hit_pixels"] >= 32 and len(np.unique(picture["t"])) > 16
    assert all(same(picture_large[p][:8, :8], picture[p]) for p in PLANES)
    again = render(camera_small)
    assert all(same(again[p], picture[p]) for p in PLANES) and again["stats"] == picture["stats"]

    # the three large buffers come back, once
    kept = LARGE * (C.sizeof(_ffi.RayC) + C.sizeof(_ffi.RayHitC)) + LARGE * (24 + 12 + 4) + 64 * 64 * 8
    assert device.trim() >= kept
    assert device.trim() == 0
    assert same(raycast(rays_small), hits)
    assert all(same(a, n) for a, n in zip(s.tree.sample_normal(0, positions_small), normals))
    again = render(camera_small)
    assert all(same(again[p], picture[p]) for p in PLANES) and again["stats"] == picture["stats"]

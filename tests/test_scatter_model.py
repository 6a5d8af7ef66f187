"""bt_atlas_scatter_instances without a GPU: the numpy model (tests/_scatter_model.py) against closed forms of the SCATTER section of
include/bevy_terrain_amd.h, every case of tests/_scatter_cases.py against the branch it is named for, and the entry point's refusals that
need no device.  tests/test_gpu_scatter.py holds the kernels to the model byte for byte."""
import ctypes as C

import numpy as np

import _normal_model as NM
import _oracle as O
import _scatter_cases as SCC
import _scatter_model as M
import _splat_cases as SC
import _splat_model as SM
from bevy_terrain_amd import ScatterRule as R
from bevy_terrain_amd import _ffi

F = np.float32
BT_ERR_INVALID_ARGUMENT = -1


# ---------------------------------------------------------------------------------------------- closed forms

def test_hash_and_unit_closed_forms():
    # mix on three known values (computed with Python integers)
    assert [int(v) for v in M.mix(np.array([0, 1, 0xFFFFFFFF], np.uint32))] == [0, 0x688990C0, 0x6768824A]
    assert int(M.draw(np.uint32(0), 1)[0]) == 0x01FCE552  # mix(0x9E3779B9)
    r = np.array([0, 255, 256, 0x80000000, 0xFFFFFFFF], np.uint32)
    f = M.unit(r)
    assert f.dtype == np.float32 and list(f) == [0.0, 0.0, 2.0 ** -24, 0.5, 1.0 - 2.0 ** -24] and (f < 1).all() and (f >= 0).all()
    everything = M.unit(M.mix(np.arange(1 << 16, dtype=np.uint32)))
    assert (everything >= 0).all() and (everything < 1).all()
    # the key holds the mosaic position, the side and the lod only
    assert int(M.key(7, 3, 2, 5, 9)[0]) == int(M.mix(M.mix(M.mix(np.uint32(7 ^ (3 << 8 | 2))) ^ np.uint32(5)) ^ np.uint32(9))[0])
    assert int(M.key(7, 3, 2, 5, 9)[0]) != int(M.key(7, 3, 2, 9, 5)[0])


def flat_tile(T, raw):
    return np.full((T, T), raw, np.uint16)


def test_constant_height_places_the_mesh_normal_at_altitude_h():
    T, b, raw = 16, 2, 30000
    rule = [R(density=0.5, scale=(2.0, 3.0))]
    for model, coord in ((SC.PLANAR[1], (0, 2, 1, 3)), (SC.SPHERE[1], (4, 1, 1, 0)), (SC.SPHERE[1], (2, 2, 3, 3))):
        out, holes = M.scatter_tile(model, flat_tile(T, raw), b, coord, rule, seed=3)
        assert holes == 0 and 30 <= len(out) <= 114  # 144 cells at 0.5: six sigma
        h = F(model.min_height) + (F(model.max_height) - F(model.min_height)) * (F(raw) / F(65535.0))
        c = T - 2 * b
        d = M.decide(model, flat_tile(T, raw), b, coord, rule, 3, 1.0)
        # a bilinear value of four equal texels is the texel; s = norm3f((0, 0, dist)): z is 1 up to the roundings of one normalisation
        assert (d["h"] == h).all() and (d["s"][0] == 0).all() and (d["s"][1] == 0).all() and (np.abs(d["s"][2] - F(1)) <= 2.0 ** -23).all()
        if int(model.kind) == 0:
            assert (out["position"][:, 1] == float(h)).all()
            assert (out["normal"][:, [0, 2]] == 0).all() and (np.abs(out["normal"][:, 1] - F(1)) <= 2.0 ** -23).all()
            # x and z inside the tile's square of the face of 1000
            lo, hi = np.array([1, 3]) / 4 * 1000 - 500, np.array([2, 4]) / 4 * 1000 - 500
            assert ((out["position"][:, [0, 2]] >= lo) & (out["position"][:, [0, 2]] < hi)).all()
        else:
            radius = np.sqrt((out["position"] ** 2).sum(axis=1))
            assert np.allclose(radius, 1000.0 + float(h), rtol=0, atol=1e-9)
            up = out["position"] / radius[:, None]
            # the mesh normal of a sphere is the direction of the position; the cast to binary32, the TBN (tan and bit are unit up to
            # roundings and s is (0, 0, 1) up to one) and three binary32 normalisations lie between them: a few units of 2^-24 each
            assert np.abs(out["normal"] - up).max() <= 16 * 2.0 ** -24
        assert ((out["scale"] >= 2) & (out["scale"] <= 3)).all() and ((out["yaw"] >= 0) & (out["yaw"] < F(6.2831855))).all()
        assert (out["cell"][:, 0] // c == coord[2]).all() and (out["cell"][:, 1] // c == coord[3]).all()
        order = out["cell"][:, 1].astype(np.int64) * 1000 + out["cell"][:, 0]
        assert (np.diff(order) > 0).all()  # j major, then i; at most one instance per cell


def test_local_position_is_the_oracles():
    rng = np.random.default_rng(5)
    for model in (SC.PLANAR[1], SC.SPHERE[1], O.make_model("ellipsoidal", (10.0, -20.0, 30.0), 1000.0, 900.0, -50.0, 450.0)):
        sides = range(6) if int(model.kind) else range(1)
        for side in sides:
            uv = rng.random((2, 16))
            local = M.local_position(model, side, uv)
            scale, pos = M.model_axes(model), [float(model.position[k]) for k in range(3)]
            up = local if int(model.kind) else [np.zeros(16), np.ones(16), np.zeros(16)]
            n = M._normalize3([scale[k] * up[k] for k in range(3)])
            for q in range(16):
                want = O.coordinate_world_position(model, side, (uv[0][q], uv[1][q]), 12.5)
                got = tuple((scale[k] * local[k][q] + pos[k]) + 12.5 * n[k][q] for k in range(3))
                assert got == want, (side, q, got, want)


def test_no_jitter_puts_uv_on_texel_centres_and_h_is_the_splat_models():
    spec = SC.SPECS["planar_b2"]
    h_tiles, _ = SC.oracle_state("planar_b2")
    model, b = SC.models(spec)[1], spec["b"]
    c = spec["T"] - 2 * b
    compared = 0
    for coord in SCC.tiles_of("planar_b2", lod=2):
        d = M.decide(model, h_tiles[coord], b, coord, SCC.RULES["three"], 4, 0.0)
        assert (d["uv"][0] == (d["i"].astype(np.float32) + F(0.5)) / F(c)).all() and (d["uv"][1] == (d["j"].astype(np.float32) + F(0.5)) / F(c)).all()
        h, _ = SM.height_and_steep(model, h_tiles[coord], b, coord[1])
        data = ~d["no_data"]
        assert (d["h"][data] == h.ravel()[data]).all()
        compared += int(data.sum())
    assert compared > 2000


def test_density_is_a_probability():
    spec = SC.SPECS["planar_72"]
    h_tiles, _ = SC.oracle_state("planar_72")
    model, b = SC.models(spec)[1], spec["b"]
    coord = (0, 2, 2, 2)
    counts = []
    for seed in (0, 1):
        d = M.decide(model, h_tiles[coord], b, coord, SCC.RULES["all_pass_quarter"], seed, 1.0)
        N, n = int((~d["no_data"]).sum()), int((d["rule"] == 0).sum())
        assert N >= 4096 and abs(n - 0.25 * N) <= 6 * np.sqrt(N * 0.25 * 0.75), (seed, N, n)
        counts.append(set(map(tuple, np.stack([d["gx"], d["gy"]], axis=1)[d["rule"] == 0].tolist())))
    assert counts[0] != counts[1] and len(counts[0] & counts[1]) < 0.5 * len(counts[0])  # two seeds: different sets


def test_density_zero_and_one():
    h_tiles, _ = SC.oracle_state("planar_b2")
    coords = SCC.tiles_of("planar_b2", lod=2)
    none, _, stats = SCC.model_scatter("planar_b2", coords, SCC.RULES["nothing"])
    assert len(none) == 0 and stats["total"] == 0 and stats["cells_no_data"] > 0
    # u == 0 against a sum of 0: `u < A` places nothing (seed 2 at lod 2 makes the key of mosaic texel (0, 0) zero; seed 4329 has f(r_0) == 0 at (22, 44))
    for seed, cell in SCC.ZERO_DRAWS:
        none, _, _ = SCC.model_scatter("planar_b2", coords, SCC.RULES["nothing"], seed=seed)
        assert len(none) == 0
        tile = (0, 2, cell[0] // 12, cell[1] // 12)
        d = M.decide(SC.models(SC.SPECS["planar_b2"])[1], h_tiles[tile], 2, tile, SCC.RULES["nothing"], seed, 1.0)
        at = np.flatnonzero((d["gx"] == cell[0]) & (d["gy"] == cell[1]))[0]
        assert M.unit(M.draw(d["key"], 0))[at] == 0 and not d["no_data"][at]
    full, first, stats = SCC.model_scatter("planar_b2", coords, SCC.RULES["everything"])
    assert stats["total"] == stats["cells"] - stats["cells_no_data"] == len(full) and first[-1] == len(full)


def test_a_tile_does_not_depend_on_the_list():
    coords = SCC.tiles_of("planar_b2", lod=2)
    whole, first, _ = SCC.model_scatter("planar_b2", coords, SCC.RULES["three"], seed=2)
    for t in (0, 5, 15):
        alone, _, _ = SCC.model_scatter("planar_b2", [coords[t]], SCC.RULES["three"], seed=2)
        assert alone.tobytes() == whole[int(first[t]):int(first[t + 1])].tobytes()


# ---------------------------------------------------------------------------------------------- the cases

def test_cases_reach_their_branches():
    """every case places at least one instance, leaves at least one data cell empty and reaches what it is named for.  The kernel's
    per-cell window test never fails on these states: the taps are clamped to the layer, where the window is cut, and elsewhere the halo
    T / (2c) + 2 bounds their reach; its HBM form runs for every cell only when no window is staged at all (a halo above MAX_HALO, a
    centre below a fourteenth of the texture, which no preprocessed state has).  What a state can reach of it is "clamped": a cell at a tile
    edge whose tap texels are clamped at the layer's edge, on an attachment whose border is below the reach (edge_clamp)."""
    for name, case in SCC.CASES.items():
        instances, first, stats, reached = SCC.model_case(name)
        spec_name, coords, rules, seed, jitter, masked = SCC.case_arguments(name)
        assert stats["total"] >= 1 and reached["empty"] >= 1, (name, stats, reached)
        for want in case["reach"]:
            assert reached.get(want, 0) >= 1, (name, want, reached)
        assert first[-1] == stats["total"] and len(first) == len(coords) + 1
        assert sum(SCC.window_fallbacks(SC.SPECS[spec_name], c, seed, jitter) for c in set(coords)) == 0, name
    c72, c136 = 72 - 4, 136 - 6
    assert c72 > SCC.LANES and c72 % SCC.LANES == 4 and -(-c72 // SCC.ROWS) == 5 and c72 % SCC.ROWS == 4
    assert c136 > 2 * SCC.LANES and -(-c136 // SCC.ROWS) == 9
    # the mask bytes: both ends
    assert {"mask_0", "mask_255"} <= {k for k, v in SCC.model_case("masked")[3].items() if v}
    # starved: the second rule passes everywhere, yet places only where the first does not reach
    inst = SCC.model_case("starved_by_the_sum")[0]
    assert 0 < (inst["rule"] == 1).sum() < (inst["rule"] == 0).sum()
    # the cube case meets all three face_up pairs
    assert set((SCC.case_arguments("cube_3")[1][k][0] >> 1) for k in range(30)) == {0, 1, 2}


# ---------------------------------------------------------------------------------------------- refusals that need no device

def test_null_arguments_are_refused():
    """fails on a library without the entry point"""
    fn = _ffi.lib().bt_atlas_scatter_instances
    model = _ffi.TerrainModelC()
    rules = (_ffi.ScatterRuleC * 1)(R()._c())
    stats = _ffi.ScatterStatsC()
    stats.total = 77
    for atlas_, model_, rules_, stats_ in ((None, C.byref(model), rules, C.byref(stats)), (None, None, rules, C.byref(stats)), (None, C.byref(model), None, C.byref(stats)),
                                           (None, C.byref(model), rules, None), (None, None, None, None)):
        assert fn(atlas_, 0, _ffi.SCATTER_NO_MASK, model_, None, 0, rules_, 1, 0, 1.0, None, 0, None, stats_) == BT_ERR_INVALID_ARGUMENT
    assert stats.total == 0  # zeroed by a refusal
    assert C.sizeof(_ffi.ScatterRuleC) == 48 and C.sizeof(_ffi.ScatterInstanceC) == 56 == M.DTYPE.itemsize and C.sizeof(_ffi.ScatterStatsC) == 104

"""The second models of the Rust-side contract (tests/_second_models.py: closed forms / whole-table numpy, written from the reference
text independently of the library's host code and the oracle) against the ORACLE, on the CPU.  tests/test_gpu_second_models.py holds the same
comparisons against the product."""
import numpy as np
import pytest

import _oracle as O
import _second_models as S
import bevy_terrain_amd as bt
from test_tile_tree_host import MODELS, positions


def oracle_indices(atlas):
    return {c: i for c, i in atlas.tiles()}


PLANAR_JOBS = {
    "full": [("tile", 0, (0.0, 0.0), (1.0, 1.0), 0, 4)],
    "sub_rectangle": [("tile", 0, (0.25, 0.0), (0.75, 0.5), 0, 5)],
    "odd_rectangle": [("tile", 0, (0.1, 0.37), (0.93, 0.81), 1, 5)],
    "partial_lods": [("tile", 0, (0.0, 0.0), (1.0, 1.0), 2, 5)],
    "overlay": [("tile", 0, (0.0, 0.0), (1.0, 1.0), 0, 4), ("tile", 0, (0.3, 0.2), (0.6, 0.9), 0, 5)],
    "side_by_side": [("tile", 0, (0.0, 0.0), (0.5, 1.0), 0, 4), ("tile", 0, (0.5, 0.0), (1.0, 1.0), 0, 4)],
    "beyond_the_face": [("tile", 0, (-0.25, 0.0), (1.5, 1.0), 0, 3)],
}


@pytest.mark.parametrize("name", sorted(PLANAR_JOBS))
def test_atlas_indices_of_planar_jobs_equal_the_oracle(name):
    jobs = PLANAR_JOBS[name]
    src = np.ones((40, 40), np.uint16)
    atlas = O.OracleAtlas(5, 2048, False, [(16, 2, 1, O.FORMAT_R16)])
    atlas.clear_attachment(0)
    for _, side, tl, br, l0, l1 in jobs:
        atlas.preprocess_tile(0, src, (l0, l1), side=side, top_left=tl, bottom_right=br)
    model = S.atlas_indices(jobs)
    assert model == oracle_indices(atlas) and len(model) > 10
    if len(jobs) == 1:  # one job on a fresh atlas: pure arithmetic
        _, side, tl, br, l0, l1 = jobs[0]
        for (s, lod, x, y), index in model.items():
            assert S.planar_closed_form(s, lod, x, y, tl, br, l0, l1) == index


@pytest.mark.parametrize("lods", [(0, 1), (0, 3), (1, 4)])
def test_atlas_indices_of_cube_jobs_equal_the_oracle(lods):
    faces = [np.ones((24, 24), np.uint16)] * 6
    atlas = O.OracleAtlas(4, 2048, True, [(16, 2, 1, O.FORMAT_R16)])
    atlas.clear_attachment(0).preprocess_spherical(0, faces, lods)
    model = S.atlas_indices([("spherical",) + lods])
    assert model == oracle_indices(atlas)
    per_side = sum(4 ** l for l in range(*lods))
    for (side, lod, x, y), index in model.items():  # full faces: side-major, then LODs downwards, x-major
        assert index == side * per_side + sum(4 ** l for l in range(lod + 1, lods[1])) + x * (1 << lod) + y


def random_jobs(rng):
    jobs = []
    for _ in range(rng.integers(1, 4)):
        a, b = np.sort(rng.random(2)), np.sort(rng.random(2))
        l0 = int(rng.integers(0, 3))
        jobs.append(("tile", 0, (float(a[0]), float(b[0])), (float(a[1]) + 0.05, float(b[1]) + 0.05), l0, int(l0 + rng.integers(1, 4))))
    return jobs


@pytest.mark.parametrize("seed", range(12))
def test_atlas_indices_of_random_job_sequences_equal_the_oracle(seed):
    jobs = random_jobs(np.random.default_rng(700 + seed))
    src = np.ones((40, 40), np.uint16)
    atlas = O.OracleAtlas(6, 4096, False, [(16, 2, 1, O.FORMAT_R16)])
    atlas.clear_attachment(0)
    for _, side, tl, br, l0, l1 in jobs:
        atlas.preprocess_tile(0, src, (l0, l1), side=side, top_left=tl, bottom_right=br)
    assert S.atlas_indices(jobs) == oracle_indices(atlas)


def tree_model(kind, lods, tree_size, load_distance=2.5):
    model, _ = MODELS[kind]
    return S.TileTreeModel(kind, model.translation, model.scale_vec, model.min_height, model.max_height, lods, tree_size, load_distance)


@pytest.mark.parametrize("kind", ["planar", "sphere", "ellipsoid"])
@pytest.mark.parametrize("lods,tree_size", [(7, 8), (12, 4), (3, 8)])
def test_tile_tree_update_model_equals_the_oracle(kind, lods, tree_size):
    _, omodel = MODELS[kind]
    otree = O.TileTree(omodel, lods, O.make_view_config(tree_size=tree_size))
    mine = tree_model(kind, lods, tree_size)
    pushed = 0
    for frame, pos in enumerate(positions(kind, 40, seed=11 + lods)):
        pos = tuple(float(v) for v in pos)
        exp_released, exp_requested = otree.update(pos)
        # the ellipsoid's view coordinate (a 1074-step bisection) is taken from the oracle: update itself is what is modelled
        vc = O.coordinate_from_world_position(omodel, pos) if kind == "ellipsoid" else None
        if kind != "ellipsoid":  # ... and where it is restated here it must agree
            side, uv = mine.view_coordinate(pos)
            oside, ouv = O.coordinate_from_world_position(omodel, pos)
            assert side == oside and tuple(uv) == ouv, (frame, pos)
        released, requested = mine.update(pos, vc)
        assert released == exp_released and requested == exp_requested, (frame, pos)
        _, origins, coords, flags = otree.read()
        my_coords, my_flags = mine.node_tables()
        assert np.array_equal(origins, mine.origins) and np.array_equal(coords, my_coords) and np.array_equal(flags, my_flags), frame
        pushed += len(requested) + len(released)
    assert pushed > 50


@pytest.mark.parametrize("fmt,T,mips", [(O.FORMAT_R16, 32, 4), (O.FORMAT_R16, 16, 5), (O.FORMAT_RGBA8, 32, 3), (O.FORMAT_RGBA8, 8, 4)])
def test_generate_mipmaps_model_equals_the_oracle(fmt, T, mips):
    rng = np.random.default_rng(T * mips)
    if fmt == O.FORMAT_R16:
        tile = rng.integers(0, 65536, size=(T, T), dtype=np.uint16)
        tile[rng.random((T, T)) < 0.3] = 0  # holes: the valid-mean and the all-zero rule
        tile[:4, :4] = 0
    else:
        tile = rng.integers(0, 256, size=(T, T, 4), dtype=np.uint8)
    exp = O.generate_mipmaps(fmt, tile, mips)
    mine = S.generate_mipmaps(tile, mips)
    assert np.array_equal(np.asarray(exp).reshape(mine.shape), mine)


def test_tc_bytes_equal_the_hand_rolled_bincode_writer():
    rng = np.random.default_rng(5)
    tiles = [(0, 0, 0, 0), (5, 31, 250, 251), (1, 17, 65535, 65536), (2, 30, (1 << 30) - 1, 4294967295), (3, 2, 1, 3)]
    tiles += [tuple(int(v) for v in rng.integers(0, [6, 20, 1 << 20, 1 << 20])) for _ in range(300)]
    mine = S.tc_encode(tiles)
    assert O.tc_encode(tiles) == mine
    assert bt.tc_encode([bt.TileCoordinate(*t) for t in tiles]) == mine
    assert mine[:3] == bytes([251]) + (305).to_bytes(2, "little")  # 305 tiles: the u16 marker
    assert [(t.side, t.lod, t.x, t.y) for t in bt.tc_decode(mine)] == tiles


@pytest.mark.parametrize("seed", range(45))
def test_tile_tree_update_model_on_the_random_sweep(seed):
    """the sweep of tests/test_gpu_tile_tree.py (random models, configurations and teleporting views) with the numpy model in the
    place of the device"""
    from test_gpu_tile_tree import draw_tree_case

    model, omodel, lods, cfg, pts = draw_tree_case(seed)
    kind = {"planar": "planar", "spherical": "sphere", "ellipsoidal": "ellipsoid"}[model.kind]
    otree = O.TileTree(omodel, lods, O.make_view_config(**cfg))
    mine = S.TileTreeModel(kind, model.translation, model.scale_vec, model.min_height, model.max_height, lods, cfg["tree_size"], cfg["load_distance"])
    for frame, pos in enumerate(pts):
        exp = otree.update(pos)
        vc = O.coordinate_from_world_position(omodel, pos) if kind == "ellipsoid" else None
        assert mine.update(pos, vc) == exp, (seed, frame, pos)
        _, origins, coords, flags = otree.read()
        my_coords, my_flags = mine.node_tables()
        assert np.array_equal(origins, mine.origins) and np.array_equal(coords, my_coords) and np.array_equal(flags, my_flags), (seed, frame)


@pytest.mark.parametrize("kind", ["planar", "sphere"])
def test_view_state_fields_follow_from_the_second_model(kind):
    """a20 (TileTree::new :133-160, TerrainViewConfigUniform::from_tile_tree, the view coordinates of
    TerrainModelApproximation::compute :283-285): bt_view_state_from_config against values derived HERE from the numpy model's view
    coordinate and side projection — not from the oracle's restatement."""
    model, _ = MODELS[kind]
    vc = bt.TerrainViewConfig(geometry_tile_count=4321, refinement_count=9, grid_size=12, origin_lod=9, morph_distance=12.5, subdivision_tolerance=0.15)
    mine = tree_model(kind, 8, 8)
    scale = float(model.scale_vec[0]) / 2.0 if kind == "planar" else float(model.scale_vec[0])  # TerrainModel::scale (terrain_model.rs:183-193)
    pts = [tuple(float(v) for v in p) for p in positions(kind, 120, 23)]
    if kind == "sphere":
        r = 7.1e6
        pts += [(r, 0.0, 0.0), (0.0, -r, 0.0), (0.0, 0.0, r), (-r, 0.25 * r, -r), (r, r, r)]
    for p in pts:
        v = bt.view_state_from_config(model, vc, p, 77.25)
        assert (v.spherical, v.geometry_tile_count, v.refinement_count, v.origin_lod) == (int(kind != "planar"), 4321, 9, 9)
        assert v.vertices_per_tile == 2 * 12 * (12 + 2)
        assert v.approximate_height == np.float32(77.25)
        assert v.subdivision_distance == np.float32(12.5 * scale * (1.0 + 0.15))
        assert tuple(v.world_position) == tuple(np.asarray(p, np.float64).astype(np.float32))
        side0, uv0 = mine.view_coordinate(p)
        for side in range(6 if kind != "planar" else 1):
            uv = mine.project_to_side(side0, uv0, side) * 512.0  # x count(origin_lod)
            xy = np.trunc(uv)  # as_ivec2
            assert tuple(v.sides[side].view_xy) == (int(xy[0]), int(xy[1])), (p, side)
            assert tuple(v.sides[side].view_uv) == tuple((uv - xy).astype(np.float32)), (p, side)  # fract() then as_vec2


@pytest.mark.parametrize("lod", [0, 1, 2, 3])
def test_cube_neighbours_are_geometric_neighbours(lod):
    """a10 (coordinate.rs:208-279 with NEIGHBOURING_SIDES and SideInfo::project_to_side): checked against GEOMETRY, not against a
    restated table — on the unit cube-sphere an edge neighbour shares exactly two corner points with the tile, a diagonal neighbour
    exactly one, whatever faces they lie on; the diagonal across a cube corner (three faces meet) does not exist.  Corner points come
    from the numpy model's own warp (TileTreeModel.world_position), the neighbours from bt_tile_neighbours and from the oracle."""
    sphere = S.TileTreeModel("sphere", (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 0.0, 0.0, 4, 4, 2.5)
    n = 1 << lod

    def corners(side, x, y):
        uv = np.array([[x, y], [x + 1, y], [x, y + 1], [x + 1, y + 1]], np.float64) / n
        return sphere.world_position(side, uv, 0.0)

    def shared(a, c):
        return sum(1 for p in a for q in c if np.abs(p - q).max() < 1e-12)

    checked = 0
    for side in range(6):
        for x in range(n):
            for y in range(n):
                mine = corners(side, x, y)
                nbs = bt.TileCoordinate(side, lod, x, y).neighbours(True)
                assert [(c.side, c.lod, c.x, c.y) for c in nbs] == O.neighbours((side, lod, x, y), True)
                for k, nb in enumerate(nbs):
                    at_cube_corner = k >= 4 and [(-1, -1), (1, -1), (1, 1), (-1, 1)][k - 4] in [
                        (dx, dy) for dx in (-1, 1) for dy in (-1, 1) if not (0 <= x + dx < n) and not (0 <= y + dy < n)]
                    if at_cube_corner:
                        assert nb.lod == 0xFFFFFFFF or nb.side == 0xFFFFFFFF, (side, x, y, k)  # TileCoordinate::INVALID
                        continue
                    assert nb.lod == lod and nb.side < 6
                    if lod == 0 and nb.side == side:
                        continue  # (never happens: a face's neighbours are other faces)
                    assert shared(mine, corners(nb.side, nb.x, nb.y)) == (2 if k < 4 else 1), (side, x, y, k, (nb.side, nb.x, nb.y))
                    checked += 1
    assert checked >= 6 * n * n * 4


def test_children_tile_their_parent_geometrically():
    """coordinate.rs:187-206: the four children of a tile cover exactly its patch of the cube-sphere (their 9 distinct corner points
    are the parent's 3 x 3 grid of corner / edge-midpoint / centre points in uv), and parent() undoes children()."""
    sphere = S.TileTreeModel("sphere", (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 0.0, 0.0, 4, 4, 2.5)
    for side, lod, x, y in [(0, 0, 0, 0), (3, 1, 1, 0), (5, 2, 3, 2), (1, 3, 0, 7), (4, 3, 5, 5)]:
        n = 1 << lod
        grid = {tuple(np.round(sphere.world_position(side, np.array([[(x + i / 2) / n, (y + j / 2) / n]]), 0.0)[0], 12)) for i in range(3) for j in range(3)}
        kids = bt.TileCoordinate(side, lod, x, y).children()
        assert [(c.side, c.lod, c.x, c.y) for c in kids] == [(side, lod + 1, 2 * x + i % 2, 2 * y + i // 2) for i in range(4)]
        pts = set()
        for c in kids:
            assert (lambda p: (p.side, p.lod, p.x, p.y))(c.parent()) == (side, lod, x, y)
            m = 1 << c.lod
            uv = np.array([[c.x, c.y], [c.x + 1, c.y], [c.x, c.y + 1], [c.x + 1, c.y + 1]], np.float64) / m
            pts |= {tuple(np.round(p, 12)) for p in sphere.world_position(c.side, uv, 0.0)}
        assert pts == grid


@pytest.mark.parametrize("seed,atlas_size,attachments", [(1, 6, 1), (2, 9, 2), (3, 24, 1), (4, 5, 3)])
def test_stream_model_equals_the_oracle_state_machine(seed, atlas_size, attachments):
    """TileAtlasState's streaming half (tile_atlas.rs:300-500): random request / release / load-completion sequences through the
    Python container model and through the oracle's restatement — same atlas slots (LRU reuse), same load queue, same best tiles
    while tiles are still loading."""
    rng = np.random.default_rng(seed)
    tiles = [(0, lod, x, y) for lod in range(4) for x in range(1 << lod) for y in range(1 << lod)]
    existing = [t for t in tiles if rng.random() < 0.85]
    mine, theirs = S.StreamModel(atlas_size, attachments, existing), O.Stream(atlas_size, attachments, existing)
    held = []  # tiles with outstanding requests (a tile may appear more than once)
    reused = 0
    for step in range(600):
        r = rng.random()
        live = len({t for t in held if t in mine.existing})
        if r < 0.5 and (live < atlas_size - 1 or rng.random() < 0.3):
            t = tiles[int(rng.integers(len(tiles)))]
            if t in mine.existing and t not in mine.states and not mine.unused:
                continue  # the reference panics ("Atlas out of indices"): not part of the comparison
            before = mine.states.get(t)
            mine.request_tile(t)
            theirs.request_tile(t)
            held.append(t)
            reused += before is None and t in mine.existing
        elif r < 0.8 and held:
            # (a tile is released only once it is loaded: the reference unwraps the state of a tile whose load completes — a slot
            # taken back while its tile is still loading makes it panic, and is not part of the comparison)
            n = mine.pending_loads()
            assert mine.finish_loads(n) == theirs.finish_loads(n)
            t = held.pop(int(rng.integers(len(held))))
            mine.release_tile(t)
            theirs.release_tile(t)
        else:
            assert mine.pending_loads() == theirs.pending_loads()
            n = int(rng.integers(0, mine.pending_loads() + 1))
            assert mine.finish_loads(n) == theirs.finish_loads(n)
        for t in tiles[:: 3]:
            assert mine.get_best_tile(t) == theirs.get_best_tile(t), (step, t)
            if t in mine.states:
                assert theirs.atlas_index(t) == mine.states[t][2]
    assert reused > atlas_size  # slots were taken back and handed out again

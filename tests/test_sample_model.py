"""No GPU: what test_gpu_sample_shapes.py assumes of its inputs (tests/_sample_cases.py), on tiles the CPU oracle makes.

For every case of the table: the best-tile table the second models derive from the loaded set is the nearest-loaded-ancestor table and has
the fallback depths its layout is named for; the second model of sample_attachment (tests/_second_models.py, both formats) equals the
oracle's (O.TileTree.sample_attachment) bit for bit on all 1000 positions; the trace of the second model shows that the batch reaches every
branch the GPU test relies on, with the minimum counts of _sample_cases.MINIMUM; and at most 1 % of the draws had to be replaced because
compute_blend's log2 sat within two representable doubles of a decision (both sides use this machine's libm here: the rule is about the
device's)."""
import numpy as np
import pytest

import _oracle as O
import _sample_cases as SC
import _second_models as S


@pytest.mark.parametrize("spec_name", list(SC.SPECS))
def test_loaded_set_gives_the_fallback_table(spec_name):
    spec = SC.SPECS[spec_name]
    tm, requested, loaded, entries, coords = SC.table(spec_name)
    existing = set(SC.oracle_tiles(spec_name))
    # every node that names an existing tile was requested (the load distance covers every window; a request of a tile that does not exist is
    # ignored), the missing ones failed, the rest loaded
    named = {tuple(c) for c in coords.tolist()} & existing
    assert set(requested) & existing == named and set(loaded) == named - spec["missing"] and len(set(loaded.values())) == len(loaded)
    assert np.array_equal(entries, SC.nearest_loaded_ancestor(coords, loaded))
    # the table's depths, node by node: own tile, parent, grandparent, (the root), nothing
    depth = {}
    for c, (index, lod) in zip(coords.tolist(), entries.tolist()):
        if tuple(c) in existing:
            depth.setdefault(None if lod == SC.INVALID else c[1] - lod, []).append(tuple(c))
    assert {0, 1, 2, None} <= set(depth), sorted(depth, key=str)
    assert any(c[1] == 3 and max(c[2], c[3]) >= SC.TREE and lod != SC.INVALID for c, (index, lod) in zip(coords.tolist(), entries.tolist())), \
        "no node with an entry sits in a wrapped slot"
    # the oracle's tile tree, given the same view, holds the same nodes in the same order
    otree = O.TileTree(SC.MODELS[spec["kind"]][1], SC.LODS, SC.view_config(spec_name)[1])
    assert otree.update(spec["view"]) == ([], requested)
    assert np.array_equal(otree.read()[2], coords)


@pytest.mark.parametrize("name", list(SC.CASES))
def test_second_model_equals_the_oracle_and_cases_reach_their_branches(name):
    c = SC.case(name)
    assert c.positions.shape == (SC.COUNT, 3) and np.isfinite(c.positions).all()
    assert np.array_equal(c.oracle_nodes, c.coords)
    # the second model == the oracle, bit for bit, no position excluded
    bad = np.flatnonzero((c.model_values.view(np.uint32) != c.oracle_values.view(np.uint32)).any(axis=1))
    assert len(bad) == 0, (len(bad), bad[:5], c.positions[bad[:3]], c.model_values[bad[:3]], c.oracle_values[bad[:3]])
    assert np.array_equal(c.model_heights.view(np.uint32), c.oracle_heights.view(np.uint32))
    # (lod, ratio) of the trace == the oracle's compute_blend of the surface position
    otree = O.TileTree(SC.MODELS[c.spec["kind"]][1], SC.LODS, SC.view_config(c.spec_name)[1])
    otree.update(c.spec["view"])
    tm = SC.table(c.spec_name)[0]
    for p, t in list(zip(c.positions, c.trace))[::7]:
        lod, ratio = otree.compute_blend(tuple(S.surface_position(tm, p, tm.approximate_height)))
        assert (lod, np.float32(ratio)) == (t.lod, t.ratio), p
    # the format's channels: R16 has one, an Rgba8 sample's four differ
    if c.fmt == SC.R16:
        assert not c.model_values[:, 1:].any() and c.model_values[:, 0].any()
    else:
        v = c.model_values[c.model_values[:, 0] != 0]
        assert len(v) > 300 and all((v[:, i] != v[:, j]).mean() > 0.9 for i in range(4) for j in range(i))
    # a sample with no loaded ancestor is exactly zero and its height exactly min_height
    none = np.array([t.lookups[0].depth is None and (len(t.lookups) == 1 or t.lookups[1].depth is None) for t in c.trace])
    lo = np.float32(SC.MODELS[c.spec["kind"]][0].min_height)
    assert not c.oracle_values[none].any() and (c.oracle_heights[none] == lo).all()
    # every branch, with its minimum count
    counts, minimum = SC.reach_counts(c), SC.minimum(c)
    print(name, counts, "draws", c.draws, "replaced", c.replaced)
    short = {k: (counts[k], m) for k, m in minimum.items() if counts[k] < m}
    assert not short, short
    # a blend really mixes two different samples somewhere, and a fallback really magnifies (uv of the coarser tile)
    assert sum(1 for t in c.trace if len(t.lookups) == 2 and t.lookups[0].atlas_index != t.lookups[1].atlas_index and None not in (t.lookups[0].depth, t.lookups[1].depth)) >= 32
    # the log2 caveat: at most 1 % of the draws were replaced
    assert c.replaced * 100 <= c.draws, (c.replaced, c.draws)


def test_wrapper_keeps_the_r16_signature():
    c = SC.case("planar_r16")
    tm = SC.table("planar")[0]
    values, heights = S.sample_attachment_r16(tm, c.spec["view"], tm.approximate_height, SC.blend_distance("planar"), SC.BLEND_RANGE, SC.LODS,
                                              c.entries.reshape(1, SC.LODS, SC.TREE, SC.TREE, 2), c.layers, 32, 2, c.positions[:40])
    assert np.array_equal(values, c.model_values[:40]) and np.array_equal(heights, c.model_heights[:40])


def test_admissibility_rule():
    """stepping the log2 two doubles either way: a value in the middle of an f32 interval is admissible, one at a rounding boundary of the f32
    target, at the cap, at 0 and at an integer (lod changes) is not"""
    ok = lambda l2: S.blend_is_admissible(l2, 4, 0.2)
    assert ok(2.1) and ok(0.5) and ok(-3.0) and ok(17.0) and ok(float("inf")) and ok(2.0)  # f32(2.0 -+ 2 ulp of a double) is 2.0
    boundary = float(np.float32(2.1)) + float(np.spacing(np.float32(2.1))) / 2  # halfway between two floats
    assert not ok(boundary) and not ok(float(np.nextafter(boundary, 0.0)))
    assert not ok(4.0 - 0.00001) and not ok(0.0)

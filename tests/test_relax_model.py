"""The protocol of the block relaxation (csrc/bt_relax.hpp) on its schedule model (tests/_relax_model.py), without a GPU.

Two things are shown.  First, that the protocol is sound on every scene of tests/_drain_cases.py and tests/_path_cases.py: in all four
block orders of the model, stale halos included, the four rules reach the planes of the sequential models, drainage byte for byte and D
bit for bit.  That is the first check of the "a stale halo cannot move the fixed point" arguments written at each rule.  Second, that the
scenes have teeth: for every rule and every one of the nine flag bits a NAMED scene exists on which the model without that bit ends
somewhere else in all four orders, so no schedule can hide a kernel that lost the bit; the same for the 3 x 3 flags around a goal, for the
corner cells of the halo, and for the host loop's steady batch of 32 sweeps.  test_gpu_drain.py and test_gpu_path.py run those scenes on
the device.

Sweep counts of the model are from Jacobi rounds, the slowest legal form: they choose scenes and are never expected values."""
import functools

import numpy as np
import pytest

import _drain_cases as DC
import _path_cases as PC
import _relax_model as R

DRAIN_RULES = ("fill", "flat", "accumulate")
RULES = DRAIN_RULES + ("path",)
CORNERS = R.DIAGONAL


def bits(plane):
    return np.ascontiguousarray(plane, dtype=np.float32).view(np.uint32)


def sequential(rule, name):
    """the sequential model's plane of the rule, D as its bits"""
    return bits(PC.expected(name)[1]) if rule == "path" else DC.expected(name)[1 + DRAIN_RULES.index(rule) + (rule == "accumulate")]


@functools.lru_cache(maxsize=None)
def model(rule, name, order, drop=(), own_block_only=False, halo_corners=True):
    """(the plane, the Result) of the schedule model on a scene; every relaxation starts from the sequential model's planes before it"""
    kw = dict(order=order, seed=11, drop=drop, halo_corners=halo_corners)
    if rule == "path":
        scene, raw = PC.SCENES[name], PC.expected(name)[0]
        D, res = R.path(raw, scene["mask"], scene["cost"], scene["goals"], own_block_only=own_block_only, **kw)
        return bits(D), res
    scene = DC.SCENES[name]
    raw, W, _, direction, _, _ = DC.expected(name)
    if rule == "fill":
        return R.fill(raw, scene["void"], **kw)
    if rule == "flat":
        return R.flat(raw, scene["void"], W, **kw)
    return R.accumulate(direction, scene["weight"], **kw)


def differs_in_every_order(rule, name, **weakened):
    """the weakened model misses the sequential plane in all four orders, and the model as it is reaches it in all four"""
    want = sequential(rule, name)
    assert all(np.array_equal(model(rule, name, order)[0], want) for order in R.ORDERS), (rule, name)
    return all(not np.array_equal(model(rule, name, order, **weakened)[0], want) for order in R.ORDERS)


# ---------------------------------------------------------------------------------------------- the protocol is sound

@pytest.mark.parametrize("name", sorted(DC.SCENES))
def test_every_drainage_scene_reaches_the_sequential_planes_in_every_order(name):
    for rule in DRAIN_RULES:
        want = sequential(rule, name)
        for order in R.ORDERS:
            got, res = model(rule, name, order)
            assert res.converged and got.dtype == want.dtype and got.tobytes() == want.tobytes(), (name, rule, order, np.argwhere(got != want)[:5])


@pytest.mark.parametrize("name", sorted(PC.SCENES))
def test_every_path_scene_reaches_the_sequential_field_in_every_order(name):
    want = sequential("path", name)
    for order in R.ORDERS:
        got, res = model("path", name, order)
        assert res.converged and np.array_equal(got, want), (name, order, np.argwhere(got != want)[:5])


def test_the_host_loop_launches_whole_batches():
    """4, then 8, 16, 32, 32, ...: the count of launched sweeps is one of 4, 12, 28, 60, 92, ..., the first that is not below `quiet`, the
    first sweep that flagged nothing; a window of fewer cells than that is cut at its cell count"""
    totals = [4, 12, 28, 60, 92, 124, 156]
    for rule, name in (("fill", "serpentine"), ("fill", "bowl"), ("accumulate", "long_walk"), ("path", "maze"), ("path", "w65"), ("flat", "crossing_up_left")):
        for order in R.ORDERS:
            res = model(rule, name, order)[1]
            assert res.sweeps == next(t for t in totals if t >= res.quiet), (rule, name, order, res.sweeps, res.quiet)
            assert len(res.log) <= res.quiet and all(res.log), "a sweep past the first quiet one ran a block"
    assert model("fill", "one_cell", "ascending")[1].sweeps == 1 and model("path", "one_cell", "stale")[1].sweeps == 1


# ---------------------------------------------------------------------------------------------- every flag bit is needed by a named scene

# (rule, bit) -> the scene on which the model without the bit fails in all four orders.  Corners: the crossings, made for it.  Edges:
# the long walks enter a block through an edge only after some seven sweeps in the block before, rightwards, upwards and downwards (the
# banded serpentine) or leftwards, rightwards and downwards (the maze); the accumulation's sums find the long walk's blocks awake (each
# works on its own 470 cells until the sums from upstream are final), so they need the upstream crossings, but for `down`, which the
# ordinary terrain of w65_h65 already needs.  kSelf: the one-block serpentine, and for the path field a crossing's
DEFEATED_BY = {}
for _rule in ("fill", "flat"):
    DEFEATED_BY.update({(_rule, bit): f"crossing_{bit}" for bit in CORNERS + ("left",)})
    DEFEATED_BY.update({(_rule, bit): "long_walk" for bit in ("right", "up", "down")})
    DEFEATED_BY[(_rule, "self")] = "serpentine"
DEFEATED_BY.update({("accumulate", bit): f"crossing_{bit}_upstream" for bit in CORNERS + ("left", "right", "up")})
DEFEATED_BY.update({("accumulate", "down"): "w65_h65", ("accumulate", "self"): "serpentine"})
DEFEATED_BY.update({("path", bit): f"crossing_{bit}" for bit in CORNERS + ("up",)})
DEFEATED_BY.update({("path", bit): "maze" for bit in ("left", "right", "down")})
DEFEATED_BY[("path", "self")] = "crossing_down_right"


@pytest.mark.parametrize("rule,bit", sorted(DEFEATED_BY))
def test_without_a_flag_bit_the_model_fails_in_every_order(rule, bit):
    assert set(DEFEATED_BY) == {(r, b) for r in RULES for b in R.BITS}
    assert differs_in_every_order(rule, DEFEATED_BY[(rule, bit)], drop=(bit,)), (rule, bit, DEFEATED_BY[(rule, bit)])


@pytest.mark.parametrize("rule", RULES)
def test_the_older_scenes_cannot_see_a_missing_corner_flag(rule):
    """why the crossings exist: the bowls, plateaus, sizes and voids, the funnel, and the path scene named for its step across a block
    corner reach the sequential planes without any of the four diagonal bits, in every order: the cardinal neighbours change too and pass
    the news on one sweep later"""
    names = ["pure_distance_through_a_block_corner", "w65", "mask_and_holes"] if rule == "path" else ["bowl", "bowl_with_island_lake", "plateau", "funnel_255", "w65_h65", "w33_h65_quantised"]
    for name in names:
        for order in R.ORDERS:
            assert np.array_equal(model(rule, name, order, drop=CORNERS)[0], sequential(rule, name)), (rule, name, order)


def plain_diagonal_channel(raw):
    """what a crossing must NOT be: a channel straight down the diagonal from the outlet (0, 0) through the corner of the four blocks"""
    z = np.full((64, 64), 60000, np.uint16)
    z[np.arange(48), np.arange(48)] = 1000
    return z


def test_a_plain_diagonal_channel_or_a_bowl_would_not_do():
    """the news crosses the corner in sweep 1 or 2, when the diagonal block is awake anyway: some order hides the missing bit"""
    for plant, rect in ((plain_diagonal_channel, (70, 71, 64, 64)), (DC.bowl(False), (70, 71, 70, 70))):
        raw = plant(np.zeros(rect[3:1:-1], np.uint16))
        want = DC.M.drainage(raw)[0]
        hidden = [order for order in R.ORDERS if np.array_equal(R.fill(raw, None, order=order, drop=("down_right",))[0], want)]
        assert hidden, plant


@pytest.mark.parametrize("bit", CORNERS)
def test_a_corner_crossing_wakes_a_quiet_block_by_its_diagonal_flag_alone(bit):
    """the far block is flagged by nothing but the one diagonal bit, after the first batch, having been idle the sweep before; without the
    bit it keeps what it had when it went quiet, the same cells and values in every order: 60000 instead of 1000 in its channel, no
    flat distance there, a corridor never reached; and sums in its channel that lack some of the serpentine's (how much is the
    schedule's).  A device whose kernel lost the bit would return exactly these planes: the bit's only effect is to flag that block"""
    dx, dy = R.BITS[bit][1:]
    _, mirror_x, mirror_y = DC.CROSSINGS[bit]
    far = (0 if mirror_x else 1, 0 if mirror_y else 1)
    far_cells = np.zeros((64, 64), bool)
    far_cells[far[1] * 32:far[1] * 32 + 32, far[0] * 32:far[0] * 32 + 32] = True
    for rule in RULES:
        name = DEFEATED_BY[(rule, bit)]
        want = sequential(rule, name)
        channel = (PC.expected(name)[0] == PC.FLOOR) if rule == "path" else (DC.expected(name)[0] == 1000)
        for order in R.ORDERS:
            log = model(rule, name, order)[1].log
            late = [s for s in range(R.BATCH_FIRST, len(log)) if far in log[s]]
            assert late and all(log[s][far] == R.BITS[bit][0] for s in late), (rule, name, order, late)
            if rule != "accumulate":  # (a growing sum flags the far block in every sweep; the level, the distance and the cost arrive once)
                assert far not in log[late[0] - 1], (rule, name, order, late)
            got = model(rule, name, order, drop=(bit,))[0]
            wrong = got != want
            if rule == "accumulate":  # the far channel, and the outlet it ends on, lack the serpentine's sums
                assert wrong.any() and not wrong[~(far_cells & channel)].any() and (got[wrong] < want[wrong]).all(), (name, order)
                continue
            stuck = dict(fill=60000, flat=R.NONE, path=R.INF_BITS)[rule]
            assert np.array_equal(wrong, far_cells & channel) and (got[wrong] == stuck).all(), (rule, name, order, int(wrong.sum()))
        if rule != "accumulate":  # (how much of the sum the far block had seen when it last ran is the schedule's)
            assert len({model(rule, name, order, drop=(bit,))[0].tobytes() for order in R.ORDERS}) == 1, (rule, name)


def test_the_serpentine_stops_at_the_round_limit_and_flags_itself():
    for rule in DRAIN_RULES:
        for order in R.ORDERS:
            res = model(rule, "serpentine", order)[1]
            assert {(s, 0, 0) for s in range(R.BATCH_FIRST)} <= res.limited and res.quiet > R.BATCH_FIRST, (rule, order)
            assert all(log == {(0, 0): R.BITS["self"][0]} for log in res.log[1:]), "one block: nothing but itself can flag it"


# ---------------------------------------------------------------------------------------------- the goal's 3 x 3 flags, the halo's corners

@pytest.mark.parametrize("name", ["goal_in_a_corner", "goal_on_an_edge"])
def test_flagging_only_the_goals_own_block_leaves_cells_unreached(name):
    want = sequential("path", name)
    for order in R.ORDERS:
        got, res = model("path", name, order, own_block_only=True)
        lost = (got == R.INF_BITS) & (want != R.INF_BITS)
        assert lost.sum() >= 7 and res.quiet == 1, (name, order)  # the goal's block changes nothing and flags nothing: the call ends there
        assert np.array_equal(model("path", name, order)[0], want)


def test_every_older_goal_has_a_way_on_in_its_own_block():
    """why the two goal scenes exist"""
    for name in sorted(set(PC.SCENES) - {"goal_in_a_corner", "goal_on_an_edge"}):
        assert np.array_equal(model("path", name, "stale", own_block_only=True)[0], sequential("path", name)), name


@pytest.mark.parametrize("rule", RULES)
def test_without_the_halos_corner_cells_the_model_fails_in_every_order(rule):
    """the four corner cells of the staged tile: a diagonal neighbour's words, and for the path field the height that the diagonal weight
    is formed from"""
    assert differs_in_every_order(rule, DEFEATED_BY[(rule, "down_right")], halo_corners=False)
    assert differs_in_every_order(rule, DEFEATED_BY[(rule, "up_left")], halo_corners=False)
    if rule == "path":
        assert differs_in_every_order(rule, "goal_in_a_corner", halo_corners=False)


# ---------------------------------------------------------------------------------------------- the steady batch

@pytest.mark.parametrize("rule", RULES)
def test_the_long_walk_needs_twice_the_sweeps_that_enter_the_steady_batch(rule):
    """More than 4 + 8 + 16 = 28 sweeps enter the batches of 32, whose count comes back from the last of 32 counters.  The model, in its
    fastest order, needs 56 or more.  The device's rounds are in place, not Jacobi, so it can be faster, but not by much: the walk runs
    along rows, a row's cells are lanes of one wave in lockstep, so the news moves one cell a round along it and at most 64 cells a
    sweep in a block; only at a row's end, where it changes rows and may change waves, can a round carry it further.  The walk is
    68 x 64 cells long (the maze: 72 x 64), and no block order lets a sweep do the work of two blocks on rows of one block's width"""
    name = "maze" if rule == "path" else "long_walk"
    quiet = [model(rule, name, order)[1].quiet for order in R.ORDERS]
    assert min(quiet) >= 2 * 28, (rule, quiet)
    assert all(model(rule, name, order)[1].sweeps > 28 + R.BATCH_MAX - 1 for order in R.ORDERS)

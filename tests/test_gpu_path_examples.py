"""examples/pathfinding.py: every route it prints ends at the goal, its cost is the field's value at its start added up again along the
route, and --ppm draws the routes"""
import re

import numpy as np
import pytest

from test_gpu_render_examples import run

pytestmark = pytest.mark.gpu


def test_the_routes_end_at_the_goal_and_cost_what_the_field_says(tmp_path):
    picture = str(tmp_path / "routes.ppm")
    out = run("pathfinding.py", "--texture-size", "32", "--lods", "3", "--ppm", picture)
    size = 28 * 4
    goal = re.search(r"field of (\d+) x \1 cells towards goal \((\d+), (\d+)\): (\d+) reachable", out)
    assert goal and int(goal.group(1)) == size and int(goal.group(4)) > size * size // 2, out
    gx, gy = int(goal.group(2)), int(goal.group(3))
    routes = re.findall(r"route from \((\d+), (\d+)\): (\w+), (\d+) cells, ([0-9.]+) long, ends at \((\d+), (\d+)\), cost (\S+), added up along the route (\S+)", out)
    assert len(routes) == 3, out
    for sx, sy, status, cells, length, ex, ey, cost, added in routes:
        assert status == "ok" and (int(ex), int(ey)) == (gx, gy), out
        assert cost == added and np.isfinite(float(cost)) and float(cost) >= float(length) > 0.0, out  # every weight is at least the step's length
        assert int(cells) >= max(abs(int(sx) - gx), abs(int(sy) - gy)) + 1
    data = open(picture, "rb").read()
    header = b"P6\n%d %d\n255\n" % (size, size)
    assert data.startswith(header) and len(data) == len(header) + size * size * 3
    rgb = np.frombuffer(data[len(header):], np.uint8).reshape(size, size, 3)
    assert (rgb[gy, gx] == 255).all() and (rgb == (255, 80, 60)).all(axis=2).sum() >= int(routes[0][3]) - 9  # the first route, less what the goal's square covers

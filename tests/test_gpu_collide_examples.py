"""examples/collision.py: every ball it drops and slides comes to rest on the ground, touching it or within the example's slack of it"""
import re

import pytest

from test_gpu_render_examples import run

pytestmark = pytest.mark.gpu


def test_every_ball_comes_to_rest_on_the_ground():
    out = run("collision.py", "--texture-size", "32", "--lods", "3", "--grid", "5", "--slides", "3")
    head = re.search(r"dropped (\d+) balls of radius (\S+) and slid each 3 times; slack (\S+)", out)
    assert head and int(head.group(1)) == 25, out
    radius, slack = float(head.group(2)), float(head.group(3))
    assert 0.0 < slack <= radius / 100.0
    balls = re.findall(r"ball (\d+): landed at \((\S+), (\S+), (\S+)\), rests at \((\S+), (\S+), (\S+)\), slid (\S+), (\w+), depth (\S+), normal \((\S+), (\S+), (\S+)\)", out)
    assert len(balls) == 25, out
    slid = 0
    for ball in balls:
        assert ball[8] in ("touching", "none") and abs(float(ball[9])) < slack, ball
        assert float(ball[5].rstrip(",")) <= float(ball[2].rstrip(",")) + slack, ball  # a ball never ends higher than it landed
        assert float(ball[11].rstrip(",")) > 0.0, ball  # the ground faces up
        slid += float(ball[7].rstrip(",")) > 0.01
    assert slid >= 5, out  # the terrain is not flat: balls slide

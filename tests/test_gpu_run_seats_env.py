"""SeatEnv.step_until (-m gpu): 30 steps of the learner's loop with random_legal against an oracle twin, under restart.  Each step's
actions are copied to the host only to drive the twin, which does Oracle.inject, then tests/run_seats_ref.py, then
tests/observe_ref.py; after every step obs, done, won, played and stopped equal the twin's, and over the run a finished game is
observed (done = 1) in a room whose `games` then rises - the end a fused step hides.  A mixed batch and Werewolf x 8, one seat and
two.  The scenarios run in tests/run_seats_env_child.py, one process for all of them that imports torch before it loads the
library; each test here reads its scenario's verdict from that process's report."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LOOPS = [("mixed", [1]), ("mixed", [3, 1]), ("ww8_h1", [1]), ("ww8_h1", [1, 5])]


@pytest.fixture(scope="module")
def report():
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(HERE, "run_seats_env_child.py")]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("name,seats", LOOPS)
def test_step_until_equals_the_oracle_twin_and_shows_every_end(report, name, seats):
    assert report[f"until-{name}-{'+'.join(map(str, seats))}"] == "ok"

"""SeatEnv.teach (-m gpu): 12 steps of a seat that plays its playout-best choice, env.step(advice_fields(env.teach(64, 48))["best"]),
with nothing crossing to the host but what the test itself reads.  At every step env.advice equals batch.advise_seats of the same
pairs, the fields are views into env.advice, best is 0 exactly where nothing is legal and no choice is refused; over the run some
action was applied and some room finished.  Werewolf x 8 and a mixed batch with restart, one seat and two.  The scenarios run in
tests/teach_env_child.py, one process that imports torch before it loads the library (tests/test_gpu_seat_env.py says why)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LOOPS = [("ww8_h1", [1]), ("ww8_h1", [1, 5]), ("mixed", [1]), ("mixed", [3, 1])]


@pytest.fixture(scope="module")
def report():
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(HERE, "teach_env_child.py")]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("name,seats", LOOPS)
def test_a_seat_that_plays_its_best_choice(report, name, seats):
    assert report[f"best-{name}-{'+'.join(map(str, seats))}"] == "ok"

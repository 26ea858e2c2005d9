"""SeatEnv (-m gpu): 40 steps of the learner's loop with random_legal against an oracle twin.  Each step's actions are copied to
the host only to drive the twin, which does Oracle.inject, then the oracle's turns, then tests/observe_ref.py; after every step
obs, done and won equal the twin's.  A mixed batch and Werewolf x 8 with restart, one seat and two, single turns and three fused
turns per step; and random_legal itself: never an illegal choice, 0 exactly where nothing is legal, uniform over the legal ones.
The scenarios run in tests/seat_env_child.py, one process for all of them that imports torch before it loads the library (torch
brings its own HIP runtime; the suite's process has loaded the library's by the time these tests run); each test here reads its
scenario's verdict from that process's report."""
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
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(HERE, "seat_env_child.py")]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("n_turns", [1, 3])
@pytest.mark.parametrize("name,seats", LOOPS)
def test_the_loop_equals_the_oracle_twin(report, name, seats, n_turns):
    assert report[f"loop-{name}-{'+'.join(map(str, seats))}-{n_turns}"] == "ok"


def test_fields_are_views_and_random_legal_is_uniform_over_the_legal_choices(report):
    assert report["fields"] == "ok"

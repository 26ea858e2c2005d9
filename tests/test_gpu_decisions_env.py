"""SeatEnv.decisions / step_decisions (-m gpu): self-play through decision lists (POLICY.md §3q) - every seat listed and
host-driven, 40 iterations of step_decisions with random_legal over all rows of the list, on Werewolf x 8 and on a mixed batch -
beside a twin SeatEnv driven through step_until with the dense actions the list implies: after every iteration the records agree,
the list equals the filter of the twin's dense obs, played / stopped and the statuses agree; and a smaller cap truncates the list
and still counts it.  The scenarios run in tests/decisions_env_child.py, one process that imports torch before it loads the
library (see tests/test_gpu_seat_env.py); each test here reads its scenario's verdict from that process's report."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def report():
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(HERE, "decisions_env_child.py")]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("kind", ["ww8", "mixed"])
def test_self_play_through_the_list_equals_the_dense_twin(report, kind):
    assert report[f"self-play-{kind}"] == "ok"


def test_a_smaller_cap_truncates_the_list_and_still_counts_it(report):
    assert report["cap"] == "ok"

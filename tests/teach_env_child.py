"""The torch side of tests/test_gpu_teach_env.py, run as a process of its own for the reason tests/seat_env_child.py gives: torch is
imported here before the library is loaded.  Runs every scenario, prints one JSON line {scenario id: "ok" or what went wrong}."""
import json
import os
import sys
import traceback

import torch  # noqa: F401  (first: see above)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
import numpy as np  # noqa: E402

from game_engine_amd import SeatEnv  # noqa: E402
from game_engine_amd.stepper import ADVICE_DTYPE  # noqa: E402
from observe_ref import make_batch  # noqa: E402
from run_ref import case_inputs  # noqa: E402
from teach_ref import PER, differing, expected  # noqa: E402

STEPS = 12
N_ROLLOUTS, MAX_TURNS = 64, 48
LOOPS = [("ww8_h1", [1]), ("ww8_h1", [1, 5]), ("mixed", [1]), ("mixed", [3, 1])]


def a_seat_that_plays_its_best_choice(name, seats):
    segs = case_inputs(name, PER, True)[0]
    acted = finished = 0
    with make_batch(segs, True) as b:
        env = SeatEnv(b, seats)
        env.observe()
        assert env.advice is None
        for step in range(STEPS):
            advice = env.teach(N_ROLLOUTS, MAX_TURNS)
            assert advice is env.advice and advice.shape == (b.n_rooms, len(seats), 224) and advice.dtype == torch.uint8 and advice.is_cuda
            f = SeatEnv.advice_fields(advice)
            base, end = advice.data_ptr(), advice.data_ptr() + advice.numel()
            for key, t in f.items():
                assert base <= t.data_ptr() < end, key + " is a copy"
                assert t.shape == ((b.n_rooms, len(seats), 12) if key in ("finished", "wins", "score") else (b.n_rooms, len(seats))), key
            got = advice.cpu().numpy().reshape(-1).view(ADVICE_DTYPE)
            want = expected(b, 0, b.n_rooms, seats, N_ROLLOUTS, MAX_TURNS)
            assert got.tobytes() == want.tobytes(), (name, seats, step, differing(got, want))
            for key, col in (("status", want["status"]), ("legal_bits", want["legal"]), ("best", want["best"]), ("phase_id", want["phase_id"]),
                             ("policy_wins", want["policy"]["wins"]), ("policy_score", want["policy"]["score"]),
                             ("policy_finished", want["policy"]["finished"]), ("finished", want["option"]["finished"]),
                             ("wins", want["option"]["wins"]), ("score", want["option"]["score"])):
                assert np.array_equal(f[key].cpu().numpy().reshape(col.shape).astype(np.int64), col.astype(np.int64)), key
            assert bool(((f["best"] == 0) == (f["legal_bits"] == 0)).all())
            best = f["best"].cpu().numpy()
            obs, done, won = env.step(f["best"])
            assert not bool(env.status.any()), "a playout-best choice was refused"
            acted += int((best != 0).sum())
            finished += int(done.sum())
        assert acted > 0 and finished > 0, (acted, finished)


def main():
    report = {}
    for name, seats in LOOPS:
        key = f"best-{name}-{'+'.join(map(str, seats))}"
        try:
            a_seat_that_plays_its_best_choice(name, seats)
            report[key] = "ok"
        except Exception:                                        # an assertion of the scenario, or an error of the library
            report[key] = traceback.format_exc()[-3000:]
    print(json.dumps(report))


if __name__ == "__main__":
    main()

"""The torch side of tests/test_gpu_run_seats_env.py, run as a process of its own that imports torch before the library is loaded
(tests/seat_env_child.py says why).  Runs every scenario, prints one JSON line {scenario id: "ok" or what went wrong}."""
import json
import os
import sys
import traceback

import torch  # noqa: F401  (first: see above)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
import numpy as np  # noqa: E402

from game_engine_amd import SeatEnv  # noqa: E402
from game_engine_amd.stepper import SEAT_OBS_DTYPE  # noqa: E402
from observe_ref import differing_fields, make_batch, observe_batch  # noqa: E402
from run_ref import case_inputs  # noqa: E402
from run_seats_ref import END, SEAT, run_seats_ref  # noqa: E402
from seats_ref import segment_masks  # noqa: E402

PER = {"ww8_h1": 67, "mixed": 35}      # rooms per segment: a full wavefront and a tail of 3; four part wavefronts (the twin's time)
STEPS = 30
MAX_TURNS = 16
LOOPS = [("mixed", [1]), ("mixed", [3, 1]), ("ww8_h1", [1]), ("ww8_h1", [1, 5])]


def _records(obs):
    return obs.cpu().numpy().reshape(-1).view(SEAT_OBS_DTYPE).reshape(obs.shape[0], obs.shape[1])


def _twin_inject(segs, rooms, seats, actions):
    base = 0
    for (orc, _, _, _, _), seg_rooms in zip(segs, rooms):
        for i in range(len(seg_rooms)):
            for j, seat in enumerate(seats):
                c = int(actions[base + i, j])
                if c:
                    assert orc.inject(seg_rooms, i, seat, c), "random_legal chose what the oracle refuses"
        base += len(seg_rooms)


def loop_equals_the_oracle_twin(name, seats):
    """step_until with random_legal against a twin that does Oracle.inject, run_seats_ref, observe_ref: after every step obs, done,
    won, played and stopped equal the twin's; and an end is seen - done = 1 in a room whose `games` then rises."""
    segs = case_inputs(name, PER[name], True)[0]
    rooms = [s[4].copy() for s in segs]
    masks = segment_masks(segs)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(len(name) + len(seats))
    acted = ends_seen = 0
    with make_batch(segs, True, max_fuse=0) as b:
        env = SeatEnv(b, seats)
        obs = env.observe()
        assert env.played is None and env.stopped is None
        for step in range(STEPS):
            actions = SeatEnv.random_legal(obs, gen)
            host_actions = actions.cpu().numpy()
            was = _records(obs)
            turn = b.turn
            obs, done, won = env.step_until(actions, MAX_TURNS)
            assert b.turn == turn + MAX_TURNS
            _twin_inject(segs, rooms, seats, host_actions)
            played, stopped = run_seats_ref(segs, rooms, masks, seats, turn, MAX_TURNS, SEAT | END, True)
            want = observe_batch([(s[0], r) for s, r in zip(segs, rooms)], seats)
            got = _records(obs)
            what = (name, seats, step)
            assert got.tobytes() == want.tobytes(), (what, differing_fields(got, want))
            assert np.array_equal(done.cpu().numpy(), want["done"] != 0) and np.array_equal(won.cpu().numpy(), want["won"] != 0)
            assert env.played.dtype == torch.int32 and env.played.shape == (b.n_rooms,) and env.stopped.shape == (b.n_rooms,)
            assert np.array_equal(env.played.cpu().numpy(), played.astype(np.int32)), what
            assert np.array_equal(env.stopped.cpu().numpy(), stopped.astype(np.int32)), what
            assert not env.status.any()
            # what the observation says is what the stop bits say: every entry is a decision point, a finished game or the limit
            assert np.array_equal((stopped & SEAT) != 0, (want["legal"] != 0).any(axis=1)), what
            assert np.array_equal((stopped & END) != 0, want["done"][:, 0] != 0), what
            assert ((stopped != 0) | (played == MAX_TURNS)).all()
            acted += int((host_actions != 0).sum())
            ends_seen += int(((was["done"][:, 0] != 0) & (want["games"][:, 0] > was["games"][:, 0])).sum())
        assert acted > 0 and ends_seen > 0, (acted, ends_seen)


def main():
    report = {}
    for name, seats in LOOPS:
        key = f"until-{name}-{'+'.join(map(str, seats))}"
        try:
            loop_equals_the_oracle_twin(name, seats)
            report[key] = "ok"
        except Exception:                                        # an assertion of the scenario, or an error of the library
            report[key] = traceback.format_exc()[-3000:]
    print(json.dumps(report))


if __name__ == "__main__":
    main()

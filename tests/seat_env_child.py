"""The torch side of tests/test_gpu_seat_env.py, run as a process of its own: torch brings a HIP runtime of its own, and a process can
drive the GPU through one runtime only, so torch is imported here before the library is loaded (game_engine_amd/env.py) - which
the suite's own process, whose other tests load the library first, cannot promise.  Runs every scenario, prints one JSON line
{scenario id: "ok" or what went wrong}."""
import json
import os
import sys
import traceback

import torch  # noqa: F401  (first: see above)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
import numpy as np  # noqa: E402

from game_engine_amd import GameTable, RoomBatch, SeatEnv  # noqa: E402
from game_engine_amd.stepper import SEAT_OBS_DTYPE  # noqa: E402
from observe_ref import differing_fields, make_batch, observe_batch  # noqa: E402
from run_ref import SEED, case_inputs, dsl_of  # noqa: E402

PER = 67                               # rooms per segment: a full wavefront and a tail of 3
FIRST_ROOM = 777                       # observe_ref.make_batch
STEPS = 40
LOOPS = [("mixed", [1]), ("mixed", [3, 1]), ("ww8_h1", [1]), ("ww8_h1", [1, 5])]


def _records(obs):
    return obs.cpu().numpy().reshape(-1).view(SEAT_OBS_DTYPE).reshape(obs.shape[0], obs.shape[1])


def _twin_step(segs, rooms, seats, actions, turn, n_turns, restart):
    base = 0
    for (orc, _, _, mask, _), seg_rooms in zip(segs, rooms):
        for i in range(len(seg_rooms)):
            for j, seat in enumerate(seats):
                c = int(actions[base + i, j])
                if c:
                    assert orc.inject(seg_rooms, i, seat, c), "random_legal chose what the oracle refuses"
        orc.run(seg_rooms, SEED, FIRST_ROOM + base, turn, n_turns, threads=1, restart=restart, human_mask=mask)
        base += len(seg_rooms)


def loop_equals_the_oracle_twin(name, seats, n_turns):
    segs = case_inputs(name, PER, True)[0]
    rooms = [s[4].copy() for s in segs]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(len(name) + n_turns)
    acted = finished = 0
    with make_batch(segs, True, max_fuse=0) as b:
        env = SeatEnv(b, seats)
        obs = env.observe()
        assert obs.shape == (b.n_rooms, len(seats), 192) and obs.dtype == torch.uint8 and obs.is_cuda
        want = observe_batch([(s[0], r) for s, r in zip(segs, rooms)], seats)
        assert _records(obs).tobytes() == want.tobytes()
        for step in range(STEPS):
            f = SeatEnv.fields(obs)
            actions = SeatEnv.random_legal(obs, gen)
            legal = f["legal"]
            chosen = torch.gather(torch.cat([torch.zeros_like(legal[..., :1]), legal], -1), -1, actions.long().unsqueeze(-1)).squeeze(-1)
            assert bool(((actions == 0) == ~legal.any(-1)).all()) and bool((chosen | (actions == 0)).all())
            host_actions = actions.cpu().numpy()
            obs, done, won = env.step(actions, n_turns)
            _twin_step(segs, rooms, seats, host_actions, b.turn - n_turns, n_turns, True)
            want = observe_batch([(s[0], r) for s, r in zip(segs, rooms)], seats)
            got = _records(obs)
            assert got.tobytes() == want.tobytes(), (name, seats, n_turns, step, differing_fields(got, want))
            assert np.array_equal(done.cpu().numpy(), want["done"] != 0) and np.array_equal(won.cpu().numpy(), want["won"] != 0)
            assert not env.status.any()
            acted += int((host_actions != 0).sum())
            finished += int(want["done"].sum())
        assert acted > 0 and finished > 0, (acted, finished)


def fields_are_views_and_random_legal_is_uniform():
    dsl_ww = dsl_of("ww")
    with RoomBatch([(GameTable(dsl_ww), 8, 4096, 1)], seed=3, restart=True) as b:
        env = SeatEnv(b, [1])
        b.step(12)
        obs = env.observe()
        f = SeatEnv.fields(obs)
        base, end = obs.data_ptr(), obs.data_ptr() + obs.numel()
        for name, t in f.items():
            if name != "legal":
                assert base <= t.data_ptr() < end, name + " is a copy"
        assert f["legal"].shape == (4096, 1, 12) and f["legal"].dtype == torch.bool
        assert f["players"].shape == (4096, 1, 12, 12) and f["det"].shape == (4096, 1, 12)
        views = b.read_rooms()
        assert np.array_equal(f["phase_id"].cpu().numpy()[:, 0], views["phase_id"])
        assert np.array_equal(f["players"].cpu().numpy()[:, 0, :8, 2], views["players"][:, :8, 2])      # is_alive is public
        legal = f["legal"][:, 0]
        waiting = legal.any(-1)
        assert bool(waiting.any()) and bool((~waiting).any())
        counts = torch.zeros(12, device="cuda")
        for _ in range(64):
            a = SeatEnv.random_legal(obs)[:, 0]
            assert bool((a[~waiting] == 0).all()) and bool((a[waiting] > 0).all())
            assert bool(legal[waiting].gather(-1, (a[waiting] - 1).long().unsqueeze(-1)).all())
            counts += torch.bincount((a[waiting] - 1).long(), minlength=12).float()
        expect = (legal[waiting].float() / legal[waiting].sum(-1, keepdim=True)).sum(0) * 64
        # a choice's count is a sum of independent draws: within six standard deviations (sd <= sqrt(expect)) of its mean
        assert bool(((counts - expect).abs() <= 6 * expect.sqrt() + 1).all()), (counts.tolist(), expect.tolist())


def main():
    report = {}
    scenarios = [(f"loop-{name}-{'+'.join(map(str, seats))}-{k}", lambda name=name, seats=seats, k=k: loop_equals_the_oracle_twin(name, seats, k))
                 for name, seats in LOOPS for k in (1, 3)]
    scenarios.append(("fields", fields_are_views_and_random_legal_is_uniform))
    for key, run in scenarios:
        try:
            run()
            report[key] = "ok"
        except Exception:                                        # an assertion of the scenario, or an error of the library
            report[key] = traceback.format_exc()[-3000:]
    print(json.dumps(report))


if __name__ == "__main__":
    main()

"""The torch side of tests/test_gpu_decisions_env.py, run as a process of its own that imports torch before the library is loaded
(see tests/seat_env_child.py).  Self-play through decision lists (POLICY.md §3q): every seat listed and host-driven, 40
iterations of SeatEnv.step_decisions with random_legal over all cap rows of the list, beside a twin SeatEnv driven through
step_until with the dense actions the list implies.  After every iteration the records agree, the list equals the filter
(tests/gather_ref.py) of the twin's dense obs, and played / stopped agree.  Prints one JSON line {scenario: "ok" or what went wrong}."""
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
from gather_ref import END, SEAT, gather  # noqa: E402
from observe_ref import differing_fields  # noqa: E402
from run_ref import dsl_of  # noqa: E402

PER = 135                              # rooms per segment: two full wavefronts and a tail of 7
ITERATIONS = 40
SCENARIOS = ["ww8", "mixed"]


def make(kind):
    """Werewolf x 8 with all eight seats listed and host-driven; a mixed batch (Werewolf x 8, Two-Truths x 4, Werewolf x 12) with
    the four seats every segment has"""
    ww, tt = GameTable(dsl_of("ww")), GameTable(dsl_of("tt"))
    n_seats = 8 if kind == "ww8" else 4
    mask = (1 << n_seats) - 1
    segs = [(ww, 8, PER, mask)] if kind == "ww8" else [(ww, 8, PER, mask), (tt, 4, PER, mask), (ww, 12, PER, mask)]
    return RoomBatch(segs, seed=77, first_room=900, restart=True), list(range(1, n_seats + 1))


def assert_list_is_the_filter(dec, dense_obs, what):
    dec_obs, dec_entries, dec_n = (t.cpu().numpy() for t in dec)
    dense = dense_obs.cpu().numpy().reshape(-1).view(SEAT_OBS_DTYPE).reshape(dense_obs.shape[0], dense_obs.shape[1])
    ref, ref_e, ref_n = gather(dense, SEAT | END)
    assert list(dec_n) == list(ref_n), (what, list(dec_n), list(ref_n))
    k = int(ref_n[0])
    assert np.array_equal(dec_entries[:k], ref_e.astype(np.int32)), what
    got = dec_obs[:k].reshape(-1).view(SEAT_OBS_DTYPE)
    assert got.tobytes() == ref.tobytes(), (what, differing_fields(got, ref))
    return k, int((ref["done"] != 0).sum())


def self_play(kind):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(len(kind))
    (b, seats), (b2, _) = make(kind), make(kind)
    with b, b2:
        env, twin = SeatEnv(b, seats), SeatEnv(b2, seats)
        cap = b.n_rooms * len(seats)
        dec = env.decisions()
        assert dec[0].shape == (cap, 192) and dec[0].dtype == torch.uint8 and dec[1].shape == (cap,) and dec[1].dtype == torch.int32
        assert dec[2].shape == (2,) and dec[2].dtype == torch.int32 and all(t.is_cuda for t in dec)
        assert_list_is_the_filter(dec, twin.observe(), (kind, "start"))
        listed = finished = acted = 0
        for it in range(ITERATIONS):
            dec_obs, dec_entries, dec_n = dec
            choices = SeatEnv.random_legal(dec_obs, gen)          # over all cap rows: stale rows get choices too, and are ignored
            n = int(dec_n[0])
            dense = torch.zeros(cap, dtype=torch.int32, device=dec_obs.device)
            played_from = dec_entries[:n].long()                  # (a copy: step_decisions writes the next list over this one)
            dense[played_from] = choices[:n]
            acted += int((choices[:n] != 0).sum())
            dec = env.step_decisions(choices)
            twin_obs, _, _ = twin.step_until(dense.view(b.n_rooms, len(seats)))
            torch.cuda.synchronize()
            what = (kind, it)
            assert b.read_rooms().tobytes() == b2.read_rooms().tobytes(), what
            k, done = assert_list_is_the_filter(dec, twin_obs, what)
            assert torch.equal(env.played, twin.played) and torch.equal(env.stopped, twin.stopped), what
            assert torch.equal(env.dec_status[:n], twin.status.reshape(-1)[played_from]), what
            assert b.turn == b2.turn
            listed += k
            finished += done
        assert 0 < listed < ITERATIONS * cap and finished > 0 and acted > 0, (listed, finished, acted)


def a_smaller_cap_truncates_and_counts():
    (b, seats) = make("ww8")
    with b:
        env = SeatEnv(b, seats)
        env.decisions()
        env.step_decisions(torch.zeros(b.n_rooms * len(seats), dtype=torch.int32))   # on to the first phase that waits for its seats
        full = [t.clone() for t in env.decisions()]
        m = int(full[2][1])
        assert m > 7 and int(full[2][0]) == m
        obs, entries, n = env.decisions(cap=7)
        assert obs.shape == (7, 192) and n.tolist() == [7, m]
        assert torch.equal(entries, full[1][:7]) and torch.equal(obs, full[0][:7])
        obs, entries, n = env.decisions(want="end")
        assert n.tolist() == [0, 0] and obs.shape[0] == b.n_rooms * len(seats)     # no game has ended at the start


def main():
    report = {}
    scenarios = [(f"self-play-{kind}", lambda kind=kind: self_play(kind)) for kind in SCENARIOS]
    scenarios.append(("cap", a_smaller_cap_truncates_and_counts))
    for key, run in scenarios:
        try:
            run()
            report[key] = "ok"
        except Exception:                                        # an assertion of the scenario, or an error of the library
            report[key] = traceback.format_exc()[-3000:]
    print(json.dumps(report))


if __name__ == "__main__":
    main()

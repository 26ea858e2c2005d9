#!/usr/bin/env python3
"""Playouts per second of ge_batch_rollout_rooms (RoomBatch.rollout_rooms) against the composition it is defined by (a fresh
batch of R copies: create + write_rooms + set_turn + step(M) + summary + destroy), median wall time of synchronised calls
after a warm-up.  Simulated room-turns come from the playouts' own end turns (endTurnSum: an ended playout counts the turns
up to its end, an unfinished one counts M), so the early exit of finished wavefronts is not counted as work.
python tools/rollout_probe.py [repeats]   (kernel times: run it under rocprofv3 --kernel-trace --stats)"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from game_engine_amd import GameTable, RoomBatch, RoomPoolService  # noqa: E402
from game_engine_amd.stepper import rollout_to_dict  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
M = 1024


def dsl_of(game):
    with open(os.path.join(ROOT, "tests", "golden", "dsl", f"{game}.json"), encoding="utf-8") as f:
        return json.load(f)


def median_s(fn, reps=REPS):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def room_turns(words, turn0, M):
    """simulated room-turns of the playouts of one entry: ended playouts up to their end turn, the others all M turns"""
    d = rollout_to_dict(words)["summary"]
    ended = sum(d["end_turn_hist"])
    return d["sum_end_turn"] - ended * (turn0 - 1) + (d["rooms"] - ended) * M


def line(what, secs, playouts, turns):
    print(f"{what:58s} {secs * 1e3:9.3f} ms  {playouts / secs / 1e6:9.3f} M playouts/s  {turns / secs / 1e9:8.3f} G room-turns/s", flush=True)
    return {"what": what, "ms": round(secs * 1e3, 3), "playouts_per_s": round(playouts / secs), "room_turns_per_s": round(turns / secs)}


results = []
ww = GameTable(dsl_of("werewolf-(mafia)"))
with RoomBatch([(ww, 8, 1)], seed=3, first_room=7) as src:
    for turn0 in (0, 9):
        if turn0:
            src.step(turn0)                                   # a mid-game position (roles dealt, first night played)
        for R in (4096, 65536, 1 << 20):
            w = src.rollout_rooms([0], [1 << 20], [turn0], R, M)[0]
            t = median_s(lambda: src.rollout_rooms([0], [1 << 20], [turn0], R, M))
            results.append(line(f"Werewolf x 8, turn {turn0}, R = {R}: rollout_rooms", t, R, room_turns(w, turn0, M)))
        view = src.read_rooms(0, 1)
        R = 65536
        w = src.rollout_rooms([0], [1 << 20], [turn0], R, M)[0]

        def composition():
            with RoomBatch([(ww, 8, R, 0)], seed=3, first_room=1 << 20) as c:
                c.write_rooms(0, np.repeat(view, R))
                c.set_turn(turn0)
                c.step(M)
                return c.summary_words()

        assert (composition() == w[:41]).all()
        t = median_s(composition)
        results.append(line(f"Werewolf x 8, turn {turn0}, R = {R}: composition", t, R, room_turns(w, turn0, M)))

# 1 024 pooled threads x 1 024 playouts in one call
pool = RoomPoolService(seed=3, chunk_rooms=1024)
tids = [f"thread-{i}" for i in range(1024)]
dsl = dsl_of("werewolf-(mafia)")
for t in tids:
    pool.create_room(t, "werewolf-(mafia)", [{"name": f"P{i + 1}"} for i in range(8)], dsl=dsl)
for k in range(12):
    pool.handle_messages([(t, "Continue") for t in tids[: 1024 - 64 * k]])
out = pool.forecasts(tids, n_rollouts=1024, max_turns=M)
turns = sum(o["endTurnSum"] - o["ended"] * (o["turn"] - 1) + (o["rollouts"] - o["ended"]) * M for o in out)
t = median_s(lambda: pool.forecasts(tids, n_rollouts=1024, max_turns=M))
results.append(line("1 024 pooled Werewolf x 8 threads x 1 024: forecasts", t, 1024 * 1024, turns))
pool.close()

tt = GameTable(dsl_of("two-truths-and-a-lie"))
with RoomBatch([(tt, 4, 1)], seed=3, first_room=7) as src:
    for R in (4096, 65536, 1 << 20):
        w = src.rollout_rooms([0], [1 << 20], [0], R, M)[0]
        t = median_s(lambda: src.rollout_rooms([0], [1 << 20], [0], R, M))
        results.append(line(f"Two-Truths x 4, turn 0, R = {R}: rollout_rooms", t, R, room_turns(w, 0, M)))
    view = src.read_rooms(0, 1)
    R = 65536

    def composition_tt():
        with RoomBatch([(tt, 4, R, 0)], seed=3, first_room=1 << 20) as c:
            c.write_rooms(0, np.repeat(view, R))
            c.set_turn(0)
            c.step(M)
            return c.summary_words()

    w = src.rollout_rooms([0], [1 << 20], [0], R, M)[0]
    assert (composition_tt() == w[:41]).all()
    t = median_s(composition_tt)
    results.append(line(f"Two-Truths x 4, turn 0, R = {R}: composition", t, R, room_turns(w, 0, M)))
print(json.dumps({"max_turns": M, "repeats": REPS, "results": results}))

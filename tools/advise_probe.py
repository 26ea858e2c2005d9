#!/usr/bin/env python3
"""Wall time of advise (RoomService.advise / RoomPoolService.advises: one ge_batch_rollout_actions call for every choice of a seat
plus the policy's) against the same answers got by separate calls: one forecast-sized rollout_rooms per option, and the
composition (per option a fresh batch of R copies: create + write_rooms + inject_actions + set_turn + step(M) + summary + destroy).
Median wall time of synchronised calls after a warm-up.
python tools/advise_probe.py [repeats]          the wall-time table
python tools/advise_probe.py kernels [repeats]  only rollout_rooms (ACT = 0) and rollout_actions (ACT = 1) at equal R, for a run
                                                under rocprofv3 --kernel-trace --stats"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from game_engine_amd import GameTable, RoomBatch, RoomPoolService, RoomService  # noqa: E402
from game_engine_amd.room_service import forecast_key, forecast_seed  # noqa: E402

KERNELS = len(sys.argv) > 1 and sys.argv[1] == "kernels"
args = sys.argv[2:] if KERNELS else sys.argv[1:]
REPS = int(args[0]) if args else 20
M, R = 1024, 4096


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


def line(what, secs, playouts):
    print(f"{what:66s} {secs * 1e3:9.3f} ms  {playouts / secs / 1e6:9.3f} M playouts/s", flush=True)
    return {"what": what, "ms": round(secs * 1e3, 4), "playouts_per_s": round(playouts / secs)}


dsl = dsl_of("werewolf-(mafia)")
ww = GameTable(dsl)
players = [{"name": f"P{i + 1}", "isBot": i != 0} for i in range(8)]
svc = RoomService(seed=3)
svc.create_room("t", "werewolf-(mafia)", players, dsl=dsl, room_index=7)
for _ in range(60):                                        # up to a phase where seat 1 has about 8 choices (a day vote)
    a = svc.advise("t", n_rollouts=64, max_turns=8)
    if len(a["options"]) >= 7 and "vote" in svc._rooms["t"]["log"].agent_state(svc._rooms["t"]["view"])["current_phase_name"].lower():
        break
    svc.continue_room("t")
room = svc._rooms["t"]
turn, view, key, seed = room["batch"].turn, room["view"], forecast_key(room["key"]), forecast_seed(svc.seed)
a = svc.advise("t", n_rollouts=R, max_turns=M)
opts = [o["choice"] for o in a["options"]]
phase = room["log"].agent_state(view)["current_phase_name"]
results = []

if KERNELS:
    # equal R, the same room: ACT = 0 (rollout_rooms), ACT = 1 with no action, ACT = 1 with one action per entry
    b = room["batch"]
    for _ in range(REPS):
        b.rollout_rooms([0], [key], [turn], 65536, M, seed=seed)
        b.rollout_actions([0], [key], [turn], [[]], 65536, M, seed=seed)
        b.rollout_actions([0], [key], [turn], [[(1, opts[0])]], 65536, M, seed=seed)
        b.rollout_actions([0] * 9, [key] * 9, [turn] * 9, [[(1, c)] for c in range(1, 9)] + [[]], R, M, seed=seed)
        b.rollout_rooms([0] * 9, [key] * 9, [turn] * 9, R, M, seed=seed)
    print(json.dumps({"kernels": True, "repeats": REPS, "turn": turn, "phase": phase, "options": opts}))
    sys.exit(0)

n_ent = len(opts) + 1
t = median_s(lambda: svc.advise("t", n_rollouts=R, max_turns=M))
results.append(line(f"Werewolf x 8 '{phase}', {len(opts)} options + policy, R = {R}: advise", t, n_ent * R))
t = median_s(lambda: [svc.forecast("t", n_rollouts=R, max_turns=M) for _ in range(9)])
results.append(line(f"  the same work as 9 separate forecast calls (no actions)", t, 9 * R))


def composition():
    out = []
    for c in opts + [None]:
        with RoomBatch([(ww, 8, R, 0)], seed=seed, first_room=key) as cb:
            cb.write_rooms(0, np.repeat(view, R))
            if c is not None:
                assert (cb.inject_actions(list(range(R)), [1] * R, [c] * R) == 0).all()
            cb.set_turn(turn)
            cb.step(M)
            out.append(cb.summary_words())
    return out


words, status = room["batch"].rollout_actions([0] * n_ent, [key] * n_ent, [turn] * n_ent, [[(1, c)] for c in opts] + [[]], R, M, seed=seed)
assert (status == 0).all() and all((w[:41] == c).all() for w, c in zip(words, composition()))
t = median_s(composition, reps=max(3, REPS // 4))
results.append(line(f"  the composition ({n_ent} fresh batches: write, inject, set_turn, step, summary)", t, n_ent * R))
svc.close()

# 1 024 pooled threads, each advised for its human seat
pool = RoomPoolService(seed=3, chunk_rooms=1024)
tids = [f"thread-{i}" for i in range(1024)]
for tid in tids:
    pool.create_room(tid, "werewolf-(mafia)", players, dsl=dsl)
for k in range(12):
    pool.handle_messages([(tid, "Continue") for tid in tids[: 1024 - 64 * k]])
out = pool.advises(tids, n_rollouts=1024, max_turns=M)
entries = sum(len(o["options"]) for o in out)
t = median_s(lambda: pool.advises(tids, n_rollouts=1024, max_turns=M), reps=max(3, REPS // 4))
results.append(line(f"1 024 pooled Werewolf x 8 threads x 1 024 (9 entries each, {entries} options): advises", t, 9 * 1024 * 1024))
pool.close()
print(json.dumps({"max_turns": M, "repeats": REPS, "turn": turn, "results": results}))

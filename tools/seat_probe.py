#!/usr/bin/env python3
"""Wall time of playouts from a seat's view (ge_batch_rollout_seats, POLICY.md §3c) against the full view: advise(view="seat")
vs advise() at the shapes of tools/advise_probe.py, and 65 536-playout forecasts per layout from a Villager's / non-speaker's
view (every hidden tuple re-dealt) vs the full view (rollout_rooms) and vs seat 0 of rollout_seats (the ACT = 2 kernel without
its re-deal).  Median wall time of synchronised calls after a warm-up.
python tools/seat_probe.py [repeats]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from game_engine_amd import GameTable, RoomBatch, RoomPoolService, RoomService  # noqa: E402
from game_engine_amd.room_service import forecast_key, forecast_seed  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
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
    print(f"{what:72s} {secs * 1e3:9.3f} ms  {playouts / secs / 1e6:9.3f} M playouts/s", flush=True)
    return {"what": what, "ms": round(secs * 1e3, 4), "playouts_per_s": round(playouts / secs)}


results = []
dsl = dsl_of("werewolf-(mafia)")
players = [{"name": f"P{i + 1}", "isBot": i != 0} for i in range(8)]
svc = RoomService(seed=3)
svc.create_room("t", "werewolf-(mafia)", players, dsl=dsl, room_index=7)
for _ in range(60):                                        # advise_probe's room: seat 1 at its first day vote
    a = svc.advise("t", n_rollouts=64, max_turns=8)
    if len(a["options"]) >= 7 and "vote" in svc._rooms["t"]["log"].agent_state(svc._rooms["t"]["view"])["current_phase_name"].lower():
        break
    svc.continue_room("t")
room = svc._rooms["t"]
phase = room["log"].agent_state(room["view"])["current_phase_name"]
n_opt = len(svc.advise("t", n_rollouts=R, max_turns=M)["options"])
t_full = median_s(lambda: svc.advise("t", n_rollouts=R, max_turns=M))
results.append(line(f"Werewolf x 8 '{phase}', {n_opt} options + policy, R = {R}: advise (full view)", t_full, (n_opt + 1) * R))
t_seat = median_s(lambda: svc.advise("t", n_rollouts=R, max_turns=M, view="seat"))
results.append(line(f"  the same, advise(view=\"seat\")", t_seat, (n_opt + 1) * R))
svc.close()

pool = RoomPoolService(seed=3, chunk_rooms=1024)
tids = [f"thread-{i}" for i in range(1024)]
for tid in tids:
    pool.create_room(tid, "werewolf-(mafia)", players, dsl=dsl)
for k in range(12):
    pool.handle_messages([(tid, "Continue") for tid in tids[: 1024 - 64 * k]])
for view in ("full", "seat"):
    t = median_s(lambda: pool.advises(tids, n_rollouts=1024, max_turns=M, view=view), reps=max(3, REPS // 4))
    results.append(line(f"1 024 pooled Werewolf x 8 threads x 1 024: advises(view=\"{view}\")", t, 9 * 1024 * 1024))
pool.close()

# 65 536-playout forecasts per layout, from a room some turns into its game
for game, n, turns in [("werewolf-(mafia)", 8, 9), ("werewolf-(mafia)", 12, 9), ("two-truths-and-a-lie", 4, 4),
                       ("two-truths-and-a-lie", 8, 4), ("two-truths-and-a-lie", 12, 4)]:
    with RoomBatch([(GameTable(dsl_of(game)), n, 1, 0)], seed=11) as b:
        b.step(turns)
        v = b.read_rooms(0, 1)
        if game.startswith("werewolf"):
            roles = [int(v["players"][0][i][0]) for i in range(n)]
            seat = 1 + next(i for i in range(n) if roles[i] == 1 and not v["players"][0][i][3])
        else:
            sp = [int(v["players"][0][i][0]) for i in range(n)]
            seat = 1 + next(i for i in range(n) if not sp[i])
        key, seed, P = 5 << 16, forecast_seed(3), 65536
        t0 = median_s(lambda: b.rollout_rooms([0], [key], [turns], P, M, seed=seed))
        t1 = median_s(lambda: b.rollout_seats([0], [key], [turns], [0], None, P, M, seed=seed))
        t2 = median_s(lambda: b.rollout_seats([0], [key], [turns], [seat], None, P, M, seed=seed))
        name = f"{'Werewolf' if game.startswith('werewolf') else 'Two-Truths'} x {n}, turn {turns}, 65 536 playouts"
        results.append(line(f"{name}: full view (rollout_rooms)", t0, P))
        results.append(line(f"  rollout_seats, seat 0 (no re-deal)", t1, P))
        results.append(line(f"  rollout_seats, seat {seat}'s view", t2, P))
print(json.dumps({"max_turns": M, "repeats": REPS, "results": results}))

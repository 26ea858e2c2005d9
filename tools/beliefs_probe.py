#!/usr/bin/env python3
"""Wall time of seat-view playouts weighted by beliefs (ge_batch_rollout_beliefs, POLICY.md §3j) against the unweighted seat view
(ge_batch_rollout_seats - unchanged code, so its figure is the parent's): per layout 65 536 playouts x 1 024 turns of one room
from a Villager's / non-speaker's view, with neutral (all 16) and with skewed beliefs, the three calls alternated in the same
run on the same entry; and one advise(view="seat") at tools/advise_probe.py's room without, with neutral and with skewed
beliefs.  Median wall time of synchronised calls after a warm-up.
python tools/beliefs_probe.py [repeats]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from game_engine_amd import GameTable, RoomBatch, RoomService  # noqa: E402
from game_engine_amd.room_service import forecast_seed  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
M, R = 1024, 4096


def dsl_of(game):
    with open(os.path.join(ROOT, "tests", "golden", "dsl", f"{game}.json"), encoding="utf-8") as f:
        return json.load(f)


def alternated(fns, reps=REPS):
    """Medians of the calls of `fns`, each repeat running every one of them once, in order, after one warm-up of each."""
    for fn in fns:
        fn()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            ts[k].append(time.perf_counter() - t0)
    return [statistics.median(t) for t in ts]


def line(what, secs, playouts, base=None):
    ratio = "" if base is None else f"  x {secs / base:5.3f} of the unweighted call"
    print(f"{what:78s} {secs * 1e3:9.3f} ms  {playouts / secs / 1e6:9.3f} M playouts/s{ratio}", flush=True)
    return {"what": what, "ms": round(secs * 1e3, 4), "playouts_per_s": round(playouts / secs), "ratio": None if base is None else round(secs / base, 4)}


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
n_opt = len(svc.advise("t", n_rollouts=R, max_turns=M, view="seat")["options"])
skew = {2: 255, 3: 0, 4: 1, 5: 64}
t = alternated([lambda: svc.advise("t", n_rollouts=R, max_turns=M, view="seat"),
                lambda: svc.advise("t", n_rollouts=R, max_turns=M, view="seat", beliefs={}),
                lambda: svc.advise("t", n_rollouts=R, max_turns=M, view="seat", beliefs=skew)])
head = f"Werewolf x 8 '{phase}', {n_opt} options + policy, R = {R}: advise(view=\"seat\")"
results.append(line(head, t[0], (n_opt + 1) * R))
results.append(line("  the same with neutral beliefs (all 16)", t[1], (n_opt + 1) * R, t[0]))
results.append(line(f"  the same with beliefs {skew}", t[2], (n_opt + 1) * R, t[0]))
svc.close()

# 65 536 playouts per layout from a Villager's / non-speaker's view of a room some turns into its game
for game, n, turns in [("werewolf-(mafia)", 4, 9), ("werewolf-(mafia)", 8, 9), ("werewolf-(mafia)", 12, 9), ("two-truths-and-a-lie", 4, 4),
                       ("two-truths-and-a-lie", 12, 4)]:
    with RoomBatch([(GameTable(dsl_of(game)), n, 1, 0)], seed=11) as b:
        b.step(turns)
        v = b.read_rooms(0, 1)
        ww = game.startswith("werewolf")
        if ww:
            roles = [int(v["players"][0][i][0]) for i in range(n)]
            seat = 1 + next(i for i in range(n) if roles[i] == 1 and not v["players"][0][i][3])
        else:
            sp = [int(v["players"][0][i][0]) for i in range(n)]
            seat = 1 + next(i for i in range(n) if not sp[i])
        slots = n if ww else 3
        neutral = [[16] * slots + [0] * (16 - slots)]
        skewed = [[(255, 0, 1, 64, 16, 3)[i % 6] for i in range(slots)] + [0] * (16 - slots)]
        key, seed, P = 5 << 16, forecast_seed(3), 65536
        t = alternated([lambda: b.rollout_seats([0], [key], [turns], [seat], None, P, M, seed=seed),
                        lambda: b.rollout_beliefs([0], [key], [turns], [seat], None, neutral, P, M, seed=seed),
                        lambda: b.rollout_beliefs([0], [key], [turns], [seat], None, skewed, P, M, seed=seed)])
        name = f"{'Werewolf' if ww else 'Two-Truths'} x {n}, turn {turns}, 65 536 playouts, seat {seat}'s view"
        results.append(line(f"{name}: rollout_seats", t[0], P))
        results.append(line("  rollout_beliefs, neutral (all 16)", t[1], P, t[0]))
        results.append(line(f"  rollout_beliefs, skewed {skewed[0][:slots]}", t[2], P, t[0]))
print(json.dumps({"max_turns": M, "repeats": REPS, "results": results}))

#!/usr/bin/env python3
"""Wall time of ge_batch_rollout_compare against ge_batch_rollout_seats on the same entries, at the shapes of tools/seat_probe.py:
the Werewolf x 8 first day vote (7 options + the policy's entry, R = 4 096, seat 1's view), and 1 024 Werewolf x 8 rooms x 9
entries x 1 024 playouts in one call.  The two calls are alternated in one process; median wall time of synchronised calls
after a warm-up.  Then, for the first shape, the paired standard error of each option's difference to the policy's entry
(from ge_compare_stats) beside the unpaired one the marginal counts alone allow.
python tools/compare_probe.py [repeats]"""
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from game_engine_amd import GameTable, RoomBatch, RoomService  # noqa: E402
from game_engine_amd.room_service import forecast_key, forecast_seed  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
M = 1024
SEAT_WINS = 41 + 12


def dsl_of(game):
    with open(os.path.join(ROOT, "tests", "golden", "dsl", f"{game}.json"), encoding="utf-8") as f:
        return json.load(f)


def alternated(f, g, reps):
    """medians of f and g, called in turn"""
    f(); g()
    tf, tg = [], []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); t1 = time.perf_counter(); g(); t2 = time.perf_counter()
        tf.append(t1 - t0); tg.append(t2 - t1)
    return statistics.median(tf), statistics.median(tg)


def report(what, t_seats, t_cmp, playouts):
    print(f"{what}\n  rollout_seats   {t_seats * 1e3:9.3f} ms  {playouts / t_seats / 1e6:9.3f} M playouts/s\n"
          f"  rollout_compare {t_cmp * 1e3:9.3f} ms  {playouts / t_cmp / 1e6:9.3f} M playouts/s   extra {100 * (t_cmp / t_seats - 1):+.1f} %",
          flush=True)
    return {"what": what, "seats_ms": round(t_seats * 1e3, 4), "compare_ms": round(t_cmp * 1e3, 4), "ratio": round(t_cmp / t_seats, 4)}


results = []
dsl = dsl_of("werewolf-(mafia)")
players = [{"name": f"P{i + 1}", "isBot": i != 0} for i in range(8)]
svc = RoomService(seed=3)
svc.create_room("t", "werewolf-(mafia)", players, dsl=dsl, room_index=7)
for _ in range(60):                                        # seat_probe's room: seat 1 at its first day vote
    a = svc.advise("t", n_rollouts=64, max_turns=8)
    if len(a["options"]) >= 7 and "vote" in svc._rooms["t"]["log"].agent_state(svc._rooms["t"]["view"])["current_phase_name"].lower():
        break
    svc.continue_room("t")
room = svc._rooms["t"]
b, turn, R = room["batch"], room["batch"].turn, 4096
cands = [int(o["choice"]) for o in a["options"]]
k = len(cands) + 1
args = ([0] * k, [forecast_key(room["key"])] * k, [turn] * k, [1] * k, [[(1, c)] for c in cands] + [[]])
seed = forecast_seed(3)
ts, tc = alternated(lambda: b.rollout_seats(*args, R, M, seed=seed),
                    lambda: b.rollout_compare(*args, [k - 1] * k, [1] * k, R, M, seed=seed), REPS)
results.append(report(f"Werewolf x 8 first day vote, {k - 1} options + policy, R = {R}, seat 1's view", ts, tc, k * R))
words, _, cmp = b.rollout_compare(*args, [k - 1] * k, [1] * k, R, M, seed=seed)
print("  seat 1's wins per option against the policy's entry (counts of R; se = standard error of the difference):")
for j, c in enumerate(cands):
    w, w0 = int(words[j][SEAT_WINS]), int(words[k - 1][SEAT_WINS])
    n, _, _, gain, loss, sq = (int(x) for x in cmp[j])
    paired = math.sqrt(max(sq - (gain - loss) ** 2 / n, 0.0))
    unpaired = math.sqrt(w * (1 - w / R) + w0 * (1 - w0 / R))
    print(f"    vote {c}: wins {w} vs {w0}, better {int(cmp[j][1])} worse {int(cmp[j][2])}: difference {gain - loss:+d}, "
          f"paired se {paired:.1f}, unpaired se {unpaired:.1f}", flush=True)
svc.close()

N = 1024
with RoomBatch([(GameTable(dsl), 8, N, 0b1)], seed=3) as b:
    b.step(7)
    R = 1024
    rooms = [r for r in range(N) for _ in range(9)]
    keys = [forecast_key(r) for r in rooms]
    acts = [a for _ in range(N) for a in [[(1, c)] for c in range(1, 9)] + [[]]]
    base = [9 * (j // 9) + 8 for j in range(9 * N)]
    args = (rooms, keys, [7] * len(rooms), [1] * len(rooms), acts)
    reps = max(3, REPS // 4)
    ts, tc = alternated(lambda: b.rollout_seats(*args, R, M, seed=seed),
                        lambda: b.rollout_compare(*args, base, [1] * len(rooms), R, M, seed=seed), reps)
    results.append(report(f"1 024 Werewolf x 8 rooms x 9 entries x {R} playouts in one call, seat 1's view", ts, tc, 9 * N * R))
print(json.dumps({"max_turns": M, "repeats": REPS, "results": results}))

#!/usr/bin/env python3
"""Playout seats (ge_batch_step_rooms_playout, POLICY.md §3d): the wall time of one call against the same decisions made by the host
composition, and what playout bots do to the win rates.
    python tools/playout_probe.py [repeats] [games]

1. 1 024 Werewolf x 8 rooms, every seat a playout seat, R = 256, M = 256, from states spread over the game (each room played
   0 .. 39 turns under its own key): median wall time of synchronised calls, each from the same records.  The split is by
   difference of three calls from the same records: the call (plan + playouts + decide + turn), the call with max_turns = 0
   (plan + empty playouts + decide + turn) and mask 0 (the turn).
2. The host composition of the same decisions: read_rooms_at, host planning (tests/playout_ref.py on oracle records),
   rollout_seats, host argmax, inject_actions, step_rooms - asserted equal to the call (events and records).
3. Win rates of `games` Werewolf x 8 games played to the end (seed fixed), seat view and full view: policy only, the village
   side's seats as playout bots, the wolf side's seats as playout bots (R = 64, M = 256: a bot's seats are read from the room
   after the deal, every turn)."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

from game_engine_amd import GameTable, RoomBatch  # noqa: E402
from oracle.oracle import Oracle  # noqa: E402
from oracle.rng import pick  # noqa: E402
from parity_util import oracle_rooms_as_views, views_as_oracle_rooms  # noqa: E402
from playout_ref import SEAT_WINS, candidates, due_seats, seat_draw  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
GAMES = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
N_ROOMS, R, M, SEED, PSEED = 1024, 256, 256, 0x5EED, 0xF00D


def dsl_of(game):
    with open(os.path.join(ROOT, "tests", "golden", "dsl", f"{game}.json"), encoding="utf-8") as f:
        return json.load(f)


dsl = dsl_of("werewolf-(mafia)")
orc = Oracle(dsl, 8)
rng = np.random.default_rng(1)
recs = orc.init_rooms(N_ROOMS)
for i in range(N_ROOMS):
    orc.run(recs[i:i + 1], SEED, int(rng.integers(0, 1 << 20)), 0, int(rng.integers(0, 40)))
views = oracle_rooms_as_views(orc, recs)
rooms = np.arange(N_ROOMS, dtype=np.uint64)
keys = rng.integers(0, 1 << 40, N_ROOMS).astype(np.uint64)
turns = rng.integers(0, 50000, N_ROOMS).astype(np.uint32)
masks = np.full(N_ROOMS, 0xFF, np.uint32)
pkeys = rng.integers(0, 1 << 63, N_ROOMS).astype(np.uint64)
b = RoomBatch([(GameTable(dsl), 8, N_ROOMS, 0)], seed=SEED)


def timed(fn, reps=REPS):
    ts = []
    for _ in range(reps + 1):
        b.write_rooms(0, views)
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts[1:])


def call(m=M, mk=masks):
    return b.step_rooms_playout(rooms, keys, turns, mk, pkeys, R, m, seed=PSEED)


b.write_rooms(0, views)
ev, dec = call()
want_rec = b.read_rooms()
n_dec = int(sum(bin(int(d)).count("1") for d in dec))
t_all, t_m0, t_turn = timed(call), timed(lambda: call(0)), timed(lambda: call(mk=np.zeros(N_ROOMS, np.uint32)))
results = {"rooms": N_ROOMS, "R": R, "M": M, "decisions": n_dec, "call_ms": t_all * 1e3, "playouts_ms": (t_all - t_m0) * 1e3,
           "plan_decide_ms": (t_m0 - t_turn) * 1e3, "turn_ms": t_turn * 1e3}
print(f"1 024 Werewolf x 8, every seat a playout seat, R = {R}, M = {M}: {n_dec} decisions")
print(f"  ge_batch_step_rooms_playout          {t_all * 1e3:9.3f} ms")
print(f"    playouts (call - call at M = 0)    {(t_all - t_m0) * 1e3:9.3f} ms")
print(f"    plan + decide (M = 0 - mask 0)     {(t_m0 - t_turn) * 1e3:9.3f} ms")
print(f"    the turn (mask 0)                  {t_turn * 1e3:9.3f} ms", flush=True)


def composition():
    v = b.read_rooms_at(rooms)
    orecs = views_as_oracle_rooms(orc, v)
    q, owner = [[], [], [], [], []], []
    for r in range(N_ROOMS):
        for s in due_seats(orc, orecs[r], SEED, int(keys[r]), int(turns[r]), False, 0):
            cand = candidates(orc, orecs[r], s)
            if len(cand) < 2:
                continue
            for c in cand:
                for lst, x in zip(q, (r, int(pkeys[r]), int(turns[r]), s, [(s, c)])):
                    lst.append(x)
                owner.append((r, s, c))
    words, _ = b.rollout_seats(q[0], q[1], q[2], q[3], q[4], R, M, seed=PSEED)
    best = {}
    for (r, s, c), w in zip(owner, words):
        best.setdefault((r, s), []).append((int(w[SEAT_WINS + s - 1]), c))
    ir, ip, ic = [], [], []
    for (r, s), vals in best.items():
        top = max(x for x, _ in vals)
        tied = [c for x, c in vals if x == top]
        ir.append(r); ip.append(s); ic.append(tied[pick(seat_draw(SEED, int(keys[r]), int(turns[r]), s), len(tied))])
    assert (b.inject_actions(ir, ip, ic) == 0).all()
    ev = b.step_rooms(rooms, keys, turns)
    for r, s, c in zip(ir, ip, ic):                         # the injected seats count as acting in the turn, as the call lists them
        ev[r]["acted_now"] |= 1 << (s - 1)
        ev[r]["choice"][s - 1] = c
    return ev


b.write_rooms(0, views)
ev2 = composition()
got = b.read_rooms()
for f in ("turn", "from_phase_id", "to_phase_id", "acted_now", "choice"):
    assert np.array_equal(ev2[f], ev[f]), f
assert got.tobytes() == want_rec.tobytes()
t_comp = timed(composition, reps=max(2, REPS // 4))
results["composition_ms"] = t_comp * 1e3
print(f"  the host composition                 {t_comp * 1e3:9.3f} ms   (read_rooms_at, host planning, rollout_seats, host argmax,"
      f" inject_actions, step_rooms; equal events and records)", flush=True)
b.close()


def play(side, full_view, n_games=GAMES, turns=220, r=64, m=256):
    """village wins / finished of n_games games to the end; side None = policy only, 1 = villagers, 2 = werewolves as bots"""
    with RoomBatch([(GameTable(dsl), 8, n_games, 0)], seed=0xACE) as g:
        rs = np.arange(n_games, dtype=np.uint64)
        ks = rs + 5000
        for t in range(turns):
            tt = np.full(n_games, t, np.uint32)
            if side is None:
                g.step_rooms(rs, ks, tt)
                continue
            v = g.read_rooms()
            mk = np.zeros(n_games, np.uint32)
            for i in range(8):
                mk |= (v["players"][:, i, 1] == side).astype(np.uint32) << i
            g.step_rooms_playout(rs, ks, tt, mk, ks + 1, r, m, seed=0xBEE, full_view=full_view)
        v = g.read_rooms()
    wolves = ((v["players"][:, :8, 2] != 0) & (v["players"][:, :8, 1] == 2)).sum(axis=1)
    fin = v["end_turn"] >= 0
    return int((fin & (wolves == 0)).sum()), int(fin.sum())


rates = {}
t0 = time.perf_counter()
v0, f0 = play(None, False)
rates["policy"] = [v0, f0]
print(f"{GAMES} Werewolf x 8 games (R = 64, M = 256 for the bots): village wins / finished")
print(f"  policy only                                {v0:5d} / {f0}", flush=True)
for full_view in (False, True):
    for side, name in ((1, "village"), (2, "wolf")):
        v1, f1 = play(side, full_view)
        rates[f"{name}_{'full' if full_view else 'seat'}"] = [v1, f1]
        print(f"  {name} seats as playout bots, {'full' if full_view else 'seat'} view{' ' * (14 - len(name))}{v1:5d} / {f1}", flush=True)
results["win_rates"] = rates
results["win_rate_wall_s"] = time.perf_counter() - t0
print(json.dumps(results))

#!/usr/bin/env python3
"""GE_PLAYOUT_HALVING (POLICY.md §3h) measured on the GPU: wall times, medians of alternated synchronised calls after a warm-up,
every call from the same records.

    python tools/halving_probe.py --parent PATH/libge_step.so [--reps 5]   1. the unflagged step_rooms_playout (tools/playout_probe.py's
                                  shape) and run_rooms_playout (tools/run_playout_probe.py's three thread counts) on a build of the
                                  parent commit and on this one: one child process per build and repetition (GE_LIB_PATH is read once
                                  per process), alternated; a child that fails or runs out of time ends the series
    python tools/halving_probe.py --flagged [--reps 9]     2. the flagged call against the unflagged call on the same records,
                                  alternated: 1 024 rooms of Werewolf x 8 (R = 256 and 1 024), Werewolf x 12 and Two-Truths x 4 (R = 256),
                                  every seat a playout seat, and the run-on call on 1, 64 and 1 024 threads.  Beside the times, the
                                  playouts of the step: c x n per decision without the flag, and §3h's closed form (no tie at a cut; a tie
                                  plays more) with it - reference arithmetic over the host's plan, no device counter
    python tools/halving_probe.py --strength [--games 4096]   3. tools/playout_probe.py's part 3 at R = 64, M = 256, seat view: the
                                  village side's and the wolf side's seats as playout bots, without and with the flag; with p the
                                  unflagged village-win share, the two counts differ by sampling alone by about sqrt(2 G p (1 - p))
    python tools/halving_probe.py --unflagged     (what 1. runs in each child: one JSON line)"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

SEED, PSEED, M, N_ROOMS = 0x5EED, 0xF00D, 256, 1024
PERSON, END = 1, 2


def dsl_of(game):
    with open(os.path.join(ROOT, "tests", "golden", "dsl", f"{game}.json"), encoding="utf-8") as f:
        return json.load(f)


def step_inputs(game, n_players, n_rooms=N_ROOMS):
    """playout_probe's records: each room played 0 .. 39 turns under its own key, every seat a playout seat"""
    from oracle.oracle import Oracle
    from parity_util import oracle_rooms_as_views
    orc = Oracle(dsl_of(game), n_players)
    rng = np.random.default_rng(1)
    recs = orc.init_rooms(n_rooms)
    for i in range(n_rooms):
        orc.run(recs[i:i + 1], SEED, int(rng.integers(0, 1 << 20)), 0, int(rng.integers(0, 40)))
    keys = rng.integers(0, 1 << 40, n_rooms).astype(np.uint64)
    turns = rng.integers(0, 50000, n_rooms).astype(np.uint32)
    pkeys = rng.integers(0, 1 << 63, n_rooms).astype(np.uint64)
    return orc, recs, oracle_rooms_as_views(orc, recs), keys, turns, np.full(n_rooms, (1 << n_players) - 1, np.uint32), pkeys


def run_inputs(n):
    """run_playout_probe's threads: one human seat, one or two playout seats, from the start of the game"""
    rng = np.random.default_rng(n)
    keys = rng.choice(1 << 40, size=n, replace=False).astype(np.uint64)
    return keys, np.zeros(n, np.uint32), np.where(np.arange(n) % 2 == 0, 0b10, 0b100100).astype(np.uint32), keys << np.uint64(16)


def alternated(b, start, calls, reps):
    """median / min / max wall ms of each call, alternated, each from the records `start`; one warm-up of each first"""
    ts = [[] for _ in calls]
    for rep in range(reps + 1):
        for i, fn in enumerate(calls):
            b.write_rooms(0, start)
            t0 = time.perf_counter()
            fn()
            if rep:
                ts[i].append((time.perf_counter() - t0) * 1e3)
    return [(statistics.median(t), min(t), max(t)) for t in ts]


def unflagged(reps):
    from game_engine_amd import GameTable, RoomBatch
    tb = GameTable(dsl_of("werewolf-(mafia)"))
    out = {}
    _, _, views, keys, turns, masks, pkeys = step_inputs("werewolf-(mafia)", 8)
    rooms = np.arange(N_ROOMS, dtype=np.uint64)
    with RoomBatch([(tb, 8, N_ROOMS, 0)], seed=SEED) as b:
        out["step_ms"] = alternated(b, views, [lambda: b.step_rooms_playout(rooms, keys, turns, masks, pkeys, 256, M, seed=PSEED)], reps)[0][0]
    for n in (1, 64, 1024):
        keys, turns, masks, pkeys = run_inputs(n)
        rooms = np.arange(n, dtype=np.uint64)
        with RoomBatch([(tb, 8, n, 1)], seed=0xBEEF, max_fuse=1) as b:
            start = b.read_rooms()
            out[f"run_{n}_ms"] = alternated(b, start, [lambda: b.run_rooms_playout(rooms, keys, turns, masks, pkeys, 256, M, seed=PSEED, max_turns=64,
                                                                                   until=PERSON | END, views=False)], reps)[0][0]
    print(json.dumps(out))


def against_parent(parent, reps):
    series = {"parent": [], "this": []}
    for rep in range(reps):
        for name in ("parent", "this"):
            env = dict(os.environ)
            if name == "parent":
                env.update(GE_LIB_PATH=os.path.abspath(parent), GE_LIB_ANY_ABI="1")
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--unflagged", "--reps", "5"], env=env, capture_output=True, text=True,
                                   timeout=120)
            except subprocess.TimeoutExpired:
                print(f"# {name} repetition {rep}: no result within 120 s; the series ends here", flush=True)
                raise SystemExit(124)
            if p.returncode != 0:
                print(f"# {name} repetition {rep}: exit status {p.returncode}; the series ends here\n{p.stderr[-800:]}", flush=True)
                raise SystemExit(p.returncode if p.returncode > 0 else 1)
            series[name].append(json.loads(p.stdout.strip().splitlines()[-1]))
    print(f"1. unflagged calls, the parent commit's build against this one: {reps} alternated processes each, per process the median of 5 calls (ms)")
    for key in series["this"][0]:
        a, c = [s[key] for s in series["parent"]], [s[key] for s in series["this"]]
        print(f"  {key:12s} parent median {statistics.median(a):8.3f} (min {min(a):.3f}, max {max(a):.3f})   this {statistics.median(c):8.3f} "
              f"(min {min(c):.3f}, max {max(c):.3f})", flush=True)


def planned_playouts(orc, recs, keys, turns, n):
    """(decisions, playouts without the flag, §3h's closed form) from the host's plan of the step"""
    from halving_ref import nominal_playouts
    from playout_ref import candidates, due_seats
    dec = uni = hal = 0
    for r in range(len(recs)):
        for s in due_seats(orc, recs[r], SEED, int(keys[r]), int(turns[r]), False, 0):
            c = len(candidates(orc, recs[r], s))
            if c >= 2:
                dec, uni, hal = dec + 1, uni + c * n, hal + nominal_playouts(n, c)
    return dec, uni, hal


def flagged(reps):
    from game_engine_amd import GameTable, RoomBatch
    print(f"2. the flagged call against the unflagged call, same build, same records, {reps} alternated repetitions: median (min .. max) ms")
    for game, npl, n in (("werewolf-(mafia)", 8, 256), ("werewolf-(mafia)", 8, 1024), ("werewolf-(mafia)", 12, 256), ("two-truths-and-a-lie", 4, 256)):
        orc, recs, views, keys, turns, masks, pkeys = step_inputs(game, npl)
        rooms = np.arange(N_ROOMS, dtype=np.uint64)
        dec, uni, hal = planned_playouts(orc, recs, keys, turns, n)
        with RoomBatch([(GameTable(dsl_of(game)), npl, N_ROOMS, 0)], seed=SEED) as b:
            (u, ulo, uhi), (h, hlo, hhi) = alternated(b, views, [
                lambda: b.step_rooms_playout(rooms, keys, turns, masks, pkeys, n, M, seed=PSEED),
                lambda: b.step_rooms_playout(rooms, keys, turns, masks, pkeys, n, M, seed=PSEED, halving=True)], reps)
        print(f"  step, 1 024 x {game} x {npl}, R = {n}: {dec} decisions; unflagged {u:.3f} ({ulo:.3f} .. {uhi:.3f}), {uni} playouts; "
              f"flagged {h:.3f} ({hlo:.3f} .. {hhi:.3f}), {hal} playouts when no cut meets a tie; time x {u / h:.2f}, playouts x {uni / hal:.2f}", flush=True)
    tb = GameTable(dsl_of("werewolf-(mafia)"))
    for n in (1, 64, 1024):
        keys, turns, masks, pkeys = run_inputs(n)
        rooms = np.arange(n, dtype=np.uint64)
        with RoomBatch([(tb, 8, n, 1)], seed=0xBEEF, max_fuse=1) as b:
            start = b.read_rooms()
            run = lambda hv: b.run_rooms_playout(rooms, keys, turns, masks, pkeys, 256, M, seed=PSEED, max_turns=64, until=PERSON | END, views=False, halving=hv)
            turns_u, turns_h = int(run(False)[0].sum()), 0
            b.write_rooms(0, start)
            turns_h = int(run(True)[0].sum())
            (u, ulo, uhi), (h, hlo, hhi) = alternated(b, start, [lambda: run(False), lambda: run(True)], reps)
        print(f"  run-on, {n} Werewolf x 8 threads, R = 256, until person | end: unflagged {u:.3f} ({ulo:.3f} .. {uhi:.3f}), {turns_u} turns played; "
              f"flagged {h:.3f} ({hlo:.3f} .. {hhi:.3f}), {turns_h} turns played; time x {u / h:.2f}", flush=True)


def strength(games):
    from game_engine_amd import GameTable, RoomBatch
    dsl = dsl_of("werewolf-(mafia)")

    def play(side, halving):
        with RoomBatch([(GameTable(dsl), 8, games, 0)], seed=0xACE) as g:
            rs = np.arange(games, dtype=np.uint64)
            ks = rs + 5000
            for t in range(220):
                v = g.read_rooms()
                mk = np.zeros(games, np.uint32)
                for i in range(8):
                    mk |= (v["players"][:, i, 1] == side).astype(np.uint32) << i
                g.step_rooms_playout(rs, ks, np.full(games, t, np.uint32), mk, ks + 1, 64, 256, seed=0xBEE, halving=halving)
            v = g.read_rooms()
        wolves = ((v["players"][:, :8, 2] != 0) & (v["players"][:, :8, 1] == 2)).sum(axis=1)
        fin = v["end_turn"] >= 0
        return int((fin & (wolves == 0)).sum()), int(fin.sum())

    print(f"3. {games} Werewolf x 8 games to the end, R = 64, M = 256, seat view: village wins / finished, without and with the flag")
    for side, name in ((1, "village"), (2, "wolf")):
        (v0, f0), (v1, f1) = play(side, False), play(side, True)
        p = v0 / games
        sd = math.sqrt(2 * games * p * (1 - p))
        worse = (v0 - v1) if side == 1 else (v1 - v0)            # a loss for the bots' side
        print(f"  {name} seats as playout bots: unflagged {v0} / {f0}, flagged {v1} / {f1}; sampling alone ~ {sd:.0f}; "
              f"shift against the bots' side with the flag: {worse} games ({worse / sd:+.2f} of that figure)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent")
    ap.add_argument("--flagged", action="store_true")
    ap.add_argument("--strength", action="store_true")
    ap.add_argument("--unflagged", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--games", type=int, default=4096)
    a = ap.parse_args()
    if a.unflagged:
        unflagged(a.reps)
    if a.parent:
        against_parent(a.parent, a.reps)
    if a.flagged:
        flagged(a.reps)
    if a.strength:
        strength(a.games)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What a run-on with playout bots costs and saves (GPU): one RoomBatch.run_rooms_playout call against the host loop it replaces -
step_rooms_playout + read_rooms_at per turn of the rooms still running - on 1, 64 and 1 024 Werewolf x 8 threads with one human seat
and one or two playout seats each, at the services' defaults (256 rollouts, 256 playout turns), until = person | end, max_turns =
64.  Wall time, medians of alternated calls after a warm-up; every call starts from the same records.

    python tools/run_playout_probe.py [--reps 9] [--threads 1,64,1024]
The A/B of the group size and of the playout grid runs the same tool under GE_RUNP_GROUP=1|8|64 and GE_RUNP_GRID=0|1 (read once per
process): tools/run_playout_probe.py --ab starts one child process per setting and prints their lines."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PERSON, END = 1, 2
R, M, MAX_TURNS, SEED, PSEED = 256, 256, 64, 0xBEEF, 0xF00D


def composition(b, terminal, human_pending, rooms, keys, turns, masks, pkeys):
    played = np.zeros(len(rooms), dtype=np.uint32)
    live = np.arange(len(rooms))
    for t in range(MAX_TURNS):
        b.step_rooms_playout(rooms[live], keys[live], turns[live] + np.uint32(t), masks[live], pkeys[live], R, M, seed=PSEED)
        vw = b.read_rooms_at(rooms[live])
        played[live] = t + 1
        live = live[~(np.isin(vw["phase_id"], terminal) | human_pending[live, t])]
        if not len(live):
            break
    return played


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--threads", default="1,64,1024")
    ap.add_argument("--ab", action="store_true")
    a = ap.parse_args()
    if a.ab:
        # one child process per setting (the library reads the switches once), one after the other; a child that fails, is killed
        # or runs out of time ends the series: nothing more is started on the card behind it
        limit = 30 + 4 * a.reps * len(a.threads.split(","))     # seconds: a setting takes ~1 s per repetition and list at these shapes
        for env in ({"GE_RUNP_GROUP": "1"}, {"GE_RUNP_GROUP": "8"}, {"GE_RUNP_GROUP": "64"}, {"GE_RUNP_GRID": "1"}):
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--threads", a.threads],
                                   env=dict(os.environ, **env), capture_output=True, text=True, timeout=limit)
            except subprocess.TimeoutExpired:
                print(f"# {env}: no result within {limit} s; the series ends here", flush=True)
                raise SystemExit(124)
            print(f"# {env}\n{p.stdout}", end="", flush=True)
            if p.returncode != 0:
                print(f"# {env}: exit status {p.returncode}; the series ends here\n{p.stderr[-800:]}", flush=True)
                raise SystemExit(p.returncode if p.returncode > 0 else 1)
        return
    from game_engine_amd import GameTable, RoomBatch
    with open(os.path.join(ROOT, "tests", "golden", "dsl", "werewolf-(mafia).json"), encoding="utf-8") as f:
        tb = GameTable(json.load(f))
    terminal = [r["phase_id"] for r in tb.rows() if not r["branches"]]
    print(f"# GE_RUNP_GROUP={os.environ.get('GE_RUNP_GROUP', 'default (8)')} GE_RUNP_GRID={os.environ.get('GE_RUNP_GRID', 'default (0: fixed grid)')}")
    for n in (int(x) for x in a.threads.split(",")):
        rng = np.random.default_rng(n)
        rooms = np.arange(n, dtype=np.uint64)
        keys = rng.choice(1 << 40, size=n, replace=False).astype(np.uint64)
        turns = np.zeros(n, dtype=np.uint32)
        masks = np.where(np.arange(n) % 2 == 0, 0b10, 0b100100).astype(np.uint32)      # one or two playout seats; seat 1 is the person
        pkeys = keys << np.uint64(16)
        with RoomBatch([(tb, 8, n, 1)], seed=SEED, max_fuse=1) as b:
            start = b.read_rooms()
            # one call first: its PERSON stops drive the composition's loop (the loop has no oracle to ask), and it warms both paths
            played, stopped, _, views, _ = b.run_rooms_playout(rooms, keys, turns, masks, pkeys, R, M, seed=PSEED, max_turns=MAX_TURNS,
                                                               until=PERSON | END)
            pending = np.zeros((n, MAX_TURNS), dtype=bool)
            pending[np.arange(n), played - 1] = (stopped & PERSON) != 0
            after = b.read_rooms().tobytes()
            b.write_rooms(0, start)
            assert np.array_equal(composition(b, terminal, pending, rooms, keys, turns, masks, pkeys), played)
            assert b.read_rooms().tobytes() == after, "the composition and the call disagree"
            t_run, t_loop = [], []
            for _ in range(a.reps):                               # alternated, each from the same records
                b.write_rooms(0, start)
                t0 = time.perf_counter()
                b.run_rooms_playout(rooms, keys, turns, masks, pkeys, R, M, seed=PSEED, max_turns=MAX_TURNS, until=PERSON | END)
                t_run.append(time.perf_counter() - t0)
                b.write_rooms(0, start)
                t0 = time.perf_counter()
                composition(b, terminal, pending, rooms, keys, turns, masks, pkeys)
                t_loop.append(time.perf_counter() - t0)
        mr, ml = statistics.median(t_run) * 1e3, statistics.median(t_loop) * 1e3
        print(f"{n:5d} threads: played {int(played.min())} .. {int(played.max())} (median {int(np.median(played))}, sum {int(played.sum())}); "
              f"run_rooms_playout {mr:.3f} ms (min {min(t_run) * 1e3:.3f}, max {max(t_run) * 1e3:.3f}), "
              f"step_rooms_playout + read_rooms_at loop {ml:.3f} ms (min {min(t_loop) * 1e3:.3f}, max {max(t_loop) * 1e3:.3f}), x {ml / mr:.2f}; "
              f"{a.reps} alternated repetitions", flush=True)


if __name__ == "__main__":
    main()

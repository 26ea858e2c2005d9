#!/usr/bin/env python3
"""ge_batch_run_rooms_forecast (POLICY.md §3i) against the composition it replaces, wall time in one process, forms alternated.
    python tools/timeline_probe.py [output file, default profiles/timeline_probe.txt] [shapes, default 1,64,4096]

Shapes: 1, 64 and 4 096 all-bot Werewolf x 8 threads from the initial state, each under its own key, max_turns = 64, until = END,
n_rollouts = 4096 per point, playouts of at most 1 024 turns, the full view.  A call takes at most 252 threads at this size
(n x 65 x 4 096 <= 2^26), so the larger shapes are runs of such calls, as RoomPoolService.run_rooms issues them.
  one call     run_rooms_forecast per run of threads
  composition  the entry points there were before: rollout_seats of the rooms as they stand (point 0), run_rooms, then per played turn
               a write_rooms_at of that turn's views into scratch rooms of a second batch and a rollout_seats of those
Both forms end in a device synchronise inside the library, so a host clock around them times finished work.  Both are asserted to give
the same words at every point.  Times are medians of 5 after a warm-up pass of both forms, the forms alternated inside every repeat;
the spread is the half range (max - min) / 2 of the same samples.  kernel = the launch interval of the one call on the stream
(ge_batch_set_timing: point 0's playouts, the run and the traced points together)."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from game_engine_amd import GameTable, RoomBatch  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "timeline_probe.txt")
SHAPES = [int(x) for x in sys.argv[2].split(",")] if len(sys.argv) > 2 else [1, 64, 4096]
REPS, MAX_TURNS, UNTIL, R, PMAX, SEED, FSEED = 5, 64, 2, 4096, 1024, 0x5EED, 0xF0CA57
PER_CALL = (1 << 26) // ((MAX_TURNS + 1) * R)                 # 252 threads
with open(os.path.join(ROOT, "tests", "golden", "dsl", "werewolf-(mafia).json"), encoding="utf-8") as f:
    dsl = json.load(f)
tb = GameTable(dsl)
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def shape(n):
    rng = np.random.default_rng(n)
    rooms = np.arange(n, dtype=np.uint64)
    keys = rng.choice(1 << 40, size=n, replace=False).astype(np.uint64)
    fkeys = keys << np.uint64(16)
    turns = np.zeros(n, dtype=np.uint32)
    seats = np.zeros(n, dtype=np.uint32)
    b = RoomBatch([(tb, 8, n, 0)], seed=SEED, max_fuse=1)
    scratch = RoomBatch([(tb, 8, n, 0)], seed=SEED, max_fuse=1)
    start = b.read_rooms()
    parts = [(lo, min(lo + PER_CALL, n)) for lo in range(0, n, PER_CALL)]

    def one_call():
        played, stats = np.zeros(n, dtype=np.uint32), np.zeros((n, MAX_TURNS + 1, 77), dtype=np.uint64)
        for lo, hi in parts:
            p, _, _, _, w = b.run_rooms_forecast(rooms[lo:hi], keys[lo:hi], turns[lo:hi], fkeys[lo:hi], R, PMAX, seats=None, seed=FSEED,
                                                 max_turns=MAX_TURNS, until=UNTIL)
            played[lo:hi], stats[lo:hi] = p, w
        return played, stats

    def composition():
        stats = np.zeros((n, MAX_TURNS + 1, 77), dtype=np.uint64)
        stats[:, 0] = b.rollout_seats(rooms, fkeys, turns, seats, None, R, PMAX, seed=FSEED)[0]
        played, _, _, views = b.run_rooms(rooms, keys, turns, MAX_TURNS, UNTIL)
        for p in range(1, int(played.max()) + 1):
            live = np.nonzero(played >= p)[0]
            scratch.write_rooms_at(rooms[live], views[live, p - 1])
            stats[live, p] = scratch.rollout_seats(rooms[live], fkeys[live], turns[live] + np.uint32(p), seats[live], None, R, PMAX, seed=FSEED)[0]
        return played, stats

    t_one, t_comp, t_kernel = [], [], []
    b.set_timing(True)
    for rep in range(REPS + 1):
        for which in ((1, 0) if rep % 2 else (0, 1)):
            b.write_rooms(0, start)
            b.kernel_time(reset=True)
            t0 = time.perf_counter()
            got = one_call() if which == 0 else composition()
            dt = time.perf_counter() - t0
            if rep == 0:                                         # warm-up: buffers grow, pages fault in, code objects load
                if which == 0:
                    played, want = got
                else:
                    assert np.array_equal(got[0], played)
                    for k in range(n):
                        assert np.array_equal(got[1][k, :int(played[k]) + 1], want[k, :int(played[k]) + 1]), "the two forms differ"
                continue
            if which == 0:
                t_one.append(dt)
                t_kernel.append(b.kernel_time(reset=True)[0] * 1e-3)
            else:
                t_comp.append(dt)
    b.close()
    scratch.close()
    med = statistics.median
    half = lambda x: (max(x) - min(x)) / 2
    o, c, k = med(t_one), med(t_comp), med(t_kernel)
    points = int(played.sum()) + n
    say(f"{n} Werewolf x 8 threads, max_turns {MAX_TURNS}, until END, {R} playouts of at most {PMAX} turns per point: {points} points, "
        f"played min / median / max {int(played.min())} / {int(np.median(played))} / {int(played.max())}, {len(parts)} call(s)")
    say(f"  one call (run_rooms_forecast)   {o * 1e3:10.2f} ms  (spread +-{half(t_one) * 1e3:.2f} ms; kernel interval {k * 1e3:.2f} ms)")
    say(f"  composition                     {c * 1e3:10.2f} ms  (spread +-{half(t_comp) * 1e3:.2f} ms; {2 * int(played.max()) + 2} calls)")
    say(f"  ratio composition / one call  x {c / o:.2f}; difference {1e3 * (c - o):.2f} ms against a summed spread of "
        f"{1e3 * (half(t_one) + half(t_comp)):.2f} ms")


say("ge_batch_run_rooms_forecast against run_rooms + per turn write_rooms_at and rollout_seats (tools/timeline_probe.py), MI355X, wall time, "
    f"medians of {REPS}")
say()
for n in SHAPES:
    shape(n)
    say()
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")

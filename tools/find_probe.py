#!/usr/bin/env python3
"""ge_batch_find_rooms (POLICY.md §3k) against the composition it replaces, wall time in one process, forms alternated.
    python tools/find_probe.py [output file, default profiles/find_probe.txt] [sizes, default 65536,1048576]

A Werewolf x 8 batch with human_mask = 1 (seat 1 host-driven), stepped 40 turns from the initial state without restart; then, over
the whole batch,
  find         find_rooms(want = person | end), every hit copied back (cap = count)
  read back    the entry points there were before: ge_batch_read_rooms of the range into a reused array (228 B of view per room,
               built by the library's host threads) and the numpy predicate for END over it (the terminal phases from the table).
               The PERSON half has no host form short of the library's own refusal rule per view, so it is left out: the read-back
               column is a lower bound of the composition.
Both forms end in a device synchronise inside the library, so a host clock around them times finished work.  END of both forms
is asserted to name the same rooms.  Times are medians of 20 calls after 3 warm-up calls of both forms, the forms alternated
inside every repeat; the spread is the half range (max - min) / 2 of the same samples.  kernel = the launch interval of the
find call on the stream (ge_batch_set_timing: the test launch, the scan and the emit together)."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from game_engine_amd import GameTable, RoomBatch  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "find_probe.txt")
SIZES = [int(x) for x in sys.argv[2].split(",")] if len(sys.argv) > 2 else [65536, 1048576]
WARM, REPS, TURNS, SEED = 3, 20, 40, 0xF1AD
with open(os.path.join(ROOT, "tests", "golden", "dsl", "werewolf-(mafia).json"), encoding="utf-8") as f:
    dsl = json.load(f)
tb = GameTable(dsl)
terminal = np.zeros(256, dtype=bool)
for r in tb.rows():
    terminal[r["phase_id"]] = not r["branches"]
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def med(xs):
    return statistics.median(xs), (max(xs) - min(xs)) / 2


def size(n):
    with RoomBatch([(tb, 8, n, 1)], seed=SEED) as b:
        b.step(TURNS)
        b.sync()
        views = b.read_rooms()                                   # the reused array

        def find():
            return b.find_rooms(("person", "end"))

        def read_back():
            b.read_rooms(out=views)
            return np.flatnonzero(terminal[views["phase_id"]])

        t_find, t_read, t_kernel = [], [], []
        b.set_timing(True)
        for rep in range(WARM + REPS):
            for which in ((1, 0) if rep % 2 else (0, 1)):
                b.kernel_time(reset=True)
                t0 = time.perf_counter()
                got = find() if which == 0 else read_back()
                dt = time.perf_counter() - t0
                if rep < WARM:
                    continue
                if which == 0:
                    t_find.append(dt)
                    t_kernel.append(b.kernel_time(reset=True)[0] * 1e-3)
                    hits, n_match = got
                else:
                    t_read.append(dt)
                    ended = got
        assert np.array_equal(hits["room"][(hits["why"] & 2) != 0], ended.astype(np.uint64)), "the two forms name different finished rooms"
        f, fs = med(t_find)
        r, rs = med(t_read)
        k, _ = med(t_kernel)
        say(f"{n:>9} rooms: {n_match} match ({int((hits['why'] & 1).astype(bool).sum())} wait for seat 1, {len(ended)} ended)")
        say(f"    find       {f * 1e6:10.1f} us  +- {fs * 1e6:.1f}   (kernel interval {k * 1e6:.1f} us; {16 * len(hits)} B of hits)")
        say(f"    read back  {r * 1e6:10.1f} us  +- {rs * 1e6:.1f}   ({228 * n} B of views)")
        say(f"    read back / find = {r / f:.1f}")


say(f"find_probe: medians of {REPS} calls after {WARM} warm-up calls, Werewolf x 8, human_mask = 1, {TURNS} turns stepped")
for n in SIZES:
    size(n)
with open(OUT, "w") as fh:
    fh.write("\n".join(lines) + "\n")

#!/usr/bin/env python3
"""ge_batch_run_rooms (POLICY.md §3f) against the composition it replaces, wall time in one process, calls alternated.
    python tools/run_probe.py [repeats] [output file, default profiles/run_probe.txt]

Two cases, 1 024 Werewolf x 8 rooms from the initial state, each under its own key:
  end     all bots, played to the end: until = END, max_turns = 256
  person  seat 1 host-driven, played until that seat has an action to give (or the game ends): until = PERSON | END, max_turns = 64
Each is timed as one run_rooms call (events and views unpacked) and as the host loop of step_rooms + read_rooms_at over the rooms
still running - the calls every service made per turn before.  The loop is given the turn counts in advance (its stop test costs it
nothing here), and both forms are asserted to leave the same records, events and views.  Times are medians over the repeats, the
spread is the half range (max - min) / 2 of the same samples; the forms alternate inside every repeat.  The split of run_rooms:
kernel = the launch interval on the stream (ge_batch_set_timing), unpack = the call with events and views minus the call with neither
(no second copy, no host unpacking: the copy is inside this figure), rest = upload, turn-count copy, synchronisation and the binding."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from game_engine_amd import EVENT_DTYPE, ROOM_VIEW_DTYPE, GameTable, RoomBatch  # noqa: E402

REPS = max(10, int(sys.argv[1])) if len(sys.argv) > 1 else 15
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "run_probe.txt")
N, SEED = 1024, 0x5EED
with open(os.path.join(ROOT, "tests", "golden", "dsl", "werewolf-(mafia).json"), encoding="utf-8") as f:
    dsl = json.load(f)
tb = GameTable(dsl)
rng = np.random.default_rng(3)
rooms = np.arange(N, dtype=np.uint64)
keys = rng.choice(1 << 40, size=N, replace=False).astype(np.uint64)
turns = np.zeros(N, dtype=np.uint32)
lines = []


def say(s=""):
    print(s)
    lines.append(s)


def case(name, mask, until, max_turns):
    b = RoomBatch([(tb, 8, N, mask)], seed=SEED, max_fuse=1)
    start = b.read_rooms()

    def run(full=True):
        if full:
            return b.run_rooms(rooms, keys, turns, max_turns, until)
        played, stopped = np.zeros(N, dtype=np.uint32), np.zeros(N, dtype=np.uint32)
        st = b._lib.ge_batch_run_rooms(b._h, N, rooms.ctypes.data, keys.ctypes.data, turns.ctypes.data, max_turns, until,
                                       played.ctypes.data, stopped.ctypes.data, None, None, 0)
        assert st == 0
        return played, stopped, None, None

    played, stopped, events, views = run()
    after = b.read_rooms()

    def loop():
        ev = np.zeros((N, max_turns), dtype=EVENT_DTYPE)
        vw = np.zeros((N, max_turns), dtype=ROOM_VIEW_DTYPE)
        for t in range(int(played.max())):
            live = np.nonzero(played > t)[0]
            ev[live, t] = b.step_rooms(rooms[live], keys[live], turns[live] + np.uint32(t))
            vw[live, t] = b.read_rooms_at(rooms[live])
        return ev, vw

    b.write_rooms(0, start)
    ev, vw = loop()
    assert b.read_rooms().tobytes() == after.tobytes()
    for k in range(N):
        p = int(played[k])
        assert ev[k, :p].tobytes() == events[k, :p].tobytes() and vw[k, :p].tobytes() == views[k, :p].tobytes()
    t_run, t_loop, t_bare, t_kernel = [], [], [], []
    b.set_timing(True)
    for rep in range(REPS + 1):
        for which in ((0, 1, 2) if rep % 2 else (1, 0, 2)):
            b.write_rooms(0, start)
            b.kernel_time(reset=True)
            t0 = time.perf_counter()
            if which == 0:
                run()
            elif which == 1:
                loop()
            else:
                run(full=False)
            dt = time.perf_counter() - t0
            if rep == 0:
                continue                                         # warm-up: buffers grow, pages fault in
            if which == 0:
                t_run.append(dt)
                t_kernel.append(b.kernel_time(reset=True)[0] * 1e-3)
            elif which == 1:
                t_loop.append(dt)
            else:
                t_bare.append(dt)
    b.close()
    med = statistics.median
    half = lambda x: (max(x) - min(x)) / 2
    r, l, k, bare = med(t_run), med(t_loop), med(t_kernel), med(t_bare)
    say(f"{name}: {N} Werewolf x 8 rooms, human mask {mask:#x}, until {until}, max_turns {max_turns}: {int(played.sum())} room-turns, "
        f"played min / median / max {int(played.min())} / {int(np.median(played))} / {int(played.max())}, "
        f"stopped person / end / limit {int((stopped & 1).astype(bool).sum())} / {int((stopped & 2).astype(bool).sum())} / {int((stopped == 0).sum())}")
    say(f"  run_rooms            {r * 1e3:9.3f} ms  (spread +-{half(t_run) * 1e3:.3f} ms, {REPS} calls)")
    say(f"  step_rooms + read_rooms_at loop {l * 1e3:9.3f} ms  (spread +-{half(t_loop) * 1e3:.3f} ms, {int(played.max())} turns = {2 * int(played.max())} calls)")
    say(f"  ratio loop / run_rooms  x {l / r:.1f}; difference {1e3 * (l - r):.3f} ms against a summed spread of {1e3 * (half(t_run) + half(t_loop)):.3f} ms")
    say(f"  split of run_rooms: kernel {k * 1e3:.3f} ms, second copy + host unpack {max(r - bare, 0) * 1e3:.3f} ms, rest {max(bare - k, 0) * 1e3:.3f} ms")
    assert l - r > half(t_run) + half(t_loop), "run_rooms is not faster than the composition by more than the spread"
    return l / r


say("ge_batch_run_rooms against the host loop of ge_batch_step_rooms + ge_batch_read_rooms_at (tools/run_probe.py), MI355X, wall time")
say()
case("end", 0, 2, 256)
say()
case("person", 1, 3, 64)
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")

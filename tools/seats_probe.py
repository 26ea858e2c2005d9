#!/usr/bin/env python3
"""Per-room seats (POLICY.md §3l): what the seat plane costs, wall time, medians of 20 calls after warm-up.
    python tools/seats_probe.py PARENT_LIB [output file, default profiles/seats_probe.txt]

(a) Batches that do not use the feature.  The indexed kernels now test a plane pointer that is null: step_rooms (1 024 entries),
    run_rooms (1 024 entries x 16 turns, until = nothing) on a 65 536-room Werewolf x 8 batch, find_rooms (person | end) over 65 536
    and 1 048 576 Werewolf x 8 rooms - on a batch WITHOUT a plane, this commit's library against PARENT_LIB, a libge_step.so built
    from the parent commit.  A library is chosen per process (GE_LIB_PATH, as tools/abn.sh does), so every measurement is a child
    process of this script; the children alternate parent, this, parent, this, ... for ROUNDS rounds, and the parent is measured
    twice per round: parent / parent of the same round is the A/A run, its largest deviation from 1 the margin.
(b) The whole-batch step with a plane.  Werewolf x 8 at 65 536 and 1 048 576 rooms, Werewolf x 12 at 2 097 152, Two-Truths x 4 at
    1 048 576; single-turn launches (max_fuse = 1, step(1)) and fused launches (max_fuse = 64, step(64)); the batch with every seat
    mask 1 set through set_seats against the same batch with human_mask = 1 and no plane (the flagship kernels of this commit), the
    two alternated inside every repeat.  A documented cost, not a gate."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARM, REPS, ROUNDS, SEED = 3, 20, 3, 0x5EA7
CALLS = ("step_rooms 1024", "run_rooms 1024 x 16", "find_rooms 65536", "find_rooms 1048576")


def load_dsl(name):
    with open(os.path.join(ROOT, "tests", "golden", "dsl", name + ".json"), encoding="utf-8") as f:
        return json.load(f)


def median_of(fn):
    ts = []
    for rep in range(WARM + REPS):
        t0 = time.perf_counter()
        fn()
        if rep >= WARM:
            ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def child():
    """The calls of (a) on the library GE_LIB_PATH names; one JSON line of medians in seconds."""
    import numpy as np
    from game_engine_amd import GameTable, RoomBatch
    tb = GameTable(load_dsl("werewolf-(mafia)"))
    rng = np.random.default_rng(1)
    out = {}
    with RoomBatch([(tb, 8, 65536, 1)], seed=SEED, restart=True) as b:
        b.step(20)
        rooms = rng.permutation(65536)[:1024].astype(np.uint64)
        keys = rng.integers(0, 1 << 40, 1024).astype(np.uint64)
        turns = rng.integers(0, 1000, 1024).astype(np.uint32)
        out[CALLS[0]] = median_of(lambda: b.step_rooms(rooms, keys, turns))
        out[CALLS[1]] = median_of(lambda: b.run_rooms(rooms, keys, turns, max_turns=16, until=0, views=False))
        out[CALLS[2]] = median_of(lambda: b.find_rooms(("person", "end")))
    with RoomBatch([(tb, 8, 1048576, 1)], seed=SEED, restart=True) as b:
        b.step(20)
        out[CALLS[3]] = median_of(lambda: b.find_rooms(("person", "end")))
    print(json.dumps(out), flush=True)


def run_child(lib):
    env = dict(os.environ)
    if lib:
        env.update(GE_LIB_PATH=os.path.abspath(lib), GE_LIB_ANY_ABI="1")     # (the parent has no seat calls: only shared entry points are used)
    else:
        env.pop("GE_LIB_PATH", None)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, timeout=300)
    if p.returncode != 0:
        raise SystemExit(f"child failed ({lib or 'this commit'}): {p.stderr[-2000:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def part_b(say):
    import numpy as np
    from game_engine_amd import GameTable, RoomBatch
    ww, tt = GameTable(load_dsl("werewolf-(mafia)")), GameTable(load_dsl("two-truths-and-a-lie"))
    for what, tb, n_players, n in (("Werewolf x 8", ww, 8, 65536), ("Werewolf x 8", ww, 8, 1048576), ("Werewolf x 12", ww, 12, 2097152),
                                   ("Two-Truths x 4", tt, 4, 1048576)):
        for max_fuse, k in ((1, 1), (64, 64)):
            with RoomBatch([(tb, n_players, n, 1)], seed=SEED, restart=True, max_fuse=max_fuse) as plain, \
                    RoomBatch([(tb, n_players, n, 1)], seed=SEED, restart=True, max_fuse=max_fuse) as seated:
                seated.set_seats(np.arange(n, dtype=np.uint64), np.ones(n, dtype=np.uint32))
                t = {0: [], 1: []}
                for rep in range(WARM + REPS):
                    for which in ((1, 0) if rep % 2 else (0, 1)):
                        b = seated if which else plain
                        t0 = time.perf_counter()
                        b.step(k)
                        b.sync()
                        if rep >= WARM:
                            t[which].append(time.perf_counter() - t0)
                assert plain.summary() == seated.summary(), "the two batches differ"
                p, s = statistics.median(t[0]), statistics.median(t[1])
                say(f"    {what:<15} {n:>8} rooms, step({k:>2}) at max_fuse {max_fuse:>2}: no plane {p / k * 1e6:9.2f} us/turn, with a plane "
                    f"{s / k * 1e6:9.2f} us/turn, with / without = {s / p:.2f}")


def main():
    parent = sys.argv[1]
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "seats_probe.txt")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"seats_probe: wall time, medians of {REPS} calls after {WARM} warm-up calls")
    say(f"(a) a batch without a plane, this commit against the parent commit's library; {ROUNDS} rounds of parent, this, parent, this")
    ratio, aa = {c: [] for c in CALLS}, {c: [] for c in CALLS}
    for _ in range(ROUNDS):
        p1, t1, p2, t2 = run_child(parent), run_child(None), run_child(parent), run_child(None)
        for c in CALLS:
            ratio[c].append((t1[c] + t2[c]) / (p1[c] + p2[c]))
            aa[c].append(p1[c] / p2[c])
        last = (p1, t1)
    for c in CALLS:
        spread = max(abs(x - 1.0) for x in aa[c])
        r = statistics.median(ratio[c])
        say(f"    {c:<20} parent {last[0][c] * 1e6:9.1f} us, this {last[1][c] * 1e6:9.1f} us (last round); this / parent = {r:.3f} "
            f"(rounds: {', '.join(f'{x:.3f}' for x in ratio[c])}); A/A parent / parent within {spread * 100:.1f} % "
            f"-> {'slower than the margin' if r - 1.0 > spread else 'within the margin'}")
    say("(b) ge_batch_step with a plane (every mask 1, set through set_seats) against the same batch with human_mask = 1 and no plane")
    part_b(say)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if "--child" in sys.argv:
        child()
    else:
        main()

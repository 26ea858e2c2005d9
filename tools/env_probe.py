#!/usr/bin/env python3
"""The learner's loop (POLICY.md §3n: ge_batch_observe_seats, ge_batch_act_seats, game_engine_amd.SeatEnv) measured on the GPU.
    python tools/env_probe.py [output file, default profiles/env_probe.txt] [sizes, default 65536,1048576]

Werewolf x 8, human_mask = 1 (seat 1 host-driven), restart on, 40 turns stepped from the initial state first; seat 1 is then played
by a uniform legal choice.  Every measurement runs in a child process of its own.
  (a) turns per second of two loops on the same batch, medians of REPS windows of LOOP turns each after WARM windows, the forms
      alternated window by window:
        device   SeatEnv.step(SeatEnv.random_legal(obs)): act_seats, step, observe_seats and the choice on torch's stream;
                 the window ends in one synchronise
        host     the way there was before: read_rooms of the batch into a reused array (228 B of view per room), a host-side
                 choice, inject_actions from host arrays, step.  The host's choice here is a uniform living player other than seat
                 1 wherever seat 1 lives - one numpy pass, cheaper than the legality and the redaction a real host has to restate
                 (POLICY.md §3, §3c) -, so the column is a lower bound of that way's cost
  (b) observe_seats alone over the whole batch, seats [1] and [1, 2, 3, 4]: the launch interval from ge_batch_kernel_time (medians
      of REPS calls after WARM), the bytes it moves - the packed records read (32 B per room) and 192 B written per room and
      seat - and their share of 8 TB/s.  (profiles/env_probe.txt also holds the run that settled the store layout of
      csrc/ge_env.inl: the two layouts that lost were in the build of that run, behind a switch that went with them.)"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARM, REPS, LOOP, TURNS, SEED = 3, 15, 16, 40, 0xE27
PEAK = 8e12


def med(xs):
    return statistics.median(xs), (max(xs) - min(xs)) / 2


def make_batch(n):
    from game_engine_amd import GameTable, RoomBatch
    with open(os.path.join(ROOT, "tests", "golden", "dsl", "werewolf-(mafia).json"), encoding="utf-8") as f:
        tb = GameTable(json.load(f))
    b = RoomBatch([(tb, 8, n, 1)], seed=SEED, restart=True)
    b.step(TURNS)
    b.sync()
    return b


def child_observe(n):
    import torch
    out = {}
    with make_batch(n) as b:
        b.set_timing(True)
        for seats in ([1], [1, 2, 3, 4]):
            obs = torch.zeros((n, len(seats), 192), dtype=torch.uint8, device="cuda")
            times = []
            for rep in range(WARM + REPS):
                b.kernel_time(reset=True)
                b.observe_seats(seats, obs)
                ms, _ = b.kernel_time(reset=True)
                if rep >= WARM:
                    times.append(ms * 1e-3)
            out[len(seats)] = times
    print(json.dumps(out))


def child_loop(n):
    import numpy as np
    import torch
    from game_engine_amd import SeatEnv
    with make_batch(n) as b:
        env = SeatEnv(b, [1])
        views = b.read_rooms()
        rooms = np.arange(n, dtype=np.uint64)
        ones = np.ones(n, dtype=np.uint32)
        rng = np.random.default_rng(1)

        def device():
            obs = env.observe()
            for _ in range(LOOP):
                obs, _, _ = env.step(SeatEnv.random_legal(obs))
            torch.cuda.synchronize()

        def host():
            for _ in range(LOOP):
                b.read_rooms(out=views)
                alive = views["players"][:, :8, 2] != 0
                alive[:, 0] = False
                draw = rng.random((n, 8)) * alive
                choice = np.where(alive.any(axis=1) & (views["players"][:, 0, 2] != 0), draw.argmax(axis=1) + 1, 0)
                act = np.flatnonzero(choice)
                b.inject_actions(rooms[act], ones[: len(act)], choice[act])
                b.step(1)
            b.sync()

        t = {"device": [], "host": []}
        for rep in range(WARM + REPS):
            for which in (("device", device), ("host", host))[:: 1 if rep % 2 else -1]:
                t0 = time.perf_counter()
                which[1]()
                dt = time.perf_counter() - t0
                if rep >= WARM:
                    t[which[0]].append(dt)
    print(json.dumps(t))


def run_child(what, n):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what, str(n)], capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        raise SystemExit(f"child {what} {n} failed ({p.returncode}):\n{p.stderr[-3000:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "env_probe.txt")
    sizes = [int(x) for x in sys.argv[2].split(",")] if len(sys.argv) > 2 else [65536, 1048576]
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"env_probe: Werewolf x 8, human_mask = 1, restart on, {TURNS} turns stepped first; medians of {REPS} after {WARM} warm-ups, +- = (max - min) / 2")
    say()
    say(f"(b) observe_seats alone, whole batch: launch interval (ge_batch_kernel_time), bytes moved, share of {PEAK / 1e12:.0f} TB/s")
    for n in sizes:
        got = run_child("observe", n)
        for s in (1, 4):
            m, sp = med(got[str(s)])
            moved = n * (32 + 192 * s)
            say(f"  {n:>8} rooms x {s} seat{'s' if s > 1 else ' '}: {m * 1e6:8.1f} us +- {sp * 1e6:5.1f}   "
                f"{moved / 1e6:7.1f} MB   {moved / m / 1e12:5.2f} TB/s = {100 * moved / m / PEAK:4.1f} %")
    say()
    say(f"(a) the loop, seat 1 played by a uniform legal choice: turns per second, windows of {LOOP} turns")
    for n in sizes:
        got = run_child("loop", n)
        d, ds = med(got["device"])
        h, hs = med(got["host"])
        say(f"  {n:>8} rooms: device (SeatEnv) {LOOP / d:9.1f} turns/s ({d / LOOP * 1e3:7.3f} ms per turn +- {ds / LOOP * 1e3:.3f})   "
            f"host (read_rooms, numpy choice, inject_actions, step) {LOOP / h:8.2f} turns/s ({h / LOOP * 1e3:8.2f} ms per turn +- {hs / LOOP * 1e3:.2f})   x {h / d:.1f}")
    with open(out_path, "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        {"observe": child_observe, "loop": child_loop}[sys.argv[2]](int(sys.argv[3]))
    else:
        main()

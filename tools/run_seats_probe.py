#!/usr/bin/env python3
"""The learner's loop stepped to its next decision (POLICY.md §3p: ge_batch_run_seats, SeatEnv.step_until) measured on the GPU.
    python tools/run_seats_probe.py [output file, default profiles/run_seats_probe.txt] [sizes, default 65536,1048576]

Werewolf x 8, human_mask = 1 (seat 1 host-driven), restart on, 40 turns stepped from the initial state first; seat 1 is then played
by SeatEnv.random_legal.  Every measurement runs in a child process of its own.
  (a) wall time per decision point delivered - an observation entry with legal != 0 or done = 1, counted on the device -, two ways
      on the same batch, medians of REPS windows after WARM, the forms alternated window by window:
        until    SeatEnv.step_until(random_legal(obs), 16): act_seats, run_seats, observe_seats; windows of CALLS calls
        single   the only way without the call that loses no game end under restart: SeatEnv.step(random_legal(obs), 1), a turn
                 per call; windows of CALLS * 16 calls.  It is timed twice in the same run (single, single'): their ratio is the
                 spread a ratio of this table has by itself
      every window ends in one synchronise.
  (b) run_seats alone inside the until loop: the launch interval from ge_batch_kernel_time, the mean of `played`, and the share of
      wavefront-turns spent by shadow lanes - 1 - mean(played) / mean over wavefronts of max(played): a wavefront leaves with its
      last room, which is the call's inherent cost."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARM, REPS, CALLS, MAX_TURNS, TURNS, SEED = 3, 15, 4, 16, 40, 0xE27


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


def child_loop(n):
    import torch
    from game_engine_amd import SeatEnv
    with make_batch(n) as b:
        env = SeatEnv(b, [1])

        def points(obs, acc):
            f = SeatEnv.fields(obs)
            acc += ((f["legal_bits"] != 0) | f["done"]).sum()

        def window(calls, step):
            acc = torch.zeros((), dtype=torch.int64, device="cuda")
            obs = env.observe()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                obs, _, _ = step(SeatEnv.random_legal(obs))
                points(obs, acc)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, int(acc.item())

        forms = {"until": lambda: window(CALLS, lambda a: env.step_until(a, MAX_TURNS)),
                 "single": lambda: window(CALLS * MAX_TURNS, lambda a: env.step(a, 1)),
                 "single'": lambda: window(CALLS * MAX_TURNS, lambda a: env.step(a, 1))}
        order = list(forms)
        t = {k: [] for k in forms}
        for rep in range(WARM + REPS):
            for k in order[rep % 3:] + order[:rep % 3]:
                dt, cnt = forms[k]()
                if rep >= WARM:
                    t[k].append((dt, cnt))
    print(json.dumps(t))


def child_alone(n):
    import torch
    from game_engine_amd import SeatEnv
    out = {"us": [], "played": [], "shadow": []}
    with make_batch(n) as b:
        env = SeatEnv(b, [1])
        obs = env.observe()
        env.step_until(SeatEnv.random_legal(obs), MAX_TURNS)
        b.set_timing(True)
        for rep in range(WARM + REPS):
            b.act_seats(env.seats, SeatEnv.random_legal(env.obs), env.status)
            b.kernel_time(reset=True)
            b.run_seats(env.seats, env.played, env.stopped, MAX_TURNS)
            ms, _ = b.kernel_time(reset=True)
            b.observe_seats(env.seats, env.obs)
            torch.cuda.synchronize()
            if rep >= WARM:
                p = env.played.double()
                full = p[: (n // 64) * 64].reshape(-1, 64)
                out["us"].append(ms * 1e3)
                out["played"].append(float(p.mean()))
                out["shadow"].append(1.0 - float(full.mean() / full.max(dim=1).values.mean()))
    print(json.dumps(out))


def run_child(what, n):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what, str(n)], capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        raise SystemExit(f"child {what} {n} failed ({p.returncode}):\n{p.stderr[-3000:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "run_seats_probe.txt")
    sizes = [int(x) for x in sys.argv[2].split(",")] if len(sys.argv) > 2 else [65536, 1048576]
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"run_seats_probe: Werewolf x 8, human_mask = 1, restart on, {TURNS} turns stepped first, seat 1 played by random_legal; "
        f"medians of {REPS} after {WARM} warm-ups, +- = (max - min) / 2")
    say()
    say(f"(a) wall time per decision point delivered (entries with legal != 0 or done): step_until(max_turns = {MAX_TURNS}), windows of {CALLS} calls, "
        f"against step(actions, 1), windows of {CALLS * MAX_TURNS} calls, timed twice")
    for n in sizes:
        got = run_child("loop", n)
        row = {}
        for k, v in got.items():
            per, sp = med([dt / max(cnt, 1) for dt, cnt in v])
            row[k] = (per, sp, statistics.median(cnt for _, cnt in v), statistics.median(dt for dt, _ in v))
        u, s, s2 = row["until"], row["single"], row["single'"]
        say(f"  {n:>8} rooms: until {u[0] * 1e9:8.2f} ns per point +- {u[1] * 1e9:.2f} ({u[2]:.0f} points in {u[3] * 1e3:.2f} ms)   "
            f"single {s[0] * 1e9:8.2f} ns +- {s[1] * 1e9:.2f} ({s[2]:.0f} points in {s[3] * 1e3:.2f} ms)   "
            f"single' {s2[0] * 1e9:8.2f} ns +- {s2[1] * 1e9:.2f}   single / until x {s[0] / u[0]:.2f}   single' / single x {s2[0] / s[0]:.2f}")
    say()
    say(f"(b) run_seats alone (max_turns = {MAX_TURNS}, until seat | end) inside the loop: launch interval (ge_batch_kernel_time), mean played, shadow share of wavefront-turns")
    for n in sizes:
        got = run_child("alone", n)
        us, sp = med(got["us"])
        say(f"  {n:>8} rooms: {us:8.1f} us +- {sp:5.1f}   mean played {statistics.median(got['played']):5.2f}   "
            f"shadow share {100 * statistics.median(got['shadow']):4.1f} %")
    with open(out_path, "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        {"loop": child_loop, "alone": child_alone}[sys.argv[2]](int(sys.argv[3]))
    else:
        main()

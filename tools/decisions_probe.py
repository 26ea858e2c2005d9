#!/usr/bin/env python3
"""Decision lists (POLICY.md §3q: ge_batch_gather_seats, ge_batch_act_listed, SeatEnv.step_decisions) measured on the GPU.
    python tools/decisions_probe.py [output file, default profiles/decisions_probe.txt] [sizes, default 65536,1048576]

Werewolf x 8, all eight seats listed and host-driven (human_mask = 255), restart on, 40 turns stepped from the initial state first;
the seats are then played by SeatEnv.random_legal, max_turns = 16.  Every measurement runs in a child process of its own.
  (a) wall time per decision point delivered - an entry with legal != 0 or done = 1 -, two ways on the same batch and the same
      build, medians of REPS windows of CALLS calls after WARM, the forms alternated window by window, every window ending in one
      synchronise.  Both ways are the RoomBatch calls themselves with the choice between them, nothing else inside the window:
        list     act_listed, run_seats, gather_seats, random_legal over all cap rows of the list (cap = rooms x 8: the caller
                 does not know the list's length)
        dense    the way there is without the two calls: act_seats, run_seats, observe_seats over eight seats, random_legal over
                 [rooms, 8].  Timed twice in the same run (dense, dense'): their ratio is the spread a ratio of this table has
                 by itself
      The decision points are counted behind the window's synchronise, outside the timed region, in both ways: each call of a
      window stores its result where the count can read it afterwards - the list's n_dev in a buffer per call, the dense
      observations in an obs tensor per call.
  (b) gather_seats alone against observe_seats alone on the same batch at the same moment of the list loop: the launch interval
      from ge_batch_kernel_time, the bytes moved (records read twice and the due words written and read, due x 196 bytes written,
      against records read and entries x 192 bytes written), the share of entries that were due, and the kernels of both loops
      from `rocprofv3 --kernel-trace` runs of their own: the split of the list calls between test, scan and emit, and the sum of
      the library's kernels per call of each loop (the torch kernels of random_legal are the same work in both and are left out).
  (c) the emit launch by store layout was measured once, on a build that held both layouts, and is recorded in
      profiles/decisions_probe_stores.txt; the slower layout has been deleted, so this tool no longer times it.
  (d) (a) at the one-seat shape of profiles/run_seats_probe.txt - human_mask = 1, seat 1 listed -, where almost every entry is due."""
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARM, REPS, CALLS, MAX_TURNS, TURNS, SEED = 3, 15, 4, 16, 40, 0xE27
SHAPES = {"all": (255, list(range(1, 9))), "one": (1, [1])}
RECORD_BYTES = 32                      # a Werewolf x 8 record


def med(xs):
    return statistics.median(xs), (max(xs) - min(xs)) / 2


def make_batch(n, shape):
    from game_engine_amd import GameTable, RoomBatch
    with open(os.path.join(ROOT, "tests", "golden", "dsl", "werewolf-(mafia).json"), encoding="utf-8") as f:
        tb = GameTable(json.load(f))
    b = RoomBatch([(tb, 8, n, SHAPES[shape][0])], seed=SEED, restart=True)
    b.step(TURNS)
    b.sync()
    return b


def loop_forms(b, env, torch):
    """the two loops as windows of CALLS calls: {name: window() -> (seconds, decision points)}; the points are counted behind the
    window's synchronise, from what each call of the window left in a buffer of its own"""
    from game_engine_amd import SeatEnv
    seats, rooms = env.seats, b.n_rooms
    cap = rooms * len(seats)
    dev = env.obs.device
    stream = lambda: int(torch.cuda.current_stream(dev).cuda_stream)
    played = torch.zeros(rooms, dtype=torch.int32, device=dev)
    stopped = torch.zeros(rooms, dtype=torch.int32, device=dev)
    # list: one list, n_dev of every call kept
    dec_obs = torch.zeros((cap, 192), dtype=torch.uint8, device=dev)
    dec_entries = torch.zeros(cap, dtype=torch.int32, device=dev)
    dec_status = torch.zeros(cap, dtype=torch.int32, device=dev)
    ns = [torch.zeros(2, dtype=torch.int32, device=dev) for _ in range(CALLS + 1)]
    # dense: the observations of every call kept
    obs = [torch.zeros((rooms, len(seats), 192), dtype=torch.uint8, device=dev) for _ in range(CALLS + 1)]
    status = torch.zeros((rooms, len(seats)), dtype=torch.int32, device=dev)

    def window_list():
        st = stream()
        b.gather_seats(seats, dec_obs, dec_entries, ns[CALLS], stream=st)
        torch.cuda.synchronize()
        n = ns[CALLS]
        t0 = time.perf_counter()
        for i in range(CALLS):
            b.act_listed(seats, n, dec_entries, SeatEnv.random_legal(dec_obs), dec_status, cap=cap, stream=st)
            b.run_seats(seats, played, stopped, MAX_TURNS, stream=st)
            n = ns[i]
            b.gather_seats(seats, dec_obs, dec_entries, n, stream=st)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return dt, sum(int(x[0]) for x in ns[:CALLS])

    def window_dense():
        st = stream()
        o = obs[CALLS]
        b.observe_seats(seats, o, stream=st)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(CALLS):
            b.act_seats(seats, SeatEnv.random_legal(o), status, stream=st)
            b.run_seats(seats, played, stopped, MAX_TURNS, stream=st)
            o = obs[i]
            b.observe_seats(seats, o, stream=st)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        cnt = 0
        for x in obs[:CALLS]:
            f = SeatEnv.fields(x)
            cnt += int(((f["legal_bits"] != 0) | f["done"]).sum())
        return dt, cnt

    return {"list": window_list, "dense": window_dense, "dense'": window_dense}


def child_loop(n, shape):
    import torch
    from game_engine_amd import SeatEnv
    with make_batch(n, shape) as b:
        env = SeatEnv(b, SHAPES[shape][1])
        forms = loop_forms(b, env, torch)
        order = list(forms)
        t = {k: [] for k in forms}
        for rep in range(WARM + REPS):
            for k in order[rep % 3:] + order[:rep % 3]:
                dt, cnt = forms[k]()
                if rep >= WARM:
                    t[k].append((dt, cnt))
    print(json.dumps(t))


def child_alone(n, shape):
    """gather_seats and observe_seats on the same records, inside the list loop"""
    import torch
    from game_engine_amd import SeatEnv
    out = {"gather_us": [], "observe_us": [], "due": [], "count_us": []}
    with make_batch(n, shape) as b:
        env = SeatEnv(b, SHAPES[shape][1])
        dec_obs, dec_entries, dec_n = env.decisions()
        env.observe()
        b.set_timing(True)
        for rep in range(WARM + REPS):
            env.step_decisions(SeatEnv.random_legal(dec_obs), MAX_TURNS)
            torch.cuda.synchronize()
            b.kernel_time(reset=True)
            b.gather_seats(env.seats, dec_obs, dec_entries, dec_n)
            g_ms, _ = b.kernel_time(reset=True)
            b.observe_seats(env.seats, env.obs)
            o_ms, _ = b.kernel_time(reset=True)
            b.gather_seats(env.seats, None, None, dec_n, cap=0)   # test and scan only
            c_ms, _ = b.kernel_time(reset=True)
            b.gather_seats(env.seats, dec_obs, dec_entries, dec_n)
            torch.cuda.synchronize()
            if rep >= WARM:
                out["gather_us"].append(g_ms * 1e3)
                out["observe_us"].append(o_ms * 1e3)
                out["count_us"].append(c_ms * 1e3)
                out["due"].append(int(dec_n[1]))
    print(json.dumps(out))


def child_trace(n, shape, form="list"):
    """the windows a kernel-trace run takes its medians over: one of the two loops of (a)"""
    import torch
    from game_engine_amd import SeatEnv
    with make_batch(n, shape) as b:
        env = SeatEnv(b, SHAPES[shape][1])
        window = loop_forms(b, env, torch)[form]
        for _ in range(WARM + REPS):
            window()


def run_child(what, n, shape):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what, str(n), shape], capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        raise SystemExit(f"child {what} {n} {shape} failed ({p.returncode}):\n{p.stderr[-3000:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


KINDS = (("ge_gather_test", "test"), ("ge_gather_scan", "scan"), ("ge_gather_emit", "emit"), ("ge_observe_kernel", "observe"),
         ("ge_list_scatter", "scatter"), ("ge_list_status", "status"), ("ge_act_kernel", "act"), ("ge_seat_run_kernel", "run"))


def trace_split(n, shape, form):
    """{kind: median ns per launch} over the steady windows of a rocprofv3 --kernel-trace run of child_trace"""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    d = tempfile.mkdtemp(prefix="decisions_probe_")
    try:
        p = subprocess.run([prof, "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--child", "trace",
                            str(n), shape, form], capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            raise SystemExit(f"rocprofv3 run failed ({p.returncode}):\n{p.stderr[-3000:]}")
        rows = []
        for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            with open(path, newline="") as f:
                rows += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(f)]
    finally:
        shutil.rmtree(d, ignore_errors=True)
    rows.sort()
    per = {}
    for s, e, name in rows:
        for key, kind in KINDS:
            if key in name:
                per.setdefault(kind, []).append(e - s)
                break
    windows = WARM + REPS
    return {kind: statistics.median(v[len(v) * WARM // windows:]) for kind, v in per.items()}


def loop_rows(say, sizes, shape):
    for n in sizes:
        got = run_child("loop", n, shape)
        row = {}
        for k, v in got.items():
            per, sp = med([dt / max(cnt, 1) for dt, cnt in v])
            row[k] = (per, sp, statistics.median(cnt for _, cnt in v), statistics.median(dt for dt, _ in v))
        ls, d, d2 = row["list"], row["dense"], row["dense'"]
        entries = CALLS * n * len(SHAPES[shape][1])
        say(f"  {n:>8} rooms: list {ls[0] * 1e9:8.2f} ns per point +- {ls[1] * 1e9:.2f} ({ls[2]:.0f} points in {ls[3] * 1e3:.2f} ms)   "
            f"dense {d[0] * 1e9:8.2f} ns +- {d[1] * 1e9:.2f} ({d[2]:.0f} points of {entries} entries in {d[3] * 1e3:.2f} ms)   "
            f"dense' {d2[0] * 1e9:8.2f} ns +- {d2[1] * 1e9:.2f}   dense / list x {d[0] / ls[0]:.2f}   dense' / dense x {d2[0] / d[0]:.2f}")


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "decisions_probe.txt")
    sizes = [int(x) for x in sys.argv[2].split(",")] if len(sys.argv) > 2 else [65536, 1048576]
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"decisions_probe: Werewolf x 8, all eight seats listed and host-driven, restart on, {TURNS} turns stepped first, seats played by "
        f"random_legal, max_turns = {MAX_TURNS}; medians of {REPS} after {WARM} warm-ups, +- = (max - min) / 2")
    say()
    say(f"(a) wall time per decision point delivered (entries with legal != 0 or done), windows of {CALLS} calls: act_listed, run_seats, gather_seats, "
        f"random_legal over the list's cap rows against act_seats, run_seats, observe_seats, random_legal over [rooms, 8], the latter timed twice; "
        f"points counted outside the timed region")
    loop_rows(say, sizes, "all")
    say()
    say("(b) gather_seats alone against observe_seats alone, eight seats, the same records: launch interval (ge_batch_kernel_time), bytes moved, share of entries due")
    for n in sizes:
        got = run_child("alone", n, "all")
        g, gs = med(got["gather_us"])
        o, os_ = med(got["observe_us"])
        c, cs = med(got["count_us"])
        due = statistics.median(got["due"])
        g_bytes = 2 * n * RECORD_BYTES + 2 * 4 * n + due * 196
        o_bytes = n * RECORD_BYTES + 8 * n * 192
        say(f"  {n:>8} rooms: gather_seats {g:8.1f} us +- {gs:5.1f} ({g_bytes / 1e6:8.1f} MB, {g_bytes / g / 1e6:5.2f} TB/s)   "
            f"observe_seats {o:8.1f} us +- {os_:5.1f} ({o_bytes / 1e6:8.1f} MB, {o_bytes / o / 1e6:5.2f} TB/s)   observe / gather x {o / g:.2f}   "
            f"due {due:.0f} of {8 * n} entries ({100 * due / (8 * n):.1f} %)   gather_seats with cap = 0 (test and scan) {c:8.1f} us +- {cs:5.1f}")
    say()
    say("(b) the library's kernels in both loops of (a): rocprofv3 --kernel-trace, median per launch, and their sum per call")
    for n in sizes:
        for form in ("list", "dense"):
            got = trace_split(n, "all", form)
            parts = "   ".join(f"{kind} {got[kind] / 1e3:8.1f} us" for _, kind in KINDS if kind in got)
            say(f"  {n:>8} rooms, {form:>5} loop: {parts}   sum {sum(got.values()) / 1e3:8.1f} us")
    say()
    say("(c) the emit launch by store layout: measured once on a build that held both layouts, profiles/decisions_probe_stores.txt")
    say()
    say("(d) (a) at human_mask = 1, seat 1 listed: the shape of profiles/run_seats_probe.txt, where almost every entry is due")
    loop_rows(say, sizes, "one")
    with open(out_path, "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        {"loop": child_loop, "alone": child_alone, "trace": child_trace}[sys.argv[2]](int(sys.argv[3]), *sys.argv[4:])
    else:
        main()

#!/usr/bin/env python3
"""The teacher of the learner's loop (POLICY.md §3o: ge_batch_teach_seats, RoomBatch.teach_seats) measured on the GPU.
    python tools/teach_probe.py [output file, default profiles/teach_probe.txt] [sizes, default 4096,65536]

Werewolf x 8, human_mask = 1 (seat 1 host-driven), restart on, 40 turns stepped from the initial state first; seat 1 of every room
is advised at 64 playouts per choice, played to the end (max_turns 1024).  Every measurement runs in a child process of its own;
medians of REPS after WARM warm-ups.
  (a) the advice of seat 1 of every room as a torch tensor on the device, end to end with a final synchronise, two ways on the
      same batch, alternated repeat by repeat; the two results are compared byte for byte before anything is timed:
        teach    teach_seats into the tensor
        before   the way there was before: observe_seats, `legal` copied to the host, the due pairs listed in numpy, advise_seats
                 over them, the refusals filled in and the records uploaded
      and the launch interval of teach_seats alone (ge_batch_kernel_time).
  (c) the dead-slot overhead: the same call on the same batch before any turn is stepped, where no pair is due (checked: every
      record is a refusal) - the plan, the memset, the playout grid of every slot, each wavefront leaving at its first test, and
      the reduce - as a share of (a)'s teach.
  (b) the split of the call's kernel time into plan, playouts, reduce (and the runtime's fill kernel of the memset, where the trace
      shows it): medians over the calls of a `rocprofv3 --kernel-trace` run of its own, per pass and summed over the call's passes.
  (d) the reduce kernel with its records staged through LDS against each lane storing its own record, from the same kind of run.
      This part needs a build that still has both (GE_TEACH_STORES=direct selects the second); the committed library keeps the
      faster one only, and profiles/teach_probe.txt holds the run that settled it.  `--stores` runs it.
  (b) and (d) also at 65 536 rooms x seats 1 .. 4 at 16 playouts per choice, where the reduce writes four times the records."""
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

WARM, REPS, TURNS, SEED = 3, 15, 40, 0xE27
N_ROLLOUTS, MAX_TURNS = 64, 1024
SHAPES = {"1": ([1], 64), "4": ([1, 2, 3, 4], 16)}              # (b), (d): seat list and playouts per choice


def med(xs):
    return statistics.median(xs), (max(xs) - min(xs)) / 2


def make_batch(n, turns=TURNS):
    from game_engine_amd import GameTable, RoomBatch
    with open(os.path.join(ROOT, "tests", "golden", "dsl", "werewolf-(mafia).json"), encoding="utf-8") as f:
        tb = GameTable(json.load(f))
    b = RoomBatch([(tb, 8, n, 1)], seed=SEED, restart=True)
    if turns:
        b.step(turns)
    b.sync()
    return b


def child_ab(n):
    import numpy as np
    import torch
    from game_engine_amd import SeatEnv
    from game_engine_amd.stepper import ADVICE_DTYPE
    out = {}
    with make_batch(n) as b:
        turn = b.turn
        obs = torch.zeros((n, 1, 192), dtype=torch.uint8, device="cuda")
        adv = torch.zeros((n, 1, 224), dtype=torch.uint8, device="cuda")
        old = torch.zeros((n, 224), dtype=torch.uint8, device="cuda")
        keys = (np.arange(n, dtype=np.uint64) << np.uint64(20))
        host = np.zeros(n, dtype=ADVICE_DTYPE)
        pinned = torch.zeros((n, 224), dtype=torch.uint8).pin_memory()

        def teach():
            b.teach_seats([1], adv, N_ROLLOUTS, MAX_TURNS)
            torch.cuda.synchronize()

        def before():
            b.observe_seats([1], obs)
            legal = SeatEnv.fields(obs)["legal_bits"][:, 0].cpu().numpy()
            due = np.flatnonzero(legal).astype(np.uint64)
            got = b.advise_seats(due, keys[due.astype(np.int64)], np.full(len(due), turn, dtype=np.uint32), np.ones(len(due), dtype=np.uint32),
                                 N_ROLLOUTS, MAX_TURNS)
            host[:] = np.zeros((), dtype=ADVICE_DTYPE)
            host["status"] = -1
            host[due.astype(np.int64)] = got
            pinned.numpy()[:] = host.view(np.uint8).reshape(n, 224)
            old.copy_(pinned, non_blocking=True)
            torch.cuda.synchronize()
            return len(due)

        teach()
        due = before()
        assert torch.equal(adv[:, 0], old), "teach_seats and the path before it disagree"
        t = {"teach": [], "before": []}
        for rep in range(WARM + REPS):
            for name, f in (("teach", teach), ("before", before))[:: 1 if rep % 2 else -1]:
                t0 = time.perf_counter()
                f()
                dt = time.perf_counter() - t0
                if rep >= WARM:
                    t[name].append(dt)
        b.set_timing(True)
        interval = []
        for rep in range(WARM + REPS):
            b.kernel_time(reset=True)
            b.teach_seats([1], adv, N_ROLLOUTS, MAX_TURNS)
            ms, _ = b.kernel_time(reset=True)
            if rep >= WARM:
                interval.append(ms * 1e-3)
        out.update(t, interval=interval, due=due)
    with make_batch(n, 0) as b:                                  # (c): nothing stepped, nobody due
        adv = torch.zeros((n, 1, 224), dtype=torch.uint8, device="cuda")
        dead = []
        for rep in range(WARM + REPS):
            t0 = time.perf_counter()
            b.teach_seats([1], adv, N_ROLLOUTS, MAX_TURNS)
            torch.cuda.synchronize()
            if rep >= WARM:
                dead.append(time.perf_counter() - t0)
        status = SeatEnv.advice_fields(adv)["status"]
        out.update(dead=dead, dead_due=int((status == 0).sum()))
    print(json.dumps(out))


def child_split(n, shape):
    """the calls a kernel-trace run takes its medians over"""
    import torch
    seats, n_rollouts = SHAPES[shape]
    with make_batch(n) as b:
        adv = torch.zeros((n, len(seats), 224), dtype=torch.uint8, device="cuda")
        for _ in range(WARM + REPS):
            b.teach_seats(seats, adv, n_rollouts, MAX_TURNS)
            torch.cuda.synchronize()


def run_child(what, *args):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what] + [str(a) for a in args], capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        raise SystemExit(f"child {what} {args} failed ({p.returncode}):\n{p.stderr[-3000:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


KINDS = (("ge_teach_plan", "plan"), ("ge_rollout_kernel", "playouts"), ("ge_teach_reduce", "reduce"), ("fill", "memset"))


def trace_split(n, shape, stores=None):
    """{kind: (median ns per launch, launches per call)} over the steady calls of a rocprofv3 --kernel-trace run of child_split"""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    d = tempfile.mkdtemp(prefix="teach_probe_")
    env = dict(os.environ)
    if stores:
        env["GE_TEACH_STORES"] = stores
    try:
        p = subprocess.run([prof, "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--child", "split",
                            str(n), shape], capture_output=True, text=True, timeout=900, env=env)
        if p.returncode != 0:
            raise SystemExit(f"rocprofv3 run failed ({p.returncode}):\n{p.stderr[-3000:]}")
        rows = []
        for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            with open(path, newline="") as f:
                rows += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(f)]
    finally:
        shutil.rmtree(d, ignore_errors=True)
    rows.sort()
    first = next(i for i, r in enumerate(rows) if "ge_teach_plan" in r[2])     # behind the batch's own fill and step launches
    per = {}
    for s, e, name in rows[first:]:
        for key, kind in KINDS:
            if key in name:
                per.setdefault(kind, []).append(e - s)
                break
    calls = WARM + REPS
    return {kind: (statistics.median(v[len(v) * WARM // calls:]), len(v) / calls) for kind, v in per.items()}


def main():
    args = [a for a in sys.argv[1:] if a != "--stores"]
    stores = "--stores" in sys.argv
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "teach_probe.txt")
    sizes = [int(x) for x in args[1].split(",")] if len(args) > 1 else [4096, 65536]
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"teach_probe: Werewolf x 8, human_mask = 1, restart on, {TURNS} turns stepped first; seat 1 of every room, {N_ROLLOUTS} playouts per choice, "
        f"max_turns {MAX_TURNS}; medians of {REPS} after {WARM} warm-ups, +- = (max - min) / 2")
    say()
    say("(a) the advice of every room as a device tensor, end to end with a final synchronise; (c) the same call where no pair is due")
    for n in sizes:
        got = run_child("ab", n)
        t, ts = med(got["teach"])
        o, os_ = med(got["before"])
        k, ks = med(got["interval"])
        dd, ds = med(got["dead"])
        say(f"  {n:>6} rooms ({got['due']} due): teach_seats {t * 1e3:8.3f} ms +- {ts * 1e3:.3f} (launch interval {k * 1e3:8.3f} ms +- {ks * 1e3:.3f})   "
            f"before (observe_seats, legal to the host, numpy, advise_seats, upload) {o * 1e3:8.3f} ms +- {os_ * 1e3:.3f}   x {o / t:.2f}")
        say(f"  {n:>6} rooms, nothing stepped ({got['dead_due']} due): teach_seats {dd * 1e3:8.3f} ms +- {ds * 1e3:.3f} = {100 * dd / t:.1f} % of the call above")
    say()
    say("(b) kernel time of one call, rocprofv3 --kernel-trace: median per launch x launches per call" + ("; (d) the reduce by store layout" if stores else ""))
    for n, shape in [(n, "1") for n in sizes] + [(sizes[-1], "4")]:
        seats, n_rollouts = SHAPES[shape]
        for mode in ([None, "direct"] if stores else [None]):
            got = trace_split(n, shape, mode)
            total = sum(m * c for m, c in got.values())
            parts = "   ".join(f"{kind} {m / 1e3:9.1f} us x {c:4.1f} = {m * c / 1e3:10.1f} us ({100 * m * c / total:4.1f} %)" for kind, (m, c) in sorted(got.items()))
            say(f"  {n:>6} rooms x {len(seats)} seat{'s' if len(seats) > 1 else ' '}, {n_rollouts} playouts"
                f"{', reduce: ' + ('each lane its own record' if mode else 'through LDS') if stores else ''}: {parts}")
    with open(out_path, "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        if sys.argv[2] == "ab":
            child_ab(int(sys.argv[3]))
        else:
            child_split(int(sys.argv[3]), sys.argv[4])
    else:
        main()

#!/usr/bin/env python3
"""Wall time of adopting Werewolf x 8 views into pool chunks: one RoomBatch.write_rooms_at per chunk (ge_batch_write_rooms_at:
one copy, one ge_pool_scatter launch) against one write_rooms per slot, for 1 024 and 65 536 views over 1 024-slot chunks.

    python tools/adopt_probe.py [--out profiles/adopt_probe.txt]

The kernel time of ge_pool_scatter comes from a run of its own under the kernel trace, read back from the trace database:
    rocprofv3 --kernel-trace --stats -d <dir> -o adopt -- python tools/adopt_probe.py --kernel-only
    python tools/adopt_probe.py --out profiles/adopt_probe.txt --trace-db <dir>/adopt_results.db
The views are mid-game rooms of a batch stepped a few turns (no test module is imported).
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kernel_lines(db_path):
    """ge_pool_scatter launches of a rocprofv3 trace database, by grid size (entries rounded up to 64)."""
    import sqlite3
    db = sqlite3.connect(db_path)
    rows = db.execute("select grid_x, count(*), avg(duration), min(duration), max(duration) from kernels "
                      "where name like '%ge_pool_scatter%' group by grid_x order by grid_x").fetchall()
    return [f"ge_pool_scatter, {g:>5} lanes: {c} launches, avg {a / 1e3:.2f} us, min {lo / 1e3:.2f} us, max {hi / 1e3:.2f} us"
            for g, c, a, lo, hi in rows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--trace-db", default=None, help="a rocprofv3 results database of a --kernel-only run: adds the kernel times")
    a = ap.parse_args()
    import json
    from game_engine_amd import GameTable, RoomBatch
    with open(os.path.join(ROOT, "tests", "golden", "dsl", "werewolf-(mafia).json"), encoding="utf-8") as f:
        tb = GameTable(json.load(f))
    chunk_rooms, lines = 1024, []
    with RoomBatch([(tb, 8, 65536)], seed=1) as src:             # mid-game rooms: a batch stepped a few turns
        src.step(9)
        pool_views = src.read_rooms()
    for n in (1024, 65536):
        views = pool_views[:n]
        chunks = [RoomBatch([(tb, 8, chunk_rooms)], max_fuse=1) for _ in range(n // chunk_rooms)]
        slots = np.arange(chunk_rooms, dtype=np.uint64)
        for c in chunks:                                         # warm: staging buffers and device scratch
            c.write_rooms_at(slots[:1], views[:1])
            c.write_rooms(0, views[:1])
        best_at = best_one = float("inf")
        for _ in range(1 if a.kernel_only else 5):
            t0 = time.perf_counter()
            for ci, c in enumerate(chunks):
                c.write_rooms_at(slots, views[ci * chunk_rooms:(ci + 1) * chunk_rooms])
            best_at = min(best_at, time.perf_counter() - t0)
            if a.kernel_only:
                break
            t0 = time.perf_counter()
            for ci, c in enumerate(chunks):
                for s in range(chunk_rooms):
                    c.write_rooms(s, views[ci * chunk_rooms + s:ci * chunk_rooms + s + 1])
            best_one = min(best_one, time.perf_counter() - t0)
        for c in chunks:
            c.close()
        if not a.kernel_only:
            lines.append(f"{n:>6} views, {len(chunks):>3} chunks: write_rooms_at per chunk {best_at * 1e3:9.2f} ms "
                         f"({n / best_at / 1e6:6.2f} M views/s); write_rooms per slot {best_one * 1e3:9.2f} ms "
                         f"({n / best_one / 1e6:6.3f} M views/s); {best_one / best_at:5.1f}x")
    if a.trace_db:
        lines += kernel_lines(a.trace_db)
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write("adopt_probe (first measurements; best of 5 wall times, Werewolf x 8, 1 024-slot chunks; kernel times from a\n"
                    "rocprofv3 --kernel-trace run of --kernel-only, 65 launches per size: 1 warm-up entry, then full chunks)\n" + text + "\n")


if __name__ == "__main__":
    main()

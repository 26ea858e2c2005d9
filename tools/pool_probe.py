#!/usr/bin/env python3
"""Messages per second for 1 024 live threads (Werewolf x 8, bots only): RoomService (one N = 1 batch per thread; per
message a launch, a read of the room, a read of the event, each synchronising) against RoomPoolService (1 024-slot chunks;
per tick and chunk one step_rooms and one read_rooms_at), at ticks of 1, 64 and 1 024 "Continue" messages to distinct
threads.  Wall time of the whole service call, rendering of the tool calls included.
python tools/pool_probe.py [messages per measurement]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from game_engine_amd import RoomPoolService, RoomService  # noqa: E402

THREADS, GAME, N = 1024, "werewolf-(mafia)", 8
msgs_per_run = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
with open(os.path.join(ROOT, "tests", "golden", "dsl", f"{GAME}.json"), encoding="utf-8") as f:
    dsl = json.load(f)
players = [{"name": f"Player {i + 1}"} for i in range(N)]
tids = [f"thread-{i}" for i in range(THREADS)]


def measure(serve_tick, tick, rng):
    """messages per second over msgs_per_run messages in ticks of `tick` distinct threads (after one warm-up tick)"""
    serve_tick([(t, "Continue") for t in rng.choice(tids, size=tick, replace=False)])
    n, t0 = 0, time.perf_counter()
    while n < msgs_per_run:
        serve_tick([(t, "Continue") for t in rng.choice(tids, size=tick, replace=False)])
        n += tick
    return n / (time.perf_counter() - t0)


results = {}
t0 = time.perf_counter()
svc = RoomService(seed=3)
for t in tids:
    svc.create_room(t, GAME, players, dsl=dsl)
create_svc = time.perf_counter() - t0
t0 = time.perf_counter()
pool = RoomPoolService(seed=3, chunk_rooms=1024)
for t in tids:
    pool.create_room(t, GAME, players, dsl=dsl)
create_pool = time.perf_counter() - t0
print(f"{THREADS} threads, {GAME} x{N}: creating them took {create_svc:.2f} s (RoomService) / {create_pool:.2f} s (RoomPoolService)")
for tick in (1, 64, 1024):
    rng = np.random.default_rng(tick)
    a = measure(lambda m: [svc.handle_message(t, x) for t, x in m], tick, rng)
    b = measure(pool.handle_messages, tick, rng)
    results[tick] = {"room_service_msgs_per_s": round(a, 1), "room_pool_msgs_per_s": round(b, 1), "ratio": round(b / a, 2)}
    print(f"tick of {tick:5d} messages: RoomService {a:9.1f} msg/s   RoomPoolService {b:9.1f} msg/s   ratio {b / a:6.2f}")
svc.close()
pool.close()
print(json.dumps({"threads": THREADS, "game": f"{GAME} x{N}", "messages_per_measurement": msgs_per_run, "ticks": results}))

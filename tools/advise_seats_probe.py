#!/usr/bin/env python3
"""ge_batch_advise_seats (POLICY.md §3m) against the host-side path it replaces, wall time in one process, forms alternated.
    python tools/advise_seats_probe.py [output file, default profiles/advise_seats_probe.txt] [sizes, default 4096,65536]

A Werewolf x 8 batch with human_mask = 1 (seat 1 host-driven), stepped 40 turns from the initial state without restart and nobody
answering, so that most rooms wait for seat 1.  One tick advises seat 1 of every waiting room at 64 playouts per choice:
  device   find_rooms(person) -> advise_seats on the hits' rooms (the ge_advice records come back: 224 B per seat)
  host     find_rooms(person) -> read_rooms_at of the hits (228 B of view per room) -> the host lists every seat id as a choice
           plus the entry without an action (room_service.advise_candidates' rule; numpy, no Python loop) -> ge_batch_rollout_seats
           on those 9 entries per room (616 B of ge_rollout_stats per entry come back) -> the host takes the maximum of seat_wins
           over the accepted entries.  This is the library's path before advise_seats existed, on the same build.
Both forms end in a device synchronise inside the library, so a host clock around them times finished work; `best` of both forms is
asserted equal for every room.  Times are medians of REPS ticks after WARM warm-up ticks of every form; each repeat runs the device
form twice (A and A') around the host form, in alternating order, so the A / A' ratio of the same code is the spread a difference
has to exceed.  Bytes are computed from the shapes: what crosses the host-device link in each form."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from game_engine_amd import GameTable, RoomBatch  # noqa: E402
from game_engine_amd import _lib  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "advise_seats_probe.txt")
SIZES = [int(x) for x in sys.argv[2].split(",")] if len(sys.argv) > 2 else [4096, 65536]
WARM, REPS, TURNS, SEED, R, MT, SEAT, N = 2, 9, 40, 0xAD71, 64, 256, 1, 8
with open(os.path.join(ROOT, "tests", "golden", "dsl", "werewolf-(mafia).json"), encoding="utf-8") as f:
    tb = GameTable(json.load(f))
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def med(xs):
    return statistics.median(xs), (max(xs) - min(xs)) / 2


def size(n):
    with RoomBatch([(tb, N, n, 1 << (SEAT - 1))], seed=SEED) as b:
        b.step(TURNS)
        b.sync()
        lib, h = b._lib, b._h

        def device():
            hits, _ = b.find_rooms("person")
            rooms = hits["room"]
            adv = b.advise_seats(rooms, rooms + np.uint64(1 << 33), np.full(len(rooms), TURNS, dtype=np.uint32),
                                 np.full(len(rooms), SEAT, dtype=np.uint32), R, MT, seed=SEED)
            return rooms, adv["best"], adv

        def host():
            hits, _ = b.find_rooms("person")
            rooms = hits["room"]
            views = b.read_rooms_at(rooms)
            m = len(rooms)
            assert (views["n_players"] == N).all()
            e_rooms = np.repeat(rooms, N + 1)                    # every seat id, then the entry without an action
            e_keys = e_rooms + np.uint64(1 << 33)
            e_turns = np.full(m * (N + 1), TURNS, dtype=np.uint32)
            e_seats = np.full(m * (N + 1), SEAT, dtype=np.uint32)
            first = (np.arange(m * (N + 1) + 1, dtype=np.uint32) - np.arange(m * (N + 1) + 1, dtype=np.uint32) // np.uint32(N + 1))
            first[-1] = m * N
            players = np.full(m * N, SEAT, dtype=np.uint32)
            choices = np.tile(np.arange(1, N + 1, dtype=np.uint32), m)
            status = np.zeros(m * (N + 1), dtype=np.int32)
            words = np.zeros((m * (N + 1), _lib.ROLLOUT_WORDS), dtype=np.uint64)
            st = lib.ge_batch_rollout_seats(h, m * (N + 1), e_rooms.ctypes.data, e_keys.ctypes.data, e_turns.ctypes.data, e_seats.ctypes.data,
                                            first.ctypes.data, players.ctypes.data, choices.ctypes.data, status.ctypes.data, R, MT, SEED,
                                            words.ctypes.data)
            assert st in (0, -1), st                             # -1: some entry was refused (a dead target), as expected
            wins = words[:, 41 + 12 + SEAT - 1].astype(np.int64).reshape(m, N + 1)[:, :N]
            wins[status.reshape(m, N + 1)[:, :N] != 0] = -1
            return rooms, (np.argmax(wins, axis=1) + 1).astype(np.uint32), status

        t = {"A": [], "A'": [], "host": [], "advise": []}
        for rep in range(WARM + REPS):
            order = ("A", "host", "A'") if rep % 2 == 0 else ("A'", "host", "A")
            for which in order:
                t0 = time.perf_counter()
                got = host() if which == "host" else device()
                dt = time.perf_counter() - t0
                if rep >= WARM:
                    t[which].append(dt)
                if which == "host":
                    h_rooms, h_best, h_status = got
                else:
                    d_rooms, d_best, adv = got
            rooms = d_rooms
            keys, turns, seats = rooms + np.uint64(1 << 33), np.full(len(rooms), TURNS, dtype=np.uint32), np.full(len(rooms), SEAT, dtype=np.uint32)
            t0 = time.perf_counter()
            b.advise_seats(rooms, keys, turns, seats, R, MT, seed=SEED)
            if rep >= WARM:
                t["advise"].append(time.perf_counter() - t0)
        assert np.array_equal(d_rooms, h_rooms) and (adv["status"] == 0).all(), "the two forms advise different rooms"
        assert np.array_equal(d_best, h_best), "the two forms name different best choices"
        m = len(d_rooms)
        legal = int(sum(bin(int(x)).count("1") for x in adv["legal"]))
        a, a_s = med(t["A"])
        a2, _ = med(t["A'"])
        hm, h_s = med(t["host"])
        ad, ad_s = med(t["advise"])
        up_dev, down_dev = m * (8 + 8 + 4 + 4), m * 224 + 8 + 16 * m
        n_e = m * (N + 1)
        up_host = 8 * m + n_e * (8 + 8 + 4 + 4) + 4 * (n_e + 1) + 2 * 4 * m * N
        down_host = 16 * m + 228 * m + n_e * (616 + 4)
        say(f"{n} rooms: {m} wait for seat {SEAT}, {legal} legal choices ({legal / m:.2f} per seat), {R} playouts x <= {MT} turns each")
        say(f"  device tick (find_rooms + advise_seats)     {a * 1e3:9.3f} ms +- {a_s * 1e3:.3f}   A'/A = {a2 / a:.3f}")
        say(f"    advise_seats alone                        {ad * 1e3:9.3f} ms +- {ad_s * 1e3:.3f}")
        say(f"  host tick (find, read, list, rollout_seats, max) {hm * 1e3:9.3f} ms +- {h_s * 1e3:.3f}   host / device = {hm / a:.2f}")
        say(f"  bytes up / down, device {up_dev} / {down_dev}; host {up_host} / {down_host}   (down: x {down_host / down_dev:.1f})")
        say(f"  playouts played: device {(legal + m) * R}, host {(legal + m) * R} (+ {n_e - legal - m} refused entries uploaded)")


def main():
    say("ge_batch_advise_seats against find_rooms + read_rooms_at + host enumeration + rollout_seats + host maximum")
    say(f"(Werewolf x 8, human_mask = 1, {TURNS} turns stepped; medians of {REPS} ticks after {WARM} warm-up ticks, +- half range)")
    for n in SIZES:
        size(n)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""Inputs and references of the per-room seat masks (POLICY.md §3l), shared by tests/test_seats_host.py and
tests/test_gpu_room_seats.py.  The reference is the oracle under each room's own mask: Oracle.run takes a mask per call, so a
per-room reference is run_ref's functions called with room i's mask - no evaluator of its own.

Masks differ from lane to lane inside one wavefront and cycle through: no seat, seat 1, the highest seat, two seats, every seat, a
random mask."""
import numpy as np

from parity_util import oracle_events, oracle_rooms_as_views
from run_ref import PERSON, SEED, case_inputs, person_pending, run_ref

SEAT_CASES = ["ww8", "ww12", "tt4", "tt8", "tt12", "draft8_h1", "ww8_generic_h1", "tt4_generic_h1", "mixed"]
SIZES = (1, 63, 64, 65, 130)       # rooms per segment: the wavefront's edge, one past it, a third wavefront partly filled
FIRST_ROOM = 777                   # first_room of the batches (a room's key in a whole-batch step is FIRST_ROOM + its index)


def seat_masks(n_players, count, rng):
    """count masks for rooms of n_players seats, cycling through the six forms."""
    top, every = 1 << (n_players - 1), (1 << n_players) - 1
    out = np.zeros(count, dtype=np.uint32)
    for i in range(count):
        form = i % 6
        out[i] = (0, 1, top, 0b11 if i % 12 < 6 else (top | 2) & every, every, int(rng.integers(0, every + 1)))[form]
    return out


_CASES = {}


def seat_case(name, per, restart):
    """(segs, listed, keys, turns, masks): run_ref.case_inputs plus one mask array per segment.  Computed once; the rooms are shared
    and never changed (every user copies)."""
    key = (name, per, restart)
    if key not in _CASES:
        segs, listed, keys, turns = case_inputs(name, per, restart)
        rng = np.random.default_rng(len(name) * 7 + per)
        # (a rotation per segment, so that the forms meet every room index of a wavefront over the segments)
        masks = [np.roll(seat_masks(n, per, rng), g) for g, (_, _, n, _, _) in enumerate(segs)]
        _CASES[key] = (segs, listed, keys, turns, masks)
    return _CASES[key]


def flat_masks(masks):
    return np.concatenate(masks).astype(np.uint32)


def segment_masks(segs):
    """What seats() reads before any set: every room its segment's human_mask."""
    return np.concatenate([np.full(len(rooms), mask, dtype=np.uint32) for _, _, _, mask, rooms in segs])


def step_rooms_ref(segs, masks, listed, keys, turns, restart):
    """One turn of each listed room under its own mask.  Returns (events in input order, rooms after per segment)."""
    after = [rooms.copy() for _, _, _, _, rooms in segs]
    per = len(after[0])
    events = []
    for k, r in enumerate(listed):
        s, i = divmod(int(r), per)
        orc = segs[s][0]
        one = after[s][i:i + 1]
        orc.run(one, SEED, int(keys[k]), int(turns[k]), 1, threads=1, restart=restart, human_mask=int(masks[s][i]))
        events.append(oracle_events(orc, one, int(turns[k]))[0])
    return events, after


def run_rooms_ref(segs, masks, listed, keys, turns, max_turns, until, restart):
    """run_ref per listed room under its own mask: (played, stopped, events, views, rooms after per segment)."""
    after = [rooms.copy() for _, _, _, _, rooms in segs]
    per = len(after[0])
    played, stopped, events, views = [], [], [], []
    for k, r in enumerate(listed):
        s, i = divmod(int(r), per)
        p, why, ev, vw = run_ref(segs[s][0], after[s], i, SEED, int(keys[k]), int(turns[k]), max_turns, until, restart, int(masks[s][i]))
        played.append(p); stopped.append(why); events.append(ev); views.append(vw)
    return np.array(played, dtype=np.uint32), np.array(stopped, dtype=np.uint32), events, views, after


def pending_of(orc, one, mask):
    """The seats of `mask` for which Oracle.inject accepts some choice on a copy of the room (find_ref.room_facts's test)."""
    pending = 0
    for seat in range(orc.n):
        if (mask >> seat) & 1 and any(orc.inject(one.copy(), 0, seat + 1, c) for c in range(1, max(orc.n, 3) + 1)):
            pending |= 1 << seat
    return pending


def lowest_choice(orc, one, seat):
    """The lowest choice Oracle.inject accepts for seat (0-based) on a copy of the room, or 0."""
    for c in range(1, max(orc.n, 3) + 1):
        if orc.inject(one.copy(), 0, seat + 1, c):
            return c
    return 0


def step_turn_ref(segs, rooms, masks, turn, restart, first_room=FIRST_ROOM, events=True):
    """One whole-batch turn in place: room r of the batch under key first_room + r and its own mask.  Returns the events in batch
    order (events False: nothing)."""
    out, base = [], 0
    for s, (orc, _, _, _, _) in enumerate(segs):
        for i in range(len(rooms[s])):
            orc.run(rooms[s][i:i + 1], SEED, first_room + base + i, turn, 1, threads=1, restart=restart, human_mask=int(masks[s][i]))
        if events:
            out.extend(oracle_events(orc, rooms[s], turn))
        base += len(rooms[s])
    return out


def views_of(segs, rooms):
    return np.concatenate([oracle_rooms_as_views(orc, rooms[s]) for s, (orc, _, _, _, _) in enumerate(segs)])


def masks_matter(name, per=130):
    """On the oracle alone, keys 1000 + i and turn 5: (rooms whose record after one turn differs from the mask-0 result, rooms that
    stop on PERSON within 12 turns)."""
    segs, _, _, _, masks = seat_case(name, per, False)
    differ = stops = 0
    for s, (orc, _, _, _, rooms) in enumerate(segs):
        for i in range(per):
            a, b = rooms[i:i + 1].copy(), rooms[i:i + 1].copy()
            orc.run(a, SEED, 1000 + i, 5, 1, threads=1, restart=False, human_mask=int(masks[s][i]))
            orc.run(b, SEED, 1000 + i, 5, 1, threads=1, restart=False, human_mask=0)
            differ += oracle_rooms_as_views(orc, a).tobytes() != oracle_rooms_as_views(orc, b).tobytes()
            c = rooms.copy()
            stops += bool(run_ref(orc, c, i, SEED, 1000 + i, 5, 12, PERSON, False, int(masks[s][i]))[1] & PERSON)
    return differ, stops


__all__ = ["SEAT_CASES", "SIZES", "FIRST_ROOM", "seat_case", "seat_masks", "flat_masks", "segment_masks", "step_rooms_ref", "run_rooms_ref",
           "pending_of", "lowest_choice", "step_turn_ref", "views_of", "masks_matter", "person_pending"]

"""Reference of ge_batch_run_seats (POLICY.md §3p), the rule as code on tests/run_ref.py and tests/seats_ref.py: room r of the
range is run_ref's room under key = its global index, turn = the batch's turn and its own seat mask, turn after turn, with one more
stop test - SEAT is person_pending(orc, room, listed mask).  Also the inputs tests/test_run_seats_host.py and
tests/test_gpu_run_seats.py share: the host test proves on the oracle alone that the GPU tests cannot pass vacuously on them."""
import numpy as np

from run_ref import END, PERSON, PHASE, SEED, is_terminal, person_pending, run_ref
from seats_ref import FIRST_ROOM, seat_case, segment_masks, flat_masks, views_of

SEAT = 8
PER = 70                               # rooms per segment: a full wavefront plus a ragged one
T0 = 41                                # the batch's turn counter at the call
MAX_TURNS = (1, 3, 24)
# (max_turns, until) of the calls the tests make on every case
CALLS = [(1, 15), (3, SEAT | END), (24, SEAT | END), (24, PERSON | SEAT | END), (3, PERSON | SEAT), (24, PERSON | SEAT | PHASE)]
# case of run_ref.CASES -> the listed seats: in every case one seat that is not host-driven anywhere is listed and one host-driven
# seat is not, so that SEAT and PERSON can hold one without the other.  Werewolf 8 / 12, Two-Truths 4 / 8 / 12 builds, one GENERIC
# table of each game, the mixed four-segment batch
RUN_SEATS_CASES = {"ww8_h2": [3, 1], "ww12_h2": [12, 2], "tt4_h2": [3, 2], "tt8_h1": [2, 3], "tt12_h2": [4, 5], "ww8_generic_h1": [1, 3],
                   "tt4_generic_h1": [2], "mixed": [2, 3]}


def listed_mask(seats, n_players):
    return sum(1 << (s - 1) for s in seats if s <= n_players)


def run_seats_room(orc, rooms, i, key, turn, max_turns, until, restart, mask, listed):
    """Plays rooms[i] on in place: run_ref's turn and stop tests under until & 7, then SEAT on the record the turn left.  Returns
    (played, stopped).  Where PHASE is asked the turn is run_ref itself, a turn at a time (it needs the turn's event); else run_ref's
    loop restated on its own functions without the per-turn events and views, which tests/test_run_seats_host.py holds against it."""
    one = rooms[i:i + 1]
    for t in range(max_turns):
        if until & PHASE:
            _, why, _, _ = run_ref(orc, rooms, i, SEED, key, turn + t, 1, until & 7, restart, mask)
        else:
            orc.run(one, SEED, key, turn + t, 1, threads=1, restart=restart, human_mask=mask)
            why = (PERSON if until & PERSON and person_pending(orc, one, mask) else 0) | (END if until & END and is_terminal(orc, one) else 0)
        if until & SEAT and person_pending(orc, one, listed):
            why |= SEAT
        if why:
            break
    return t + 1, why


def run_seats_ref(segs, rooms, masks, seats, turn, max_turns, until, restart, first=0, count=None, first_room=FIRST_ROOM):
    """The call over batch rooms first .. first + count - 1, in place on `rooms` (one oracle array per segment); masks: one mask
    per batch room.  Returns (played, stopped) of the range."""
    total = sum(len(r) for r in rooms)
    count = total - first if count is None else count
    played, stopped = np.zeros(count, dtype=np.uint32), np.zeros(count, dtype=np.uint32)
    base = 0
    for (orc, _, n, _, _), seg_rooms in zip(segs, rooms):
        listed = listed_mask(seats, n)
        for i in range(len(seg_rooms)):
            r = base + i
            if first <= r < first + count:
                played[r - first], stopped[r - first] = run_seats_room(orc, seg_rooms, i, first_room + r, turn, max_turns, until, restart,
                                                                       int(masks[r]), listed)
        base += len(seg_rooms)
    return played, stopped


def case_rooms(name, restart):
    """Fresh copies of the case's start rooms, one oracle array per segment: seat_case's rooms (up to 70 turns into a game); in a
    Two-Truths segment of seven players or more, whose game is longer than that, room i is played (i % 4) * 60 turns further by the
    policy alone, so that some of its rooms reach their end too."""
    segs = seat_case(name, PER, restart)[0]
    rooms = [s[4].copy() for s in segs]
    for (orc, _, n, _, _), seg_rooms in zip(segs, rooms):
        if orc.table.pack == 1 or n < 7:
            continue
        for i in range(len(seg_rooms)):
            orc.run(seg_rooms[i:i + 1], SEED, 5000 + i, 100, (i % 4) * 60, threads=1, restart=restart, human_mask=0)
    return rooms


_REFS = {}


def case_ref(name, restart, plane, max_turns, until):
    """The whole batch of a case after the call, computed once and never changed: (segs, masks of the batch rooms, played, stopped,
    views before, views after, oracle rooms after).  plane: the per-room masks of seats_ref.seat_case instead of the segments' own."""
    key = (name, restart, plane, max_turns, until)
    if key not in _REFS:
        segs, _, _, _, masks = seat_case(name, PER, restart)
        flat = flat_masks(masks) if plane else segment_masks(segs)
        rooms = case_rooms(name, restart)
        before = views_of(segs, rooms)
        played, stopped = run_seats_ref(segs, rooms, flat, RUN_SEATS_CASES[name], T0, max_turns, until, restart)
        _REFS[key] = (segs, flat, played, stopped, before, views_of(segs, rooms), rooms)
    return _REFS[key]


__all__ = ["SEAT", "PERSON", "END", "PHASE", "PER", "T0", "MAX_TURNS", "CALLS", "RUN_SEATS_CASES", "listed_mask", "run_seats_room",
           "run_seats_ref", "case_rooms", "case_ref"]

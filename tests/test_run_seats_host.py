"""The inputs of tests/test_gpu_run_seats.py on the oracle alone (CPU): they do not let the GPU tests pass vacuously.  Per layout
(tests/run_seats_ref.py RUN_SEATS_CASES) and over its calls: every stop bit occurs, SEAT without PERSON and PERSON without SEAT,
some room hits the limit; under restart some room stops at END before the limit, and the same room played the limit's turns fused
has started another game - the end a fused step hides."""
import numpy as np
import pytest

from run_ref import SEED, run_ref
from run_seats_ref import CALLS, END, MAX_TURNS, PER, PERSON, PHASE, RUN_SEATS_CASES, SEAT, T0, case_ref, case_rooms, listed_mask, run_seats_room
from seats_ref import FIRST_ROOM


def test_the_calls_cover_the_turn_limits_and_every_bit():
    assert {m for m, _ in CALLS} == set(MAX_TURNS)
    assert any(u == 15 for _, u in CALLS) and all(u & SEAT for _, u in CALLS)


@pytest.mark.parametrize("plane", [False, True])
@pytest.mark.parametrize("restart", [False, True])
@pytest.mark.parametrize("name", sorted(RUN_SEATS_CASES))
def test_every_stop_reason_occurs(name, restart, plane):
    bits = 0
    seat_alone = person_alone = limit = early = 0
    for max_turns, until in CALLS:
        _, _, played, stopped, before, after, _ = case_ref(name, restart, plane, max_turns, until)
        assert len(played) == PER * len(case_ref(name, restart, plane, max_turns, until)[0])
        assert (played >= 1).all() and (played <= max_turns).all() and not (stopped & ~np.uint32(until)).any()
        assert ((stopped != 0) | (played == max_turns)).all()
        bits |= int(np.bitwise_or.reduce(stopped))
        if until & PERSON:
            seat_alone += int(((stopped & (SEAT | PERSON)) == SEAT).sum())
            person_alone += int(((stopped & (SEAT | PERSON)) == PERSON).sum())
        limit += int((stopped == 0).sum())
        early += int((played < max_turns).sum())
        assert before.tobytes() != after.tobytes()
    assert bits == 15, bits
    assert seat_alone > 0 and person_alone > 0, (seat_alone, person_alone)
    assert limit > 0 and early > 0, (limit, early)


@pytest.mark.parametrize("plane", [False, True])
@pytest.mark.parametrize("name", sorted(RUN_SEATS_CASES))
def test_under_restart_a_fused_step_hides_an_end_that_the_run_on_shows(name, plane):
    hidden = 0
    for max_turns, until in CALLS:
        if max_turns == 1 or not until & END:
            continue
        segs, masks, played, stopped, _, _, after = case_ref(name, True, plane, max_turns, until)
        base = 0
        for (orc, _, _, _, _), start, seg_after in zip(segs, case_rooms(name, True), after):
            for i in range(len(start)):
                r = base + i
                if stopped[r] & END and played[r] < max_turns:
                    fused = start[i:i + 1].copy()
                    orc.run(fused, SEED, FIRST_ROOM + r, T0, max_turns, threads=1, restart=True, human_mask=int(masks[r]))
                    assert int(fused["games"][0]) > int(seg_after["games"][i]), (name, r)
                    hidden += 1
            base += len(start)
    assert hidden > 0


@pytest.mark.parametrize("name", ["mixed", "ww12_h2", "tt8_h1"])
def test_without_the_seat_bit_the_reference_is_run_ref(name):
    """played, stopped and the record of run_ref itself, for PERSON | END (the loop restated) and with PHASE (run_ref a turn at a
    time)."""
    segs = case_ref(name, True, False, 3, SEAT | END)[0]
    for until in (PERSON | END, PERSON | END | PHASE, 0):
        mine, theirs = case_rooms(name, True), case_rooms(name, True)
        for s, (orc, _, _, mask, _) in enumerate(segs):
            for i in range(0, PER, 3):
                got = run_seats_room(orc, mine[s], i, FIRST_ROOM + i, T0, 24, until, True, mask, 0)
                want = run_ref(orc, theirs[s], i, SEED, FIRST_ROOM + i, T0, 24, until, True, mask)[:2]
                assert got == want, (name, until, s, i)
            assert mine[s].tobytes() == theirs[s].tobytes()


def test_the_listed_mask_is_clipped_to_the_segment():
    assert listed_mask([2, 3], 4) == 0b110 and listed_mask([12, 2], 11) == 0b10 and listed_mask([], 8) == 0

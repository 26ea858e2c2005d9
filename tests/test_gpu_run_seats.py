"""ge_batch_run_seats (-m gpu) against tests/run_seats_ref.py (POLICY.md §3p restated on the oracle): 70 rooms per segment (a full
wavefront plus a ragged one), max_turns 1 / 3 / 24, the whole batch, ranges inside a wavefront, across a wavefront edge, across a
segment edge and an empty one; turn counts and stop bits, every room of the batch as views with the unlisted rooms unchanged, the
turn counter; with and without restart, with and without a seat plane that differs per room, and on a tracing batch whose trace
buffer must not change.  Then the identities of the definition - ge_batch_step_rooms over the range, ge_batch_step on a plane batch,
ge_batch_run_rooms on a twin -, a plain step behind the call against the oracle (the prepared deals are still right), and every
refusal in its order.  tests/test_run_seats_host.py proves that every stop reason occurs in these inputs."""
import ctypes as C

import numpy as np
import pytest

from game_engine_amd import GameTable, GeError, RoomBatch
from observe_ref import DeviceBuffer, make_batch
from parity_util import oracle_rooms_as_views
from run_ref import SEED
from run_seats_ref import (CALLS, END, PER, PERSON, PHASE, RUN_SEATS_CASES, SEAT, T0, case_ref, case_rooms, run_seats_ref)
from seats_ref import FIRST_ROOM, flat_masks, seat_case, segment_masks, step_turn_ref, views_of

pytestmark = pytest.mark.gpu

GE_ERR_ARG, GE_ERR_RANGE = -1, -6
FILL = 0x4D


def start_batch(segs, rooms, restart, masks=None, turn=T0, **kw):
    """The rooms written as views, the turn counter set, and a seat plane where `masks` (one per batch room) is given."""
    b = make_batch(segs, restart, views=[oracle_rooms_as_views(s[0], r) for s, r in zip(segs, rooms)], **kw)
    b.set_turn(turn)
    if masks is not None:
        b.set_seats(np.arange(b.n_rooms), masks)
    return b


def run(b, seats, max_turns, until, first=0, count=None, with_stopped=True):
    """The call into fresh device memory: (played, stopped) of the range as uint32 arrays (stopped None without the buffer)."""
    count = b.n_rooms - first if count is None else count
    played, stopped = DeviceBuffer(4 * count, FILL), DeviceBuffer(4 * count, FILL) if with_stopped else None
    b.run_seats(seats, played, stopped, max_turns, until, first, count)
    b.sync()
    return played.host(np.uint32), stopped.host(np.uint32) if with_stopped else None


def ranges(n_seg):
    out = [(0, PER * n_seg), (3, 5), (60, 10), (17, 0)]         # whole, inside a wavefront, across a wavefront edge, empty
    if n_seg > 1:
        out.append((PER - 4, 10))                               # across a segment edge
        out.append((2 * PER - 1, PER + 2))                      # one room of segment 1, all of segment 2, one of segment 3
    return out


@pytest.mark.parametrize("plane", [False, True])
@pytest.mark.parametrize("restart", [False, True])
@pytest.mark.parametrize("name", sorted(RUN_SEATS_CASES))
def test_every_range_equals_the_reference(name, restart, plane):
    seats = RUN_SEATS_CASES[name]
    for max_turns, until in CALLS:
        segs, masks, played, stopped, before, after, _ = case_ref(name, restart, plane, max_turns, until)
        for first, count in ranges(len(segs)):
            what = (name, restart, plane, max_turns, until, first, count)
            with start_batch(segs, case_rooms(name, restart), restart, masks if plane else None) as b:
                got_played, got_stopped = run(b, seats, max_turns, until, first, count)
                assert np.array_equal(got_played, played[first:first + count]), (what, np.flatnonzero(got_played != played[first:first + count])[:5])
                assert np.array_equal(got_stopped, stopped[first:first + count]), (what, np.flatnonzero(got_stopped != stopped[first:first + count])[:5])
                want = before.copy()
                want[first:first + count] = after[first:first + count]
                got = b.read_rooms()
                assert got.tobytes() == want.tobytes(), (what, [i for i in range(len(got)) if got[i].tobytes() != want[i].tobytes()][:5])
                assert b.turn == (T0 + max_turns if count else T0), what


def test_stopped_may_be_null_and_until_takes_names():
    segs, _, played, _, _, after, _ = case_ref("mixed", True, False, 24, SEAT | END)
    with start_batch(segs, case_rooms("mixed", True), True) as b:
        got, none = run(b, RUN_SEATS_CASES["mixed"], 24, ("seat", "end"), with_stopped=False)
        assert none is None and np.array_equal(got, played) and b.read_rooms().tobytes() == after.tobytes()


@pytest.mark.parametrize("name", ["ww8_h2", "mixed"])
def test_a_tracing_batch_keeps_its_trace_buffer(name):
    """One traced step, then the call: what ge_batch_read_events reports is byte for byte what it reported before, and the call
    equals the reference from the stepped rooms."""
    segs = seat_case(name, PER, True)[0]
    rooms = case_rooms(name, True)
    flat = segment_masks(segs)
    with start_batch(segs, rooms, True, trace=True) as b:
        b.step(1)
        events = b.read_events().tobytes()
        step_turn_ref(segs, rooms, [np.full(PER, s[3]) for s in segs], T0, True, events=False)
        want_played, want_stopped = run_seats_ref(segs, rooms, flat, RUN_SEATS_CASES[name], T0 + 1, 24, SEAT | END | PERSON, True)
        played, stopped = run(b, RUN_SEATS_CASES[name], 24, SEAT | END | PERSON)
        assert np.array_equal(played, want_played) and np.array_equal(stopped, want_stopped)
        assert b.read_rooms().tobytes() == views_of(segs, rooms).tobytes()
        assert b.read_events().tobytes() == events and len(events) > 0
        assert b.turn == T0 + 1 + 24


@pytest.mark.parametrize("name", sorted(RUN_SEATS_CASES))
def test_one_turn_without_a_stop_test_is_step_rooms_over_the_range(name):
    segs, _, _, _, masks = seat_case(name, PER, True)
    flat = flat_masks(masks)
    for plane in (None, flat):
        for first, count in ranges(len(segs)):
            with start_batch(segs, case_rooms(name, True), True, plane) as b, start_batch(segs, case_rooms(name, True), True, plane) as twin:
                played, stopped = run(b, RUN_SEATS_CASES[name], 1, 0, first, count)
                r = np.arange(first, first + count)
                twin.step_rooms(r, FIRST_ROOM + r, np.full(count, T0))
                assert (played == 1).all() and (stopped == 0).all()
                assert b.read_rooms().tobytes() == twin.read_rooms().tobytes(), (name, plane is not None, first, count)


@pytest.mark.parametrize("max_turns", [1, 3, 24])
@pytest.mark.parametrize("name", sorted(RUN_SEATS_CASES))
def test_without_a_stop_test_the_records_are_those_of_a_step_on_a_plane_batch(name, max_turns):
    segs, _, _, _, masks = seat_case(name, PER, True)
    flat = flat_masks(masks)
    with start_batch(segs, case_rooms(name, True), True, flat) as b, start_batch(segs, case_rooms(name, True), True, flat, max_fuse=0) as twin:
        played, stopped = run(b, [], max_turns, 0)
        twin.step(max_turns)
        assert (played == max_turns).all() and (stopped == 0).all()
        assert b.read_rooms().tobytes() == twin.read_rooms().tobytes() and b.turn == twin.turn == T0 + max_turns


@pytest.mark.parametrize("plane", [False, True])
@pytest.mark.parametrize("name", sorted(RUN_SEATS_CASES))
def test_run_rooms_on_a_twin_gives_the_same_counts_bits_and_records(name, plane):
    segs, _, _, _, masks = seat_case(name, PER, True)
    flat = flat_masks(masks) if plane else None
    for max_turns, until in ((24, PERSON | END), (3, 7), (24, SEAT | PERSON | END)):
        with start_batch(segs, case_rooms(name, True), True, flat) as b, start_batch(segs, case_rooms(name, True), True, flat) as twin:
            played, stopped = run(b, RUN_SEATS_CASES[name], max_turns, until)
            r = np.arange(b.n_rooms)
            want_played, want_stopped, _, _ = twin.run_rooms(r, FIRST_ROOM + r, np.full(len(r), T0), max_turns, until & 7, views=False)
            if not until & SEAT:
                assert np.array_equal(played, want_played) and np.array_equal(stopped, want_stopped)
                assert b.read_rooms().tobytes() == twin.read_rooms().tobytes()
            else:                                               # one more stop test: never later, and the same where SEAT did not hold
                assert (played <= want_played).all()
                same = (stopped & SEAT) == 0
                assert same.any() and np.array_equal(played[same], want_played[same]) and np.array_equal(stopped[same], want_stopped[same])
                assert b.read_rooms()[same].tobytes() == twin.read_rooms()[same].tobytes()
            assert twin.turn == T0 and b.turn == T0 + max_turns


@pytest.mark.parametrize("name,max_fuse", [("ww8_h2", 0), ("ww8_h2", 1), ("ww12_h2", 0), ("ww12_h2", 1), ("mixed", 0)])
def test_a_plain_step_behind_the_call_equals_the_oracle(name, max_fuse):
    """Prepared deals (Werewolf x 8: in the record; Werewolf x 12: the side plane) are still right: steps before the call prepare
    them, the call stores records without one, and the steps behind it deal as the oracle does."""
    segs = seat_case(name, PER, True)[0]
    rooms = case_rooms(name, True)
    flat = segment_masks(segs)
    seg_masks = [np.full(PER, s[3]) for s in segs]
    with start_batch(segs, rooms, True, max_fuse=max_fuse) as b:
        b.step(3)
        for t in range(3):
            step_turn_ref(segs, rooms, seg_masks, T0 + t, True, events=False)
        played, stopped = run(b, RUN_SEATS_CASES[name], 24, SEAT | END)
        want_played, want_stopped = run_seats_ref(segs, rooms, flat, RUN_SEATS_CASES[name], T0 + 3, 24, SEAT | END, True)
        assert np.array_equal(played, want_played) and np.array_equal(stopped, want_stopped)
        b.step(30)
        for t in range(30):
            step_turn_ref(segs, rooms, seg_masks, T0 + 27 + t, True, events=False)
        assert b.turn == T0 + 57
        assert b.read_rooms().tobytes() == views_of(segs, rooms).tobytes()


def test_refusals_in_their_order_leave_the_outputs_and_the_batch_untouched(dsl_ww, dsl_tt):
    with RoomBatch([(GameTable(dsl_ww), 6, 300, 1), (GameTable(dsl_tt), 4, 200, 2)], seed=1, max_fuse=1) as b:
        b.step(9)
        before = b.read_rooms().tobytes()
        call = b._lib.ge_batch_run_seats
        played, stopped = DeviceBuffer(500 * 4, FILL), DeviceBuffer(500 * 4, FILL)
        P, S = C.c_void_p(played.data_ptr()), C.c_void_p(stopped.data_ptr())
        heap = np.zeros(500, dtype=np.uint32)                            # pageable host memory: not vetted
        H = C.c_void_p(heap.ctypes.data)
        u32 = lambda *v: (C.c_uint32 * len(v))(*v)
        assert call(None, 0, 10, 1, u32(1), 4, SEAT, P, S, None) == GE_ERR_ARG                  # 1
        calls = [
            # (first, count, n_seats, seats, max_turns, until, played, stopped) -> status; later errors are present too where they can be
            ((0, 501, 1, u32(0), 0, SEAT, P, S), GE_ERR_ARG),            # 2 max_turns 0, before the range
            ((0, 501, 1, u32(0), 4097, SEAT, P, S), GE_ERR_ARG),         # 2 above 4096
            ((0, 501, 1, u32(0), 4, 16, P, S), GE_ERR_ARG),              # 3 a bit above 15
            ((0, 501, 1, u32(0), 4, 31, P, S), GE_ERR_ARG),
            ((0, 501, 0, None, 4, SEAT | END, P, S), GE_ERR_ARG),        # 3 SEAT without a seat
            ((0, 501, 1, u32(0), 4, SEAT, None, S), GE_ERR_ARG),         # 4 played NULL
            ((0, 501, 1, None, 4, SEAT, P, S), GE_ERR_ARG),              # 5 seats NULL
            ((0, 501, 13, u32(*range(1, 14)), 4, SEAT, P, S), GE_ERR_ARG),   # 5 more than twelve seats
            ((0, 501, 2, u32(2, 2), 4, SEAT, P, S), GE_ERR_ARG),         # 5 a repeated seat, before the range
            ((0, 501, 1, u32(0), 4, SEAT, P, S), GE_ERR_RANGE),          # 6 the range, before the seat of 0
            ((500, 1, 1, u32(1), 4, SEAT, P, S), GE_ERR_RANGE),
            ((1 << 63, 1 << 63, 1, u32(1), 4, SEAT, P, S), GE_ERR_RANGE),    # first + count wraps
            ((0, 10, 1, u32(0), 4, SEAT, H, S), GE_ERR_ARG),             # 7 a seat of 0, before the pointers
            ((0, 10, 1, u32(7), 4, SEAT, P, S), GE_ERR_ARG),             # 7 above segment 0's six players
            ((290, 20, 1, u32(5), 4, SEAT, P, S), GE_ERR_ARG),           # 7 above segment 1's four, which the range touches
            ((17, 0, 1, u32(0), 4, SEAT, P, S), GE_ERR_ARG),             # 7 a seat of 0 in an empty range
            ((0, 10, 1, u32(1), 4, SEAT, H, S), GE_ERR_ARG),             # 8 played not device memory
            ((0, 10, 1, u32(1), 4, SEAT, P, H), GE_ERR_ARG),             # 8 stopped not device memory
        ]
        for args, status in calls:
            assert call(b._h, *args, None) == status, args
        b.set_turn(0xFFFFFFFF - 3)
        for args, status in [((0, 10, 1, u32(1), 4, SEAT, H, S), GE_ERR_ARG),          # 8 before 9
                             ((0, 10, 1, u32(1), 4, SEAT, P, S), GE_ERR_RANGE),        # 9 T + max_turns > 0xFFFFFFFF
                             ((17, 0, 1, u32(1), 4, SEAT, None, None), GE_ERR_RANGE)]:  # 9 before 10
            assert call(b._h, *args, None) == status, args
        assert b.turn == 0xFFFFFFFF - 3
        b.set_turn(9)
        for args in ((17, 0, 1, u32(1), 4, SEAT, None, None), (500, 0, 0, None, 4096, 7, None, None), (0, 0, 2, u32(6, 1), 1, 15, P, S)):   # 10
            assert call(b._h, *args, None) == 0, args
        b.sync()
        assert b.turn == 9 and b.read_rooms().tobytes() == before
        assert set(played.host().tobytes()) == {FILL} and set(stopped.host().tobytes()) == {FILL} and not heap.any()
        assert call(b._h, 0, 300, 1, u32(6), 4, SEAT, P, S, None) == 0   # seat 6 while the range stays in segment 0
        b.sync()
        assert b.turn == 13 and set(played.host()[300 * 4:].tobytes()) == {FILL} and (played.host(np.uint32)[:300] <= 4).all()
        with pytest.raises(GeError) as e:
            b.run_seats([1, 1], played)
        assert e.value.status == GE_ERR_ARG
        with pytest.raises(GeError) as e:
            b.run_seats([1], played, first=400, count=200)
        assert e.value.status == GE_ERR_RANGE
        with pytest.raises(GeError):
            b.run_seats([1], DeviceBuffer(10 * 4), None, 4, first=0, count=500)   # (the binding: fewer entries than count)
        with pytest.raises(ValueError):
            b.run_seats([1], played, until=("seat", "nobody"))
        assert b.turn == 13


def test_run_rooms_goes_on_refusing_the_seat_bit(dsl_ww):
    with RoomBatch([(GameTable(dsl_ww), 8, 100, 1)], seed=1) as b:
        before = b.read_rooms().tobytes()
        for until in (SEAT, SEAT | END, 15):
            with pytest.raises(GeError) as e:
                b.run_rooms([0, 1], [0, 1], [0, 0], 4, until)
            assert e.value.status == GE_ERR_ARG
        with pytest.raises(ValueError):
            b.run_rooms([0], [0], [0], 4, ("seat",))
        assert b.read_rooms().tobytes() == before and b.turn == 0


def test_a_stream_of_the_callers_and_one_timed_interval(dsl_ww, dsl_tt):
    """step on one stream, the call on another, no host wait in between: it runs behind the step, and a later step behind it; with
    timing on the call is one interval of kernel_time, one launch per segment of the range."""
    mk = lambda: RoomBatch([(GameTable(dsl_ww), 8, 3000, 1), (GameTable(dsl_tt), 4, 2000, 2)], seed=4, restart=True)
    with mk() as a, mk() as twin:
        played, twin_played = DeviceBuffer(5000 * 4), DeviceBuffer(5000 * 4)
        hip = played.hip
        s1, s2 = C.c_void_p(), C.c_void_p()
        assert hip.hipStreamCreate(C.byref(s1)) == 0 and hip.hipStreamCreate(C.byref(s2)) == 0
        try:
            a.step(30, stream=s1.value)
            a.run_seats([1], played, None, 16, stream=s2.value)
            a.step(5, stream=s1.value)                           # ordered behind the call
            a.sync()
            assert hip.hipStreamSynchronize(s2) == 0
        finally:
            a.sync()
            hip.hipStreamDestroy(s1)
            hip.hipStreamDestroy(s2)
        twin.step(30)
        twin.set_timing(True)
        twin.kernel_time(reset=True)
        twin.run_seats([1], twin_played, None, 16)
        ms, launches = twin.kernel_time(reset=True)
        assert ms > 0.0 and launches == 2
        twin.set_timing(False)
        twin.step(5)
        assert a.turn == twin.turn == 51
        assert np.array_equal(played.host(np.uint32), twin_played.host(np.uint32))
        assert a.read_rooms().tobytes() == twin.read_rooms().tobytes()

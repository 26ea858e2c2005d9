"""ge_batch_gather_seats (-m gpu) against tests/gather_ref.py (POLICY.md §3q: the filter over the records of tests/observe_ref.py):
the cases of tests/test_gpu_observe_seats.py as they are - every layout, shipped, draft and GENERIC tables, a mixed batch, restart
on and off, 135 rooms per segment (two full wavefronts and a tail of 7) -, its seat lists and windows, each `want`: the list, the
entry indices and both count words byte-equal, the tail of the outputs untouched; caps of 0, 1, M - 1, M, between two seats of a
room and at a wavefront boundary; that the call only reads; the same list under a seat plane; the refusals in their order; a
second stream of the caller's; the timing interval; and one larger range - more wavefronts than a pass of the scan covers and a
ragged tail - against the filter over ge_batch_observe_seats's own dense output.  tests/test_gather_host.py proves that the
filter keeps some entries and drops some in every case here."""
import ctypes as C
import json

import numpy as np
import pytest

from game_engine_amd import GameTable, GeError, RoomBatch
from game_engine_amd.stepper import SEAT_OBS_DTYPE
from gather_ref import END, SEAT, WANTS, due, gather
from observe_ref import OBSERVE_CASES, PER, DeviceBuffer, case_all_seats, case_records, differing_fields, make_batch, seat_lists, windows

pytestmark = pytest.mark.gpu

GE_ERR_ARG, GE_ERR_RANGE = -1, -6
FILL = 0xA5
TAIL = 5                                          # entries allocated behind cap: nothing there may be written


def call(b, seats, want, first=0, count=None, cap=None, stream=0):
    """The call into fresh device memory filled with FILL, cap + TAIL entries long: (records, entries, n) as the device holds them"""
    count = b.n_rooms - first if count is None else count
    cap = count * len(seats) if cap is None else cap
    out, entries, n = DeviceBuffer((cap + TAIL) * 192, FILL), DeviceBuffer((cap + TAIL) * 4, FILL), DeviceBuffer(8, FILL)
    b.gather_seats(seats, out, entries, n, want, first, count, cap=cap, stream=stream)
    b.sync()
    return out.host(SEAT_OBS_DTYPE), entries.host(np.uint32), n.host(np.uint32)


def assert_list(got, want_records, want, cap, what):
    """got = call(..); the reference list of the dense records `want_records` [count, n_seats]"""
    out, entries, n = got
    ref, ref_e, ref_n = gather(want_records, want, cap)
    assert list(n) == list(ref_n), (what, list(n), list(ref_n))
    k = int(ref_n[0])
    assert np.array_equal(entries[:k], ref_e), (what, np.flatnonzero(entries[:k] != ref_e)[:5])
    if out[:k].tobytes() != ref.tobytes():
        bad = [i for i in range(k) if out[i].tobytes() != ref[i].tobytes()]
        raise AssertionError(f"{what}: {len(bad)} of {k} records differ, fields {differing_fields(out[:k], ref)}; first at list position {bad[0]} "
                             f"(entry {ref_e[bad[0]]}): got {out[bad[0]]} want {ref[bad[0]]}")
    assert set(out[k:].tobytes()) == {FILL} and set(entries[k:].tobytes()) == {FILL}, (what, "written behind the list")
    return k


def caps_of(records, want):
    """0, 1, M - 1, M, a cap that falls between two seats of one room, one that falls at a wavefront boundary"""
    d = due(records, want)
    m = int(d.sum())
    caps = {0, 1, max(m - 1, 0), m}
    per_room = d.sum(axis=1)
    split = np.flatnonzero(per_room >= 2)
    if len(split):
        caps.add(int(per_room[:split[0]].sum()) + 1)              # the room's first due seat is kept, its second dropped
    if len(per_room) > 64:
        caps.add(int(per_room[:64].sum()))                          # all of wavefront 0, nothing of wavefront 1
        caps.add(int(per_room[:128].sum()))
    return sorted(caps)


@pytest.mark.parametrize("restart", [False, True])
@pytest.mark.parametrize("name", OBSERVE_CASES)
def test_every_list_equals_the_reference(name, restart):
    segs, _ = case_all_seats(name, restart)
    listed = 0
    with make_batch(segs, restart) as b:
        for seats in seat_lists(segs):
            dense = case_records(name, restart, seats)
            for want in WANTS:
                for first, count in windows(len(segs)):
                    what = (name, restart, seats, want, first, count)
                    listed += assert_list(call(b, seats, want, first, count), dense[first:first + count], want, None, what)
                for cap in caps_of(dense, want):
                    assert_list(call(b, seats, want, cap=cap), dense, want, cap, (name, restart, seats, want, "cap", cap))
        out, entries, n = DeviceBuffer(192, FILL), DeviceBuffer(4, FILL), DeviceBuffer(8, FILL)
        b.gather_seats(seats, None, None, n, "seat", cap=0)        # cap = 0 counts only: no list to point at
        b.sync()
        assert list(n.host(np.uint32)) == [0, int(due(dense, SEAT).sum())]
    assert listed > 0


@pytest.mark.parametrize("name", ["ww8_h1", "ww12_h2", "tt4_h1", "mixed"])
def test_a_seat_plane_plays_no_part(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    segs, _ = case_all_seats(name, True)
    seats = seat_lists(segs)[1]
    dense = case_records(name, True, seats)
    with make_batch(segs, True) as b:
        rooms = rng.permutation(b.n_rooms)[: b.n_rooms // 3]
        n_of = np.repeat([s[2] for s in segs], PER)
        b.set_seats(rooms, [int(rng.integers(0, 1 << n_of[r])) for r in rooms])
        for want in WANTS:
            assert_list(call(b, seats, want), dense, want, None, (name, "seat plane", want))
            assert_list(call(b, seats, want, 63, 67), dense[63:130], want, None, (name, "seat plane, window", want))


def _hip_copy_back(ptr, nbytes):
    raw = np.empty(nbytes, dtype=np.uint8)
    assert C.CDLL("libamdhip64.so").hipMemcpy(C.c_void_p(raw.ctypes.data), C.c_void_p(ptr), C.c_size_t(nbytes), 2) == 0
    return raw.tobytes()


def _state(b):
    """records as they lie in HBM (prepared deals of Werewolf x 8 included), summary, turn counter, trace buffer"""
    b.sync()
    raw = [_hip_copy_back(*b.state(g)[:2]) for g in range(len(b.segments))]
    return raw, json.dumps(b.summary(), sort_keys=True, default=int), b.turn, b.read_events().tobytes() if b._trace else b""


@pytest.mark.parametrize("name", ["ww8_h1", "ww12_h2", "tt4_h1", "mixed"])
def test_the_call_only_reads(name):
    segs, _ = case_all_seats(name, True)
    with make_batch(segs, True, trace=True) as b:
        b.step(1)
        before = _state(b)
        for seats in seat_lists(segs):
            for want in WANTS:
                call(b, seats, want)
                call(b, seats, want, 63, 67, cap=9)
        assert _state(b) == before


def test_refusals_in_their_order_leave_the_outputs_untouched(dsl_ww, dsl_tt):
    with RoomBatch([(GameTable(dsl_ww), 6, 300, 1), (GameTable(dsl_tt), 4, 200, 2)], seed=1, max_fuse=1) as b:
        b.step(9)
        before = b.read_rooms().tobytes()
        fn = b._lib.ge_batch_gather_seats
        out, entries, n = DeviceBuffer(1500 * 192, 0x5A), DeviceBuffer(1500 * 4, 0x5A), DeviceBuffer(8, 0x5A)
        heap = np.zeros(1500 * 48, dtype=np.uint32)                     # pageable host memory: not vetted
        O, E, N, H = C.c_void_p(out.ptr), C.c_void_p(entries.ptr), C.c_void_p(n.ptr), C.c_void_p(heap.ctypes.data)
        u32 = lambda *v: (C.c_uint32 * len(v))(*v)
        calls = [
            # (first, count, n_seats, seats, want, obs, entries, cap, n) -> status; later errors are present too where they can be
            ((0, 501, 1, None, 0, None, None, 5, None), GE_ERR_ARG),               # 2 want 0 (everything else wrong as well)
            ((0, 501, 1, None, 4, None, None, 5, None), GE_ERR_ARG),               # 2 a bit above 3
            ((0, 501, 1, None, 7, None, None, 5, None), GE_ERR_ARG),
            ((0, 501, 1, None, 3, None, None, 5, None), GE_ERR_ARG),               # 3 n NULL
            ((0, 501, 1, None, 3, None, E, 5, N), GE_ERR_ARG),                     # 4 obs NULL with cap > 0
            ((0, 501, 1, None, 3, O, None, 5, N), GE_ERR_ARG),                     # 4 entries NULL with cap > 0
            ((0, 501, 1, None, 3, O, E, 5, N), GE_ERR_ARG),                        # 5 seats NULL (range wrong as well)
            ((0, 501, 13, u32(*range(1, 14)), 3, O, E, 5, N), GE_ERR_ARG),         # 5 more than twelve seats
            ((0, 501, 2, u32(2, 2), 3, O, E, 5, N), GE_ERR_ARG),                   # 5 a repeated seat, before the range
            ((0, 501, 1, u32(0), 3, O, E, 5, N), GE_ERR_RANGE),                    # 6 the range, before the seat of 0
            ((500, 1, 1, u32(1), 3, O, E, 5, N), GE_ERR_RANGE),
            ((1 << 63, 1 << 63, 1, u32(1), 3, O, E, 5, N), GE_ERR_RANGE),          # first + count wraps
            ((0, 10, 1, u32(0), 3, H, E, 5, N), GE_ERR_ARG),                       # 7 a seat of 0, before the pointers
            ((0, 10, 1, u32(7), 3, O, E, 5, N), GE_ERR_ARG),                       # 7 above segment 0's six players
            ((290, 20, 1, u32(5), 3, O, E, 5, N), GE_ERR_ARG),                     # 7 above segment 1's four, which the range touches
            ((17, 0, 1, u32(0), 3, O, E, 5, N), GE_ERR_ARG),                       # 7 a seat of 0 in an empty range
            ((0, 10, 2, u32(1, 2), 3, H, E, 5, N), GE_ERR_ARG),                    # 8 obs the device does not reach
            ((0, 10, 2, u32(1, 2), 3, O, H, 5, N), GE_ERR_ARG),                    # 8 entries
            ((0, 10, 2, u32(1, 2), 3, O, E, 5, H), GE_ERR_ARG),                    # 8 n
            ((17, 0, 2, u32(1, 2), 3, None, None, 0, H), GE_ERR_ARG),              # 8 n is vetted in an empty range too: it is stored
        ]
        for args, status in calls:
            assert fn(b._h, *args, None) == status, args
        b.sync()
        untouched = lambda: set(out.host().tobytes()) == {0x5A} and set(entries.host().tobytes()) == {0x5A} and not heap.any()
        assert untouched() and set(n.host().tobytes()) == {0x5A}
        # an empty range or an empty seat list: GE_OK, and n = {0, 0} is stored
        for args in ((17, 0, 2, u32(1, 2), 3, O, E, 5, N), (500, 0, 1, u32(1), 1, None, None, 0, N), (0, 0, 0, None, 2, None, None, 7, N),
                     (0, 10, 0, None, 3, None, None, 7, N)):
            assert out.hip.hipMemset(N, 0x5A, C.c_size_t(8)) == 0
            assert fn(b._h, *args, None) == 0, args
            b.sync()
            assert list(n.host(np.uint32)) == [0, 0] and untouched(), args
        assert fn(b._h, 0, 300, 1, u32(6), 3, O, E, 300, N, None) == 0           # seat 6 while the range stays in segment 0
        b.sync()
        k = int(n.host(np.uint32)[0])
        assert set(out.host()[k * 192:].tobytes()) == {0x5A} and set(entries.host()[k * 4:].tobytes()) == {0x5A}
        with pytest.raises(GeError) as e:
            b.gather_seats([1, 1], out, entries, n)
        assert e.value.status == GE_ERR_ARG
        with pytest.raises(GeError) as e:
            b.gather_seats([1], out, entries, n, first=400, count=200)
        assert e.value.status == GE_ERR_RANGE
        with pytest.raises(GeError) as e:
            b.gather_seats([1], out, entries, n, want=0)
        assert e.value.status == GE_ERR_ARG
        with pytest.raises(ValueError):
            b.gather_seats([1], out, entries, n, want=("person",))
        assert b.read_rooms().tobytes() == before


def _dense(b, seats, first=0, count=None):
    count = b.n_rooms - first if count is None else count
    out = DeviceBuffer(count * len(seats) * 192)
    b.observe_seats(seats, out, first, count)
    b.sync()
    return out.host(SEAT_OBS_DTYPE).reshape(count, len(seats))


def test_a_stream_of_the_callers_orders_the_call_behind_the_step(dsl_ww):
    """step on one stream, the call on another, no host wait in between: the list is of the stepped batch."""
    tb = GameTable(dsl_ww)
    mk = lambda: RoomBatch([(tb, 8, 5000, 0b10000001)], seed=4, restart=True)
    with mk() as a, mk() as twin:
        twin.step(30)
        want = _dense(twin, [1, 8])
        out, entries, n = DeviceBuffer(10000 * 192, FILL), DeviceBuffer(10000 * 4, FILL), DeviceBuffer(8, FILL)
        hip = out.hip
        s1, s2 = C.c_void_p(), C.c_void_p()
        assert hip.hipStreamCreate(C.byref(s1)) == 0 and hip.hipStreamCreate(C.byref(s2)) == 0
        try:
            a.step(30, stream=s1.value)
            a.gather_seats([1, 8], out, entries, n, stream=s2.value)
            a.step(5, stream=s1.value)                           # ordered behind the list
            a.sync()
            assert hip.hipStreamSynchronize(s2) == 0
            k = assert_list((out.host(SEAT_OBS_DTYPE), entries.host(np.uint32), n.host(np.uint32)), want, SEAT | END, 10000 - TAIL, "two streams")
            assert 0 < k < 10000
        finally:
            a.sync()
            hip.hipStreamDestroy(s1)
            hip.hipStreamDestroy(s2)
        twin.step(5)
        assert a.read_rooms().tobytes() == twin.read_rooms().tobytes()


def test_kernel_time_counts_the_call_as_one_interval(dsl_ww, dsl_tt):
    with RoomBatch([(GameTable(dsl_ww), 8, 5000, 1), (GameTable(dsl_tt), 4, 300, 1)], seed=2, restart=True) as b:
        b.step(30)
        b.set_timing(True)
        b.kernel_time(reset=True)
        call(b, [1], "seat", 0, 5000)                            # one segment: its test launch, the scan, its emit launch
        ms, launches = b.kernel_time(reset=True)
        assert ms > 0.0 and launches == 3
        call(b, [1, 2], ("seat", "end"))                         # two segments
        assert b.kernel_time(reset=True)[1] == 5
        call(b, [1, 2], "end", cap=0)                            # counting only: nothing is emitted
        assert b.kernel_time(reset=True)[1] == 3


def test_more_wavefronts_than_a_pass_of_the_scan_and_a_ragged_tail(dsl_ww):
    """65 536 + 64 + 7 Werewolf x 8 rooms are 1 026 wavefronts, the last of 7 rooms; ge_find_scan's block covers 1 024 per pass.
    Stepped 40 turns with restart, then three seats made host-driven so that some are pending.  The list must equal the filter
    over ge_batch_observe_seats's own dense output of the same range (the records themselves are checked above)."""
    rooms = 65536 + 64 + 7
    seats = [8, 1, 4]
    with RoomBatch([(GameTable(dsl_ww), 8, rooms, 0)], seed=11, first_room=1 << 20, restart=True) as b:
        b.step(40)
        b.set_seats(np.arange(rooms), np.full(rooms, 0b10001001))
        b.step(3)
        dense = _dense(b, seats)
        for want in WANTS:
            k = assert_list(call(b, seats, want), dense, want, None, ("large", want))
            assert 0 < k < dense.size
        d = due(dense, SEAT | END)
        assert d[65536:].any() and d[:64].any()                  # the second pass of the scan and the ragged wavefront carry entries
        first, count = 60, rooms - 100                           # ... and a window that is not aligned to wavefronts
        assert_list(call(b, seats, SEAT | END, first, count, cap=100000), dense[first:first + count], SEAT | END, 100000, "large window")

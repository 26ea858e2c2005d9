"""ge_batch_observe_seats (-m gpu): every record byte-equal to tests/observe_ref.py (POLICY.md §3n restated on the oracle) - every
layout, shipped, draft and GENERIC tables, a mixed batch, restart on and off; 135 rooms per segment (two full wavefronts and a
tail of 7); seat lists of one, three and all seats; the whole batch, a window inside a segment, a window across segments and an
empty one -, the same after write_rooms of fuzzed views and under a seat plane, that the call only reads, the refusals in their
order, a stream of the caller's and the timing interval."""
import ctypes as C
import json

import numpy as np
import pytest

from game_engine_amd import GameTable, GeError, RoomBatch
from game_engine_amd.stepper import SEAT_OBS_DTYPE
from observe_ref import OBSERVE_CASES, PER, case_all_seats, case_records, DeviceBuffer, differing_fields, make_batch, observe_batch, seat_lists, windows
from parity_util import oracle_rooms_as_views, views_as_oracle_rooms

pytestmark = pytest.mark.gpu

GE_ERR_ARG, GE_ERR_RANGE = -1, -6


def observe(b, seats, first=0, count=None, stream=None, fill=0):
    """The call into fresh device memory; the records of the range as a SEAT_OBS_DTYPE array [count, len(seats)]."""
    count = b.n_rooms - first if count is None else count
    out = DeviceBuffer(count * len(seats) * 192, fill)
    b.observe_seats(seats, out, first, count, stream=stream or 0)
    b.sync()
    return out.host(SEAT_OBS_DTYPE).reshape(count, len(seats))


def assert_records(got, want, what):
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(np.array([[g.tobytes() != w.tobytes() for g, w in zip(gr, wr)] for gr, wr in zip(got, want)]))
        r, j = bad[0]
        raise AssertionError(f"{what}: {len(bad)} records differ, fields {differing_fields(got, want)}; first at room {r} entry {j}: "
                             f"got {got[r, j]} want {want[r, j]}")


@pytest.mark.parametrize("restart", [False, True])
@pytest.mark.parametrize("name", OBSERVE_CASES)
def test_every_record_equals_the_reference(name, restart):
    segs, _ = case_all_seats(name, restart)
    seen = 0
    with make_batch(segs, restart) as b:
        for seats in seat_lists(segs):
            want = case_records(name, restart, seats)
            for first, count in windows(len(segs)):
                got = observe(b, seats, first, count, fill=0xA5)
                assert_records(got, want[first:first + count], (name, restart, seats, first, count))
                seen += got.size
    assert seen > 0
    want = case_records(name, restart, seat_lists(segs)[2])
    assert want["unknown"].any() and want["legal"].any() and (want["legal"] == 0).any()


def test_done_and_won_occur_in_the_cases():
    """(the outcome words are exercised: finished rooms with winners and losers, in both games)"""
    for name in ("ww8_h1", "tt4_h1"):
        segs, per_seg = case_all_seats(name, False)
        rec = per_seg[0]
        assert rec["done"].any() and not rec["done"].all()
        assert rec["won"][rec["done"] == 1].any() and (rec["won"][rec["done"] == 1] == 0).any() and not rec["won"][rec["done"] == 0].any()


def fuzzed_views(orc, rooms, rng):
    """The rooms' views with every player field and the Detective's memory random (values a view may hold: ge_host.h view_fits)."""
    v = oracle_rooms_as_views(orc, rooms)
    n = orc.n
    shape = (len(v), n)
    if orc.table.pack == 1:
        hi = [5, 3, 2, 2, 2, 2, 2, 2, n + 1, 2, n + 1]
    else:
        hi = [2, 2, 4, 2, 2, 4, 2, 256, 16, 2, 4]
    for f, h in enumerate(hi):
        v["players"][:, :n, f] = rng.integers(0, h, shape)
    if orc.table.pack == 1:
        v["det"][:, :n] = rng.integers(0, 3, shape)
    return v


@pytest.mark.parametrize("name", OBSERVE_CASES)
def test_fuzzed_views_and_a_seat_plane(name):
    """Records no game reaches - random fields, random Detective memory - and, on the same batch, a seat plane over some rooms:
    the plane must not matter."""
    rng = np.random.default_rng(sum(map(ord, name)))
    segs, _ = case_all_seats(name, True)
    views = [fuzzed_views(orc, rooms, rng) for orc, _, _, _, rooms in segs]
    fuzzed = [(orc, views_as_oracle_rooms(orc, v)) for (orc, _, _, _, _), v in zip(segs, views)]
    seats = seat_lists(segs)[1]
    want = observe_batch(fuzzed, seats)
    with make_batch(segs, True, views=views) as b:
        assert_records(observe(b, seats), want, (name, "fuzzed"))
        rooms = rng.permutation(b.n_rooms)[: b.n_rooms // 3]
        n_of = np.repeat([s[2] for s in segs], PER)
        b.set_seats(rooms, [int(rng.integers(0, 1 << n_of[r])) for r in rooms])
        assert_records(observe(b, seats), want, (name, "fuzzed, seat plane"))
        assert_records(observe(b, seats, 63, 67), want[63:130], (name, "fuzzed, seat plane, window"))
    assert want["unknown"].any() and want["legal"].any()


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
            observe(b, seats)
            observe(b, seats, 63, 67)
        assert _state(b) == before


@pytest.mark.parametrize("n_players,max_fuse", [(8, 0), (8, 1), (12, 1)])
def test_steps_with_observations_in_between_end_as_a_twin_that_never_looked(dsl_ww, n_players, max_fuse):
    """Fused steps, single-turn launches, and a Werewolf x 12 batch with its deal side plane: prepared deals stay as they are."""
    tb = GameTable(dsl_ww)
    mk = lambda: RoomBatch([(tb, n_players, 700, 0b101)], seed=99, first_room=1 << 33, max_fuse=max_fuse, restart=True)
    with mk() as a, mk() as twin:
        for k in (1, 3, 64, 1, 17, 2):
            a.step(k)
            twin.step(k)
            observe(a, [1, 3])
        assert a.summary() == twin.summary() and a.turn == twin.turn
        assert a.read_rooms().tobytes() == twin.read_rooms().tobytes()
        a.step(40)
        twin.step(40)
        assert a.summary() == twin.summary()


def test_a_stream_of_the_callers_orders_the_call_behind_the_step(dsl_ww):
    """step on one stream, observe on another, no host wait in between: the observation is of the stepped batch."""
    tb = GameTable(dsl_ww)
    mk = lambda: RoomBatch([(tb, 8, 5000, 1)], seed=4, restart=True)
    with mk() as a, mk() as twin:
        twin.step(30)
        want = observe(twin, [1, 8])
        out = DeviceBuffer(5000 * 2 * 192)
        hip = out.hip
        s1, s2 = C.c_void_p(), C.c_void_p()
        assert hip.hipStreamCreate(C.byref(s1)) == 0 and hip.hipStreamCreate(C.byref(s2)) == 0
        try:
            a.step(30, stream=s1.value)
            a.observe_seats([1, 8], out, stream=s2.value)
            a.step(5, stream=s1.value)                           # ordered behind the observation
            a.sync()
            assert hip.hipStreamSynchronize(s2) == 0
            assert_records(out.host(SEAT_OBS_DTYPE).reshape(5000, 2), want, "two streams")
        finally:
            a.sync()
            hip.hipStreamDestroy(s1)
            hip.hipStreamDestroy(s2)
        twin.step(5)
        assert a.read_rooms().tobytes() == twin.read_rooms().tobytes()


def test_refusals_in_their_order_leave_the_output_untouched(dsl_ww, dsl_tt):
    with RoomBatch([(GameTable(dsl_ww), 6, 300, 1), (GameTable(dsl_tt), 4, 200, 2)], seed=1, max_fuse=1) as b:
        b.step(9)
        before = b.read_rooms().tobytes()
        call = b._lib.ge_batch_observe_seats
        out = DeviceBuffer(500 * 3 * 192, 0x5A)
        P, CAP = C.c_void_p(out.data_ptr()), out.nbytes
        u32 = lambda *v: (C.c_uint32 * len(v))(*v)
        calls = [
            # (first, count, n_seats, seats, obs, cap) -> status; later errors are present too where they can be
            ((0, 501, 1, None, P, CAP), GE_ERR_ARG),                     # 2 seats NULL (range wrong as well)
            ((0, 501, 1, u32(1), None, CAP), GE_ERR_ARG),                # 2 obs NULL
            ((0, 501, 13, u32(*range(1, 14)), P, CAP), GE_ERR_ARG),      # 3 more than twelve seats
            ((0, 501, 2, u32(2, 2), P, CAP), GE_ERR_ARG),                # 4 a repeated seat, before the range
            ((0, 501, 1, u32(0), P, CAP), GE_ERR_RANGE),                 # 5 the range, before the seat of 0
            ((500, 1, 1, u32(1), P, CAP), GE_ERR_RANGE),
            ((1 << 63, 1 << 63, 1, u32(1), P, CAP), GE_ERR_RANGE),       # first + count wraps
            ((0, 10, 1, u32(0), P, 0), GE_ERR_ARG),                      # 6 a seat of 0, before the capacity
            ((0, 10, 1, u32(7), P, CAP), GE_ERR_ARG),                    # 6 above segment 0's six players
            ((290, 20, 1, u32(5), P, CAP), GE_ERR_ARG),                  # 6 above segment 1's four, which the range touches
            ((17, 0, 1, u32(0), P, CAP), GE_ERR_ARG),                    # 6 a seat of 0 in an empty range
            ((0, 10, 2, u32(1, 2), P, 10 * 2 * 192 - 1), GE_ERR_ARG),    # 7 one byte short
        ]
        for args, status in calls:
            first, count, n_seats, seats, obs, cap = args
            assert call(b._h, first, count, n_seats, seats, obs, cap, None) == status, args
        assert call(b._h, 0, 300, 1, u32(6), P, CAP, None) == 0          # seat 6 while the range stays in segment 0
        b.sync()
        assert set(out.host()[300 * 192:].tobytes()) == {0x5A}
        assert out.hip.hipMemset(C.c_void_p(out.ptr), 0x5A, C.c_size_t(out.nbytes)) == 0
        for args in ((17, 0, 2, u32(1, 2), P, 0), (500, 0, 1, u32(1), None, 0), (0, 0, 0, None, None, 0), (0, 10, 0, None, None, 0)):   # 9
            first, count, n_seats, seats, obs, cap = args
            assert call(b._h, first, count, n_seats, seats, obs, cap, None) == 0, args
        b.sync()
        assert set(out.host().tobytes()) == {0x5A}
        with pytest.raises(GeError) as e:
            b.observe_seats([1, 1], out)
        assert e.value.status == GE_ERR_ARG
        with pytest.raises(GeError) as e:
            b.observe_seats([1], out, first=400, count=200)
        assert e.value.status == GE_ERR_RANGE
        assert b.read_rooms().tobytes() == before


def test_kernel_time_includes_the_call(dsl_ww):
    with RoomBatch([(GameTable(dsl_ww), 8, 5000, 1)], seed=2, restart=True) as b:
        b.step(30)
        b.set_timing(True)
        b.kernel_time(reset=True)
        observe(b, [1])
        ms, launches = b.kernel_time(reset=True)
        assert ms > 0.0 and launches == 1

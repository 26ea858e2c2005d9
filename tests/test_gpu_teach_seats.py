"""ge_batch_teach_seats (-m gpu): a seat list of every room of a range advised into device memory, against the call's composition
rule (tests/teach_ref.py: the batch's own advise_seats over the same pairs) byte for byte - every layout, seat lists and windows
across segment borders, one and two wavefronts per entry, the full view, keys on the device, more slots than one pass holds -, two
cases against the oracle directly, that the call only reads, its ordering on the stream without a synchronisation in between, the
scratch it shares with the indexed calls, and every structural refusal in the header's order."""
import ctypes as C

import numpy as np
import pytest

from advise_ref import ADVICE_REF_DTYPE, GE_ERR_ARG, reference_advice
from game_engine_amd import GeError
from game_engine_amd.stepper import ADVICE_DTYPE
from observe_ref import DeviceBuffer, make_batch, seat_lists
from parity_util import assert_views_equal, oracle_events, oracle_rooms_as_views
from run_ref import SEED, case_inputs
from teach_ref import M, PER, R, STEPS, TEACH_CASES, differing, expected, key_of, oracle_rooms_after, stepped_batch, teach, windows

pytestmark = pytest.mark.gpu

GE_ERR_RANGE = -6
REC = ADVICE_DTYPE.itemsize
EV_FIELDS = ("turn", "from_phase_id", "to_phase_id", "acted_now", "restarted", "choice")


def _same(got, tail, want, what):
    assert got.tobytes() == want.tobytes(), (what, differing(got, want))
    assert (tail == 0xA5).all(), f"{what}: bytes behind the records were written"


@pytest.mark.parametrize("name", TEACH_CASES)
def test_every_window_and_seat_list_equals_advise_seats(name):
    """The seat list (1, 2) over the whole batch must put both halves of the answer to the test - a fifth of its pairs advised, a
    fifth refused, judged from the expected records alone (on the oracle: 49 of 134 in ww8_h1, 70 of 134 in tt4_h1, 144 of 536 in
    mixed); the lists of observe_ref.seat_lists are compared as well, whatever their share."""
    segs, b = stepped_batch(name)
    with b:
        assert b.turn == STEPS and b.n_rooms == PER * len(segs)
        for seats in [[1, 2]] + seat_lists(segs):
            for first, count in windows(len(segs)):
                want = expected(b, first, count, seats, R, M, key0=11)
                if seats == [1, 2] and count == b.n_rooms:
                    advised, pairs = int((want["status"] == 0).sum()), len(want)
                    assert set(want["status"].tolist()) == {0, GE_ERR_ARG}
                    assert 5 * advised >= pairs and 5 * (pairs - advised) >= pairs, (name, advised, pairs)
                got, tail = teach(b, first, count, seats, R, M, key0=11)
                assert len(got) == count * len(seats)
                _same(got, tail, want, (name, seats, first, count))


def test_a_window_of_no_rooms_writes_nothing():
    segs, b = stepped_batch("ww8_h1")
    with b:
        buf = DeviceBuffer(2 * REC, fill=0xA5)
        b.teach_seats([1, 2], buf, R, M, first=17, count=0)
        b.teach_seats([], buf, R, M)
        b.teach_seats([1], buf, R, M, first=PER, count=0)        # the end of the batch is a valid place for no rooms
        assert (buf.host() == 0xA5).all()


@pytest.mark.parametrize("name", ["ww8_h1", "tt4_h1"])
def test_against_the_oracle_directly(name):
    key0 = (1 << 40) + 5                                         # keys on both sides of 2^32: r << 20 crosses it inside the batch
    segs, b = stepped_batch(name)
    (orc, rooms), = oracle_rooms_after(segs)
    want = np.array([reference_advice(orc, rooms[r], SEED, key_of(r, key0), STEPS, 1, R, M) for r in range(PER)], dtype=ADVICE_REF_DTYPE)
    with b:
        got, tail = teach(b, 0, PER, [1], R, M, key0=key0)
    assert (want["status"] == 0).any() and (want["status"] != 0).any()
    _same(got, tail, want, name)


@pytest.mark.parametrize("n_rollouts,full_view", [(1, False), (64, False), (R, True)])
def test_one_wavefront_and_the_full_view(n_rollouts, full_view):
    segs, b = stepped_batch("ww8_h1")
    with b:
        want = expected(b, 0, PER, [1, 2], n_rollouts, M, key0=3, full_view=full_view)
        got, tail = teach(b, 0, PER, [1, 2], n_rollouts, M, key0=3, full_view=full_view)
        _same(got, tail, want, (n_rollouts, full_view))
        if full_view:                                            # (the view matters: the same seats advised from what they know)
            seat_view = teach(b, 0, PER, [1, 2], n_rollouts, M, key0=3)[0]
            assert not np.array_equal(got["option"]["wins"], seat_view["option"]["wins"])


def test_keys_on_the_device():
    segs, b = stepped_batch("mixed")
    rng = np.random.default_rng(9)
    first, count = PER - 5, PER + 40
    keys = rng.choice(1 << 40, size=count, replace=False).astype(np.uint64)
    keys[::2] = rng.choice(1 << 20, size=len(keys[::2]), replace=False)
    with b:
        kbuf = DeviceBuffer.of(keys)
        got, tail = teach(b, first, count, [3, 1], R, M, keys=kbuf, key0=99)   # (key0 plays no part beside keys)
        _same(got, tail, expected(b, first, count, [3, 1], R, M, keys=keys), "keys_dev")
        a = teach(b, first, count, [3, 1], R, M, key0=0)[0]
        c = teach(b, first, count, [3, 1], R, M, key0=1 << 33)[0]
        assert np.array_equal(a["legal"], c["legal"]) and not np.array_equal(a["option"]["wins"], c["option"]["wins"])
        with pytest.raises(GeError):
            b.teach_seats([1], DeviceBuffer(count * REC), R, M, first=first, count=count, keys=DeviceBuffer(8 * count - 8))


def test_more_slots_than_a_pass_holds():
    """Werewolf x 12, 512 rooms, all 12 seats: 6 144 pairs of 13 slots each reserve 79 872 > 65 536, so the call takes two passes."""
    segs = case_inputs("ww12_h2", 512, True)[0]
    seats = list(range(1, 13))
    assert 512 * 12 * 13 > 65536
    with make_batch(segs, True) as b:
        b.step(STEPS)
        want = expected(b, 0, 512, seats, 1, 8, key0=5)
        got, tail = teach(b, 0, 512, seats, 1, 8, key0=5)
        assert (want["status"] == 0).sum() > 100 and (want["status"] != 0).sum() > 100
        _same(got, tail, want, "two passes")


def _state(b, trace):
    return (b.read_rooms().tobytes(), b.seats().tobytes(), b.turn, b.read_events().tobytes() if trace else b"", b.summary()["checksum"])


@pytest.mark.parametrize("how", ["plain", "restart_trace"])
def test_teach_seats_reads_only(how):
    segs = case_inputs("mixed", PER, True)[0]
    trace = how == "restart_trace"
    with make_batch(segs, trace, max_fuse=3, trace=trace) as b:  # (a trace holds max_fuse turns)
        b.step(3)
        before = _state(b, trace)
        got = teach(b, 0, b.n_rooms, [1, 2], 5, 20)[0]
        assert _state(b, trace) == before
        assert (got["status"] == 0).any() and (got["status"] != 0).any()


def test_calls_are_ordered_on_the_stream_without_a_wait():
    """step(3), teach_seats, step(3), teach_seats into a second buffer, nothing synchronised in between: the first buffer holds the
    advice of the state after 3 turns, the second that of the state after 6 - both established afterwards from twin batches."""
    segs = case_inputs("ww8_h1", PER, True)[0]
    seats, need = [1, 2], PER * 2 * REC
    with make_batch(segs, True) as b:
        one, two, again = DeviceBuffer(need, fill=0xA5), DeviceBuffer(need, fill=0xA5), DeviceBuffer(need, fill=0xA5)
        b.teach_seats(seats, DeviceBuffer(need), R, M)           # (the scratch is grown here: the calls below allocate nothing)
        b.step(3)
        b.teach_seats(seats, one, R, M, key0=21)
        b.step(3)
        b.teach_seats(seats, two, R, M, key0=21)
        b.teach_seats(seats, again, R, M, key0=21)
        got = [x.host(ADVICE_DTYPE) for x in (one, two, again)]
    assert got[1].tobytes() == got[2].tobytes(), "two identical calls differ"
    for turns, have in ((3, got[0]), (6, got[1])):
        with make_batch(segs, True) as twin:
            twin.step(turns)
            want = expected(twin, 0, PER, seats, R, M, key0=21)
        assert have.tobytes() == want.tobytes(), (turns, differing(have, want))
    assert got[0].tobytes() != got[1].tobytes()


def test_teach_seats_shares_the_scratch_of_the_indexed_calls():
    """step_rooms, a teach_seats large enough to regrow the scratch, step_rooms and read_rooms_at: events and views equal the
    oracle's."""
    segs = case_inputs("ww12_h2", 192, False)[0]
    orc, _, _, mask, recs = segs[0]
    recs = recs.copy()
    listed = np.array([3, 0, 11, 7], dtype=np.uint64)
    with make_batch(segs, False) as b:
        for rnd, (skeys, sturns) in enumerate([([5, 1 << 35, 7, 8], [0, 4, 9, 100]), ([9, 10, 1 << 40, 12], [1, 5, 10, 101])]):
            ev = b.step_rooms(listed, skeys, sturns)
            for k, r in enumerate(listed):
                one = recs[int(r):int(r) + 1]
                orc.run(one, SEED, int(skeys[k]), int(sturns[k]), 1, threads=1, restart=False, human_mask=mask)
                want = oracle_events(orc, one, int(sturns[k]))[0]
                for f in EV_FIELDS:
                    assert np.array_equal(ev[k][f], want[f]), (rnd, int(r), f)
            if rnd == 0:
                got = teach(b, 0, 192, list(range(1, 13)), 1, 4)[0]
                assert len(got) == 192 * 12
        assert_views_equal(b.read_rooms_at(listed), oracle_rooms_as_views(orc, recs[listed.astype(np.int64)]), "after the advice")


def test_structural_errors_leave_the_output_untouched():
    segs = case_inputs("mixed", 16, True)[0]                     # segments of 6, 4, 10 and 7 players, 16 rooms each
    libc = C.CDLL(None)
    libc.malloc.restype = C.c_void_p
    libc.malloc.argtypes = [C.c_size_t]
    libc.free.argtypes = [C.c_void_p]
    with make_batch(segs, True) as b:
        lib = b._lib
        buf = DeviceBuffer(64 * 12 * REC, fill=0xA5)
        keys = DeviceBuffer(64 * 8)
        heap = libc.malloc(64 * 12 * REC)

        def call(first, count, seats, n_rollouts=4, max_turns=4, flags=0, turn=0, out=buf.ptr, cap=buf.nbytes, kdev=None, handle=b._h):
            arr = np.asarray(seats if seats is not None else [], dtype=np.uint32)
            st = lib.ge_batch_teach_seats(handle, first, count, len(arr) if seats is not None else 1, arr.ctypes.data if seats is not None else None,
                                          kdev, 0, turn, n_rollouts, max_turns, 7, flags, out, cap, None)
            return st, bool((buf.host() == 0xA5).all())

        cases = [
            (dict(first=0, count=1, seats=[1], handle=None), GE_ERR_ARG),                        # 1. no batch
            (dict(first=0, count=1, seats=[1], flags=2), GE_ERR_ARG),                            # 2. an unknown flag bit
            (dict(first=0, count=1, seats=[1], flags=0x80000001), GE_ERR_ARG),
            (dict(first=0, count=1, seats=[1], n_rollouts=0), GE_ERR_ARG),                       # 3. the caps
            (dict(first=0, count=1, seats=[1], n_rollouts=(1 << 20) + 1), GE_ERR_ARG),
            (dict(first=0, count=1, seats=[1], max_turns=4097), GE_ERR_ARG),
            (dict(first=0, count=1, seats=None), GE_ERR_ARG),                                    # 4. env_check's, in its order
            (dict(first=0, count=1, seats=[1], out=None), GE_ERR_ARG),
            (dict(first=0, count=1, seats=list(range(1, 14))), GE_ERR_ARG),
            (dict(first=0, count=1, seats=[2, 3, 2]), GE_ERR_ARG),
            (dict(first=60, count=5, seats=[1]), GE_ERR_RANGE),
            (dict(first=1 << 63, count=1 << 63, seats=[1]), GE_ERR_RANGE),
            (dict(first=0, count=1, seats=[0]), GE_ERR_ARG),
            (dict(first=0, count=1, seats=[7]), GE_ERR_ARG),                                     # above segment 0's 6
            (dict(first=10, count=10, seats=[5]), GE_ERR_ARG),                                   # above segment 1's 4
            (dict(first=0, count=3, seats=[1, 2], cap=3 * 2 * REC - 1), GE_ERR_ARG),             # one byte short
            (dict(first=0, count=3, seats=[1, 2], out=heap), GE_ERR_ARG),                        # pageable host memory
            (dict(first=0, count=3, seats=[1, 2], kdev=heap), GE_ERR_ARG),
            (dict(first=0, count=1, seats=[1], turn=0xFFFFFFFF - 3), GE_ERR_RANGE),              # 5. turn + max_turns
            (dict(first=0, count=10, seats=[1], n_rollouts=1 << 20), GE_ERR_ARG),                # 6. 10 x 7 x 2^20 > 2^26
            (dict(first=16, count=13, seats=[1], n_rollouts=1 << 20), GE_ERR_ARG),               #    Two-Truths x 4: 13 x 5 x 2^20
            (dict(first=0, count=5, seats=[1, 2], n_rollouts=1 << 20), GE_ERR_ARG),              #    5 x 2 x 7 x 2^20
        ]
        for kw, want in cases:
            assert call(**kw) == (want, True), (kw, want, call(**kw))
        # the order: a call that fails two checks answers with the earlier one's code
        assert call(60, 5, [1], flags=2)[0] == GE_ERR_ARG                                        # 2 before 4's range
        assert call(60, 5, [2, 2])[0] == GE_ERR_ARG                                              # a repeated seat before the range
        assert call(60, 5, [7])[0] == GE_ERR_RANGE                                               # the range before the seat's bound
        assert call(0, 10, [1], n_rollouts=1 << 20, turn=0xFFFFFFFF)[0] == GE_ERR_RANGE          # 5 before 6
        assert call(0, 3, [1, 2], turn=0xFFFFFFFF, out=heap)[0] == GE_ERR_ARG                    # 4 before 5
        assert call(0, 0, [1], turn=0xFFFFFFFF) == (GE_ERR_RANGE, True)                          # 5 before 7
        assert call(17, 0, [1, 2], out=None, cap=0) == (0, True)                                 # 7. nothing to do
        assert call(0, 5, []) == (0, True)
        # the last of everything that is accepted
        assert call(0, 1, [1], turn=0xFFFFFFFF - 4)[0] == 0
        assert call(0, 9, [1], n_rollouts=1 << 20, max_turns=0)[0] == 0                          # 9 x 7 x 2^20 <= 2^26 (no turns played)
        assert call(0, 3, [1, 2], cap=3 * 2 * REC, kdev=keys.ptr)[0] == 0
        with pytest.raises(GeError):
            b.teach_seats([7], buf, 4, 4, count=1)
        libc.free(heap)

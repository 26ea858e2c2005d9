"""ge_batch_act_listed (-m gpu) against its definition (POLICY.md §3q): a batch and its twin, 40 turns stepped; a list from
ge_batch_gather_seats with random legal and illegal choices, as gathered and in shuffled order; records and statuses equal the
twin's after ge_batch_act_seats with the dense array D of tests/gather_ref.py.  Entries at or beyond count * n_seats are refused
and harmless, *n_dev smaller and larger than cap, a window inside the mixed batch, a room without a listed entry is not written,
status behind the list is not written, and the refusals in their order."""
import ctypes as C

import numpy as np
import pytest

from game_engine_amd import GameTable, GeError, RoomBatch
from game_engine_amd.stepper import SEAT_OBS_DTYPE
from gather_ref import GE_ERR_ARG, dense_choices, listed_status
from observe_ref import DeviceBuffer
from run_ref import dsl_of

pytestmark = pytest.mark.gpu

GE_ERR_RANGE = -6
FILL = 0x4D
FILL32 = int(np.frombuffer(bytes([FILL] * 4), dtype=np.int32)[0])


def make(kind, rooms=300):
    """Werewolf x 8 with every seat host-driven, or a mixed batch (Werewolf x 8, Two-Truths x 4, Werewolf x 12) with four; 40 turns
    stepped before the seats become host-driven, then three more, so that rooms wait at every phase and some have ended"""
    ww, tt = GameTable(dsl_of("ww")), GameTable(dsl_of("tt"))
    segs = [(ww, 8, rooms, 0)] if kind == "ww8" else [(ww, 8, rooms, 0), (tt, 4, rooms // 2 + 7, 0), (ww, 12, rooms, 0)]
    b = RoomBatch(segs, seed=21, first_room=5000, restart=True)
    b.step(40)
    n_seats = 8 if kind == "ww8" else 4
    b.set_seats(np.arange(b.n_rooms), np.full(b.n_rooms, (1 << n_seats) - 1))
    b.step(3)
    return b, list(range(1, n_seats + 1))


def gathered(b, seats, first, count):
    """(entries, legal of each listed entry) of the range's decision list"""
    total = count * len(seats)
    out, entries, n = DeviceBuffer(total * 192), DeviceBuffer(total * 4), DeviceBuffer(8)
    b.gather_seats(seats, out, entries, n, ("seat", "end"), first, count)
    b.sync()
    k = int(n.host(np.uint32)[0])
    return entries.host(np.uint32)[:k].copy(), out.host(SEAT_OBS_DTYPE)[:k]["legal"].copy()


def random_choices(rng, legal):
    """per listed entry one of: no action, a legal choice (where there is one), any choice 1 .. 15, a negative one, one above 15"""
    kind = rng.choice(5, size=len(legal), p=[0.15, 0.5, 0.2, 0.07, 0.08])
    out = np.zeros(len(legal), dtype=np.int32)
    for i in range(len(legal)):
        bits = [c + 1 for c in range(12) if (int(legal[i]) >> c) & 1]
        if kind[i] == 1:
            out[i] = rng.choice(bits) if bits else 0
        elif kind[i] == 2:
            out[i] = rng.integers(1, 16)
        elif kind[i] == 3:
            out[i] = -int(rng.integers(1, 1 << 31))
        elif kind[i] == 4:
            out[i] = rng.integers(16, 1 << 31)
    return out


def act_listed(b, seats, n_word, cap, entries, choices, first, count, slots=None, with_status=True):
    """The call with the list in fresh device memory of `slots` entries (cap by default); the status buffer as it was left"""
    slots = max(cap, len(entries)) if slots is None else slots
    e = np.full(slots, 0xFFFFFFFF, dtype=np.uint32)
    c = np.full(slots, 1, dtype=np.int32)
    e[:len(entries)] = entries
    c[:len(choices)] = choices
    n = DeviceBuffer.of(np.array([n_word, 0], dtype=np.uint32))
    status = DeviceBuffer(slots * 4, FILL) if with_status else None
    b.act_listed(seats, n, DeviceBuffer.of(e), DeviceBuffer.of(c), status, first, count, cap=cap)
    b.sync()
    return status.host(np.int32) if with_status else None


def act_dense(twin, seats, dense, first, count):
    status = DeviceBuffer(dense.size * 4, FILL)
    twin.act_seats(seats, DeviceBuffer.of(dense), status, first, count)
    twin.sync()
    return status.host(np.int32)


@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("kind,first,count", [("ww8", 0, None), ("mixed", 0, None), ("mixed", 250, 300), ("mixed", 17, 0)])
def test_the_call_is_act_seats_with_the_dense_array_of_the_list(kind, first, count, shuffled):
    rng = np.random.default_rng(len(kind) + first + shuffled)
    (b, seats), (twin, _) = make(kind), make(kind)
    with b, twin:
        count = b.n_rooms - first if count is None else count
        total = count * len(seats)
        entries, legal = gathered(b, seats, first, count)
        assert (0 < len(entries) < total) or count == 0
        choices = random_choices(rng, legal)
        if shuffled:
            order = rng.permutation(len(entries))
            entries, choices = entries[order], choices[order]
        before = b.read_rooms()
        got = act_listed(b, seats, len(entries), len(entries), entries, choices, first, count)
        dense = dense_choices(total, len(entries), len(entries), entries, choices)
        dense_status = act_dense(twin, seats, dense, first, count)
        want = listed_status(dense_status, total, len(entries), len(entries), entries, np.full(len(got), FILL32))
        assert np.array_equal(got, want), np.flatnonzero(got != want)[:5]
        after = b.read_rooms()
        assert after.tobytes() == twin.read_rooms().tobytes()
        if count:
            assert (got == 0).any() and (got == GE_ERR_ARG).any() and after.tobytes() != before.tobytes()
            idle = np.setdiff1d(np.arange(first, first + count), first + entries // len(seats))
            assert len(idle) and after[idle].tobytes() == before[idle].tobytes()     # a room without a listed entry is as it was
            outside = np.r_[0:first, first + count:b.n_rooms]
            assert after[outside].tobytes() == before[outside].tobytes()


@pytest.mark.parametrize("n_word,cap", [(10, 40), (40, 10), (0, 40), (40, 40)])
def test_n_is_read_on_the_device_and_bounded_by_cap(n_word, cap):
    """*n_dev smaller and larger than cap: min(*n_dev, cap) positions count, the rest of the list - valid entries with legal
    choices - is ignored, and status behind it is not written"""
    rng = np.random.default_rng(n_word * 41 + cap)
    (b, seats), (twin, _) = make("ww8"), make("ww8")
    with b, twin:
        total = b.n_rooms * len(seats)
        entries, legal = gathered(b, seats, 0, b.n_rooms)
        pick = np.sort(rng.choice(np.flatnonzero(legal != 0), 40, replace=False))
        entries, choices = entries[pick], np.array([int(x).bit_length() for x in legal[pick]], dtype=np.int32)   # the highest legal choice
        got = act_listed(b, seats, n_word, cap, entries, choices, 0, b.n_rooms, slots=40)
        n = min(n_word, cap)
        dense = dense_choices(total, n_word, cap, entries, choices)
        assert np.count_nonzero(dense) == n
        want = listed_status(act_dense(twin, seats, dense, 0, b.n_rooms), total, n_word, cap, entries, np.full(40, FILL32))
        assert np.array_equal(got, want) and (n == 0 or (got[:n] == 0).any()) and list(got[n:]) == [FILL32] * (40 - n)
        assert b.read_rooms().tobytes() == twin.read_rooms().tobytes()


def test_entries_beyond_the_grid_are_refused_and_harmless_and_a_twice_named_entry_reports_one_status():
    (b, seats), (twin, _) = make("mixed"), make("mixed")
    with b, twin:
        first, count = 100, 200                                  # inside segment 0: entries 0 .. 799
        total = count * len(seats)
        entries, legal = gathered(b, seats, first, count)
        ok = np.flatnonzero(legal != 0)[:6]
        good = np.array([int(x).bit_length() for x in legal[ok]], dtype=np.int32)
        # the grid's last entry + 1, far beyond, and entries that would be rooms of the batch beyond the range
        wild = np.array([total, total + 1, 0xFFFFFFFF, 0x80000000, total + 4 * 50], dtype=np.uint32)
        twice = np.array([entries[ok[0]], entries[ok[0]]], dtype=np.uint32)      # the same choice in both copies
        e = np.concatenate([wild[:2], entries[ok], wild[2:], twice])
        c = np.concatenate([[1, 2], good, [3, 1, 1], [good[0], good[0]]]).astype(np.int32)
        before = b.read_rooms()
        got = act_listed(b, seats, len(e), len(e), e, c, first, count)
        dense = dense_choices(total, len(e), len(e), e, c)
        want = listed_status(act_dense(twin, seats, dense, first, count), total, len(e), len(e), e, np.full(len(e), FILL32))
        assert np.array_equal(got, want) and list(got[:2]) == [GE_ERR_ARG] * 2 and list(got[8:11]) == [GE_ERR_ARG] * 3
        assert list(got[2:8]) == [0] * 6 and got[11] == got[12] == 0
        after = b.read_rooms()
        assert after.tobytes() == twin.read_rooms().tobytes()
        outside = np.r_[0:first, first + count:b.n_rooms]
        assert after[outside].tobytes() == before[outside].tobytes() and after.tobytes() != before.tobytes()
        # two different choices for one entry: one of them is applied, and both copies report its status
        j = ok[1]
        bits = [k + 1 for k in range(12) if (int(legal[j]) >> k) & 1]
        illegal = next(k for k in range(1, 16) if k not in bits)
        got = act_listed(b, seats, 2, 2, np.array([entries[j]] * 2, dtype=np.uint32), np.array([bits[0], illegal], dtype=np.int32), first, count)
        assert got[0] == got[1] and got[0] in (0, GE_ERR_ARG)


def test_status_may_be_null_and_the_refusals_keep_their_order(dsl_ww, dsl_tt):
    mk = lambda: RoomBatch([(GameTable(dsl_ww), 6, 300, 1), (GameTable(dsl_tt), 4, 200, 2)], seed=1, max_fuse=1)
    with mk() as b, mk() as twin:
        b.step(9)
        twin.step(9)
        before = b.read_rooms().tobytes()
        fn = b._lib.ge_batch_act_listed
        n = DeviceBuffer.of(np.array([1000], dtype=np.uint32))
        en = DeviceBuffer.of(np.arange(1000, dtype=np.uint32))
        ch = DeviceBuffer.of(np.ones(1000, dtype=np.int32))
        st = DeviceBuffer(1000 * 4, FILL)
        heap = np.zeros(1000, dtype=np.uint32)                              # pageable host memory: not vetted
        N, E, P, S, H = (C.c_void_p(x) for x in (n.ptr, en.ptr, ch.ptr, st.ptr, heap.ctypes.data))
        u32 = lambda *v: (C.c_uint32 * len(v))(*v)
        calls = [
            # (first, count, n_seats, seats, n, cap, entries, choices, status) -> status
            ((0, 501, 1, None, N, 1000, E, P, S), GE_ERR_ARG),                    # 2 seats NULL (range wrong as well)
            ((0, 501, 1, u32(1), None, 1000, E, P, S), GE_ERR_ARG),               # 2 n NULL
            ((0, 501, 1, u32(1), N, 1000, None, P, S), GE_ERR_ARG),               # 2 entries NULL with cap > 0
            ((0, 501, 1, u32(1), N, 1000, E, None, S), GE_ERR_ARG),               # 2 choices NULL with cap > 0
            ((0, 501, 13, u32(*range(1, 14)), N, 1000, E, P, S), GE_ERR_ARG),     # 3
            ((0, 501, 2, u32(2, 2), N, 1000, E, P, S), GE_ERR_ARG),               # 4 before 5
            ((0, 501, 1, u32(0), N, 1000, E, P, S), GE_ERR_RANGE),                # 5 before 6
            ((0, 10, 1, u32(0), H, 1000, E, P, S), GE_ERR_ARG),                   # 6 before the pointers
            ((290, 20, 1, u32(5), N, 1000, E, P, S), GE_ERR_ARG),                 # 6 above the four players of segment 1
            ((0, 10, 1, u32(1), H, 1000, E, P, S), GE_ERR_ARG),                   # 7 n the device does not reach
            ((0, 10, 1, u32(1), N, 1000, H, P, S), GE_ERR_ARG),                   # 7 entries
            ((0, 10, 1, u32(1), N, 1000, E, H, S), GE_ERR_ARG),                   # 7 choices
            ((0, 10, 1, u32(1), N, 1000, E, P, H), GE_ERR_ARG),                   # 7 status
        ]
        for args, status in calls:
            assert fn(b._h, *args, None) == status, args
        for args in ((17, 0, 2, u32(1, 2), None, 5, None, None, None), (0, 10, 0, None, None, 5, None, None, None),
                     (0, 10, 1, u32(1), N, 0, None, None, None)):            # nothing to do: an empty range, no seat, an empty list
            assert fn(b._h, *args, None) == 0, args
        b.sync()
        assert b.read_rooms().tobytes() == before and set(st.host().tobytes()) == {FILL} and not heap.any()
        with pytest.raises(GeError):
            b.act_listed([1, 2], n, en, DeviceBuffer(10 * 4), None, cap=1000)     # (the binding: fewer entries than cap)
        b.act_listed([1, 2], n, en, ch, None)                                    # status NULL; the list is the whole dense grid
        b.sync()
        twin.act_seats([1, 2], DeviceBuffer.of(np.ones((500, 2), dtype=np.int32)))
        assert b.read_rooms().tobytes() == twin.read_rooms().tobytes() != before

"""ge_batch_act_seats (-m gpu) against its definition: a twin batch driven by ge_batch_inject_actions with the composed entry list -
the entries (room, seat, choice) with a non-zero choice, in ascending (room, seat index) order.  Random choice tensors hold zeros,
legal choices, illegal ones, negative ones and choices above 15; status for status, every room's view equal, rooms outside the
range untouched; over the cases, seat lists and ranges of tests/test_gpu_observe_seats.py."""
import ctypes as C

import numpy as np
import pytest

from game_engine_amd import GameTable, GeError, RoomBatch
from observe_ref import OBSERVE_CASES, case_all_seats, DeviceBuffer, case_records, make_batch, seat_lists, windows

pytestmark = pytest.mark.gpu

GE_ERR_ARG, GE_ERR_RANGE = -1, -6


def random_choices(rng, legal):
    """legal: uint16 [count, S].  Per entry one of: no action, a legal choice (where there is one), any choice 1 .. 15, a
    negative choice, a choice above 15."""
    kind = rng.choice(5, size=legal.shape, p=[0.3, 0.4, 0.15, 0.07, 0.08])
    out = np.zeros(legal.shape, dtype=np.int32)
    for idx in np.ndindex(*legal.shape):
        bits = [c + 1 for c in range(12) if (int(legal[idx]) >> c) & 1]
        k = kind[idx]
        if k == 1:
            out[idx] = rng.choice(bits) if bits else 0
        elif k == 2:
            out[idx] = rng.integers(1, 16)
        elif k == 3:
            out[idx] = -int(rng.integers(1, 1 << 31))
        elif k == 4:
            out[idx] = rng.integers(16, 1 << 31)
    return out


def act(b, seats, choices, first, count, with_status=True):
    dev = DeviceBuffer.of(choices.astype(np.int32))
    status = DeviceBuffer(choices.size * 4, 0x4D) if with_status else None
    b.act_seats(seats, dev, status, first, count)
    b.sync()
    return status.host(np.int32).reshape(choices.shape) if with_status else None


def inject_composed(twin, seats, choices, first):
    """the definition: inject_actions over the non-zero entries in ascending (room, j) order; status per entry, 0 for a zero choice"""
    r, j = np.nonzero(choices)                                   # (row-major: ascending (room, j))
    status = np.zeros(choices.shape, dtype=np.int32)
    if len(r):
        status[r, j] = twin.inject_actions(first + r, np.asarray(seats, dtype=np.uint32)[j], choices[r, j].astype(np.int64) & 0xFFFFFFFF)
    return status


@pytest.mark.parametrize("restart", [False, True])
@pytest.mark.parametrize("name", OBSERVE_CASES)
def test_act_seats_is_inject_actions_over_the_composed_entries(name, restart):
    rng = np.random.default_rng(sum(map(ord, name)) + restart)
    segs, _ = case_all_seats(name, restart)
    applied = refused = 0
    for seats in seat_lists(segs):
        legal = case_records(name, restart, seats)["legal"]
        for first, count in windows(len(segs)):
            choices = random_choices(rng, legal[first:first + count])
            with make_batch(segs, restart) as b, make_batch(segs, restart) as twin:
                got = act(b, seats, choices, first, count)
                want = inject_composed(twin, seats, choices, first)
                what = (name, restart, seats, first, count)
                assert np.array_equal(got, want), (what, np.argwhere(got != want)[:5].tolist())
                assert set(np.unique(got)) <= {0, GE_ERR_ARG}
                assert b.read_rooms().tobytes() == twin.read_rooms().tobytes(), what
                applied += int(((got == 0) & (choices != 0)).sum())
                refused += int((got != 0).sum())
                assert (got[(choices < 0) | (choices > 15)] == GE_ERR_ARG).all()
    assert applied > 0 and refused > 0


def test_a_legal_choice_is_applied_and_an_illegal_one_changes_nothing():
    """`legal` of the observation is the verdict of the action: every legal choice of seat 1 is applied, every other refused, and
    a batch that got only refused choices is the batch it was."""
    segs, _ = case_all_seats("ww8_h1", True)
    legal = case_records("ww8_h1", True, [1])["legal"][:, 0]
    for c in range(1, 9):
        with make_batch(segs, True) as b:
            before = b.read_rooms().tobytes()
            choices = np.full((b.n_rooms, 1), c, dtype=np.int32)
            status = act(b, [1], choices, 0, b.n_rooms)[:, 0]
            assert np.array_equal(status == 0, ((legal >> (c - 1)) & 1) == 1)
            only_bad = np.where(status == 0, 0, c).astype(np.int32).reshape(-1, 1)
            b.write_rooms(0, np.frombuffer(before, dtype=b.read_rooms().dtype))
            assert (act(b, [1], only_bad, 0, b.n_rooms)[only_bad != 0] == GE_ERR_ARG).all()
            assert b.read_rooms().tobytes() == before


def test_status_may_be_null_and_the_refusals_keep_their_order(dsl_ww, dsl_tt):
    with RoomBatch([(GameTable(dsl_ww), 6, 300, 1), (GameTable(dsl_tt), 4, 200, 2)], seed=1, max_fuse=1) as b, \
            RoomBatch([(GameTable(dsl_ww), 6, 300, 1), (GameTable(dsl_tt), 4, 200, 2)], seed=1, max_fuse=1) as twin:
        b.step(9)
        twin.step(9)
        before = b.read_rooms().tobytes()
        call = b._lib.ge_batch_act_seats
        ch = DeviceBuffer.of(np.ones((500, 2), dtype=np.int32))
        st = DeviceBuffer(500 * 2 * 4, 0x4D)
        P, S = C.c_void_p(ch.data_ptr()), C.c_void_p(st.data_ptr())
        u32 = lambda *v: (C.c_uint32 * len(v))(*v)
        calls = [
            ((0, 501, 1, None, P, S), GE_ERR_ARG),                       # 2 seats NULL (range wrong as well)
            ((0, 501, 1, u32(1), None, S), GE_ERR_ARG),                  # 2 choices NULL
            ((0, 501, 13, u32(*range(1, 14)), P, S), GE_ERR_ARG),        # 3
            ((0, 501, 2, u32(2, 2), P, S), GE_ERR_ARG),                  # 4 before 5
            ((0, 501, 1, u32(0), P, S), GE_ERR_RANGE),                   # 5 before 6
            ((0, 10, 1, u32(0), P, S), GE_ERR_ARG),                      # 6
            ((290, 20, 1, u32(5), P, S), GE_ERR_ARG),                    # 6 above the four players of segment 1
        ]
        for (first, count, n_seats, seats, c, s), status in calls:
            assert call(b._h, first, count, n_seats, seats, c, s, None) == status, (first, count, n_seats)
        assert call(b._h, 17, 0, 2, u32(1, 2), None, None, None) == 0    # 9
        b.sync()
        assert b.read_rooms().tobytes() == before and set(st.host().tobytes()) == {0x4D}
        with pytest.raises(GeError):
            b.act_seats([1, 2], DeviceBuffer(10 * 2 * 4), None, 0, 500)  # (the binding: fewer entries than count * seats)
        b.act_seats([1, 2], ch, None, 0, 500)                            # status NULL
        b.sync()
        choices = np.ones((500, 2), dtype=np.int32)
        inject_composed(twin, [1, 2], choices, 0)
        assert b.read_rooms().tobytes() == twin.read_rooms().tobytes() != before

"""ge_batch_run_rooms_forecast (-m gpu; POLICY.md §3i): a run-on with the forecast of every turn it played, word for word against
tests/timeline_ref.py (the definition restated on the oracle) and against the GPU composition it replaces (run_rooms, then per
point a scratch batch holding that point's view and a rollout_seats call) - all 77 words of every point up to `played`, the slots
past it untouched, the run's own outputs and records equal to a run_rooms call on a twin batch - plus list lengths and playout
counts around a wavefront, the invariants of §3i, what must stay untouched, and every refusal in the ABI's order.

Sizes (timeline_ref.py): 6 entries per segment, max_turns 5 without a condition and 40 with PERSON | END, 70 playouts (one full
wavefront and one of 6 lanes) of at most 48 turns, seats alternating between the full view and a living bot seat: the smallest at
which the block -> (entry, turn, wavefront) map, the early return and the lanes past the playout count can go wrong."""
import functools

import numpy as np
import pytest

from game_engine_amd import EVENT_DTYPE, ROOM_VIEW_DTYPE, GameTable, RoomBatch
from parity_util import assert_views_equal, oracle_rooms_as_views
from run_ref import CASES, END, PERSON, SEED, case_inputs
from timeline_ref import FSEED, N_ROLLOUTS, PLAYOUT_MAX_TURNS, SHAPES, reference_timeline, timeline_inputs

pytestmark = pytest.mark.gpu

GE_ERR_ARG, GE_ERR_RANGE = -1, -6
PATTERN = np.uint64(0xA5A5A5A5A5A5A5A5)
_TABLES = {}


def _table(dsl):
    key = id(dsl)
    if key not in _TABLES:
        _TABLES[key] = (GameTable(dsl), dsl)                     # (the dsl is kept alive: its id is the key)
    return _TABLES[key][0]


def _batch(segs, restart, trace=False):
    b = RoomBatch([(_table(dsl), n, len(rooms), mask) for _, dsl, n, mask, rooms in segs], seed=SEED, first_room=777, max_fuse=1,
                  restart=restart, trace=trace)
    _put_starts(b, segs)
    return b


def _put_starts(b, segs):
    base = 0
    for orc, _, _, _, rooms in segs:
        b.write_rooms(base, oracle_rooms_as_views(orc, rooms))
        base += len(rooms)


def _call(b, listed, keys, turns, max_turns, until, fkeys, seats, n_rollouts=N_ROLLOUTS, pmax=PLAYOUT_MAX_TURNS, seed=FSEED):
    """The raw call with every output pre-filled: (status, played, stopped, events, views, stats)."""
    n = len(listed)
    rooms = np.ascontiguousarray(listed, dtype=np.uint64)
    keys, fkeys = np.ascontiguousarray(keys, dtype=np.uint64), np.ascontiguousarray(fkeys, dtype=np.uint64)
    turns = np.ascontiguousarray(turns, dtype=np.uint32)
    seats = None if seats is None else np.ascontiguousarray(seats, dtype=np.uint32)
    played, stopped = np.full(n, 77, dtype=np.uint32), np.full(n, 77, dtype=np.uint32)
    events = np.full((n, max_turns), 0xA5, dtype=np.uint8).repeat(EVENT_DTYPE.itemsize, axis=1).view(EVENT_DTYPE).reshape(n, max_turns)
    views = np.full((n, max_turns), 0x5A, dtype=np.uint8).repeat(ROOM_VIEW_DTYPE.itemsize, axis=1).view(ROOM_VIEW_DTYPE).reshape(n, max_turns)
    stats = np.full((n, max_turns + 1, 77), PATTERN, dtype=np.uint64)
    st = b._lib.ge_batch_run_rooms_forecast(b._h, n, rooms.ctypes.data, keys.ctypes.data, turns.ctypes.data, max_turns, until, fkeys.ctypes.data,
                                            None if seats is None else seats.ctypes.data, n_rollouts, pmax, seed, played.ctypes.data,
                                            stopped.ctypes.data, events.ctypes.data, views.ctypes.data, views.nbytes, stats.ctypes.data, stats.nbytes)
    return st, played, stopped, events, views, stats


@functools.lru_cache(maxsize=None)
def _case(name, restart):
    """The shared inputs of a case and, per shape, the reference's outputs: computed once."""
    inputs = timeline_inputs(name, restart)
    segs, listed, keys, turns, fkeys, seats = inputs
    refs = [reference_timeline(segs, listed, keys, turns, mt, until, restart, fkeys, seats, N_ROLLOUTS, PLAYOUT_MAX_TURNS, FSEED)
            for mt, until in SHAPES]
    return inputs, refs


def _check_stats(stats, played, want, what):
    for k in range(len(played)):
        p = int(played[k])
        assert want[k].shape[0] == p + 1
        bad = np.argwhere(stats[k, :p + 1] != want[k])
        assert not len(bad), (what, "entry", k, "first (point, word)", bad[0].tolist(), int(stats[k][tuple(bad[0])]), int(want[k][tuple(bad[0])]))
        assert (stats[k, p + 1:] == PATTERN).all(), f"{what}: entry {k} wrote a slot past played"


@pytest.mark.parametrize("restart", [False, True])
@pytest.mark.parametrize("name", sorted(CASES))
def test_timeline_matches_the_reference_and_a_twin_run(name, restart):
    """Every layout and table kind: the 77 words of every point against the oracle; played, stopped, events, views and every record
    against run_rooms on a twin batch; the turn counter and the trace buffer untouched; ordinary steps afterwards equal the twin's."""
    (segs, listed, keys, turns, fkeys, seats), refs = _case(name, restart)
    for (max_turns, until), (want_p, want_s, _, want_v, after, want) in zip(SHAPES, refs):
        what = f"{name} restart={restart} max_turns={max_turns}"
        with _batch(segs, restart, trace=True) as b, _batch(segs, restart, trace=True) as twin:
            for x in (b, twin):
                x.step(1)                                         # something in the trace buffer and on the turn counter
                _put_starts(x, segs)
            trace_before, turn_before = b.read_events().tobytes(), b.turn
            st, played, stopped, events, views, stats = _call(b, listed, keys, turns, max_turns, until, fkeys, seats)
            assert st == 0, what
            assert b.turn == turn_before and b.read_events().tobytes() == trace_before, f"{what}: turn counter or trace buffer touched"
            tp, ts, te, tv = twin.run_rooms(listed, keys, turns, max_turns=max_turns, until=until)
            got_rooms = b.read_rooms()
            assert got_rooms.tobytes() == twin.read_rooms().tobytes(), f"{what}: records differ from the twin run's"
            for _ in range(3):
                b.step(1)
                twin.step(1)
            assert b.read_rooms().tobytes() == twin.read_rooms().tobytes(), f"{what}: steps after the call differ from the twin's"
        assert np.array_equal(played, want_p) and np.array_equal(stopped, want_s), (what, played.tolist(), want_p.tolist())
        assert np.array_equal(played, tp) and np.array_equal(stopped, ts)
        for k in range(len(listed)):
            p = int(played[k])
            assert events[k, :p].tobytes() == te[k, :p].tobytes() and views[k, :p].tobytes() == tv[k, :p].tobytes(), (what, k)
            assert_views_equal(views[k, :p], np.array(want_v[k], dtype=ROOM_VIEW_DTYPE), f"{what}: views of entry {k}")
            assert set(events[k, p:].tobytes()) <= {0xA5} and set(views[k, p:].tobytes()) <= {0x5A}, f"{what}: entry {k} wrote past played"
        want_rooms = np.concatenate([oracle_rooms_as_views(orc, r) for (orc, _, _, _, _), r in zip(segs, after)])
        assert_views_equal(got_rooms, want_rooms, f"{what}: records after the call (listed and unlisted)")
        _check_stats(stats, played, want, what)


@pytest.mark.parametrize("restart", [False, True])
@pytest.mark.parametrize("name", sorted(CASES))
def test_timeline_is_the_gpu_composition(name, restart):
    """Every point equals rollout_seats of a scratch batch that holds the point's view: the start view for point 0, then
    views[k][p - 1].  A step(3) afterwards equals the step(3) of a twin batch after its run_rooms (these batches hold no trace, whose
    buffer takes one launch only)."""
    segs, listed, keys, turns, fkeys, seats = timeline_inputs(name, restart)
    for max_turns, until in SHAPES:
        with _batch(segs, restart) as b, _batch(segs, restart) as scratch, _batch(segs, restart) as twin:
            start = scratch.read_rooms_at(listed)
            st, played, _, _, views, stats = _call(b, listed, keys, turns, max_turns, until, fkeys, seats)
            assert st == 0
            twin.run_rooms(listed, keys, turns, max_turns=max_turns, until=until, views=False)
            b.step(3)
            twin.step(3)
            assert b.turn == twin.turn == 3 and b.read_rooms().tobytes() == twin.read_rooms().tobytes(), (name, restart, max_turns, "step(3)")
            for p in range(int(played.max()) + 1):
                live = np.nonzero(played >= p)[0]
                scratch.write_rooms_at(listed[live], start[live] if p == 0 else views[live, p - 1])
                words, status = scratch.rollout_seats(listed[live], fkeys[live], turns[live] + np.uint32(p), seats[live], None, N_ROLLOUTS,
                                                      PLAYOUT_MAX_TURNS, seed=FSEED)
                assert not status.any()
                assert np.array_equal(stats[live, p], words), (name, restart, max_turns, "point", p)


def _list_inputs(n, rng_seed):
    segs, _, _, _ = case_inputs("ww8_h1", 100, True, rng_seed=rng_seed)
    rng = np.random.default_rng(rng_seed)
    listed = rng.permutation(100)[:n]
    keys = rng.choice(1 << 44, size=n, replace=False).astype(np.uint64)
    turns = rng.integers(0, 1000, n).astype(np.uint32)
    fkeys = rng.choice(1 << 44, size=n, replace=False).astype(np.uint64)
    seats = (np.arange(n) % 3 * 3).astype(np.uint32)             # 0, 3, 6: seat 1 is the person
    return segs, listed, keys, turns, fkeys, seats


@pytest.mark.parametrize("n,n_rollouts", [(1, 70), (63, 70), (64, 70), (65, 70), (5, 1), (5, 64), (5, 65)])
def test_timeline_list_lengths_and_playout_counts(n, n_rollouts):
    """Lists that fill no wavefront of the run, exactly one, one and a lane; playouts of one lane, one wavefront, one and a lane."""
    segs, listed, keys, turns, fkeys, seats = _list_inputs(n, 64 + n + n_rollouts)
    want_p, want_s, _, _, _, want = reference_timeline(segs, listed, keys, turns, 3, PERSON | END, True, fkeys, seats, n_rollouts, 24, FSEED)
    with _batch(segs, True) as b:
        st, played, stopped, _, _, stats = _call(b, listed, keys, turns, 3, PERSON | END, fkeys, seats, n_rollouts, 24)
    assert st == 0 and np.array_equal(played, want_p) and np.array_equal(stopped, want_s)
    assert (stats[:, 0, 0] == n_rollouts).all()
    _check_stats(stats, played, want, f"n={n} R={n_rollouts}")


def test_invariants_continuity_and_one_turn():
    """Point played[k] of a call is point 0 of the next call on the room from turns[k] + played[k]; max_turns = 1 is a forecast, a
    step_rooms and a forecast; seats NULL is the full view."""
    segs, listed, keys, turns, fkeys, seats = timeline_inputs("mixed", True)
    with _batch(segs, True) as b:
        st, played, _, _, _, stats = _call(b, listed, keys, turns, 6, PERSON | END, fkeys, seats)
        st2, played2, _, _, _, stats2 = _call(b, listed, keys, turns + played, 4, 0, fkeys, seats)
        assert st == 0 and st2 == 0 and (played2 == 4).all()
        for k in range(len(listed)):
            assert np.array_equal(stats[k, int(played[k])], stats2[k, 0]), k
    with _batch(segs, True) as a, _batch(segs, True) as b:
        zero = np.zeros(len(listed), dtype=np.uint32)
        w0, _ = a.rollout_seats(listed, fkeys, turns, zero, None, N_ROLLOUTS, PLAYOUT_MAX_TURNS, seed=FSEED)
        ev = a.step_rooms(listed, keys, turns)
        vw = a.read_rooms_at(listed)
        w1, _ = a.rollout_seats(listed, fkeys, turns + np.uint32(1), zero, None, N_ROLLOUTS, PLAYOUT_MAX_TURNS, seed=FSEED)
        st, played, _, events, views, stats = _call(b, listed, keys, turns, 1, 7, fkeys, None)
        assert st == 0 and (played == 1).all()
        assert events[:, 0].tobytes() == ev.tobytes() and views[:, 0].tobytes() == vw.tobytes()
        assert np.array_equal(stats[:, 0], w0) and np.array_equal(stats[:, 1], w1)
        assert a.read_rooms().tobytes() == b.read_rooms().tobytes()
        p, s, e, v, w = b.run_rooms_forecast(listed, keys, turns + np.uint32(1), fkeys, 8, 16, seats=seats, seed=FSEED, max_turns=2, until=())
        assert (p == 2).all() and w.shape == (len(listed), 3, 77) and (w[:, :, 0] == 8).all()


def test_refusals_in_the_abi_order_change_nothing(dsl_ww, dsl_tt):
    with RoomBatch([(GameTable(dsl_ww), 8, 300, 1), (GameTable(dsl_tt), 4, 200)], seed=1, max_fuse=1) as b:
        b.step(7)
        before, turn = b.read_rooms().tobytes(), b.turn
        ok = dict(listed=[1, 2, 301], keys=[1, 2, 3], turns=[0, 5, 9], max_turns=4, until=3, fkeys=[7, 8, 9], seats=[0, 8, 4], n_rollouts=10,
                  pmax=10)
        last = 0xFFFFFFFF - 4 - 10                                # the last first turn the ok call can take
        bad = [  # ge_batch_run_rooms's checks, in its order, come first
               (dict(listed=[1, 2, 1]), GE_ERR_ARG), (dict(listed=[1, 500, 3]), GE_ERR_RANGE), (dict(max_turns=0), GE_ERR_ARG),
               (dict(until=8), GE_ERR_ARG), (dict(turns=[0, 0xFFFFFFFC, 0]), GE_ERR_RANGE),
               (dict(listed=[1, 500, 3], n_rollouts=0), GE_ERR_RANGE), (dict(turns=[0, 0xFFFFFFFC, 0], seats=[9, 0, 0]), GE_ERR_RANGE),
               # then this call's GE_ERR_ARG checks
               (dict(n_rollouts=0), GE_ERR_ARG), (dict(n_rollouts=(1 << 20) + 1), GE_ERR_ARG), (dict(pmax=4097), GE_ERR_ARG),
               (dict(max_turns=64, n_rollouts=1 << 20), GE_ERR_ARG),                      # n * (max_turns + 1) * n_rollouts > 2^26
               (dict(seats=[0, 9, 0]), GE_ERR_ARG), (dict(seats=[0, 0, 5]), GE_ERR_ARG),
               (dict(seats=[0, 9, 0], turns=[0, last + 1, 0]), GE_ERR_ARG),               # ... before the turn range
               (dict(n_rollouts=0, turns=[0, last + 1, 0]), GE_ERR_ARG),
               # then GE_ERR_RANGE for turns[k] + max_turns + playout_max_turns
               (dict(turns=[0, last + 1, 0]), GE_ERR_RANGE), (dict(turns=[last + 1, 0, 0], pmax=10), GE_ERR_RANGE)]
        for change, status in bad:
            st, played, stopped, events, views, stats = _call(b, **{**ok, **change})
            assert st == status, (change, st)
            assert (played == 77).all() and (stopped == 77).all() and (stats == PATTERN).all() and set(views.tobytes()) <= {0x5A}, change
            assert b.read_rooms().tobytes() == before and b.turn == turn, change
        st, played, _, _, _, stats = _call(b, **{**ok, "turns": [0, last, 0]})           # the last turns are taken
        assert st == 0 and (played >= 1).all() and b.turn == turn
        before = b.read_rooms().tobytes()
        # pointers and capacities, through the raw symbol
        n, cap = 3, 4
        r, k, f = (np.array(ok[x], dtype=np.uint64) for x in ("listed", "keys", "fkeys"))
        t = np.array(ok["turns"], dtype=np.uint32)
        played = np.full(n, 77, dtype=np.uint32)
        stats = np.full((n, cap + 1, 77), PATTERN, dtype=np.uint64)
        run = b._lib.ge_batch_run_rooms_forecast

        def raw(fk=f.ctypes.data, st_ptr=stats.ctypes.data, st_cap=stats.nbytes, pl=played.ctypes.data):
            return run(b._h, n, r.ctypes.data, k.ctypes.data, t.ctypes.data, cap, 3, fk, None, 10, 10, 0, pl, None, None, None, 0, st_ptr, st_cap)

        assert raw(pl=None) == GE_ERR_ARG and raw(fk=None) == GE_ERR_ARG and raw(st_ptr=None) == GE_ERR_ARG
        assert raw(st_cap=stats.nbytes - 1) == GE_ERR_ARG
        assert (played == 77).all() and (stats == PATTERN).all() and b.read_rooms().tobytes() == before
        # n * (max_turns + 1) > 2^16 with n * max_turns <= 2^20
        m = 17
        big = np.zeros((m, 4097, 77), dtype=np.uint64)
        ids = np.arange(m, dtype=np.uint64)
        tz = np.zeros(m, dtype=np.uint32)
        pm = np.full(m, 77, dtype=np.uint32)
        assert run(b._h, m, ids.ctypes.data, ids.ctypes.data, tz.ctypes.data, 4096, 0, ids.ctypes.data, None, 1, 0, 0, pm.ctypes.data, None, None,
                   None, 0, big.ctypes.data, big.nbytes) == GE_ERR_ARG
        assert (pm == 77).all() and not big.any() and b.read_rooms().tobytes() == before and b.turn == turn
        # n == 0 comes last: its own checks still hold
        assert run(b._h, 0, None, None, None, 0, 99, f.ctypes.data, None, 10, 10, 0, None, None, None, None, 0, stats.ctypes.data, 0) == 0
        assert run(b._h, 0, None, None, None, 0, 99, f.ctypes.data, None, 0, 10, 0, None, None, None, None, 0, stats.ctypes.data, 0) == GE_ERR_ARG
        p, s, e, v, w = b.run_rooms_forecast([], [], [], [], 4, max_turns=5)
        assert len(p) == 0 and w.shape == (0, 6, 77)

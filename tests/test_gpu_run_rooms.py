"""ge_batch_run_rooms (-m gpu): listed rooms played on until a person is needed, bit for bit against tests/run_ref.py (the
definition restated on the oracle) and against the GPU composition it replaces (step_rooms + read_rooms_at in a host loop) -
turn counts, stop bits, every event and view below `played`, the records of listed and unlisted rooms - plus what must stay
untouched, the invariants of POLICY.md §3f, the PERSON stop against inject_action, refusals, and ordinary steps around it."""
import numpy as np
import pytest

from game_engine_amd import EVENT_DTYPE, ROOM_VIEW_DTYPE, GameTable, GeError, RoomBatch
from oracle.oracle import Oracle
from parity_util import assert_views_equal, oracle_rooms_as_views
from run_ref import CASES, END, PERSON, PHASE, SEED, case_inputs, dsl_of, person_pending, reference_call, run_ref

pytestmark = pytest.mark.gpu

GE_ERR_ARG, GE_ERR_RANGE = -1, -6
EV_FIELDS = ("turn", "from_phase_id", "to_phase_id", "acted_now", "restarted", "choice")
_TABLES = {}


def _table(dsl):
    key = id(dsl)
    if key not in _TABLES:
        _TABLES[key] = (GameTable(dsl), dsl)                     # (the dsl is kept alive: its id is the key)
    return _TABLES[key][0]


def _batch(segs, restart, first_room=777, trace=False):
    b = RoomBatch([(_table(dsl), n, len(rooms), mask) for _, dsl, n, mask, rooms in segs], seed=SEED, first_room=first_room,
                  max_fuse=1, restart=restart, trace=trace)
    base = 0
    for orc, _, _, _, rooms in segs:
        b.write_rooms(base, oracle_rooms_as_views(orc, rooms))
        base += len(rooms)
    return b


def _composition(b, listed, keys, turns, max_turns, until, human_pending):
    """The host loop run_rooms replaces, on batch b: per turn one step_rooms and one read_rooms_at of the rooms still running.
    The stop tests read the event and the view; PERSON comes from `human_pending(k, view)` (the reference's verdicts)."""
    n = len(listed)
    played, stopped = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    events = np.zeros((n, max_turns), dtype=EVENT_DTYPE)
    views = np.zeros((n, max_turns), dtype=ROOM_VIEW_DTYPE)
    live = np.arange(n)
    for t in range(max_turns):
        ev = b.step_rooms(listed[live], keys[live], turns[live] + np.uint32(t))
        vw = b.read_rooms_at(listed[live])
        events[live, t], views[live, t] = ev, vw
        played[live] = t + 1
        why = np.array([human_pending(int(k), t) for k in live], dtype=np.uint32) & np.uint32(until)
        stopped[live] = why
        live = live[why == 0]
        if not len(live):
            break
    return played, stopped, events, views


def _check_call(name, segs, listed, keys, turns, max_turns, until, restart, what):
    """One run_rooms call on a fresh batch against the reference; returns (batch outputs, reference outputs)."""
    per = len(segs[0][4])
    want_p, want_s, want_e, want_v, after = reference_call(segs, listed, keys, turns, max_turns, until, restart)
    with _batch(segs, restart, trace=True) as b:
        b.step(1)                                                # something in the trace buffer and on the turn counter
        base = 0
        for orc, _, _, _, rooms in segs:                         # (the step moved every room: put the starts back)
            b.write_rooms(base, oracle_rooms_as_views(orc, rooms))
            base += len(rooms)
        trace_before, turn_before = b.read_events().tobytes(), b.turn
        played, stopped, events, views = b.run_rooms(listed, keys, turns, max_turns=max_turns, until=until)
        assert b.turn == turn_before and b.read_events().tobytes() == trace_before, f"{what}: turn counter or trace buffer touched"
        got_rooms = b.read_rooms()
    assert np.array_equal(played, want_p), (what, "played", played.tolist(), want_p.tolist())
    assert np.array_equal(stopped, want_s), (what, "stopped", stopped.tolist(), want_s.tolist())
    for k in range(len(listed)):
        p = int(played[k])
        for t in range(p):
            for f in EV_FIELDS:
                assert np.array_equal(events[k, t][f], want_e[k][t][f]), (what, "event", k, t, f, events[k, t][f], want_e[k][t][f])
        assert_views_equal(views[k, :p], np.array(want_v[k], dtype=ROOM_VIEW_DTYPE), f"{what}: views of entry {k}")
        assert not events[k, p:].tobytes().strip(b"\0") and not views[k, p:].tobytes().strip(b"\0"), f"{what}: slots past played written"
    want_rooms = np.concatenate([oracle_rooms_as_views(orc, r) for (orc, _, _, _, _), r in zip(segs, after)])
    assert_views_equal(got_rooms, want_rooms, f"{what}: records after the call (listed and unlisted)")
    assert per * len(segs) == len(got_rooms)
    return (played, stopped, events, views), (want_p, want_s, want_e, want_v)


@pytest.mark.parametrize("restart", [False, True])
@pytest.mark.parametrize("name", sorted(CASES))
def test_run_rooms_matches_the_reference(name, restart):
    """Every layout and table kind, human masks of 0 / 1 / 2 seats, each `until` combination, distinct keys and turns per entry
    (entry 0 on the last turns a room can take)."""
    segs, listed, keys, turns = case_inputs(name, 24 if name == "mixed" else 48, restart)
    for until in range(8):
        max_turns = (5, 64, 17, 40)[until % 4]
        _check_call(name, segs, listed, keys, turns, max_turns, until, restart, f"{name} restart={restart} until={until}")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_run_rooms_list_lengths(n):
    """Lists that fill no wavefront, exactly one, one and a lane, and many blocks (the copy-back in two parts)."""
    segs, _, _, _ = case_inputs("ww8_h1", 1500 if n == 1000 else 100, True, rng_seed=n)
    rng = np.random.default_rng(n)
    listed = rng.permutation(len(segs[0][4]))[:n]
    keys = rng.choice(1 << 44, size=n, replace=False).astype(np.uint64)
    turns = rng.integers(0, 1000, n).astype(np.uint32)
    (played, stopped, _, _), _ = _check_call("ww8_h1", segs, listed, keys, turns, 12, PERSON | END, True, f"n={n}")
    if n >= 63:
        assert (stopped & PERSON).any() and (played == 12).any()


@pytest.mark.parametrize("name", ["mixed", "ww12_h2", "tt8_generic_h1"])
def test_run_rooms_is_the_gpu_composition_and_slots_past_played_stay(name):
    """Against step_rooms + read_rooms_at in a host loop on a twin batch; output slots at t >= played keep a pattern."""
    restart, max_turns, until = True, 20, PERSON | PHASE
    segs, listed, keys, turns = case_inputs(name, 40, restart)
    after = [rooms.copy() for _, _, _, _, rooms in segs]
    per = len(after[0])

    def human_pending(k, t):
        # PERSON from the definition, on the oracle stepped beside the twin batch; PHASE from the oracle's event
        s, i = divmod(int(listed[k]), per)
        orc, _, _, mask, _ = segs[s]
        one = after[s][i:i + 1]
        orc.run(one, SEED, int(keys[k]), int(turns[k]) + t, 1, threads=1, restart=restart, human_mask=mask)
        why = PERSON if person_pending(orc, one, mask) else 0
        return why | (PHASE if one["ev_from"][0] != one["ev_to"][0] else 0)

    with _batch(segs, restart) as twin:
        cp, cs, ce, cv = _composition(twin, listed, keys, turns, max_turns, until, human_pending)
        twin_rooms = twin.read_rooms()
    n = len(listed)
    played, stopped = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    events = np.full((n, max_turns), 0xA5, dtype=np.uint8).repeat(EVENT_DTYPE.itemsize, axis=1).view(EVENT_DTYPE).reshape(n, max_turns)
    views = np.full((n, max_turns), 0x5A, dtype=np.uint8).repeat(ROOM_VIEW_DTYPE.itemsize, axis=1).view(ROOM_VIEW_DTYPE).reshape(n, max_turns)
    with _batch(segs, restart) as b:
        st = b._lib.ge_batch_run_rooms(b._h, n, listed.astype(np.uint64).ctypes.data, keys.ctypes.data, turns.ctypes.data, max_turns, until,
                                       played.ctypes.data, stopped.ctypes.data, events.ctypes.data, views.ctypes.data, views.nbytes)
        assert st == 0
        assert b.read_rooms().tobytes() == twin_rooms.tobytes()
    assert np.array_equal(played, cp) and np.array_equal(stopped, cs)
    assert int(played.min()) < max_turns
    for k in range(n):
        p = int(played[k])
        assert events[k, :p].tobytes() == ce[k, :p].tobytes() and views[k, :p].tobytes() == cv[k, :p].tobytes(), (name, k)
        assert set(events[k, p:].tobytes()) <= {0xA5} and set(views[k, p:].tobytes()) <= {0x5A}, f"{name}: entry {k} wrote past played"


def test_invariants_one_turn_and_no_condition():
    """max_turns = 1 with any `until` is step_rooms word for word; until = 0 is max_turns calls of step_rooms."""
    segs, listed, keys, turns = case_inputs("mixed", 30, True)
    for until in (0, PERSON, END | PHASE, 7):
        with _batch(segs, True) as a, _batch(segs, True) as b:
            ev = a.step_rooms(listed, keys, turns)
            vw = a.read_rooms_at(listed)
            played, stopped, events, views = b.run_rooms(listed, keys, turns, max_turns=1, until=until)
            assert (played == 1).all() and not (stopped & ~np.uint32(until)).any()
            assert events[:, 0].tobytes() == ev.tobytes() and views[:, 0].tobytes() == vw.tobytes()
            assert a.read_rooms().tobytes() == b.read_rooms().tobytes()
    with _batch(segs, True) as a, _batch(segs, True) as b:
        played, stopped, events, views = b.run_rooms(listed, keys, turns, max_turns=9, until=())
        assert (played == 9).all() and not stopped.any()
        for t in range(9):
            ev = a.step_rooms(listed, keys, turns + np.uint32(t))
            assert events[:, t].tobytes() == ev.tobytes() and views[:, t].tobytes() == a.read_rooms_at(listed).tobytes()
        assert a.read_rooms().tobytes() == b.read_rooms().tobytes()


@pytest.mark.parametrize("game,n", [("ww", 8), ("ww", 12), ("tt", 4)])
def test_invariant_all_bot_run_to_the_end_is_a_lone_batch(game, n):
    """All bots, until = END: entry k leaves what a lone batch with first_room = keys[k] has after played[k] turns of step()."""
    dsl = dsl_of(game)
    tb = GameTable(dsl)
    keys = np.array([5, (1 << 33) + 11, 123456789], dtype=np.uint64)
    with RoomBatch([(tb, n, 10)], seed=SEED, first_room=0, max_fuse=1) as b:
        played, stopped, _, _ = b.run_rooms([7, 2, 4], keys, [0, 0, 0], max_turns=400, until=("end",))
        got = b.read_rooms_at([7, 2, 4])
    assert (stopped == END).all() and (played > 5).all() and (played < 400).all()
    for k in range(3):
        with RoomBatch([(tb, n, 1)], seed=SEED, first_room=int(keys[k]), max_fuse=1) as lone:
            lone.step(int(played[k]))
            assert lone.read_rooms().tobytes() == got[k:k + 1].tobytes()
            assert lone.read_rooms()["end_turn"][0] == int(played[k]) - 1


@pytest.mark.parametrize("name", ["ww8_h2", "tt4_h1", "ww12_generic_h2", "draft8_h1"])
def test_person_stop_is_what_inject_action_accepts(name):
    """After a PERSON stop an inject_action of some human seat is accepted; after any other stop in a player_action phase none is."""
    segs, listed, keys, turns = case_inputs(name, 64, False)
    orc, dsl, n, mask, _ = segs[0]
    action_ids = {p.id for p in orc.table.phases if p.completion == 2}
    with _batch(segs, False) as b:
        played, stopped, _, views = b.run_rooms(listed, keys, turns, max_turns=30, until=("person", "phase"))
        seen = {True: 0, False: 0}
        for k, r in enumerate(listed):
            last = views[k, int(played[k]) - 1]
            person = bool(stopped[k] & PERSON)
            if not person and int(last["phase_id"]) not in action_ids:
                continue
            ok = False
            for seat in range(n):
                for c in range(1, max(n, 3) + 1):
                    if (mask >> seat) & 1 and not ok:
                        try:
                            b.inject_action(int(r), seat + 1, c)
                            ok = True
                        except GeError:
                            pass
            assert ok == person, (name, k, int(r), person)
            seen[person] += 1
    assert seen[True] > 0 and seen[False] > 0, seen


def test_refusals_change_nothing(dsl_ww, dsl_tt):
    with RoomBatch([(GameTable(dsl_ww), 8, 300, 1), (GameTable(dsl_tt), 4, 200)], seed=1, max_fuse=1) as b:
        b.step(7)
        before = b.read_rooms().tobytes()
        turn = b.turn
        ok = dict(rooms=[1, 2, 301], keys=[1, 2, 3], turns=[0, 5, 9], max_turns=4, until=3)
        bad = [(dict(rooms=[1, 2, 1]), GE_ERR_ARG), (dict(rooms=[1, 500, 3]), GE_ERR_RANGE), (dict(turns=[0, 0xFFFFFFFF, 0]), GE_ERR_RANGE),
               (dict(max_turns=0), GE_ERR_ARG), (dict(max_turns=4097), GE_ERR_ARG), (dict(until=8), GE_ERR_ARG), (dict(until=15), GE_ERR_ARG),
               (dict(turns=[0, 0xFFFFFFFC, 0]), GE_ERR_RANGE), (dict(rooms=[1, 500, 3], max_turns=0), GE_ERR_RANGE),
               (dict(turns=[0, 0xFFFFFFFC, 0], until=8), GE_ERR_ARG)]
        for change, status in bad:
            with pytest.raises(GeError) as e:
                b.run_rooms(**{**ok, **change})
            assert e.value.status == status, (change, e.value.status)
            assert b.read_rooms().tobytes() == before and b.turn == turn
        n, cap = 3, 4
        r, k, t = (np.array(ok[x], dtype=d) for x, d in (("rooms", np.uint64), ("keys", np.uint64), ("turns", np.uint32)))
        played = np.full(n, 77, dtype=np.uint32)
        views = np.full(n * cap, 0x5A, dtype=np.uint8).repeat(ROOM_VIEW_DTYPE.itemsize)
        run = b._lib.ge_batch_run_rooms
        assert run(b._h, n, r.ctypes.data, k.ctypes.data, t.ctypes.data, cap, 3, None, None, None, None, 0) == GE_ERR_ARG       # played NULL
        assert run(b._h, n, r.ctypes.data, k.ctypes.data, t.ctypes.data, cap, 3, played.ctypes.data, None, None, views.ctypes.data,
                   views.nbytes - 1) == GE_ERR_ARG                                                                              # views cap too small
        assert set(views.tobytes()) == {0x5A} and (played == 77).all()
        assert run(b._h, 300, np.arange(300, dtype=np.uint64).ctypes.data, np.arange(300, dtype=np.uint64).ctypes.data,
                   np.zeros(300, dtype=np.uint32).ctypes.data, 4000, 0, played.ctypes.data, None, None, None, 0) == GE_ERR_ARG  # n * max_turns > 2^20
        assert run(b._h, 0, None, None, None, 0, 99, None, None, None, None, 0) == 0                                           # n == 0
        p, s, e, v = b.run_rooms([], [], [], max_turns=5)
        assert len(p) == 0 and e.shape == (0, 5)


def test_ordinary_steps_around_run_rooms_stay_exact(dsl_ww):
    """step(64) -> run_rooms under other keys -> step(64): both segments equal the oracle (the prepared-deal rule)."""
    seed, first, sizes = 4040, 1 << 36, (300, 200)
    parts = [(Oracle(dsl_ww, 8), sizes[0]), (Oracle(dsl_ww, 12), sizes[1])]
    rooms = [orc.init_rooms(R) for orc, R in parts]
    rng = np.random.default_rng(5)
    with RoomBatch([(GameTable(dsl_ww), 8, sizes[0]), (GameTable(dsl_ww), 12, sizes[1])], seed=seed, first_room=first,
                   max_fuse=1, restart=True) as b:
        b.step(64)
        for (orc, _), r, base in zip(parts, rooms, (0, sizes[0])):
            orc.run(r, seed, first + base, 0, 64, threads=0, restart=True)
        chosen = rng.choice(sum(sizes), size=250, replace=False)
        keys = rng.choice(1 << 40, size=250, replace=False).astype(np.uint64)
        turns = rng.integers(0, 100, 250).astype(np.uint32)
        played, _, _, _ = b.run_rooms(chosen, keys, turns, max_turns=40, until=("phase",), views=False)
        for k, c in enumerate(chosen):
            s = 0 if c < sizes[0] else 1
            i = int(c) - (0 if s == 0 else sizes[0])
            p, _, _, _ = run_ref(parts[s][0], rooms[s], i, seed, int(keys[k]), int(turns[k]), 40, PHASE, True, 0)
            assert p == played[k]
        b.step(64)
        for (orc, _), r, base in zip(parts, rooms, (0, sizes[0])):
            orc.run(r, seed, first + base, 64, 64, threads=0, restart=True)
            assert_views_equal(b.read_rooms(base, len(r)), oracle_rooms_as_views(orc, r), f"x{orc.n} after step / run_rooms / step")

"""ge_batch_run_rooms_playout (-m gpu): listed rooms with playout seats played on until a person is needed (POLICY.md §3g), bit for
bit against tests/run_playout_ref.py (the definition restated on the oracle) and against the GPU composition it replaces
(step_rooms_playout + read_rooms_at in a host loop) - turn counts, stop bits, every event, view and decided mask below `played`,
the records of listed and unlisted rooms - plus the three invariants of §3g, what must stay untouched, and the refusals."""
import numpy as np
import pytest

from game_engine_amd import EVENT_DTYPE, ROOM_VIEW_DTYPE, GameTable, GeError, RoomBatch
from parity_util import assert_views_equal, oracle_rooms_as_views
from run_playout_ref import M_SMALL, PSEED, R_SMALL, REF_CALLS, REF_CASES, playout_inputs, shared_reference
from run_ref import END, PERSON, PHASE, SEED, case_inputs
from test_gpu_run_rooms import EV_FIELDS, _batch

pytestmark = pytest.mark.gpu

GE_ERR_ARG, GE_ERR_RANGE = -1, -6


@pytest.mark.parametrize("restart", [False, True])
@pytest.mark.parametrize("name", REF_CASES)
def test_run_rooms_playout_matches_the_reference(name, restart):
    """24 listed rooms, masks of 1 - 3 bot seats (some 0), distinct keys and turns (entry 0 on the last turns a room can take)."""
    for until, max_turns in REF_CALLS:
        what = f"{name} restart={restart} until={until}"
        (segs, listed, keys, turns, masks, pkeys), (want_p, want_s, want_e, want_v, want_d, after) = shared_reference(name, restart, until, max_turns)
        with _batch(segs, restart, trace=True) as b:
            b.step(1)                                            # something in the trace buffer and on the turn counter
            base = 0
            for orc, _, _, _, rooms in segs:                     # (the step moved every room: put the starts back)
                b.write_rooms(base, oracle_rooms_as_views(orc, rooms))
                base += len(rooms)
            trace_before, turn_before = b.read_events().tobytes(), b.turn
            played, stopped, events, views, decided = b.run_rooms_playout(listed, keys, turns, masks, pkeys, R_SMALL, M_SMALL, seed=PSEED,
                                                                          max_turns=max_turns, until=until)
            assert b.turn == turn_before and b.read_events().tobytes() == trace_before, f"{what}: turn counter or trace buffer touched"
            got_rooms = b.read_rooms()
        assert np.array_equal(played, want_p), (what, "played", played.tolist(), want_p.tolist())
        assert np.array_equal(stopped, want_s), (what, "stopped", stopped.tolist(), want_s.tolist())
        for k in range(len(listed)):
            p = int(played[k])
            assert decided[k, :p].tolist() == want_d[k], (what, "decided", k, decided[k, :p].tolist(), want_d[k])
            for t in range(p):
                for f in EV_FIELDS:
                    assert np.array_equal(events[k, t][f], want_e[k][t][f]), (what, "event", k, t, f, events[k, t][f], want_e[k][t][f])
            assert_views_equal(views[k, :p], np.array(want_v[k], dtype=ROOM_VIEW_DTYPE), f"{what}: views of entry {k}")
            assert not events[k, p:].tobytes().strip(b"\0") and not views[k, p:].tobytes().strip(b"\0") and not decided[k, p:].any(), \
                f"{what}: slots past played written"
        want_rooms = np.concatenate([oracle_rooms_as_views(orc, r) for (orc, _, _, _, _), r in zip(segs, after)])
        assert_views_equal(got_rooms, want_rooms, f"{what}: records after the call (listed and unlisted)")


def _composition(b, terminal_ids, listed, keys, turns, masks, pkeys, R, M, max_turns, until, full_view=False):
    """The host loop run_rooms_playout replaces, on batch b: per turn one step_rooms_playout and one read_rooms_at of the rooms
    still running.  END and PHASE are read from the view and the event (no PERSON here: it needs the oracle)."""
    n = len(listed)
    played, stopped = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    events = np.zeros((n, max_turns), dtype=EVENT_DTYPE)
    views = np.zeros((n, max_turns), dtype=ROOM_VIEW_DTYPE)
    decided = np.zeros((n, max_turns), dtype=np.uint32)
    live = np.arange(n)
    for t in range(max_turns):
        ev, dec = b.step_rooms_playout(listed[live], keys[live], turns[live] + np.uint32(t), masks[live], pkeys[live], R, M, seed=PSEED,
                                       full_view=full_view)
        vw = b.read_rooms_at(listed[live])
        events[live, t], views[live, t], decided[live, t] = ev, vw, dec
        played[live] = t + 1
        why = np.where(np.isin(vw["phase_id"], terminal_ids), END, 0) | np.where(ev["to_phase_id"] != ev["from_phase_id"], PHASE, 0)
        why = why.astype(np.uint32) & np.uint32(until)
        stopped[live] = why
        live = live[why == 0]
        if not len(live):
            break
    return played, stopped, events, views, decided


def _all_bot_ww8(per, n, rng_seed):
    """Werewolf x 8 without a human seat, every seat a playout seat: n listed rooms of `per`, their keys, turns and playout keys."""
    segs, _, _, _ = case_inputs("ww8", per, True, rng_seed=rng_seed)
    rng = np.random.default_rng(rng_seed)
    listed = rng.permutation(per)[:n].astype(np.uint64)
    keys = rng.choice(1 << 44, size=n, replace=False).astype(np.uint64)
    turns = rng.integers(0, 1000, n).astype(np.uint32)
    pkeys = rng.integers(0, 1 << 63, n).astype(np.uint64)
    orc = segs[0][0]
    terminal_ids = [p.id for p in orc.table.phases if not p.branches]
    return segs, listed, keys, turns, np.full(n, 0xFF, dtype=np.uint32), pkeys, terminal_ids


def _against_composition(segs, terminal_ids, listed, keys, turns, masks, pkeys, R, M, max_turns, until, restart, what, full_view=False):
    with _batch(segs, restart) as twin:
        cp, cs, ce, cv, cd = _composition(twin, terminal_ids, listed, keys, turns, masks, pkeys, R, M, max_turns, until, full_view)
        twin_rooms = twin.read_rooms()
    n = len(listed)
    played, stopped = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    events = np.full((n, max_turns), 0xA5, dtype=np.uint8).repeat(EVENT_DTYPE.itemsize, axis=1).view(EVENT_DTYPE).reshape(n, max_turns)
    views = np.full((n, max_turns), 0x5A, dtype=np.uint8).repeat(ROOM_VIEW_DTYPE.itemsize, axis=1).view(ROOM_VIEW_DTYPE).reshape(n, max_turns)
    decided = np.full((n, max_turns), 0xC3C3C3C3, dtype=np.uint32)
    with _batch(segs, restart) as b:
        st = b._lib.ge_batch_run_rooms_playout(b._h, n, listed.ctypes.data, keys.ctypes.data, turns.ctypes.data, masks.ctypes.data, pkeys.ctypes.data,
                                               R, M, PSEED, 1 if full_view else 0, max_turns, until, played.ctypes.data, stopped.ctypes.data,
                                               decided.ctypes.data, events.ctypes.data, views.ctypes.data, views.nbytes)
        assert st == 0, (what, st)
        assert b.read_rooms().tobytes() == twin_rooms.tobytes(), what
    assert np.array_equal(played, cp) and np.array_equal(stopped, cs), (what, played.tolist(), cp.tolist(), stopped.tolist(), cs.tolist())
    for k in range(n):
        p = int(played[k])
        assert events[k, :p].tobytes() == ce[k, :p].tobytes() and views[k, :p].tobytes() == cv[k, :p].tobytes(), (what, k)
        assert decided[k, :p].tolist() == cd[k, :p].tolist(), (what, k)
        assert set(events[k, p:].tobytes()) <= {0xA5} and set(views[k, p:].tobytes()) <= {0x5A} and (decided[k, p:] == 0xC3C3C3C3).all(), \
            f"{what}: entry {k} wrote past played"
    return played, stopped, decided


@pytest.mark.parametrize("n,until", [(1, END | PHASE), (63, PHASE), (64, END), (65, 0)])
def test_run_rooms_playout_is_the_gpu_composition(n, until):
    """All-bot Werewolf x 8, every seat a playout seat; lists that fill no wavefront, exactly one, and one and a lane; more turns
    than one group of enqueued turns.  Output slots at t >= played keep a pattern."""
    segs, listed, keys, turns, masks, pkeys, terminal_ids = _all_bot_ww8(100, n, n)
    played, _, decided = _against_composition(segs, terminal_ids, listed, keys, turns, masks, pkeys, R_SMALL, M_SMALL, 12, until, True, f"n={n}")
    if n > 1:
        assert decided[:, 1:][np.arange(12)[None, 1:] < played[:, None]].any(), "no decision behind the first turn"
    if until == PHASE:
        assert int(played.min()) < int(played.max()), "no room ran on past another's stop"


def test_run_rooms_playout_across_the_pass_boundary():
    """1 025 rooms x 8 playout seats x 8 candidates: a capacity of 65 600 entries, two passes per turn."""
    segs, listed, keys, turns, masks, pkeys, terminal_ids = _all_bot_ww8(1100, 1025, 5)
    played, _, decided = _against_composition(segs, terminal_ids, listed, keys, turns, masks, pkeys, 4, 8, 6, PHASE, True, "n=1025")
    assert decided[-1, :int(played[-1])].any() or decided[-64:].any(), "the second pass decided nothing"


def test_run_rooms_playout_two_wavefronts_per_entry():
    """n_rollouts = 65: two wavefronts per entry, the second holding one replica."""
    segs, listed, keys, turns, masks, pkeys, terminal_ids = _all_bot_ww8(40, 20, 9)
    _against_composition(segs, terminal_ids, listed, keys, turns, masks, pkeys, 65, M_SMALL, 6, END, True, "R=65")


def test_invariant_no_playout_seat_is_run_rooms():
    """All masks 0: ge_batch_run_rooms word for word, decided all zero."""
    segs, listed, keys, turns, masks, pkeys = playout_inputs("mixed", 9, True)
    for until, max_turns in ((PERSON | END, 20), (PHASE, 9)):
        with _batch(segs, True) as a, _batch(segs, True) as b:
            p0, s0, e0, v0 = a.run_rooms(listed, keys, turns, max_turns=max_turns, until=until)
            p1, s1, e1, v1, d1 = b.run_rooms_playout(listed, keys, turns, np.zeros_like(masks), pkeys, R_SMALL, M_SMALL, seed=PSEED,
                                                     max_turns=max_turns, until=until)
            assert p0.tobytes() == p1.tobytes() and s0.tobytes() == s1.tobytes() and e0.tobytes() == e1.tobytes() and v0.tobytes() == v1.tobytes()
            assert not d1.any() and a.read_rooms().tobytes() == b.read_rooms().tobytes()


def test_invariant_no_playout_turn_is_run_rooms():
    """playout_max_turns = 0: every candidate has 0 wins, every tie goes to the policy's own pick - ge_batch_run_rooms word for word,
    although decisions were made."""
    segs, listed, keys, turns, masks, pkeys = playout_inputs("ww8_h1", 36, False)
    with _batch(segs, False) as a, _batch(segs, False) as b:
        p0, s0, e0, v0 = a.run_rooms(listed, keys, turns, max_turns=24, until=PERSON | END)
        p1, s1, e1, v1, d1 = b.run_rooms_playout(listed, keys, turns, masks, pkeys, R_SMALL, 0, seed=PSEED, max_turns=24, until=PERSON | END)
        assert p0.tobytes() == p1.tobytes() and s0.tobytes() == s1.tobytes() and e0.tobytes() == e1.tobytes() and v0.tobytes() == v1.tobytes()
        assert d1.any() and a.read_rooms().tobytes() == b.read_rooms().tobytes()


def test_invariant_one_turn_is_step_rooms_playout_and_a_read():
    """max_turns = 1: ge_batch_step_rooms_playout followed by ge_batch_read_rooms_at, word for word."""
    segs, listed, keys, turns, masks, pkeys = playout_inputs("mixed", 9, True)
    for until in (0, PERSON, END | PHASE):
        with _batch(segs, True) as a, _batch(segs, True) as b:
            ev, dec = a.step_rooms_playout(listed, keys, turns, masks, pkeys, R_SMALL, M_SMALL, seed=PSEED)
            vw = a.read_rooms_at(listed)
            played, stopped, events, views, decided = b.run_rooms_playout(listed, keys, turns, masks, pkeys, R_SMALL, M_SMALL, seed=PSEED,
                                                                          max_turns=1, until=until)
            assert (played == 1).all() and not (stopped & ~np.uint32(until)).any()
            assert events[:, 0].tobytes() == ev.tobytes() and views[:, 0].tobytes() == vw.tobytes() and decided[:, 0].tobytes() == dec.tobytes()
            assert a.read_rooms().tobytes() == b.read_rooms().tobytes()


def test_full_view_and_ordinary_steps_around_the_call():
    """GE_PLAYOUT_FULL_VIEW once; an ordinary step before and after the call leaves the summary checksum of a twin batch driven by
    the composition."""
    segs, listed, keys, turns, masks, pkeys, terminal_ids = _all_bot_ww8(60, 40, 3)
    _against_composition(segs, terminal_ids, listed, keys, turns, masks, pkeys, R_SMALL, M_SMALL, 9, PHASE, True, "full view", full_view=True)
    with _batch(segs, True) as twin, _batch(segs, True) as b:
        twin.step(3)
        b.step(3)
        _composition(twin, terminal_ids, listed, keys, turns, masks, pkeys, R_SMALL, M_SMALL, 9, END | PHASE)
        b.run_rooms_playout(listed, keys, turns, masks, pkeys, R_SMALL, M_SMALL, seed=PSEED, max_turns=9, until=END | PHASE, views=False)
        twin.step(5)
        b.step(5)
        assert b.turn == twin.turn == 8
        assert b.summary()["checksum"] == twin.summary()["checksum"]


def test_refusals_change_nothing(dsl_ww, dsl_tt):
    with RoomBatch([(GameTable(dsl_ww), 8, 300, 1), (GameTable(dsl_tt), 4, 200)], seed=1, max_fuse=1) as b:
        b.step(7)
        before = b.read_rooms().tobytes()
        turn = b.turn
        ok = dict(rooms=[1, 2, 301], keys=[1, 2, 3], turns=[0, 5, 9], masks=[2, 6, 1], playout_keys=[7, 8, 9], n_rollouts=8, playout_max_turns=16,
                  max_turns=4, until=3)
        bad = [(dict(rooms=[1, 2, 1]), GE_ERR_ARG), (dict(rooms=[1, 500, 3]), GE_ERR_RANGE), (dict(turns=[0, 0xFFFFFFFF, 0]), GE_ERR_RANGE),
               (dict(max_turns=0), GE_ERR_ARG), (dict(max_turns=4097), GE_ERR_ARG), (dict(until=8), GE_ERR_ARG),
               (dict(turns=[0, 0xFFFFFFFC, 0]), GE_ERR_RANGE),                       # run_rooms's: first + max_turns
               (dict(rooms=[1, 500, 3], n_rollouts=0), GE_ERR_RANGE),                # run_rooms's checks come first
               (dict(n_rollouts=0), GE_ERR_ARG), (dict(n_rollouts=(1 << 20) + 1), GE_ERR_ARG), (dict(playout_max_turns=4097), GE_ERR_ARG),
               (dict(masks=[2, 1 << 8, 1]), GE_ERR_ARG),                             # a bit at the room's player count
               (dict(masks=[2, 6, 1 << 4]), GE_ERR_ARG),                             # ... of a Two-Truths x 4 room
               (dict(masks=[3, 6, 1]), GE_ERR_ARG),                                  # a host-driven seat
               (dict(masks=[0xFE, 0xFE, 0xF], n_rollouts=1 << 20), GE_ERR_ARG),      # the cost cap, per turn
               (dict(turns=[0, 0xFFFFFFFF - 4 - 14, 0]), GE_ERR_RANGE)]              # the last turn's playouts: first + 3 + 16 > 2^32 - 1
        for change, status in bad:
            with pytest.raises(GeError) as e:
                b.run_rooms_playout(**{**ok, **change})
            assert e.value.status == status, (change, e.value.status)
            assert b.read_rooms().tobytes() == before and b.turn == turn
        b.run_rooms_playout(**{**ok, "turns": [0, 0xFFFFFFFF - 4 - 15, 0], "until": 0})   # the last turns that fit
        b.write_rooms(0, np.frombuffer(before, dtype=ROOM_VIEW_DTYPE))
        n, cap = 3, 4
        r, k, t, m, pk = (np.array(ok[x], dtype=d) for x, d in (("rooms", np.uint64), ("keys", np.uint64), ("turns", np.uint32),
                                                                  ("masks", np.uint32), ("playout_keys", np.uint64)))
        played = np.full(n, 77, dtype=np.uint32)
        views = np.full(n * cap, 0x5A, dtype=np.uint8).repeat(ROOM_VIEW_DTYPE.itemsize)
        run = b._lib.ge_batch_run_rooms_playout
        args = (b._h, n, r.ctypes.data, k.ctypes.data, t.ctypes.data)
        assert run(*args, m.ctypes.data, pk.ctypes.data, 8, 16, 0, 0, cap, 3, None, None, None, None, None, 0) == GE_ERR_ARG       # played NULL
        assert run(*args, None, pk.ctypes.data, 8, 16, 0, 0, cap, 3, played.ctypes.data, None, None, None, None, 0) == GE_ERR_ARG  # masks NULL
        assert run(*args, m.ctypes.data, None, 8, 16, 0, 0, cap, 3, played.ctypes.data, None, None, None, None, 0) == GE_ERR_ARG   # keys NULL
        assert run(*args, m.ctypes.data, pk.ctypes.data, 8, 16, 0, 2, cap, 3, played.ctypes.data, None, None, None, None, 0) == GE_ERR_ARG   # flags
        assert run(*args, m.ctypes.data, pk.ctypes.data, 8, 16, 0, 0, cap, 3, played.ctypes.data, None, None, None, views.ctypes.data,
                   views.nbytes - 1) == GE_ERR_ARG                                                                                 # views cap too small
        assert set(views.tobytes()) == {0x5A} and (played == 77).all()
        assert b.read_rooms().tobytes() == before and b.turn == turn
        assert run(b._h, 0, None, None, None, m.ctypes.data, pk.ctypes.data, 8, 16, 0, 0, 0, 99, None, None, None, None, None, 0) == 0   # n == 0
        assert run(b._h, 0, None, None, None, m.ctypes.data, pk.ctypes.data, 0, 16, 0, 0, 0, 99, None, None, None, None, None, 0) == GE_ERR_ARG
        p, s, e, v, d = b.run_rooms_playout([], [], [], [], [], 8, max_turns=5)
        assert len(p) == 0 and e.shape == (0, 5) and d.shape == (0, 5)

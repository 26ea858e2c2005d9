"""GE_PLAYOUT_HALVING (-m gpu; POLICY.md §3h): ge_batch_step_rooms_playout and ge_batch_run_rooms_playout under the flag, word for
word against tests/halving_ref.py (the rule restated on the oracle; its room sets hold the decisions that matter - proved on the
CPU by tests/test_halving_host.py) and against the composition of public calls on the GPU (per round one ge_batch_rollout_seats
call over key + o_j, the cut and the pick in numpy, inject_actions, step_rooms); the invariants of §3h; the run-on call against
the loop of flagged steps; a two-segment list (two units in one pass) against the per-segment calls, step and run-on; the
refusals; Python and Node giving the same bytes; both services playing a thread alike."""
import copy
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import halving_ref as H
from conftest import ROOT, load_dsl
from game_engine_amd import EVENT_DTYPE, ROOM_VIEW_DTYPE, GameTable, GeError, RoomBatch, RoomPoolService, RoomService
from oracle.oracle import Oracle
from oracle.rng import pick
from parity_util import assert_views_equal, oracle_rooms_as_views, views_as_oracle_rooms
from playout_ref import SEAT_WINS, candidates, due_seats, seat_draw
from run_ref import END, PERSON, PHASE, person_pending
from test_gpu_playout import _all_bots, _twins

pytestmark = pytest.mark.gpu

GE_ERR_ARG = -1
EV_FIELDS = ("turn", "from_phase_id", "to_phase_id", "acted_now", "restarted", "choice")


def _batch(dsl, orc, rooms, hmask=0):
    b = RoomBatch([(GameTable(dsl), orc.n, len(rooms), hmask)], seed=H.SEED, first_room=41, max_fuse=1)
    b.write_rooms(0, oracle_rooms_as_views(orc, rooms))
    return b


@pytest.mark.parametrize("name,full_view", [("ww8", False), ("ww12", False), ("tt4", False), ("ww_generic", False), ("ww8", True), ("tt4", True)])
def test_flagged_step_matches_the_reference(name, full_view):
    dsl, orc, rooms, listed, keys, turns, masks, pkeys = H.case_inputs(name)
    after, want_ev, want_dec, log = H.shared_reference(name, full_view)
    assert len(log) > 10
    with _batch(dsl, orc, rooms) as b:
        ev, dec = b.step_rooms_playout(listed, keys, turns, masks, pkeys, H.N_REF, H.M_REF, seed=H.PSEED, full_view=full_view, halving=True)
        assert_views_equal(b.read_rooms(), oracle_rooms_as_views(orc, after), f"{name} full_view={full_view}")
    for k in range(len(listed)):
        for f in EV_FIELDS:
            assert np.array_equal(ev[k][f], want_ev[k][f]), (name, k, int(listed[k]), f, ev[k][f], want_ev[k][f])
    assert dec.tolist() == want_dec.tolist()


def _compose(b, orc, recs, listed, keys, turns, masks, pkeys, n, M, full_view):
    """§3h from public calls on batch b (whose rooms are `recs`): per round one rollout_seats call, the cut and the pick in numpy.
    Returns [(k, seat, choice)] and the playouts played."""
    seats = []                                                   # [k, seat, candidates, live, V]
    for k, r in enumerate(listed):
        room = recs[int(r)]
        for s in due_seats(orc, room, H.SEED, int(keys[k]), int(turns[k]), False, 0):
            cand = candidates(orc, room, s)
            if (int(masks[k]) >> (s - 1)) & 1 and len(cand) >= 2:
                seats.append([k, s, cand, list(cand), {x: 0 for x in cand}])
    played = 0
    for j in range(4):
        q = [(e, x) for e, (k, s, cand, live, V) in enumerate(seats) for x in live
             if j < H.rounds(len(cand)) and H.offsets(n, len(cand))[j + 1] > H.offsets(n, len(cand))[j]]
        # entries of equal length share a call (n_rollouts is per call)
        for length in sorted({H.offsets(n, len(seats[e][2]))[j + 1] - H.offsets(n, len(seats[e][2]))[j] for e, _ in q}):
            part = [(e, x) for e, x in q if H.offsets(n, len(seats[e][2]))[j + 1] - H.offsets(n, len(seats[e][2]))[j] == length]
            words, st = b.rollout_seats([int(listed[seats[e][0]]) for e, _ in part],
                                        [(int(pkeys[seats[e][0]]) + H.offsets(n, len(seats[e][2]))[j]) & H.M64 for e, _ in part],
                                        [int(turns[seats[e][0]]) for e, _ in part], [0 if full_view else seats[e][1] for e, _ in part],
                                        [[(seats[e][1], x)] for e, x in part], length, M, seed=H.PSEED)
            assert not st.any()
            for (e, x), w in zip(part, words):
                seats[e][4][x] += int(w[SEAT_WINS + seats[e][1] - 1])
            played += length * len(part)
        for sd in seats:
            k, s, cand, live, V = sd
            if j < H.rounds(len(cand)) - 1:
                kk = -(-len(cand) // (1 << (j + 1)))
                theta = sorted((V[x] for x in live), reverse=True)[kk - 1]
                sd[3] = [x for x in live if V[x] >= theta]
    out = []
    for k, s, cand, live, V in seats:
        top = max(V[x] for x in live)
        tied = [x for x in live if V[x] == top]
        out.append((k, s, tied[pick(seat_draw(H.SEED, int(keys[k]), int(turns[k]), s), len(tied))]))
    return out, played, sum(len(sd[2]) for sd in seats)


@pytest.mark.parametrize("n", [200, 5])
@pytest.mark.parametrize("name", ["ww8", "ww12", "tt4"])
def test_flagged_step_is_the_composition_of_public_calls(name, n):
    """n = 200: offsets 0/66/200, 0/28/85/200, 0/13/40/93/200 - ranges that start off a 64 boundary, straddle one and span several
    wavefronts; n = 5: empty early rounds (0/1/5, 0/0/2/5, 0/0/1/2/5)."""
    dsl, orc, rooms, listed, keys, turns, masks, pkeys = H.case_inputs(name)
    M = 64
    with _batch(dsl, orc, rooms) as b1, _batch(dsl, orc, rooms) as b2:
        chosen, played, uniform = _compose(b2, orc, rooms, listed, keys, turns, masks, pkeys, n, M, False)
        assert chosen and played < uniform * n
        st = b2.inject_actions([int(listed[k]) for k, _, _ in chosen], [s for _, s, _ in chosen], [c for _, _, c in chosen])
        assert not st.any()
        want = b2.step_rooms(listed, keys, turns)
        for k, s, c in chosen:
            want[k]["acted_now"] |= 1 << (s - 1)
            want[k]["choice"][s - 1] |= c
        ev, dec = b1.step_rooms_playout(listed, keys, turns, masks, pkeys, n, M, seed=H.PSEED, halving=True)
        assert ev.tobytes() == want.tobytes()
        assert b1.read_rooms().tobytes() == b2.read_rooms().tobytes()
        want_dec = np.zeros(len(listed), np.uint32)
        for k, s, _ in chosen:
            want_dec[k] |= 1 << (s - 1)
        assert dec.tolist() == want_dec.tolist()


@pytest.mark.parametrize("name", ["ww8", "ww12", "tt4"])
def test_invariants_mask_zero_no_playout_turn_and_one_rollout(name):
    dsl, orc, rooms, listed, keys, turns, masks, pkeys = H.case_inputs(name)
    with _batch(dsl, orc, rooms) as b1, _batch(dsl, orc, rooms) as b2:
        start = b1.read_rooms()
        want = b2.step_rooms(listed, keys, turns)
        after = b2.read_rooms().tobytes()
        ev, dec = b1.step_rooms_playout(listed, keys, turns, np.zeros_like(masks), pkeys, 24, 48, seed=3, halving=True)
        assert ev.tobytes() == want.tobytes() and b1.read_rooms().tobytes() == after and not dec.any()     # mask 0
        b1.write_rooms(0, start)
        ev, dec = b1.step_rooms_playout(listed, keys, turns, masks, pkeys, 24, 0, seed=3, halving=True)
        assert ev.tobytes() == want.tobytes() and b1.read_rooms().tobytes() == after and dec.any()         # max_turns = 0
        b1.write_rooms(0, start)
        b2.write_rooms(0, start)
        ev1, dec1 = b1.step_rooms_playout(listed, keys, turns, masks, pkeys, 1, 48, seed=3, halving=True)  # n = 1
        ev0, dec0 = b2.step_rooms_playout(listed, keys, turns, masks, pkeys, 1, 48, seed=3)
        assert ev1.tobytes() == ev0.tobytes() and dec1.tolist() == dec0.tolist() and b1.read_rooms().tobytes() == b2.read_rooms().tobytes()
        assert dec1.any()


def test_two_player_two_truths_every_seat_has_three_candidates():
    """A Two-Truths x 2 segment (the entry space reserves 3 candidates for 2 players; every decision has c = 3, two rounds over
    replicas 0 .. 7 and 8 .. 23).  The oracle takes no 2-player game, so the reference's rule (halving_ref.halve, the pick) is fed
    with the values of separate rollout_seats calls, as tests/test_gpu_playout.py checks the unflagged call on this segment."""
    dsl = copy.deepcopy(load_dsl("two-truths-and-a-lie"))
    dsl["declaration"]["min_players"] = 2
    tb, R_src, n, M = GameTable(dsl), H.ROOMS, 24, 40
    o = H.offsets(n, 3)
    assert o == [0, 8, 24]
    b1 = RoomBatch([(tb, 2, R_src, 0)], seed=0x5EED, max_fuse=1)
    b2 = RoomBatch([(tb, 2, R_src, 0)], seed=0x5EED, max_fuse=1)
    rng = np.random.default_rng(29)
    rooms = np.arange(R_src, dtype=np.uint64)
    masks = np.full(R_src, 0b11, np.uint32)
    checked = cut = 0
    for t in range(16):
        keys = (rooms + 1000).astype(np.uint64)
        turns = np.full(R_src, t, np.uint32)
        pkeys = rng.integers(0, 1 << 62, R_src).astype(np.uint64)
        b2.write_rooms(0, b1.read_rooms())
        q = [(r, s, c) for r in range(R_src) for s in (1, 2) for c in (1, 2, 3)]
        vals = {}
        for lo, hi in zip(o, o[1:]):
            words, st = b2.rollout_seats([r for r, _, _ in q], [int(pkeys[r]) + lo for r, _, _ in q], [t] * len(q), [s for _, s, _ in q],
                                         [[(s, c)] for _, s, c in q], hi - lo, M, seed=0xAB)
            for (r, s, c), w, bad in zip(q, words, st):
                vals[(r, s, c, lo)] = None if bad else int(w[SEAT_WINS + s - 1])
        ev, dec = b1.step_rooms_playout(rooms, keys, turns, masks, pkeys, n, M, seed=0xAB, halving=True)
        chosen = []
        for r in range(R_src):
            for s in (1, 2):
                if not (int(dec[r]) >> (s - 1)) & 1:
                    continue
                assert seat_draw(0x5EED, 1000 + r, t, s) & 3 and vals[(r, s, 1, 0)] is not None, (t, r, s)   # due, and a target
                V, last, played, _ = H.halve([1, 2, 3], n, lambda x, lo, hi: vals[(r, s, x, lo)])
                top = max(V[x] for x in last)
                tied = [x for x in last if V[x] == top]
                assert int(ev[r]["choice"][s - 1]) == tied[pick(seat_draw(0x5EED, 1000 + r, t, s), len(tied))], (t, r, s, V, last)
                chosen.append((r, s, int(ev[r]["choice"][s - 1])))
                checked += 1
                cut += len(last) < 3
        # and word for word: the chosen actions injected and the turn played by step_rooms on the twin
        assert not b2.inject_actions([r for r, _, _ in chosen], [s for _, s, _ in chosen], [c for _, _, c in chosen]).any()
        want = b2.step_rooms(rooms, keys, turns)
        for r, s, c in chosen:
            want[r]["acted_now"] |= 1 << (s - 1)
            want[r]["choice"][s - 1] |= c
        assert ev.tobytes() == want.tobytes() and b1.read_rooms().tobytes() == b2.read_rooms().tobytes(), t
    assert checked > 0 and cut > 0
    b1.close(); b2.close()


# ---- the run-on call: a mixed two-segment list, one human seat each, every fifth room without a playout seat
RUN_SEGS = [("ww", 8, 0b1), ("tt", 4, 0b10)]
RUN_PER = 35


def _run_inputs():
    rng = np.random.default_rng(77)
    segs = []
    for game, n, hmask in RUN_SEGS:
        dsl = H.case_dsl(game)
        orc = Oracle(dsl, n)
        segs.append((orc, dsl, n, hmask, H.played_rooms(orc, RUN_PER, rng)))
    total = RUN_PER * len(segs)
    listed = rng.permutation(total)[:60].astype(np.uint64)
    keys = rng.choice(1 << 40, size=60, replace=False).astype(np.uint64)
    turns = rng.integers(0, 300, 60).astype(np.uint32)
    masks = np.array([((1 << segs[int(r) // RUN_PER][2]) - 1) & ~segs[int(r) // RUN_PER][3] for r in listed], dtype=np.uint32)
    masks[4::5] = 0
    pkeys = rng.integers(0, 1 << 63, 60).astype(np.uint64)
    return segs, listed, keys, turns, masks, pkeys


def _run_batch(segs):
    b = RoomBatch([(GameTable(dsl), n, len(rooms), hmask) for _, dsl, n, hmask, rooms in segs], seed=H.SEED, first_room=777, max_fuse=1)
    for g, (orc, _, _, _, rooms) in enumerate(segs):
        b.write_rooms(g * RUN_PER, oracle_rooms_as_views(orc, rooms))
    return b


@pytest.mark.parametrize("until,max_turns", [(PERSON | END, 9), (PHASE, 9), (PERSON | END, 1), (PHASE, 1)])
def test_flagged_run_is_the_loop_of_flagged_steps(until, max_turns):
    segs, listed, keys, turns, masks, pkeys = _run_inputs()
    n, R, M = len(listed), 24, 32
    with _run_batch(segs) as twin, _run_batch(segs) as b:
        played, stopped = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        events, views = np.zeros((n, max_turns), EVENT_DTYPE), np.zeros((n, max_turns), ROOM_VIEW_DTYPE)
        decided = np.zeros((n, max_turns), np.uint32)
        live = np.arange(n)
        for t in range(max_turns):
            ev, dec = twin.step_rooms_playout(listed[live], keys[live], turns[live] + np.uint32(t), masks[live], pkeys[live], R, M, seed=H.PSEED,
                                              halving=True)
            vw = twin.read_rooms_at(listed[live])
            events[live, t], views[live, t], decided[live, t] = ev, vw, dec
            played[live] = t + 1
            why = np.zeros(len(live), np.uint32)
            for x, k in enumerate(live):
                orc, _, _, hmask, _ = segs[int(listed[k]) // RUN_PER]
                one = views_as_oracle_rooms(orc, vw[x:x + 1])
                if not orc.table.phases[int(one["phase"][0])].branches:
                    why[x] |= END
                if ev[x]["to_phase_id"] != ev[x]["from_phase_id"]:
                    why[x] |= PHASE
                if person_pending(orc, one, hmask):
                    why[x] |= PERSON
            why &= np.uint32(until)
            stopped[live] = why
            live = live[why == 0]
            if not len(live):
                break
        p, s, e, v, d = b.run_rooms_playout(listed, keys, turns, masks, pkeys, R, M, seed=H.PSEED, max_turns=max_turns, until=until, halving=True)
        assert np.array_equal(p, played) and np.array_equal(s, stopped), (p.tolist(), played.tolist(), s.tolist(), stopped.tolist())
        for k in range(n):
            q = int(p[k])
            assert e[k, :q].tobytes() == events[k, :q].tobytes() and v[k, :q].tobytes() == views[k, :q].tobytes(), k
            assert d[k, :q].tolist() == decided[k, :q].tolist(), k
        assert b.read_rooms().tobytes() == twin.read_rooms().tobytes()
        assert d.any()
        if max_turns == 9 and until == PHASE:
            assert int(p.max()) == 9 or int(p.min()) < int(p.max())


# ---- two units in one pass: a two-segment list, the second segment's entries behind the first's (e_base != 0)
TWO_SEGMENTS = [("ww", 6, 0), ("tt", 4, 0b10)]


def _two_segment_list():
    """Twin batches of both segments and a list of all their rooms, the segments interleaved, every bot seat a playout seat."""
    b1, b2, parts, R_src = _twins(TWO_SEGMENTS, seed=19, R=16)
    rng = np.random.default_rng(19)
    rooms = rng.permutation(2 * R_src).astype(np.uint64)
    keys = rng.choice(1 << 40, size=len(rooms), replace=False).astype(np.uint64)
    turns = rng.integers(0, 50000, len(rooms)).astype(np.uint32)
    masks = np.array(_all_bots(parts, R_src, rooms), dtype=np.uint32)
    pkeys = rng.integers(0, 1 << 63, len(rooms)).astype(np.uint64)
    per_segment = [np.nonzero(rooms // R_src == g)[0] for g in range(2)]
    return b1, b2, (rooms, keys, turns, masks, pkeys), per_segment


@pytest.mark.parametrize("halving", [True, False], ids=["halving", "plain"])
@pytest.mark.parametrize("n", [5, 200])
def test_two_segment_step_is_the_per_segment_steps(n, halving):
    """A listed room's result depends only on its own record, keys and turn: the whole list in one call (two units sharing one
    pass's arrays) equals one call per segment on a twin, byte for byte.  n = 5 and n = 200: the two replica-range regimes of
    test_flagged_step_is_the_composition_of_public_calls."""
    b1, b2, cols, per_segment = _two_segment_list()
    with b1, b2:
        ev, dec = b1.step_rooms_playout(*cols, n, 48, seed=H.PSEED, halving=halving)
        for idx in per_segment:
            ev_g, dec_g = b2.step_rooms_playout(*(c[idx] for c in cols), n, 48, seed=H.PSEED, halving=halving)
            assert ev[idx].tobytes() == ev_g.tobytes() and dec[idx].tolist() == dec_g.tolist()
            assert dec_g.any(), "a segment without a decision"
        assert b1.read_rooms().tobytes() == b2.read_rooms().tobytes()


def _filled_run(b, cols, n_rollouts, max_turns, until):
    """ge_batch_run_rooms_playout under the flag into outputs that hold a pattern: (played, stopped, events, views, decided)"""
    rooms, keys, turns, masks, pkeys = (np.ascontiguousarray(c) for c in cols)
    n = len(rooms)
    played, stopped = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    events = np.full((n, max_turns, EVENT_DTYPE.itemsize), 0xA5, np.uint8)
    views = np.full((n, max_turns, ROOM_VIEW_DTYPE.itemsize), 0x5A, np.uint8)
    decided = np.full((n, max_turns), 0xC3C3C3C3, np.uint32)
    st = b._lib.ge_batch_run_rooms_playout(b._h, n, rooms.ctypes.data, keys.ctypes.data, turns.ctypes.data, masks.ctypes.data, pkeys.ctypes.data,
                                           n_rollouts, 48, H.PSEED, 4, max_turns, until, played.ctypes.data, stopped.ctypes.data,
                                           decided.ctypes.data, events.ctypes.data, views.ctypes.data, views.nbytes)
    assert st == 0, st
    return played, stopped, events, views, decided


def test_two_segment_flagged_run_is_the_per_segment_runs():
    """The same list through the run-on call under the flag, against one call per segment on a twin: turn counts, stop bits,
    everything below `played`, the records; the slots behind `played` keep their pattern."""
    b1, b2, cols, per_segment = _two_segment_list()
    max_turns = 9
    with b1, b2:
        played, stopped, events, views, decided = _filled_run(b1, cols, 24, max_turns, PERSON | END)
        for idx in per_segment:
            p_g, s_g, e_g, v_g, d_g = _filled_run(b2, [c[idx] for c in cols], 24, max_turns, PERSON | END)
            assert played[idx].tolist() == p_g.tolist() and stopped[idx].tolist() == s_g.tolist()
            for x, k in enumerate(idx):
                q = int(played[k])
                assert events[k, :q].tobytes() == e_g[x, :q].tobytes() and views[k, :q].tobytes() == v_g[x, :q].tobytes(), k
                assert decided[k, :q].tolist() == d_g[x, :q].tolist(), k
            assert any(d_g[x, :int(p_g[x])].any() for x in range(len(idx))), "a segment without a decision"
        for k in range(len(played)):
            q = int(played[k])
            assert 1 <= q <= max_turns
            assert (events[k, q:] == 0xA5).all() and (views[k, q:] == 0x5A).all() and (decided[k, q:] == 0xC3C3C3C3).all(), k
        assert (played < max_turns).any(), "no room stopped before the last turn: no slot behind `played`"
        assert b1.read_rooms().tobytes() == b2.read_rooms().tobytes()


def test_flag_values_refused_and_accepted(dsl_ww):
    with RoomBatch([(GameTable(dsl_ww), 8, 16, 0)], seed=1, max_fuse=1) as b:
        b.step(5)
        before = b.read_rooms().tobytes()
        r, k, pk = (np.arange(3, dtype=np.uint64) + x for x in (0, 10, 20))
        t, m = np.array([5, 5, 5], np.uint32), np.array([0xFF, 0xFF, 0xFF], np.uint32)
        played = np.zeros(3, np.uint32)
        step = lambda flags: b._lib.ge_batch_step_rooms_playout(b._h, 3, r.ctypes.data, k.ctypes.data, t.ctypes.data, m.ctypes.data, pk.ctypes.data,
                                                                8, 8, 1, flags, None, None)
        run = lambda flags: b._lib.ge_batch_run_rooms_playout(b._h, 3, r.ctypes.data, k.ctypes.data, t.ctypes.data, m.ctypes.data, pk.ctypes.data,
                                                              8, 8, 1, flags, 2, 0, played.ctypes.data, None, None, None, None, 0)
        for flags in (2, 8, 2 | 4, 8 | 1, 1 << 31):
            assert step(flags) == GE_ERR_ARG and run(flags) == GE_ERR_ARG, flags
            assert b.read_rooms().tobytes() == before and not played.any()
        for flags in (4, 5):
            assert step(flags) == 0, flags
            assert run(flags) == 0 and (played == 2).all(), flags
        assert b.read_rooms().tobytes() != before


def _players(n):
    return [{"name": f"P{i + 1}", "gamePlayerId": i + 1, "isBot": True} for i in range(n)]


def _thread_lines(svc, seats, turns, room=71):
    svc.create_room("t", "werewolf-(mafia)", _players(8), dsl=load_dsl("werewolf-(mafia)"), room_index=room, playout_seats=seats)
    lines = []
    for _ in range(turns):
        out = svc.handle_message("t", "Continue")
        lines.append(json.dumps({"toolCalls": out["toolCalls"], "uiCalls": out["uiCalls"]}, separators=(",", ":"), ensure_ascii=False))
    svc.close()
    return lines


def _event_dict(e):
    return {"turn": int(e["turn"]), "from_phase_id": int(e["from_phase_id"]), "to_phase_id": int(e["to_phase_id"]), "acted_now": int(e["acted_now"]),
            "restarted": int(e["restarted"]), "choice": [int(c) for c in e["choice"]]}


SVC = dict(playout_rollouts=48, playout_max_turns=64, playout_halving=True)


def test_both_services_play_a_thread_alike():
    flagged = [_thread_lines(cls(seed=21, **SVC), (1, 2, 3, 4, 5, 6, 7, 8), 14) for cls in (RoomService, RoomPoolService)]
    assert flagged[0] == flagged[1]
    # run-on: a thread with a person on seat 1 is played to that person's turn identically by both services
    outs = []
    for cls in (RoomService, RoomPoolService):
        svc = cls(seed=22, **SVC)
        players = [{"name": f"P{i + 1}", "gamePlayerId": i + 1, "isBot": i != 0} for i in range(8)]
        svc.create_room("t", "werewolf-(mafia)", players, dsl=load_dsl("werewolf-(mafia)"), room_index=5, playout_seats=(2, 3, 4, 5, 6, 7, 8))
        out = svc.run_room("t", 40, ("person", "end"), playout=True)
        assert out["played"] >= 1
        outs.append(json.dumps([out["played"], out["stopped"], [[x["toolCalls"], x["uiCalls"]] for x in out["turns"]]], sort_keys=True))
        svc.close()
    assert outs[0] == outs[1]


@pytest.mark.skipif(shutil.which("node") is None or not os.path.exists(os.path.join(ROOT, "game_engine_amd", "node", "ge_addon.node")),
                    reason="node or the N-API addon is not built here")
def test_python_and_node_give_the_same_bytes(tmp_path):
    """node/selftest_halving.js: one flagged step and one flagged run on a Werewolf x 8 batch (events, decided masks, counts and
    records), then a thread through both Node services - against the same calls through RoomBatch and the Python services."""
    rooms = list(range(0, 64, 2))
    script = {"dsl": os.path.join(ROOT, "tests", "golden", "dsl", "werewolf-(mafia).json"), "seed": 0x5EED, "pseed": 9, "nRooms": 64, "warm": 6,
              "rooms": rooms, "keys": [r + 1000 for r in rooms], "masks": [0xFF] * 32, "playoutKeys": [r + 77 for r in rooms], "rollouts": 40,
              "maxTurns": 48, "runTurns": 5, "game": "werewolf-(mafia)", "names": [f"P{i + 1}" for i in range(8)], "room": 71,
              "seats": [1, 2, 3, 4, 5, 6, 7, 8], "turns": 12}
    sp = tmp_path / "script.json"
    sp.write_text(json.dumps(script))
    p = subprocess.run(["node", os.path.join(ROOT, "game_engine_amd", "node", "selftest_halving.js"), str(sp)], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    with RoomBatch([(GameTable(load_dsl("werewolf-(mafia)")), 8, 64, 0)], seed=0x5EED, max_fuse=1) as b:
        b.step(6)
        turns = np.full(32, 6, np.uint32)
        ev, dec = b.step_rooms_playout(rooms, script["keys"], turns, script["masks"], script["playoutKeys"], 40, 48, seed=9, halving=True)
        assert got["stepEvents"] == [_event_dict(e) for e in ev] and got["stepDecided"] == dec.tolist()
        assert dec.any()
        pl, st, e, _, d = b.run_rooms_playout(rooms, script["keys"], turns + 1, script["masks"], script["playoutKeys"], 40, 48, seed=9,
                                              max_turns=5, until=("phase",), views=False, halving=True)
        assert got["runPlayed"] == pl.tolist() and got["runStopped"] == st.tolist()
        for k in range(32):
            q = int(pl[k])
            assert got["runEvents"][k] == [_event_dict(x) for x in e[k, :q]] and got["runDecided"][k] == d[k, :q].tolist(), k
        assert got["records"] == b.read_rooms(0, 64).tobytes().hex()
    for lines, cls in zip(got["threads"], (RoomService, RoomPoolService)):
        assert lines == _thread_lines(cls(seed=0x5EED, **SVC), script["seats"], script["turns"])

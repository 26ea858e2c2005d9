"""Per-room host-driven seats (-m gpu; POLICY.md §3l): ge_batch_set_seats / get_seats / clear_seats and every call that honours
the mask - step_rooms, the run-ons, find_rooms, the playout-seat check and ge_batch_step itself - against the oracle run under each
room's own mask (tests/seats_ref.py).  Masks differ from lane to lane inside a wavefront; tests/test_seats_host.py proves on the
oracle alone that they change what the rooms do, so no comparison here passes vacuously."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from game_engine_amd import ROOM_VIEW_DTYPE, GameTable, GeError, RoomBatch
from oracle.summary import reference_summary_words
from parity_util import assert_summary_equal, assert_views_equal, oracle_rooms_as_views
from run_ref import END, PERSON, SEED
from seats_ref import (FIRST_ROOM, SEAT_CASES, SIZES, flat_masks, lowest_choice, pending_of, run_rooms_ref, seat_case, segment_masks,
                       step_rooms_ref, step_turn_ref, views_of)

pytestmark = pytest.mark.gpu

GE_ERR_ARG, GE_ERR_RANGE = -1, -6
EV_FIELDS = ("turn", "from_phase_id", "to_phase_id", "acted_now", "restarted", "choice")
_TABLES = {}


def _table(dsl):
    key = id(dsl)
    if key not in _TABLES:
        _TABLES[key] = (GameTable(dsl), dsl)                     # (the dsl is kept alive: its id is the key)
    return _TABLES[key][0]


def _write(b, segs, rooms=None):
    base = 0
    for s, (orc, _, _, _, start) in enumerate(segs):
        b.write_rooms(base, oracle_rooms_as_views(orc, start if rooms is None else rooms[s]))
        base += len(start)


def _batch(segs, restart, max_fuse=1, trace=False, seg_masks=None):
    """The start rooms written as views; seg_masks: the segments' human_mask (default: the case's)."""
    b = RoomBatch([(_table(dsl), n, len(rooms), mask if seg_masks is None else seg_masks[g]) for g, (_, dsl, n, mask, rooms) in enumerate(segs)],
                  seed=SEED, first_room=FIRST_ROOM, max_fuse=max_fuse, restart=restart, trace=trace)
    _write(b, segs)
    return b


def _set_all(b, masks):
    flat = flat_masks(masks)
    order = np.random.default_rng(len(flat)).permutation(len(flat))      # the list in any order
    b.set_seats(order, flat[order])
    assert np.array_equal(b.seats(), flat)


def _assert_events(got, want, what):
    for k, w in enumerate(want):
        for f in EV_FIELDS:
            assert np.array_equal(got[k][f], w[f]), (what, "event", k, f, got[k][f], w[f])


# ---- 1. the three calls

@pytest.mark.parametrize("name", ["ww8_generic_h1", "mixed"])
def test_seats_reads_what_was_set_and_clear_gives_the_segment_masks_back(name):
    for per in (1, 65):
        segs, _, _, _, masks = seat_case(name, per, False)
        with _batch(segs, False) as b:
            assert np.array_equal(b.seats(), segment_masks(segs))
            assert b.seats().dtype == np.uint32 and len(b.seats(3 % per, 0)) == 0
            _set_all(b, masks)
            flat = flat_masks(masks)
            assert np.array_equal(b.seats(per - 1, 1), flat[per - 1:per])
            b.set_seats([0], [0])                                # a second set changes the listed room alone
            flat[0] = 0
            assert np.array_equal(b.seats(), flat)
            b.clear_seats()
            assert np.array_equal(b.seats(), segment_masks(segs))
            b.clear_seats()                                      # without a plane: nothing to do
            b.set_seats([], [])
            assert np.array_equal(b.seats(), segment_masks(segs))


# ---- 2. step_rooms

@pytest.mark.parametrize("restart", [False, True])
@pytest.mark.parametrize("name", SEAT_CASES)
def test_step_rooms_plays_each_room_under_its_own_mask(name, restart):
    for per in SIZES:
        segs, listed, keys, turns, masks = seat_case(name, per, restart)
        want_e, after = step_rooms_ref(segs, masks, listed, keys, turns, restart)
        with _batch(segs, restart) as b:
            _set_all(b, masks)
            events = b.step_rooms(listed, keys, turns)
            got = b.read_rooms()
        _assert_events(events, want_e, (name, restart, per))
        assert_views_equal(got, views_of(segs, after), f"{name} restart={restart} per={per}: records (listed and unlisted)")


# ---- 3. the run-ons

def _check_run(got, ref, what):
    played, stopped, events, views = got
    want_p, want_s, want_e, want_v = ref
    assert np.array_equal(played, want_p), (what, "played", played.tolist(), want_p.tolist())
    assert np.array_equal(stopped, want_s), (what, "stopped", stopped.tolist(), want_s.tolist())
    for k in range(len(played)):
        p = int(played[k])
        _assert_events(events[k, :p], want_e[k], (what, k))
        assert_views_equal(views[k, :p], np.array(want_v[k], dtype=ROOM_VIEW_DTYPE), f"{what}: views of entry {k}")


@pytest.mark.parametrize("per", SIZES)
@pytest.mark.parametrize("name", SEAT_CASES)
def test_run_rooms_stops_for_the_rooms_own_people(name, per):
    restart = True
    segs, listed, keys, turns, masks = seat_case(name, per, restart)
    person_stops = 0
    with _batch(segs, restart) as b:
        _set_all(b, masks)
        for until in range(1, 8):
            max_turns = 6 if until & PERSON else 3
            _write(b, segs)
            *ref, after = run_rooms_ref(segs, masks, listed, keys, turns, max_turns, until, restart)
            got = b.run_rooms(listed, keys, turns, max_turns=max_turns, until=until)
            _check_run(got, ref, f"{name} per={per} until={until}")
            assert_views_equal(b.read_rooms(), views_of(segs, after), f"{name} per={per} until={until}: records after the call")
            person_stops += int(((got[1] & PERSON) != 0).sum())
    assert per < 63 or person_stops > 0


@pytest.mark.parametrize("name", ["ww12", "tt8", "mixed"])
def test_run_rooms_forecast_runs_as_run_rooms_does(name):
    per, restart = 65, True
    segs, listed, keys, turns, masks = seat_case(name, per, restart)
    listed, keys, turns = listed[:40], keys[:40], turns[:40]
    with _batch(segs, restart) as b:
        _set_all(b, masks)
        played, stopped, events, views = b.run_rooms(listed, keys, turns, max_turns=6, until=PERSON | END)
        _write(b, segs)
        fp, fs, fe, fv, _ = b.run_rooms_forecast(listed, keys, turns, keys, n_rollouts=2, playout_max_turns=4, max_turns=6, until=PERSON | END)
    assert np.array_equal(fp, played) and np.array_equal(fs, stopped) and (stopped & PERSON).any()
    assert fe.tobytes() == events.tobytes() and fv.tobytes() == views.tobytes()


# ---- 4. find_rooms

def _windows(per, n_seg):
    total = per * n_seg
    w = [(0, total), (5, 50), (63, 2), (1, total - 2), (70, 59), (total - 1, 1)]
    for k in range(1, n_seg):                                    # across each segment boundary
        w += [(k * per - 3, 7), (k * per, 1), (max(0, k * per - 70), 140)]
    return sorted({(f, c) for f, c in w if f >= 0 and c > 0 and f + c <= total})


@pytest.mark.parametrize("name", SEAT_CASES)
def test_find_rooms_reports_pending_seat_by_seat_under_each_rooms_mask(name):
    seen = 0
    for per in SIZES:
        segs, _, _, _, masks = seat_case(name, per, True)
        pend = np.concatenate([[pending_of(orc, rooms[i:i + 1], int(masks[s][i])) for i in range(per)]
                               for s, (orc, _, _, _, rooms) in enumerate(segs)])
        with _batch(segs, True) as b:
            _set_all(b, masks)
            for first, count in _windows(per, len(segs)):
                hits, n_match = b.find_rooms("person", first=first, count=count)
                want = [(r, int(pend[r])) for r in range(first, first + count) if pend[r]]
                assert n_match == len(want) and [(int(h["room"]), int(h["pending"])) for h in hits] == want, (name, per, first, count)
                seen += len(want)
    assert seen > 0


@pytest.mark.parametrize("name", ["ww12", "tt12"])
def test_pending_is_what_inject_actions_accepts(name):
    segs, _, _, _, masks = seat_case(name, 130, True)
    orc, _, n, _, rooms = segs[0]
    views = oracle_rooms_as_views(orc, rooms)
    with _batch(segs, True) as b, _batch(segs, True) as twin:
        _set_all(b, masks)
        hits, _ = b.find_rooms("person")
        pending = np.zeros(130, dtype=np.uint32)
        pending[hits["room"].astype(np.int64)] = hits["pending"]
        accepted = np.zeros(130, dtype=np.uint32)
        for seat in range(n):
            for choice in range(1, max(n, 3) + 1):
                twin.write_rooms(0, views)
                status = twin.inject_actions(np.arange(130), np.full(130, seat + 1), np.full(130, choice))
                accepted |= np.where(status == 0, np.uint32(1 << seat), np.uint32(0))
    assert np.array_equal(accepted & masks[0], pending), np.flatnonzero((accepted & masks[0]) != pending).tolist()
    assert (pending != 0).sum() >= 10


# ---- 5. ge_batch_step with a plane

def _answer(b, segs, rooms, masks):
    """The scripted person: for every pending seat of every room the lowest accepted choice, on both sides."""
    at, who, what, base = [], [], [], 0
    for s, (orc, _, _, _, _) in enumerate(segs):
        for i in range(len(rooms[s])):
            for seat in range(orc.n):
                if (int(masks[s][i]) >> seat) & 1:
                    c = lowest_choice(orc, rooms[s][i:i + 1], seat)
                    if c and orc.inject(rooms[s], i, seat + 1, c):
                        at.append(base + i); who.append(seat + 1); what.append(c)
        base += len(rooms[s])
    if at:
        assert not b.inject_actions(at, who, what).any()
    return len(at)


def _summary_ref(segs, rooms, turn):
    return reference_summary_words([(orc.table, orc.n, rooms[s]) for s, (orc, _, _, _, _) in enumerate(segs)], FIRST_ROOM, turn)


@pytest.mark.parametrize("restart", [False, True])
@pytest.mark.parametrize("max_fuse,n_turns", [(1, 1), (1, 5), (1, 64), (1, 70), (64, 1), (64, 5), (64, 64), (64, 70)])
@pytest.mark.parametrize("name", ["ww8", "tt8", "mixed"])
def test_step_with_a_plane_is_the_per_room_oracle(name, max_fuse, n_turns, restart):
    assert _check_step_with_a_plane(name, max_fuse, n_turns, restart) > 0


# the builds of the stepping kernel no case above launches - Two-Truths x 12 and every GENERIC one: 65 rooms, the turns of one launch, traced
@pytest.mark.parametrize("name", ["tt12", "ww8_generic_h1", "ww12_generic_h2", "tt4_generic_h1", "tt8_generic_h1", "tt12_generic"])
def test_step_with_a_plane_on_the_other_layouts_and_generic_tables(name):
    _check_step_with_a_plane(name, 64, 5, True)


def _check_step_with_a_plane(name, max_fuse, n_turns, restart):
    """Returns the number of scripted answers that were injected."""
    per = 65
    trace = n_turns <= max_fuse
    segs, _, _, _, masks = seat_case(name, per, restart)
    rooms = [r.copy() for _, _, _, _, r in segs]
    answered = 0
    with _batch(segs, restart, max_fuse=max_fuse, trace=trace) as b:
        _set_all(b, masks)
        for call in range(2 if n_turns > 5 else 4):
            turn0 = b.turn
            events = [step_turn_ref(segs, rooms, masks, turn0 + t, restart) for t in range(n_turns)]
            b.step(n_turns)
            what = f"{name} max_fuse={max_fuse} n_turns={n_turns} restart={restart} call {call}"
            assert b.turn == turn0 + n_turns
            assert_views_equal(b.read_rooms(), views_of(segs, rooms), what)
            if trace:
                got = b.read_events()
                assert got.shape == (per * len(segs), n_turns)
                for t in range(n_turns):
                    _assert_events(got[:, t], events[t], (what, t))
            assert_summary_equal(b.summary_words(), _summary_ref(segs, rooms, b.turn), what)
            answered += _answer(b, segs, rooms, masks)
    return answered


@pytest.mark.parametrize("max_fuse", [1, 64])
@pytest.mark.parametrize("name", ["ww8", "ww12", "tt4", "mixed"])
def test_step_with_every_mask_the_segments_equals_the_batch_without_a_plane(name, max_fuse):
    per, restart = 130, True
    segs, _, _, _, _ = seat_case(name, per, restart)
    m = [(0b101, 0b10, 0b1000, 0b1)[g] for g in range(len(segs))]
    for n_turns in (1, 5, 64, 70):
        trace = n_turns <= max_fuse
        with _batch(segs, restart, max_fuse, trace, seg_masks=[0] * len(segs)) as a, _batch(segs, restart, max_fuse, trace, seg_masks=m) as twin:
            a.set_seats(np.arange(per * len(segs)), np.repeat(np.array(m, dtype=np.uint32), per))
            for _ in range(2):
                a.step(n_turns)
                twin.step(n_turns)
                what = f"{name} max_fuse={max_fuse} n_turns={n_turns}"
                assert a.turn == twin.turn
                assert_views_equal(a.read_rooms(), twin.read_rooms(), what)
                assert a.summary() == twin.summary(), what
                if trace:
                    assert a.read_events().tobytes() == twin.read_events().tobytes(), what


# ---- 6. changing hands

@pytest.mark.parametrize("name", ["ww8", "tt8"])
def test_seats_change_hands_between_turns(name):
    per, restart = 130, False
    segs, _, _, _, masks = seat_case(name, per, restart)
    orc, _, n, _, start = segs[0]
    rooms, masks = [start.copy()], [masks[0].copy()]
    every = (1 << n) - 1
    stayed_acted = handed_to_policy_acted = 0
    with _batch(segs, restart, trace=True) as b:
        _set_all(b, masks)
        for turn in range(12):
            ev = step_turn_ref(segs, rooms, masks, b.turn, restart)
            b.step(1)
            what = f"{name} turn {turn}"
            _assert_events(b.read_events()[:, 0], ev, what)
            assert_views_equal(b.read_rooms(), views_of(segs, rooms), what)
            # person -> bot: every third room hands its people's seats to the policy; bot -> person: the next room takes the seats that
            # have just acted and whose visit goes on (they stay acted); a swap inside the first wavefront
            new = masks[0].copy()
            new[turn % 3::3] = 0
            for i in range((turn + 1) % 3, per, 3):
                acted = int(ev[i]["acted_now"]) if ev[i]["from_phase_id"] == ev[i]["to_phase_id"] and not ev[i]["restarted"] else 0
                new[i] = (int(new[i]) | acted | (1 << (turn % n))) & every
            new[[5, 40]] = new[[40, 5]]
            changed = np.flatnonzero(new != masks[0])
            b.set_seats(changed, new[changed])
            for i in range((turn + 1) % 3, per, 3):
                took = int(ev[i]["acted_now"]) & int(new[i]) & ~int(masks[0][i])
                if took and ev[i]["from_phase_id"] == ev[i]["to_phase_id"] and not ev[i]["restarted"]:
                    stayed_acted += 1
                    assert not pending_of(orc, rooms[0][i:i + 1], took), (what, i)
            if turn:
                handed_to_policy_acted += sum(1 for i in range(per) if int(ev[i]["acted_now"]) & int(before[i]) & ~int(masks[0][i]))
            before, masks[0] = masks[0], new
            assert np.array_equal(b.seats(), new)
            hits, _ = b.find_rooms("person")
            pend = {int(h["room"]): int(h["pending"]) for h in hits}
            assert pend == {i: p for i in range(per) for p in [pending_of(orc, rooms[0][i:i + 1], int(new[i]))] if p}, what
    assert stayed_acted > 0 and handed_to_policy_acted > 0


# ---- 7. prepared deals across the switch of step paths

@pytest.mark.parametrize("name", ["ww12", "ww8"])
def test_prepared_deals_survive_the_switch_of_step_paths(name):
    per, restart = 130, True
    segs, _, _, _, masks = seat_case(name, per, restart)
    orc, _, n, _, start = segs[0]
    rooms = [start.copy()]
    seg_mask = [np.full(per, 0b101, dtype=np.uint32)]
    with _batch(segs, restart, max_fuse=1, seg_masks=[0b101]) as b:
        def play(k, m, what):
            for t in range(k):
                step_turn_ref(segs, rooms, m, b.turn, restart)
                b.step(1)
                assert_views_equal(b.read_rooms(), views_of(segs, rooms), f"{name}: {what}, turn {t}")
        play(40, seg_mask, "the flagship path (fills the prepared deals)")
        assert int(rooms[0]["games"].max()) > 0
        _set_all(b, masks)
        play(40, masks, "with a plane")
        b.clear_seats()
        play(40, seg_mask, "the flagship path again")


# ---- 8. persistence

def test_the_mask_is_configuration_not_game_state():
    segs, listed, _, _, masks = seat_case("mixed", 65, True)
    flat = flat_masks(masks)
    with _batch(segs, True) as b:
        _set_all(b, masks)
        views = b.read_rooms()
        b.step(3)
        b.reset()
        assert np.array_equal(b.seats(), flat)
        b.set_turn(9)
        assert np.array_equal(b.seats(), flat)
        b.write_rooms(0, views)
        b.write_rooms_at(listed[:20], views[listed[:20]])
        assert np.array_equal(b.seats(), flat) and b.read_rooms().tobytes() == views.tobytes()


@pytest.mark.parametrize("name", ["ww8", "tt8"])
def test_rollouts_do_not_see_the_plane(name):
    segs, listed, keys, turns, masks = seat_case(name, 65, False)
    listed, keys, turns = listed[:20], keys[:20], turns[:20]
    seats = np.arange(20, dtype=np.uint32) % segs[0][2] + 1
    with _batch(segs, False) as b:
        before = b.rollout_rooms(listed, keys, turns, 64, max_turns=40)
        before_seats = b.rollout_seats(listed, keys, turns, seats, n_rollouts=64, max_turns=40)
        _set_all(b, masks)
        assert b.rollout_rooms(listed, keys, turns, 64, max_turns=40).tobytes() == before.tobytes()
        after_seats = b.rollout_seats(listed, keys, turns, seats, n_rollouts=64, max_turns=40)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(before_seats, after_seats))


# ---- 9. playout seats

def test_a_playout_seat_is_refused_where_that_room_has_a_person():
    segs, _, _, _, _ = seat_case("ww8", 65, False)
    for seg_mask, room_mask, playout, ok in ((0, 0b100, 0b100, False), (0b1, 0, 0b1, True), (0b1, 0b10, 0b1, True), (0b1, 0b10, 0b10, False)):
        with _batch(segs, False, seg_masks=[seg_mask]) as b:
            b.set_seats([7], [room_mask])
            before = b.read_rooms().tobytes()
            rooms, keys, turns = np.array([3, 7], dtype=np.uint64), np.array([11, 12], dtype=np.uint64), np.array([4, 4], dtype=np.uint32)
            pm = np.array([0, playout], dtype=np.uint32)
            if ok:
                b.step_rooms_playout(rooms, keys, turns, pm, keys, 4, max_turns=8)
                b.run_rooms_playout(rooms, keys, turns, pm, keys, 4, playout_max_turns=8, max_turns=2)
                assert b.read_rooms().tobytes() != before
                continue
            with pytest.raises(GeError) as e:
                b.step_rooms_playout(rooms, keys, turns, pm, keys, 4, max_turns=8)
            assert e.value.status == GE_ERR_ARG
            with pytest.raises(GeError) as e:
                b.run_rooms_playout(rooms, keys, turns, pm, keys, 4, playout_max_turns=8, max_turns=2)
            assert e.value.status == GE_ERR_ARG
            assert b.read_rooms().tobytes() == before, "something ran on a refusal"


# ---- 10. refusals

def test_refusals_come_in_the_documented_order_and_change_nothing():
    segs, _, _, _, masks = seat_case("mixed", 65, False)      # segments of 6, 4, 10 and 7 players
    total = 65 * 4
    u64 = lambda *x: np.array(x, dtype=np.uint64)
    u32 = lambda *x: np.array(x, dtype=np.uint32)
    with _batch(segs, False) as b:
        lib, h = b._lib, b._h

        def set_(n, rooms, m, handle=h):
            return lib.ge_batch_set_seats(handle, n, None if rooms is None else rooms.ctypes.data, None if m is None else m.ctypes.data)

        for planned in (False, True):
            if planned:
                _set_all(b, masks)
            seats, records = b.seats().copy(), b.read_rooms().tobytes()
            assert set_(1, u64(0), u32(0), None) == GE_ERR_ARG
            assert set_(1, None, u32(0)) == GE_ERR_ARG and set_(1, u64(0), None) == GE_ERR_ARG
            assert set_(0, None, None) == 0
            assert set_(4, u64(1, 1, total, 2), u32(0, 0, 0, 1 << 6)) == GE_ERR_RANGE     # outside before repeated before a bad mask
            assert set_(3, u64(1, 2, 1), u32(0, 1 << 6, 0)) == GE_ERR_ARG
            assert set_(2, u64(1, 2), u32(0, 1 << 6)) == GE_ERR_ARG                       # six players: bits 0 .. 5
            assert set_(1, u64(65), u32(1 << 4)) == GE_ERR_ARG and set_(1, u64(130), u32(1 << 10)) == GE_ERR_ARG
            assert set_(1, u64(total - 1), u32(1 << 7)) == GE_ERR_ARG
            dst = np.zeros(4, dtype=np.uint32)
            assert lib.ge_batch_get_seats(None, 0, 1, dst.ctypes.data) == GE_ERR_ARG
            assert lib.ge_batch_get_seats(h, 0, 1, None) == GE_ERR_ARG
            assert lib.ge_batch_get_seats(h, total - 1, 2, dst.ctypes.data) == GE_ERR_RANGE
            assert lib.ge_batch_get_seats(h, total, 0, None) == 0
            assert lib.ge_batch_clear_seats(None) == GE_ERR_ARG
            assert np.array_equal(b.seats(), seats) and b.read_rooms().tobytes() == records
        # the highest seat of every segment is a seat
        b.set_seats(u64(0, 65, 130, 195), u32(1 << 5, 1 << 3, 1 << 9, 1 << 6))
        assert b.seats()[[0, 65, 130, 195]].tolist() == [1 << 5, 1 << 3, 1 << 9, 1 << 6]


# ---- 12. the services

def _players(n, humans=()):
    return [{"name": f"P{i + 1}", "gamePlayerId": i + 1, "isBot": (i + 1) not in humans} for i in range(n)]


def _person_answers(services, thread_id, seats, n):
    """The first (seat, choice) the thread accepts, the same in every service."""
    from game_engine_amd import GeError as E
    for seat in seats:
        for c in range(1, max(n, 3) + 1):
            ok = []
            for s in services:
                try:
                    s.human_action(thread_id, seat, c)
                    ok.append(True)
                except E as e:
                    assert e.status == GE_ERR_ARG
                    ok.append(False)
            assert len(set(ok)) == 1, (thread_id, seat, c, ok)
            if ok[0]:
                return seat, c
    return None


@pytest.mark.parametrize("game,n", [("werewolf-(mafia)", 8), ("two-truths-and-a-lie", 4)])
def test_services_hand_seats_over_mid_game(game, n):
    from conftest import load_dsl
    from game_engine_amd import RoomPoolService, RoomService
    from test_strings_golden import _strip
    dsl = load_dsl(game)
    one, pool = RoomService(seed=5), RoomPoolService(seed=5, chunk_rooms=8)
    threads = ["t0", "t1", "t2", "t3"]                           # several games: what a seat gets to do depends on the game's luck
    try:
        for s in (one, pool):
            s.create_room("other", game, _players(n, (1, 3)), dsl=dsl, room_index=40)
            for k, t in enumerate(threads):
                s.create_room(t, game, _players(n, (1, 3)), dsl=dsl, room_index=41 + k)
        slots = {t: pool._rooms[t]["slot"] for t in threads}
        for t in threads:
            for _ in range(5):
                assert _strip(one.handle_message(t, "Continue")) == _strip(pool.handle_message(t, "Continue"))
                _person_answers((one, pool), t, (1, 3), n)
        for s in (one, pool):                                    # refused before anything changes
            for bad in ([0], [n + 1], [1, 2.5]):
                with pytest.raises(ValueError):
                    s.set_human_seats("t0", bad)
            with pytest.raises(ValueError):
                s.set_human_seats("nobody", [1])
            assert s._rooms["t0"]["human_seats"] == [1, 3]
        new = [2, 4]
        for t in threads:
            assert one.set_human_seats(t, new) == new and pool.set_human_seats(t, new) == new
            assert pool._rooms[t]["slot"] == slots[t] and pool._rooms[t]["chunk"].seats(slots[t], 1)[0] == 0b1010
        freed_acted = people_acted = waited = 0
        for _ in range(30):
            for t in threads:
                a, b = one.handle_message(t, "Continue"), pool.handle_message(t, "Continue")
                assert _strip(a) == _strip(b), t
                acted = int(one._rooms[t]["batch"].read_events(0, 1)[0][0]["acted_now"])
                freed_acted += bool(acted & 0b101)
                people_acted += bool(acted & 0b1010)
                w = pool.waiting()                               # after the turn, before the people answer
                assert all(set(w.get(x, [])) <= set(new) for x in threads) and set(w.get("other", [])) <= {1, 3}
                waited += bool(w.get(t))
                _person_answers((one, pool), t, new, n)
        assert not people_acted, "the policy acted for a seat that was handed to a person"
        assert freed_acted > 0, "no freed seat was ever played by the policy"
        assert waited > 0, "waiting() never named a new seat"
        # a closed thread's slot, reused by a thread of the pool's own seating, has the pool's mask again
        pool.close("t3")
        pool.create_room("u", game, _players(n, (1, 3)), dsl=dsl, room_index=50)
        assert pool._rooms["u"]["slot"] == slots["t3"] and pool._rooms["u"]["chunk"].seats(slots["t3"], 1)[0] == 0b101
        # a seat given to a person leaves the thread's playout seats
        one.create_room("p", game, _players(n, (1,)), dsl=dsl, room_index=43, playout_seats=(2, 4))
        one.set_human_seats("p", [2])
        assert one._rooms["p"]["playout_mask"] == 0b1000 and one._rooms["p"]["human_seats"] == [2]
    finally:
        one.close()
        pool.close()


# ---- 11. the Node host

NODE_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "game_engine_amd", "node")
needs_node = pytest.mark.skipif(shutil.which("node") is None or not os.path.exists(os.path.join(NODE_DIR, "ge_addon.node")),
                                reason="node or the built addon is not available")
SERVICE_SPEC = dict(seed=5, humans=[1, 3], seats=[2, 4], before=5, after=30)


def _node_batch_spec():
    rng = np.random.default_rng(8)
    rooms = rng.permutation(200)[:150]
    masks = [int(rng.integers(0, 256 if r < 130 else 16)) if k % 5 else 0 for k, r in enumerate(rooms)]
    listed = rng.permutation(200)[:90]
    return dict(rooms=rooms.tolist(), masks=masks, listed=listed.tolist(), keys=rng.integers(0, 1 << 40, 90).tolist(),
                turns=rng.integers(0, 300, 90).tolist())


def _python_batch(dsl_ww, dsl_tt, s):
    from game_engine_amd.stepper import find_want_names, pending_seats
    with RoomBatch([(GameTable(dsl_ww), 8, 130, 0b1), (GameTable(dsl_tt), 4, 70, 0b10)], seed=11, first_room=5, restart=True) as b:
        b.step(23)
        r = {"before": b.seats().tolist()}
        b.set_seats(s["rooms"], s["masks"])
        r["set"], r["window"] = b.seats().tolist(), b.seats(128, 5).tolist()
        b.clear_seats()
        r["cleared"] = b.seats().tolist()
        b.set_seats(s["rooms"], s["masks"])
        ev = b.step_rooms(s["listed"], s["keys"], s["turns"])
        r["events"] = [{f: (e[f].tolist() if f == "choice" else int(e[f])) for f in EV_FIELDS} for e in ev]
        hits, n = b.find_rooms("person")
        r["find"] = {"matched": n, "hits": [{"room": int(h["room"]), "why": find_want_names(int(h["why"])), "pending": pending_seats(h["pending"]),
                                             "phaseId": int(h["phase_id"]), "segment": int(h["segment"])} for h in hits]}
        b.step(3)
        sm = b.summary()
        r["checksum"], r["turn"] = str(int(sm["checksum"])), int(sm["turn"])
    return r


def _python_service(dsl_ww):
    from game_engine_amd import RoomPoolService, RoomService
    from test_strings_golden import _strip
    p = SERVICE_SPEC
    one, pool = RoomService(seed=p["seed"]), RoomPoolService(seed=p["seed"], chunk_rooms=4)
    log, seats = [], p["humans"]
    try:
        for s in (one, pool):
            s.create_room("t", "werewolf-(mafia)", _players(8, p["humans"]), dsl=dsl_ww, room_index=41)
        for k in range(p["before"] + p["after"]):
            if k == p["before"]:
                for s in (one, pool):
                    s.set_human_seats("t", p["seats"])
                seats = p["seats"]
            a, b = one.handle_message("t", "Continue"), pool.handle_message("t", "Continue")
            assert _strip(a["state"]) == _strip(b["state"])
            waiting = pool.waiting().get("t", [])                # after the turn, before the person answers
            ans = _person_answers((one, pool), "t", seats, 8)
            log.append({"waiting": waiting, "phase": a["state"]["current_phase_id"], "answer": list(ans) if ans else None})
    finally:
        one.close()
        pool.close()
    return log


@needs_node
def test_node_seats_calls_and_services_are_the_python_hosts(dsl_ww, dsl_tt, tmp_path):
    batch_spec = _node_batch_spec()
    want = _python_batch(dsl_ww, dsl_tt, batch_spec)
    assert want["before"] == [1] * 130 + [2] * 70 == want["cleared"] and want["set"] != want["before"] and want["find"]["hits"]
    log = _python_service(dsl_ww)
    assert any(e["answer"] for e in log[:SERVICE_SPEC["before"]]) or any(e["answer"] for e in log[SERVICE_SPEC["before"]:]), "nobody ever answered"
    spec = tmp_path / "spec.json"
    spec.write_text(json.dumps({"ww": dsl_ww, "tt": dsl_tt, "batch": batch_spec, "service": SERVICE_SPEC}))
    p = subprocess.run(["node", os.path.join(NODE_DIR, "selftest_room_seats.js"), str(spec)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    for key in want:
        assert got["batch"][key] == want[key], key
    assert got["service"] == json.loads(json.dumps(log))

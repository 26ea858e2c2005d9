"""GPU parity (-m gpu) of the lone-wavefront Werewolf x 8 turn around the two things it does once per game and no longer once
per turn (ge_device.h DEAL_WORDS, TAIL_RECYCLE / TAIL_KEEP): a prepared deal kept as the words a role assignment writes
(converted when it is dealt, when the record's 16-bit cache is loaded and when it is stored), and a fused launch whose turns know
at compile time whether they recycle finished rooms - a restart-on launch runs its last turn, which stores terminal rooms as they
are, as one peeled turn behind the recycling loop; a restart-off launch is a kernel of its own.  The tests pin behaviour, not a
build: they pass on the kernels before that as well.

  launch lengths   one step(k), k = 2 / 3 / 17 / 48, from turn 0 and from turn 17, restart on and off: the peeled turn behind a loop of
                   one, two, 16 and 47 turns, and a deal preparation (every 16th turn) on the first and on the last turn of a launch
                   (a launch of one turn is the single-turn kernel: it cannot be forced onto the fused one);
  terminal, last   restart on, the launches cut where the oracle says some room enters a terminal row on a launch's last turn: it is
                   stored terminal with its end_turn, and the next launch recycles it in front of its loop with one more game;
  restart off      64 turns from the initial state in one launch and as 3 + 13 + 48: every finished room keeps the oracle's end_turn;
  deal, launches   24 turns as 3 + 5 + 16 (the deal cache written from the word form and read back into it), and the `all`, lane and
                   `none` plans of test_gpu_lone_cold_deal.py at 64 and 65 rooms, under this file's seed and first room.
Rooms 1 / 33 / 64 / 65 / 128: a lone lane, a half-filled wavefront, a full one, one with a single valid lane, two wavefronts.  Rooms
as views, summary words and (traced: the second copy of every loop) each turn's events against the oracle.  Integer path: bit-exact."""
import functools

import numpy as np
import pytest

from conftest import load_dsl
from game_engine_amd import GameTable, RoomBatch
from parity_util import assert_summary_equal, assert_views_equal, oracle_events, oracle_rooms_as_views, views_as_oracle_rooms

pytestmark = pytest.mark.gpu
WW, N, SEED, FIRST, FUSE = "werewolf-(mafia)", 8, 0x0CE9A3E, 9001, 64
ROOMS = [1, 33, 64, 65, 128]
HORIZON = 112                                              # turns of the oracle's timeline (a game lasts about 40)
LENGTHS, STARTS = (2, 3, 17, 48), (0, 17)


@functools.lru_cache(maxsize=None)
def _timeline(n_rooms, restart):
    """The oracle's run from the initial state, turn by turn: rooms[t] / views[t] = the state after t turns (t = 0 .. HORIZON),
    events[t] = the events of turn t.  Shared by every test and trace setting, read-only."""
    from oracle.oracle import Oracle
    orc = Oracle(load_dsl(WW), N)
    cur = orc.init_rooms(n_rooms)
    rooms, views, events = [cur.copy()], [oracle_rooms_as_views(orc, cur).copy()], []
    for t in range(HORIZON):
        orc.run(cur, SEED, FIRST, t, 1, threads=0, restart=restart)
        events.append(oracle_events(orc, cur, t))
        rooms.append(cur.copy())
        views.append(oracle_rooms_as_views(orc, cur).copy())
    for a in (*rooms, *views, *events):
        a.setflags(write=False)
    return orc, rooms, views, events


def _summary(orc, rooms, turn):
    from oracle.summary import reference_summary_words
    return reference_summary_words([(orc.table, orc.n, rooms[turn])], FIRST, turn)


def _batch(n_rooms, restart, trace):
    return RoomBatch([(GameTable(load_dsl(WW)), N, n_rooms)], seed=SEED, first_room=FIRST, max_fuse=FUSE, restart=restart, trace=trace)


def _launch(b, k, ref, trace, what):
    """one step(k) - one launch for 2 <= k <= FUSE - against the timeline: events of its turns, rooms and summary behind it"""
    orc, rooms, views, events = ref
    t0 = b.turn
    b.step(k)
    if trace:
        ev = b.read_events()
        assert ev.shape == (len(views[0]), k)
        for t in range(k):
            assert ev[:, t].tobytes() == events[t0 + t].tobytes(), f"{what}: events of turn {t0 + t} (launch of {k} from {t0}) differ"
    assert_views_equal(b.read_rooms(), views[t0 + k], f"{what}: rooms behind the launch of {k} from {t0}")
    assert_summary_equal(b.summary_words(), _summary(orc, rooms, t0 + k), f"{what}: launch of {k} from {t0}")


@pytest.mark.parametrize("trace", [False, True])
@pytest.mark.parametrize("restart", [True, False])
@pytest.mark.parametrize("n_rooms", ROOMS)
def test_launch_lengths_around_the_peeled_turn(n_rooms, restart, trace):
    ref = _timeline(n_rooms, restart)
    what = f"werewolf x 8, {n_rooms} rooms, restart={restart}, trace={trace}"
    with _batch(n_rooms, restart, trace) as b:
        for start in STARTS:
            for k in LENGTHS:
                b.reset()
                if start:
                    b.step(start)
                assert b.turn == start
                _launch(b, k, ref, trace, what)


def _cut(n_rooms):
    """the first turn count T >= 3 after which some room stands in a terminal row it entered on turn T - 1 (the oracle recycles
    it on turn T: its `restarted` event), and the rooms that do"""
    _, _, views, events = _timeline(n_rooms, True)
    for T in range(3, HORIZON - 3):
        hit = np.nonzero((events[T]["restarted"] != 0) & (views[T]["end_turn"] == T - 1))[0]
        if len(hit):
            return T, hit
    raise AssertionError(f"no room of {n_rooms} enters a terminal row within {HORIZON} turns")


@pytest.mark.parametrize("trace", [False, True])
@pytest.mark.parametrize("n_rooms", ROOMS)
def test_room_that_finishes_on_a_launchs_last_turn(n_rooms, trace):
    ref = _timeline(n_rooms, True)
    orc, rooms, views, events = ref
    T, hit = _cut(n_rooms)
    assert len(hit) >= 1 and T <= 2 * FUSE - 16
    what = f"werewolf x 8, {n_rooms} rooms, cut behind turn {T - 1}, trace={trace}"
    last = min(T, 48)                                       # the launch that ends on the cut: fused, at least 3 turns
    with _batch(n_rooms, True, trace) as b:
        if T > last:
            b.step(T - last)
        _launch(b, last, ref, trace, what)
        got = b.read_rooms()
        assert (got["end_turn"][hit] == T - 1).all(), f"{what}: a room that finished on the launch's last turn is not stored terminal"
        assert (got["games"][hit] == views[T - 1]["games"][hit]).all()
        _launch(b, 3, ref, trace, what)                     # recycled in front of the loop
        got = b.read_rooms()
        assert (got["games"][hit] == views[T]["games"][hit] + 1).all(), f"{what}: the finished room was not recycled by the next launch"
        assert (got["end_turn"][hit] == views[T + 3]["end_turn"][hit]).all()
        _launch(b, 17, ref, trace, what)


@pytest.mark.parametrize("trace", [False, True])
@pytest.mark.parametrize("cuts", [(64,), (3, 13, 48)])
@pytest.mark.parametrize("n_rooms", ROOMS)
def test_restart_off_keeps_every_end_turn(n_rooms, cuts, trace):
    ref = _timeline(n_rooms, False)
    views = ref[2]
    finished = views[64]["end_turn"] >= 0
    assert 3 * int(finished.sum()) >= n_rooms, "fewer than a third of the rooms finish in 64 turns: the case checks too little"
    what = f"werewolf x 8, {n_rooms} rooms, restart off, launches {cuts}, trace={trace}"
    with _batch(n_rooms, False, trace) as b:
        for k in cuts:
            _launch(b, k, ref, trace, what)
        got = b.read_rooms()
        assert (got["end_turn"][finished] == views[64]["end_turn"][finished]).all() and (got["end_turn"][~finished] < 0).all()
        assert (got["games"] == 0).all()


@pytest.mark.parametrize("trace", [False, True])
@pytest.mark.parametrize("n_rooms", ROOMS)
def test_deal_kept_across_launches(n_rooms, trace):
    ref = _timeline(n_rooms, True)
    what = f"werewolf x 8, {n_rooms} rooms, 3 + 5 + 16, trace={trace}"
    with _batch(n_rooms, True, trace) as b:
        for k in (3, 5, 16):
            _launch(b, k, ref, trace, what)


# (rooms, who lacks a deal): the plans of tests/test_gpu_lone_cold_deal.py at 64 and 65 rooms, under this file's seed and rooms
NO_DEAL = [(64, "all"), (65, "all"), (64, 0), (64, 63), (65, 64), (64, "none"), (65, "none")]
NO_DEAL_TURNS = 48


def _no_deal_plan(n_rooms, who):
    """(turns before the rewrite, the rooms rewritten to their initial view: the room-write calls store records without a deal)"""
    return (1, list(range(n_rooms))) if who == "all" else (16, []) if who == "none" else (17, [who])


@functools.lru_cache(maxsize=None)
def _no_deal_reference(n_rooms, who):
    """the oracle from the rewritten state on: views and summary behind NO_DEAL_TURNS further turns, and each turn's events"""
    from oracle.summary import reference_summary_words
    orc, rooms, views, _ = _timeline(n_rooms, True)
    pre, rewritten = _no_deal_plan(n_rooms, who)
    v = views[pre].copy()
    v[rewritten] = views[0][rewritten]
    cur = views_as_oracle_rooms(orc, v)
    events = []
    for t in range(pre, pre + NO_DEAL_TURNS):
        orc.run(cur, SEED, FIRST, t, 1, threads=0, restart=True)
        events.append(oracle_events(orc, cur, t))
    out = oracle_rooms_as_views(orc, cur).copy()
    summary = reference_summary_words([(orc.table, orc.n, cur)], FIRST, pre + NO_DEAL_TURNS)
    for a in (out, *events):
        a.setflags(write=False)
    return out, summary, events


@pytest.mark.parametrize("trace", [False, True])
@pytest.mark.parametrize("n_rooms,who", NO_DEAL)
def test_rooms_without_a_prepared_deal(n_rooms, who, trace):
    """rooms rewritten without a deal in front of a fused launch that starts off the 16-turn grid: the word-form deal made on the
    spot (all lanes, one lane, none), and the preparation block in a later turn or the first turn of the launch"""
    views0 = _timeline(n_rooms, True)[2][0]
    want, summary, events = _no_deal_reference(n_rooms, who)
    pre, rewritten = _no_deal_plan(n_rooms, who)
    what = f"werewolf x 8, {n_rooms} rooms, no deal: {who}, trace={trace}"
    with _batch(n_rooms, True, trace) as b:
        b.step(pre)
        if rewritten:
            b.write_rooms(rewritten[0], np.ascontiguousarray(views0[rewritten]))
        b.step(NO_DEAL_TURNS)                              # one fused launch
        if trace:
            ev = b.read_events()
            assert ev.shape == (n_rooms, NO_DEAL_TURNS)
            for t in range(NO_DEAL_TURNS):
                assert ev[:, t].tobytes() == events[t].tobytes(), f"{what}: events of turn {pre + t} differ"
        assert_views_equal(b.read_rooms(), want, f"{what}, turn {pre + NO_DEAL_TURNS}")
        assert_summary_equal(b.summary_words(), summary, what)
    if rewritten:
        left = (want["phase_id"][rewritten] != views0["phase_id"][rewritten]) | (want["games"][rewritten] > 0)
        assert left.all(), "a rewritten room never left its first phase: it assigned no roles"

"""GPU parity (-m gpu) of the fused lone-wavefront Werewolf x 8 turn, which recycles a finished room where it enters its
terminal row instead of at the head of the next turn (ge_device.h WwRestart).  What that form must keep: a room that reaches
a terminal row on a launch's LAST turn is stored terminal, with end_turn set, and is recycled by the next launch's first
turn; `games` stops at 0xFFFF; the trace's `restarted` bit and target row are those of the head form.  Every room against
the oracle, every field, plus the summary words (their checksum among them).  Integer path: bit-exact."""
import numpy as np
import pytest

from conftest import load_dsl
from game_engine_amd import GameTable, RoomBatch
from parity_util import (assert_summary_equal, assert_views_equal, oracle_events, oracle_rooms_as_views)

pytestmark = pytest.mark.gpu
GAME, N, SEED, FIRST = "werewolf-(mafia)", 8, 0xC0FFEE, 4242


def _oracle(dsl, n):
    from oracle.oracle import Oracle
    return Oracle(dsl, n)


def _summary(orc, rooms, first, turn):
    from oracle.summary import reference_summary_words
    return reference_summary_words([(orc.table, orc.n, rooms)], first, turn)


def _terminal(orc, rooms):
    """rooms in a terminal phase (one without branches), as the summary reference counts `finished`"""
    return np.array([len(ph.branches) == 0 for ph in orc.table.phases])[rooms["phase"]]


@pytest.fixture(scope="module")
def dsl():
    return load_dsl(GAME)


# 4 097 rooms: 65 wavefronts, the last with one room and 63 shadow lanes; 65: a second wavefront with 63 shadow lanes
@pytest.mark.parametrize("n_rooms", [64, 65, 1000, 4097])
@pytest.mark.parametrize("fuse,plan", [(1, [45]), (2, [46, 3]), (7, [42, 7, 7]), (64, [64, 64, 13]), (200, [200, 57])])
@pytest.mark.parametrize("restart", [True, False])
def test_launch_boundaries_room_by_room(dsl, n_rooms, fuse, plan, restart):
    """Launches of `fuse` turns; after every step() every room equals the oracle's.  At the turn counts of `plan` some
    rooms sit in a terminal row exactly at a launch boundary (a game lasts ~40 turns): those are stored terminal with
    end_turn set, and with restart the next launch's first turn recycles them with one more game."""
    orc = _oracle(dsl, N)
    rooms = orc.init_rooms(n_rooms)
    turn = 0
    seen_boundary = 0
    with RoomBatch([(GameTable(dsl), N, n_rooms)], seed=SEED, first_room=FIRST, max_fuse=fuse, restart=restart) as b:
        for k in plan:
            before_games = rooms["games"].copy()
            was_terminal = _terminal(orc, rooms)
            b.step(k)
            orc.run(rooms, SEED, FIRST, turn, k, threads=0, restart=restart)
            turn += k
            got = b.read_rooms()
            assert_views_equal(got, oracle_rooms_as_views(orc, rooms), f"{n_rooms} rooms fuse={fuse} restart={restart} turn={turn}")
            assert_summary_equal(b.summary_words(), _summary(orc, rooms, FIRST, turn), f"{n_rooms} rooms fuse={fuse} turn={turn}")
            now_terminal = _terminal(orc, rooms)
            # stored terminal: the end turn is set (the oracle agrees field by field above; this pins the property itself)
            assert (got["end_turn"][now_terminal] != 0xFFFF).all()
            if restart:
                # terminal at the previous boundary -> recycled by this launch's first turn
                assert (rooms["games"][was_terminal] >= before_games[was_terminal] + 1).all()
            seen_boundary += int(now_terminal.sum())
        if restart:
            # one more turn: exactly the rooms stored terminal are recycled by it, each with one more game, none else
            was_terminal, before_games = _terminal(orc, rooms), rooms["games"].copy()
            b.step(1)
            orc.run(rooms, SEED, FIRST, turn, 1, threads=0, restart=True)
            got = b.read_rooms()
            assert_views_equal(got, oracle_rooms_as_views(orc, rooms), f"{n_rooms} rooms fuse={fuse}: the turn after a boundary")
            assert (got["games"] == before_games + was_terminal).all()
    if n_rooms >= 1000:
        assert seen_boundary > 0, "no room was terminal at a launch boundary: the plan does not test what it is for"


@pytest.mark.parametrize("n_rooms", [64, 65, 1000, 4097])
@pytest.mark.parametrize("fuse", [1, 2, 7, 64, 200])
@pytest.mark.parametrize("restart", [True, False])
def test_traced_events_and_restarted_bit(dsl, n_rooms, fuse, restart):
    """GE_FLAG_TRACE: every turn's event of every room - rows, who acted, choices and the `restarted` bit - and the states."""
    orc = _oracle(dsl, N)
    rooms = orc.init_rooms(n_rooms)
    turn, restarts = 0, 0
    with RoomBatch([(GameTable(dsl), N, n_rooms)], seed=SEED, first_room=FIRST, max_fuse=fuse, restart=restart, trace=True) as b:
        for _ in range(max(2, 56 // fuse)):
            b.step(fuse)
            ev = b.read_events()
            assert ev.shape == (n_rooms, fuse)
            for t in range(fuse):
                orc.run(rooms, SEED, FIRST, turn, 1, threads=0, restart=restart)
                want = oracle_events(orc, rooms, turn)
                assert ev[:, t].tobytes() == want.tobytes(), f"{n_rooms} rooms fuse={fuse} restart={restart}: events of turn {turn} differ"
                restarts += int(want["restarted"].sum())
                turn += 1
            assert_views_equal(b.read_rooms(), oracle_rooms_as_views(orc, rooms), f"traced, {n_rooms} rooms fuse={fuse} turn={turn}")
    if fuse * max(2, 56 // fuse) >= 50:
        assert (restarts > 0) == restart


@pytest.mark.parametrize("fuse", [7, 64])
def test_games_saturate_across_the_tail_restart(dsl, fuse):
    """Rooms written with games = 0xFFFF (and just below): recycled inside fused launches, the counter stops at 0xFFFF."""
    orc = _oracle(dsl, N)
    R = 130
    rooms = orc.init_rooms(R)
    rooms["games"] = 0xFFFF - (np.arange(R) % 3)
    rooms["games"][0] = 0xFFFF
    with RoomBatch([(GameTable(dsl), N, R)], seed=SEED, first_room=FIRST, max_fuse=fuse, restart=True) as b:
        b.write_rooms(0, oracle_rooms_as_views(orc, rooms))
        b.step(140)
        got = b.read_rooms()
        orc.run(rooms, SEED, FIRST, 0, 140, threads=0, restart=True)
        assert int(rooms["games"].min()) == 0xFFFF
        assert_views_equal(got, oracle_rooms_as_views(orc, rooms), f"saturation fuse={fuse}")
        assert_summary_equal(b.summary_words(), _summary(orc, rooms, FIRST, 140), f"saturation fuse={fuse}")


@pytest.mark.parametrize("trace", [False, True])
def test_first_phase_terminal_keeps_the_head_form(dsl, trace):
    """A table whose FIRST phase has no branch: with restart every room is recycled on every turn without ever moving, which
    only the restart block at the head of a turn does - the lone kernel keeps that loop for such tables (run_ww)."""
    import copy
    d = copy.deepcopy(dsl)
    del d["phases"]["0"]["next_phase"]
    orc = _oracle(d, N)
    R, turns = 130, 21
    rooms = orc.init_rooms(R)
    with RoomBatch([(GameTable(d), N, R)], seed=SEED, first_room=FIRST, max_fuse=7, restart=True, trace=trace) as b:
        for _ in range(turns // 7):                              # (a traced step() is one launch)
            b.step(7)
        orc.run(rooms, SEED, FIRST, 0, turns, threads=0, restart=True)
        assert int(rooms["games"].min()) == turns
        assert_views_equal(b.read_rooms(), oracle_rooms_as_views(orc, rooms), f"first phase terminal, trace={trace}")
        assert_summary_equal(b.summary_words(), _summary(orc, rooms, FIRST, turns), "first phase terminal")


def test_terminal_rooms_written_before_a_launch(dsl):
    """Rooms that are terminal when a fused launch LOADS them (stored by a launch that ended on their last turn, then written
    back through write_rooms): recycled by the first turn with restart, left alone without."""
    orc = _oracle(dsl, N)
    R = 1000
    rooms = orc.init_rooms(R)
    orc.run(rooms, SEED, FIRST, 0, 44, threads=0, restart=False)
    assert _terminal(orc, rooms).sum() > 0
    for restart in (True, False):
        ref = rooms.copy()
        with RoomBatch([(GameTable(dsl), N, R)], seed=SEED, first_room=FIRST, max_fuse=7, restart=restart) as b:
            b.write_rooms(0, oracle_rooms_as_views(orc, ref))
            b.set_turn(44)
            b.step(21)
            orc.run(ref, SEED, FIRST, 44, 21, threads=0, restart=restart)
            assert_views_equal(b.read_rooms(), oracle_rooms_as_views(orc, ref), f"terminal as loaded, restart={restart}")


def test_neighbouring_builds(dsl):
    """A Werewolf x 8 segment inside a mixed batch (the mixed kernel's lone form) and a 6-player Werewolf table (same record
    layout, fewer players), restart on, launches of 7 turns."""
    dsl_tt = load_dsl("two-truths-and-a-lie")
    tb, tt = GameTable(dsl), GameTable(dsl_tt)
    o8, o4, o6 = _oracle(dsl, 8), _oracle(dsl_tt, 4), _oracle(dsl, 6)
    R, turns = 1000, 56
    with RoomBatch([(tb, 8, R), (tt, 4, R)], seed=SEED, first_room=FIRST, max_fuse=7, restart=True) as b:
        b.step(turns)
        got = b.read_rooms()
    for orc, lo in ((o8, 0), (o4, R)):
        rooms = orc.init_rooms(R)
        orc.run(rooms, SEED, FIRST + lo, 0, turns, threads=0, restart=True)
        assert_views_equal(got[lo:lo + R], oracle_rooms_as_views(orc, rooms), f"mixed batch, segment at {lo}")
    with RoomBatch([(tb, 6, R)], seed=SEED, first_room=FIRST, max_fuse=7, restart=True) as b:
        b.step(turns)
        got = b.read_rooms()
        rooms = o6.init_rooms(R)
        o6.run(rooms, SEED, FIRST, 0, turns, threads=0, restart=True)
        assert_views_equal(got, oracle_rooms_as_views(o6, rooms), "werewolf x 6")
        assert_summary_equal(b.summary_words(), _summary(o6, rooms, FIRST, turns), "werewolf x 6")

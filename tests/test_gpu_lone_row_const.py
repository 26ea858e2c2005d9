"""GPU parity (-m gpu) of the fused lone-wavefront Werewolf x 8 turn around what it no longer works out on every turn
(ge_device.h ww_turn): constants of the table row taken from the row's derived word - and, measured beside it and not adopted
(profiles/ab_lone_row_const.txt), the slot context built by a byte permute, the lanes past a segment's end and the host-driven
players folded into one mask made in front of the turn loop, and the first queue round's result returned from every lane.  The
tests pin results, not a build: they pass on the kernels before that as well.

  rooms      64 (one full wavefront), 65 (a second wavefront with 63 lanes past the segment's end), 130 (three, the last with 2 rooms)
  launches   of 1 turn (x 3: the single-turn kernel beside the fused ones), of 17 (x 2: a deal preparation, every 16th turn, inside a
             launch, and a launch that starts off that grid) and of 256 (many recycled games; the peeled last turn behind 255)
  settings   restart on and off, traced and untraced
  people     one case with a human mask that nobody injects for: those players never act, their rooms wait
  tables     one case per Werewolf table among the committed DSLs
Against the oracle: every room's whole view, the summary words (checksum included) and, traced, every turn's events.  Integer path:
bit-exact."""
import functools
import os

import pytest

from conftest import GOLD, load_dsl
from game_engine_amd import GameTable, RoomBatch
from parity_util import assert_summary_equal, assert_views_equal, oracle_events, oracle_rooms_as_views

pytestmark = pytest.mark.gpu
WW, N, SEED, FIRST, FUSE = "werewolf-(mafia)", 8, 0x20C0257, 7300, 256
ROOMS = [64, 65, 130]
PLANS = {1: (1, 1, 1), 17: (17, 17), 256: (256,)}
HUMANS = 0b00100100                                        # players 3 and 6
PACK_WEREWOLF = 1


def _werewolf_tables():
    from oracle import dsl_table
    names = sorted(f[:-5] for f in os.listdir(os.path.join(GOLD, "dsl")) if f.endswith(".json"))
    return [g for g in names if dsl_table.compile_dsl(load_dsl(g)).pack == PACK_WEREWOLF]


@functools.lru_cache(maxsize=None)
def _timeline(game, n_rooms, restart, human_mask, horizon):
    """The oracle's run from the initial state, turn by turn: rooms[t] / views[t] = the state after t turns, events[t] = the events
    of turn t.  Computed once per setting, shared by the trace settings and launch plans, read-only."""
    from oracle.oracle import Oracle
    orc = Oracle(load_dsl(game), N)
    cur = orc.init_rooms(n_rooms)
    rooms, views, events = [cur.copy()], [oracle_rooms_as_views(orc, cur).copy()], []
    for t in range(horizon):
        orc.run(cur, SEED, FIRST, t, 1, threads=1, restart=restart, human_mask=human_mask)
        events.append(oracle_events(orc, cur, t))
        rooms.append(cur.copy())
        views.append(oracle_rooms_as_views(orc, cur).copy())
    for a in (*rooms, *views, *events):
        a.setflags(write=False)
    return orc, rooms, views, events


def _run(game, n_rooms, restart, trace, human_mask, plan, horizon=256):
    from oracle.summary import reference_summary_words
    assert sum(plan) <= horizon
    orc, rooms, views, events = _timeline(game, n_rooms, restart, human_mask, horizon)
    what = f"{game} x {N}, {n_rooms} rooms, restart={restart}, trace={trace}, humans={human_mask:#x}, launches {plan}"
    seg = (GameTable(load_dsl(game)), N, n_rooms, human_mask)
    with RoomBatch([seg], seed=SEED, first_room=FIRST, max_fuse=FUSE, restart=restart, trace=trace) as b:
        for k in plan:
            t0 = b.turn
            b.step(k)
            assert b.turn == t0 + k
            if trace:
                ev = b.read_events()
                assert ev.shape == (n_rooms, k)
                for t in range(k):
                    assert ev[:, t].tobytes() == events[t0 + t].tobytes(), f"{what}: events of turn {t0 + t} (launch of {k} from {t0}) differ"
            assert_views_equal(b.read_rooms(), views[t0 + k], f"{what}: rooms behind the launch of {k} from {t0}")
            assert_summary_equal(b.summary_words(), reference_summary_words([(orc.table, orc.n, rooms[t0 + k])], FIRST, t0 + k),
                                 f"{what}: launch of {k} from {t0}")
    return views


@pytest.mark.parametrize("k", sorted(PLANS))
@pytest.mark.parametrize("trace", [False, True])
@pytest.mark.parametrize("restart", [True, False])
@pytest.mark.parametrize("n_rooms", ROOMS)
def test_rooms_equal_the_oracle(n_rooms, restart, trace, k):
    views = _run(WW, n_rooms, restart, trace, 0, PLANS[k])
    if k == 256 and restart:
        assert int(views[256]["games"].min()) >= 3, "few recycled games: the case checks too little"
    if k == 256 and not restart:
        assert (views[256]["end_turn"] >= 0).all(), "a room is still playing after 256 turns without restart"


@pytest.mark.parametrize("trace", [False, True])
def test_host_driven_players_nobody_injects_for(trace):
    """players 3 and 6 of every room are left to people who never act: a phase that waits for one of them does not complete"""
    views = _run(WW, 65, True, trace, HUMANS, (17, 256), horizon=273)
    bots_only = _timeline(WW, 65, True, 0, 256)[2]
    assert views[256]["games"].sum() < bots_only[256]["games"].sum(), "the human mask changed nothing: the case checks too little"


@pytest.mark.parametrize("game", _werewolf_tables())
def test_every_committed_werewolf_table(game):
    _run(game, 130, True, True, 0, (17, 256), horizon=273)


def test_the_committed_werewolf_tables():
    assert WW in _werewolf_tables() and len(_werewolf_tables()) >= 2

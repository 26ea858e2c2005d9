"""GPU parity (-m gpu) of the fused lone-wavefront turn whose first queue round stands outside the loop over rounds, with the
work that does not depend on this turn's actions - the next turn's key, the prepared deal and its role words - in that round's
block (ge_device.h ww_queue_actions, PEEL).  What such a change can break: a value computed there and used a turn or a launch
later (the next-turn key across every launch boundary, a deal prepared in one launch and applied in a later one, launches that
start on and off a multiple of GE_DEAL_PERIOD = 16), the later queue rounds, which now run in a loop of their own (more than
64 due bots in a wavefront), and the copy of the turn loop that each trace setting compiles.  Every room against the oracle,
every field, plus the summary words (their checksum among them); traced: every event of every turn.  Integer path: bit-exact."""
import functools

import pytest

from conftest import load_dsl
from game_engine_amd import GameTable, RoomBatch
from parity_util import assert_summary_equal, assert_views_equal, oracle_events, oracle_rooms_as_views

pytestmark = pytest.mark.gpu
WW, TT, FIRST, FUSE = "werewolf-(mafia)", "two-truths-and-a-lie", 4242, 64
SEEDS = [0, 0xC0FFEE]
PLAN_WW8 = (16, 1, 15, 33, 64, 100)      # launches of 16 | 1 | 15 | 33 | 64 | 64 + 36 turns: boundaries at 16, 17, 32, 65, 129, 193, 229
PLAN_WW12 = (16, 17, 64)
PLAN_TT8 = (7, 64)


@functools.lru_cache(maxsize=None)
def _reference(game, n, n_rooms, seed, restart, plan):
    """The oracle's run of `plan`, turn by turn, computed once per case and shared by the trace settings: per plan entry the
    rooms as views and the summary words at its end, and every turn's events; plus the largest number of bots of the first 64
    rooms that acted in one turn (a lower bound of the bots that were due in it)."""
    from oracle.oracle import Oracle
    from oracle.summary import reference_summary_words
    orc = Oracle(load_dsl(game), n)
    rooms = orc.init_rooms(n_rooms)
    turn, steps, most = 0, [], 0
    for k in plan:
        events = []
        for _ in range(k):
            orc.run(rooms, seed, FIRST, turn, 1, threads=0, restart=restart)
            events.append(oracle_events(orc, rooms, turn))
            most = max(most, sum(bin(int(x)).count("1") for x in rooms["ev_newly"][:64]))
            turn += 1
        views = oracle_rooms_as_views(orc, rooms)
        words = reference_summary_words([(orc.table, orc.n, rooms)], FIRST, turn)
        for a in (views, words, *events):
            a.setflags(write=False)
        steps.append((views, words, events))
    return steps, most


def _run_plan(game, n, n_rooms, seed, restart, trace, plan):
    """Steps a batch through `plan` and compares it with the oracle after every entry; returns the reference's `most`."""
    steps, most = _reference(game, n, n_rooms, seed, restart, plan)
    what = f"{game} x {n}, {n_rooms} rooms, seed {seed:#x}, restart={restart}, trace={trace}"
    turn = 0
    with RoomBatch([(GameTable(load_dsl(game)), n, n_rooms)], seed=seed, first_room=FIRST, max_fuse=FUSE, restart=restart, trace=trace) as b:
        for k, (views, words, events) in zip(plan, steps):
            # untraced, step(k) cuts k into launches of at most max_fuse turns itself; a traced step() is one launch (the trace
            # holds one), so the same cuts are made here
            done = 0
            for part in ([FUSE] * (k // FUSE) + ([k % FUSE] if k % FUSE else []) if trace else [k]):
                b.step(part)
                if trace:
                    ev = b.read_events()
                    assert ev.shape == (n_rooms, part)
                    for t in range(part):
                        assert ev[:, t].tobytes() == events[done + t].tobytes(), f"{what}: events of turn {turn + done + t} differ"
                done += part
            turn += k
            assert_views_equal(b.read_rooms(), views, f"{what}, turn {turn}")
            assert_summary_equal(b.summary_words(), words, f"{what}, turn {turn}")
    return most


# 64: one full wavefront; 65: a second wavefront with 63 shadow lanes; 130: three; 32: one 64-lane block half filled
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("trace", [False, True])
@pytest.mark.parametrize("restart", [True, False])
@pytest.mark.parametrize("n_rooms", [32, 64, 65, 130])
def test_werewolf_8_launch_plan(n_rooms, restart, trace, seed):
    """From the initial state all rooms share a phase, so the first day vote puts 8 x min(n_rooms, 64) actions into one
    wavefront's queue - several rounds, the later rounds' slot read; with restart the later turns mix phases."""
    most = _run_plan(WW, 8, n_rooms, seed, restart, trace, PLAN_WW8)
    assert most > 64, f"no turn had more than 64 acting bots in the first wavefront ({most}): the queue never took a second round"


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n_rooms", [64, 65])
def test_werewolf_12_launch_plan(n_rooms, seed):
    most = _run_plan(WW, 12, n_rooms, seed, True, False, PLAN_WW12)
    assert most > 64


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n_rooms", [64, 65])
def test_two_truths_8_queue_form(n_rooms, seed):
    """The lone Two-Truths builds with five players or more queue their actions the same way (tt_turn)."""
    _run_plan(TT, 8, n_rooms, seed, True, False, PLAN_TT8)

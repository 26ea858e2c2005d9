"""GPU parity (-m gpu) of the fused lone-wavefront Werewolf x 8 turn around its action queue (ge_device.h WaveLdsPull): in the pull
form an owner stores its context once and a stamp into the head word of its first slot, and a slot finds its owner by counting
the heads up to itself - across the rounds of a long queue too.  The tests pin results, not a build: they pass on the slot form
as well.

  rooms      64, 65, 33, 1 (full, padding-lane, half-filled and one-room wavefronts; up to 32 768 rooms a fused launch runs 32 rooms per
             wavefront: the first day vote is 32 x 8 = 256 due actions, four rounds, with segments that straddle a round boundary as
             soon as someone has died) and 32 833 = 513 x 64 + 1 (64 rooms per wavefront: the same vote is 512 actions, eight rounds)
  launches   from the initial state, where every room of a wavefront is in the same phase: of 1 turn (the single-turn kernel beside
             the others), of 2 (one turn of the loop and the peeled last turn that keeps terminal rooms), of 200 (rooms recycle inside
             the loop) and 150 + 50 (the stamps are absolute turns: the second launch starts where the first stopped)
  settings   restart on; off in one case (that kernel has the queue as well); traced in one (the traced loop is a copy of its own)
  people     one case with two host-driven seats nobody injects for
  segments   one batch of two segments whose boundary falls inside a wavefront (the mixed lone kernel)
Against the oracle: every room's whole view and the summary words behind every launch and, traced, every turn's events.  Integer
path: bit-exact."""
import functools
import itertools

import pytest

from conftest import load_dsl
from game_engine_amd import GameTable, RoomBatch
from parity_util import assert_summary_equal, assert_views_equal, oracle_events, oracle_rooms_as_views

pytestmark = pytest.mark.gpu
WW, N, SEED, FIRST, FUSE = "werewolf-(mafia)", 8, 0x9011E0E, 41000, 256
ROOMS = [64, 65, 33, 1]
FULL_WAVES = 32768 + 65                                    # above the half-wave threshold, last wavefront with one room
PLANS = {"1": (1, 1, 1), "2": (2, 2, 2, 2, 2, 2), "200": (200,), "150+50": (150, 50)}
HUMANS = 0b01000010                                        # players 2 and 7


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle.oracle import Oracle
    return Oracle(load_dsl(WW), N)


@functools.lru_cache(maxsize=None)
def _timeline(n_rooms, first, restart, human_mask, horizon):
    """The oracle's run from the initial state, turn by turn: rooms[t] = the state after t turns, events[t] = the events of turn t.
    Computed once per setting, shared by the launch plans, read-only."""
    orc = _oracle()
    cur = orc.init_rooms(n_rooms)
    rooms, events = [cur.copy()], []
    for t in range(horizon):
        orc.run(cur, SEED, first, t, 1, threads=1, restart=restart, human_mask=human_mask)
        events.append(oracle_events(orc, cur, t))
        rooms.append(cur.copy())
    for a in (*rooms, *events):
        a.setflags(write=False)
    return rooms, events


@functools.lru_cache(maxsize=None)
def _checkpoints(n_rooms, first, restart, stops):
    """The same for a batch too large to keep every turn of: the states after the turns in `stops` only."""
    orc = _oracle()
    cur = orc.init_rooms(n_rooms)
    out, t = {}, 0
    for stop in stops:
        orc.run(cur, SEED, first, t, stop - t, threads=0, restart=restart)
        t = stop
        out[stop] = cur.copy()
        out[stop].setflags(write=False)
    return out


def _check(b, state, what):
    from oracle.summary import reference_summary_words
    orc = _oracle()
    assert_views_equal(b.read_rooms(), oracle_rooms_as_views(orc, state), what)
    assert_summary_equal(b.summary_words(), reference_summary_words([(orc.table, orc.n, state)], FIRST, b.turn), what)


def _run(n_rooms, plan, restart=True, trace=False, human_mask=0):
    rooms, events = _timeline(n_rooms, FIRST, restart, human_mask, 200)
    what = f"{n_rooms} rooms, restart={restart}, trace={trace}, humans={human_mask:#x}, launches {plan}"
    with RoomBatch([(GameTable(load_dsl(WW)), N, n_rooms, human_mask)], seed=SEED, first_room=FIRST, max_fuse=FUSE, restart=restart, trace=trace) as b:
        for k in plan:
            t0 = b.turn
            b.step(k)
            assert b.turn == t0 + k
            if trace:
                ev = b.read_events()
                assert ev.shape == (n_rooms, k)
                for t in range(k):
                    assert ev[:, t].tobytes() == events[t0 + t].tobytes(), f"{what}: events of turn {t0 + t} (launch of {k} from {t0}) differ"
            _check(b, rooms[t0 + k], f"{what}: behind the launch of {k} from {t0}")
    return rooms


@pytest.mark.parametrize("plan", sorted(PLANS))
@pytest.mark.parametrize("n_rooms", ROOMS)
def test_rooms_equal_the_oracle(n_rooms, plan):
    rooms = _run(n_rooms, PLANS[plan])
    if plan == "200":
        assert int(rooms[200]["games"].min()) >= 2, "few recycled games: the case checks too little"


def test_the_first_vote_fills_several_rounds():
    """what the shapes above are chosen for (the oracle alone): on an early turn every room opens its day vote at once - every living
    player is due, more than four rounds' worth in 64 rooms, and more than one round's worth act on that very turn - and by then someone
    has died in some rooms and not in others (segments of seven and of eight slots: they straddle the rounds' boundaries)"""
    rooms, events = _timeline(64, FIRST, True, 0, 200)
    acted = [int(sum(bin(int(x)).count("1") for x in e["acted_now"])) for e in events[:12]]
    t = acted.index(max(acted))
    alive = rooms[t]["p"][:, :N, 2].sum(axis=1)
    assert acted[t] > 64 and alive.sum() > 64 * 4, (acted, alive.tolist())
    assert alive.min() < alive.max() == N, alive.tolist()


@pytest.mark.parametrize("plan", ["2", "200"])
def test_wavefronts_of_64_rooms(plan):
    """above 32 768 rooms a wavefront holds 64: eight rounds on the first vote, 513 full wavefronts and one with a single room"""
    stops = tuple(itertools.accumulate(PLANS[plan]))
    want = _checkpoints(FULL_WAVES, FIRST, True, stops)
    with RoomBatch([(GameTable(load_dsl(WW)), N, FULL_WAVES)], seed=SEED, first_room=FIRST, max_fuse=FUSE, restart=True) as b:
        for k in PLANS[plan]:
            b.step(k)
            _check(b, want[b.turn], f"{FULL_WAVES} rooms, launches {PLANS[plan]}: behind turn {b.turn}")


def test_restart_off():
    rooms = _run(65, (2, 198), restart=False)
    assert (rooms[200]["end_turn"] >= 0).all(), "a room is still playing after 200 turns without restart"


def test_traced():
    _run(65, (2, 150, 48), trace=True)


def test_host_driven_seats_nobody_injects_for():
    """players 2 and 7 of every room are left to people who never act: they are never queued, and a phase that waits for one of them does not complete"""
    rooms = _run(65, (2, 198), human_mask=HUMANS)
    bots_only = _timeline(65, FIRST, True, 0, 200)[0]
    assert rooms[200]["games"].sum() < bots_only[200]["games"].sum(), "the human mask changed nothing: the case checks too little"


def test_two_segments_whose_boundary_falls_inside_a_wavefront():
    """33 + 65 Werewolf x 8 rooms as two segments of one batch (the mixed lone kernel): the first segment's only wavefront ends in lanes
    past its end, the second starts a wavefront of its own; global room indices run across the segments"""
    tb, sizes = GameTable(load_dsl(WW)), (33, 65)
    with RoomBatch([(tb, N, r) for r in sizes], seed=SEED, first_room=FIRST, max_fuse=FUSE, restart=True) as b:
        for k in (2, 150, 48):
            b.step(k)
            got, lo = b.read_rooms(), 0
            for r in sizes:
                want = _timeline(r, FIRST + lo, True, 0, 200)[0][b.turn]
                assert_views_equal(got[lo:lo + r], oracle_rooms_as_views(_oracle(), want), f"segment of {r} rooms at {lo}, behind turn {b.turn}")
                lo += r

"""GPU parity (-m gpu) of the lone-wavefront Werewolf x 8 turn around its two rare role-deal paths (ge_device.h): the deal a room
makes on the spot when it assigns roles without a prepared one (ww_apply_effect; in the tail-recycling loops behind a wave-uniform
vote), and the preparation block of every GE_DEAL_PERIOD = 16th turn (ww_prepare_deal).  Both are laid out behind the turn loop;
the tests pin behaviour, not a build: they pass on the kernels before that as well.

A room stands in front of a role assignment without a prepared deal after write_rooms() stored its initial view (the room-write
calls store records without a deal) and the fused launch that follows starts on a turn that is not a multiple of 16:
  all    a one-turn step, every room rewritten, 48 fused turns from turn 1: every lane of every wavefront deals on the spot;
  lane   17 turns (preparations at turns 0 and 16), ONE room rewritten, 48 fused turns from turn 17: the vote has one bit set -
         lane 0, lane 63, or the only valid lane of the 65th room's wavefront; the preparation of turn 32 runs in a later turn
         of the launch, and rooms recycled in these 48 turns (a game lasts about 40) take their prepared deals;
  none   16 turns, 48 fused turns from turn 16: no lane lacks its deal, and the preparation runs in the launch's first turn.
Rooms, summary words and (traced: the second copy of the loop) every turn's events against the oracle.  Integer path: bit-exact."""
import functools

import numpy as np
import pytest

from conftest import load_dsl
from game_engine_amd import GameTable, RoomBatch
from parity_util import (assert_summary_equal, assert_views_equal, oracle_events, oracle_rooms_as_views, views_as_oracle_rooms)

pytestmark = pytest.mark.gpu
WW, N, SEED, FIRST, FUSE, TURNS = "werewolf-(mafia)", 8, 0xDEA1, 7001, 64, 48
# (rooms, who lacks a deal): a lone lane, two half-filled wavefronts, a full one, one with a single valid lane, two wavefronts
CASES = [(1, "all"), (33, "all"), (64, "all"), (65, "all"), (128, "all"),
         (64, 0), (64, 63), (65, 64), (128, 0), (128, 127),
         (1, "none"), (33, "none"), (64, "none"), (65, "none"), (128, "none")]


def _plan(n_rooms, who):
    """(turns before the rewrite, the rooms rewritten)"""
    if who == "all":
        return 1, list(range(n_rooms))
    if who == "none":
        return 16, []
    return 17, [who]


@functools.lru_cache(maxsize=None)
def _reference(n_rooms, who):
    """The oracle's run of a case, shared by the trace settings: the initial views, then the rooms as views, the summary words
    and the events of each of the TURNS compared turns."""
    from oracle.oracle import Oracle
    from oracle.summary import reference_summary_words
    orc = Oracle(load_dsl(WW), N)
    rooms = orc.init_rooms(n_rooms)
    init = oracle_rooms_as_views(orc, rooms).copy()
    pre, rewritten = _plan(n_rooms, who)
    orc.run(rooms, SEED, FIRST, 0, pre, threads=0, restart=True)
    if rewritten:
        v = oracle_rooms_as_views(orc, rooms).copy()
        v[rewritten] = init[rewritten]
        rooms = views_as_oracle_rooms(orc, v)
    events = []
    for t in range(pre, pre + TURNS):
        orc.run(rooms, SEED, FIRST, t, 1, threads=0, restart=True)
        events.append(oracle_events(orc, rooms, t))
    views = oracle_rooms_as_views(orc, rooms)
    summary = reference_summary_words([(orc.table, orc.n, rooms)], FIRST, pre + TURNS)
    for a in (init, views, *events):
        a.setflags(write=False)
    return init, views, summary, events


@pytest.mark.parametrize("trace", [False, True])
@pytest.mark.parametrize("n_rooms,who", CASES)
def test_rooms_without_a_prepared_deal(n_rooms, who, trace):
    init, views, summary, events = _reference(n_rooms, who)
    pre, rewritten = _plan(n_rooms, who)
    what = f"werewolf x 8, {n_rooms} rooms, no deal: {who}, trace={trace}"
    with RoomBatch([(GameTable(load_dsl(WW)), N, n_rooms)], seed=SEED, first_room=FIRST, max_fuse=FUSE, restart=True, trace=trace) as b:
        assert_views_equal(b.read_rooms(), init, what + ": initial rooms")
        b.step(pre)
        if rewritten:
            b.write_rooms(rewritten[0], np.ascontiguousarray(init[rewritten]))
        b.step(TURNS)                                   # one fused launch
        if trace:
            ev = b.read_events()
            assert ev.shape == (n_rooms, TURNS)
            for t in range(TURNS):
                assert ev[:, t].tobytes() == events[t].tobytes(), f"{what}: events of turn {pre + t} differ"
        assert_views_equal(b.read_rooms(), views, f"{what}, turn {pre + TURNS}")
        assert_summary_equal(b.summary_words(), summary, what)
    # the cases did what they are there for: a rewritten room was dealt roles, and some room was recycled inside the launch
    if rewritten:
        left = (views["phase_id"][rewritten] != init["phase_id"][rewritten]) | (views["games"][rewritten] > 0)
        assert left.all(), "a rewritten room never left its first phase: it assigned no roles"
    if n_rooms >= 33:
        assert int(views["games"].max()) >= 1, "no room finished a game: no recycled room took a prepared deal"

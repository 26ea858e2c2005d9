"""GPU parity (-m gpu) of the lone-wavefront Werewolf x 8 turn around its vote tally and its queue results: the computed
plurality (ge_device.h plurality<8>: the byte-expanded votes and the byte-selected shift of each voter's counter) and the way a
queue slot's result comes back to its room (ww_queue_actions, both copies of the round: who acted, derived from the choice
nibbles).  The tests pin behaviour, not a build: they pass on the kernels before the byte-shift tally as well.

test_parity_through_the_lone_kernels: every room against the oracle from the initial state, at the smallest shapes that reach
every compiled copy of the turn loop (restart x trace), a second, nearly empty wavefront, a batch below a whole wavefront, 5
players (high nibbles empty) and 8 (the wrapped counter of player 8), and the mixed kernel's copy.  How many rooms the launcher
puts into a wavefront (64, or 32 for small fused batches) is its choice; the suite's knob runs force either.

test_directed_tallies: hand-written rooms in the last turn of a day vote and of a night, one case per lane.  Integer path:
bit-exact, every field."""
import functools

import numpy as np
import pytest

from conftest import load_dsl
from game_engine_amd import GameTable, RoomBatch
from game_engine_amd.stepper import ROOM_VIEW_DTYPE
from parity_util import assert_views_equal, oracle_events, oracle_rooms_as_views, views_as_oracle_rooms

pytestmark = pytest.mark.gpu
WW, TT, FIRST, FUSE = "werewolf-(mafia)", "two-truths-and-a-lie", 9001, 64
PLAN = (FUSE, FUSE, 3)                  # 2 x 64 + 3 turns from the initial state


@functools.lru_cache(maxsize=None)
def _reference(game, n, n_rooms, first, seed, restart):
    """The oracle's run of PLAN, computed once per case and shared by the trace settings: per entry the rooms as views and
    every turn's events."""
    from oracle.oracle import Oracle
    orc = Oracle(load_dsl(game), n)
    rooms = orc.init_rooms(n_rooms)
    turn, steps = 0, []
    for k in PLAN:
        events = []
        for _ in range(k):
            orc.run(rooms, seed, first, turn, 1, threads=0, restart=restart)
            events.append(oracle_events(orc, rooms, turn))
            turn += 1
        views = oracle_rooms_as_views(orc, rooms)
        for a in (views, *events):
            a.setflags(write=False)
        steps.append((views, events))
    return steps


@pytest.mark.parametrize("trace", [False, True])
@pytest.mark.parametrize("restart", [True, False])
@pytest.mark.parametrize("n", [5, 8])
@pytest.mark.parametrize("n_rooms", [64, 65, 40])
def test_parity_through_the_lone_kernels(n_rooms, n, restart, trace):
    seed = 0xBEEF
    steps = _reference(WW, n, n_rooms, FIRST, seed, restart)
    what = f"werewolf x {n}, {n_rooms} rooms, restart={restart}, trace={trace}"
    turn = 0
    with RoomBatch([(GameTable(load_dsl(WW)), n, n_rooms)], seed=seed, first_room=FIRST, max_fuse=FUSE, restart=restart, trace=trace) as b:
        for k, (views, events) in zip(PLAN, steps):
            b.step(k)
            if trace:
                ev = b.read_events()
                assert ev.shape == (n_rooms, k)
                for t in range(k):
                    assert ev[:, t].tobytes() == events[t].tobytes(), f"{what}: events of turn {turn + t} differ"
            turn += k
            assert_views_equal(b.read_rooms(), views, f"{what}, turn {turn}")
    if restart:
        assert int(steps[-1][0]["games"].max()) >= 1, "no room finished a game: the recycling form of the turn never recycled"


@pytest.mark.parametrize("restart", [True, False])
def test_parity_through_the_mixed_kernel(restart):
    """64 Werewolf x 8 + 64 Two-Truths x 4 in one batch: the mixed kernel's copy of the turn."""
    seed, R = 0xBEEF, 64
    ww = _reference(WW, 8, R, FIRST, seed, restart)
    tt = _reference(TT, 4, R, FIRST + R, seed, restart)          # rooms are keyed by their global index
    turn = 0
    with RoomBatch([(GameTable(load_dsl(WW)), 8, R), (GameTable(load_dsl(TT)), 4, R)], seed=seed, first_room=FIRST, max_fuse=FUSE, restart=restart) as b:
        for k, (vw, _), (vt, _) in zip(PLAN, ww, tt):
            b.step(k)
            turn += k
            got = b.read_rooms()
            assert_views_equal(got[:R], vw, f"mixed, restart={restart}: werewolf rooms, turn {turn}")
            assert_views_equal(got[R:], vt, f"mixed, restart={restart}: two-truths rooms, turn {turn}")


# ---- directed tallies.  Player columns of a view: 0 role (1 Villager, 2 Werewolf, 3 Doctor, 4 Detective), 1 team, 2 is_alive,
# 3 role_revealed, 4 can_vote, 5 has_secret_role, 6 night_action_eligible, 7 night_action_submitted, 8 selected_target_id,
# 9 acted in this phase visit, 10 the logged choice.  Phases: 12 the Detective's night action (the night's last; leaving it
# resolves the night: the werewolves' plurality target dies unless the highest-id living Doctor selected it), 15 the day vote
# (leaving it resolves the day: the plurality of the living voters' choices dies)
ROLES = [2, 2, 3, 4, 1, 1, 1, 1]
DAY, NIGHT = (15, 14), (12, 11)


def _room(phase, roles=ROLES):
    v = np.zeros(1, dtype=ROOM_VIEW_DTYPE)
    v["phase_id"], v["prev_phase_id"], v["phase0_done"], v["end_turn"] = phase[0], phase[1], 1, -1
    v["n_players"], v["pack"] = 8, 1
    for i, r in enumerate(roles):
        v["players"][0, i, :9] = [r, 2 if r == 2 else 1, 1, 0, 1, int(r != 1), int(r != 1), 0, 0]
    return v


def _day(votes, acted=None, dead=(), no_vote=()):
    """A day vote in its last turn: `votes` are the logged choices, `acted` who has voted (default: everyone alive who may)."""
    v = _room(DAY)
    p = v["players"][0]
    for i in dead:
        p[i, 2] = 0; p[i, 4] = 0
    for i in no_vote:
        p[i, 4] = 0
    p[:8, 10] = votes
    p[:8, 9] = [int(i not in dead and i not in no_vote) for i in range(8)] if acted is None else acted
    return v


def _night(wolf_targets, doctor_target, dead=(), roles=ROLES, stale=None):
    """The night's last phase with the Detective done: werewolf i selected wolf_targets[i]; the Doctors selected doctor_target
    (a number, or one per Doctor in seat order); `stale`: {seat: selected_target_id} written over whatever the seat holds."""
    v = _room(NIGHT, roles)
    p = v["players"][0]
    wolves = [i for i, r in enumerate(roles) if r == 2]
    docs = [i for i, r in enumerate(roles) if r == 3]
    for i, t in zip(wolves, wolf_targets):
        p[i, 7:9] = [1, t]
    for k, i in enumerate(docs):
        p[i, 7:9] = [1, doctor_target[k] if isinstance(doctor_target, (list, tuple)) else doctor_target]
    for i, r in enumerate(roles):
        if r == 4:
            p[i, 7] = 1; p[i, 9:11] = [1, 6]
    for i, t in (stale or {}).items():
        p[i, 8] = t
    for i in dead:
        p[i, 2] = 0; p[i, 4] = 0; p[i, 6] = 0
    return v


def _directed_views():
    cases = [
        ("nobody may vote, stale choices", _day([3, 3, 5, 5, 5, 8, 8, 8], acted=[0] * 8, no_vote=range(8))),
        ("nobody may vote, stale choices of players marked as acted", _day([3, 3, 5, 5, 5, 8, 8, 8], acted=[1] * 8, dead=range(2, 8))),
        ("all eight vote for player 3", _day([3] * 8)),
        ("all eight vote for player 8", _day([8] * 8)),
        ("all eight vote for player 1", _day([1] * 8)),
        ("one vote, for player 8", _day([0, 0, 8, 0, 0, 0, 0, 0], no_vote=(0, 1, 3, 4, 5, 6, 7))),
        ("tie 3 / 7: the lowest id", _day([7, 7, 7, 7, 3, 3, 3, 3])),
        ("tie 8 / 2", _day([8, 8, 8, 8, 2, 2, 2, 2])),
        ("tie 8 / 7 / 6", _day([8, 8, 7, 7, 6, 6, 1, 2])),
        ("8 wins against 7", _day([8, 8, 8, 7, 7, 6, 1, 2])),
        ("7 wins against 8", _day([8, 8, 7, 7, 7, 6, 1, 2])),
        ("stale choices of dead players outvote the living", _day([5, 5, 5, 5, 5, 2, 2, 4], acted=[1] * 8, dead=(0, 1, 2, 3, 4))),
        ("stale choices of players who may not vote", _day([8, 8, 8, 8, 6, 6, 6, 1], no_vote=(0, 1, 2, 3))),
        ("the Doctor guards the victim", _night([5, 5], 5)),
        ("the Doctor guards another player", _night([5, 5], 6)),
        ("the werewolves disagree: the lowest id, guarded", _night([6, 5], 5)),
        ("the werewolves disagree: the lowest id, the other one guarded", _night([6, 5], 6)),
        ("the victim is player 8, guarded", _night([8, 8], 8)),
        ("the victim is player 8, not guarded", _night([8, 8], 7)),
        ("a dead Doctor's stale guard", _night([5, 5], 5, dead=(2,))),
        ("a dead werewolf's stale target", _night([7, 5], 6, dead=(0,))),
        ("a Villager's stale selected target", _night([5, 5], 6, stale={6: 5, 7: 8})),
        ("two Doctors: the highest id guards", _night([5, 5], [6, 5], roles=[2, 2, 3, 4, 1, 1, 3, 1])),
        ("two Doctors: the lower one's guard does not count", _night([5, 5], [5, 6], roles=[2, 2, 3, 4, 1, 1, 3, 1])),
        ("the Doctor is the victim and guards itself", _night([3, 3], 3)),
    ]
    # every living bot due in one turn: a day vote nobody has cast yet (8 results for one room in one queue round); 11 such
    # rooms in each half of the batch put more than 64 due actions into a wavefront of 32 rooms as well as into one of 64
    fresh = _day([0] * 8, acted=[0] * 8)
    views = [c[1] for c in cases]
    rows = []
    for half in range(2):
        part = views[half::2] + [fresh] * 11
        part += [views[(3 * j + half) % len(views)] for j in range(32 - len(part))]
        rows += part[:32]
    v = np.concatenate(rows)
    assert len(v) == 64
    for half in (v[:32], v[32:]):
        due = int(((half["phase_id"] == 15)[:, None] & (half["players"][:, :8, 4] == 1) & (half["players"][:, :8, 9] == 0)).sum())
        assert due > 64, due
    return v


@pytest.mark.parametrize("restart", [True, False])
def test_directed_tallies(restart):
    from oracle.oracle import Oracle
    seed, first = 77, 123456
    orc = Oracle(load_dsl(WW), 8)
    views = _directed_views()
    rooms = views_as_oracle_rooms(orc, views)
    with RoomBatch([(GameTable(load_dsl(WW)), 8, len(views))], seed=seed, first_room=first, max_fuse=FUSE, restart=restart) as b:
        b.step(3)                                   # advance the clock: turns 3 and 4 are the ones compared
        b.write_rooms(0, views)
        assert_views_equal(b.read_rooms(), oracle_rooms_as_views(orc, rooms), "write / read of the directed views")
        before = oracle_rooms_as_views(orc, rooms)
        b.step(2)                                   # one fused launch of two turns
        orc.run(rooms, seed, first, 3, 2, threads=0, restart=restart)
        want = oracle_rooms_as_views(orc, rooms)
        assert_views_equal(b.read_rooms(), want, f"directed tallies, restart={restart}")
    # the cases did what they are there for: resolutions happened, with and without a death
    died = (before["players"][:, :8, 2] == 1) & (want["players"][:, :8, 2] == 0)
    moved = want["phase_id"] != before["phase_id"]
    if not restart:
        assert died.any(axis=1).sum() >= 16 and (moved & ~died.any(axis=1)).sum() >= 6
        assert died[:, 7].any(), "no case killed player 8"

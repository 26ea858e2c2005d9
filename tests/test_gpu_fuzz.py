"""GPU vs oracle from ARBITRARY states (-m gpu): rooms are overwritten with random — mostly
unreachable — canonical views (ge_batch_write_rooms), stepped, and compared with the oracle started
from the same views.  Catches any reliance on invariants that only hold along real games
(e.g. 'a player who has not acted has choice 0'), and the edge cases the reference's prose rules
imply: ties, empty target sets (dead Doctor / Detective), nobody alive on a team, all players dead."""
import numpy as np
import pytest

from conftest import load_dsl
from game_engine_amd import GameTable, RoomBatch
from game_engine_amd.stepper import ROOM_VIEW_DTYPE
from parity_util import assert_views_equal, oracle_rooms_as_views, views_as_oracle_rooms

pytestmark = pytest.mark.gpu


def _oracle(dsl, n, rounds=1):
    from oracle.oracle import Oracle
    return Oracle(dsl, n, rounds=rounds)


def _random_ww_views(orc, n, R, rng, consistent):
    v = np.zeros(R, dtype=ROOM_VIEW_DTYPE)
    ids = np.array(orc.ids)
    v["phase_id"] = ids[rng.integers(0, len(ids), R)]
    v["prev_phase_id"] = ids[rng.integers(0, len(ids), R)]
    v["phase0_done"] = rng.integers(0, 2, R)
    v["phase0_done"][v["phase_id"] != 0] = 1
    v["end_turn"] = -1
    v["n_players"], v["pack"] = n, 1
    p = v["players"]
    p[:, :n, 0] = rng.integers(0, 5, (R, n))                       # role class (0 = unassigned)
    # the packed model keeps ONE investigated_alignments memory per room (POLICY §3 assigns exactly one
    # Detective): keep the first Detective of each random room, demote the others
    det = p[:, :n, 0] == 4
    extra = det & (np.cumsum(det, axis=1) > 1)
    p[:, :n, 0][extra] = 1
    p[:, :n, 1] = rng.integers(0, 3, (R, n))                       # team
    if consistent:                                                 # team follows role, as the policy assigns them
        p[:, :n, 1] = np.where(p[:, :n, 0] == 2, 2, np.where(p[:, :n, 0] == 0, 0, 1))
    for f in (2, 3, 4, 5, 6, 7, 9):
        p[:, :n, f] = rng.integers(0, 2, (R, n))
    p[:, :n, 2] |= rng.integers(0, 2, (R, n)).astype(np.uint8)      # bias towards alive
    p[:, :n, 8] = rng.integers(0, n + 1, (R, n))                   # selected_target_id
    p[:, :n, 10] = rng.integers(0, n + 1, (R, n))                  # logged choice
    if consistent:
        p[:, :n, 10] *= p[:, :n, 9]                                # no choice without an action
    v["det"][:, :n] = rng.integers(0, 3, (R, n))
    return v


def _random_tt_views(orc, n, R, rng, rounds):
    v = np.zeros(R, dtype=ROOM_VIEW_DTYPE)
    ids = np.array(orc.ids)
    v["phase_id"] = ids[rng.integers(0, len(ids), R)]
    v["prev_phase_id"] = ids[rng.integers(0, len(ids), R)]
    v["phase0_done"] = 1
    v["end_turn"] = -1
    v["n_players"], v["pack"] = n, 2
    p = v["players"]
    for f in (0, 1, 3, 4, 6, 9):
        p[:, :n, f] = rng.integers(0, 2, (R, n))
    p[:, :n, 2] = rng.integers(0, 4, (R, n))
    p[:, :n, 5] = rng.integers(0, 4, (R, n))
    p[:, :n, 7] = rng.integers(0, 200, (R, n))
    p[:, :n, 8] = rng.integers(0, rounds + 1, (R, n))
    p[:, :n, 10] = rng.integers(0, 4, (R, n)) * p[:, :n, 9]
    return v


# R below / above the room count at which the launcher switches kernel builds (branch-lean vs LDS tables)
@pytest.mark.parametrize("n,consistent,R", [(8, True, 20000), (8, False, 20000), (12, True, 20000), (12, False, 20000),
                                            (4, True, 20000), (6, False, 20000), (8, False, 120000), (12, False, 110000)])
def test_werewolf_from_random_states(dsl_ww, n, consistent, R):
    seed, first = 99, 777
    rng = np.random.default_rng(n * 2 + consistent)
    orc = _oracle(dsl_ww, n)
    views = _random_ww_views(orc, n, R, rng, consistent)
    rooms = views_as_oracle_rooms(orc, views)
    with RoomBatch([(GameTable(dsl_ww), n, R)], seed=seed, first_room=first, max_fuse=3) as b:
        b.step(5)                                   # advance the clock: turns 5.. are the ones compared
        b.write_rooms(0, views)
        assert_views_equal(b.read_rooms(), oracle_rooms_as_views(orc, rooms), "write/read of random views")
        for chunk in (1, 3, 2):
            b.step(chunk)
            orc.run(rooms, seed, first, b.turn - chunk, chunk, threads=0)
            assert_views_equal(b.read_rooms(), oracle_rooms_as_views(orc, rooms), f"n={n} after turn {b.turn}")


@pytest.mark.parametrize("n,R,fuse", [(8, 20000, 1), (8, 20000, 16), (8, 150000, 1), (12, 20000, 1), (12, 120000, 8), (5, 20000, 1)])
def test_werewolf_random_states_played_on_in_steady_state(dsl_ww, n, R, fuse):
    """From random (mostly unreachable) states through whole games with recycling: single-turn launches (their own kernel
    builds; for N <= 8 they prepare role deals into the records' spare half-word) mixed with fused ones, finished rooms
    restarted from the template, roles dealt again - every block of turns against the oracle."""
    seed, first = 4242, 1 << 35
    rng = np.random.default_rng(n * 31 + R % 7 + fuse)
    orc = _oracle(dsl_ww, n)
    views = _random_ww_views(orc, n, R, rng, consistent=False)
    rooms = views_as_oracle_rooms(orc, views)
    with RoomBatch([(GameTable(dsl_ww), n, R)], seed=seed, first_room=first, max_fuse=fuse, restart=True) as b:
        b.step(3)
        b.write_rooms(0, views)
        for chunk in (1, 1, 17, 1, 40, 2, 64, 1, 33):
            b.step(chunk)
            orc.run(rooms, seed, first, b.turn - chunk, chunk, threads=0, restart=True)
            assert_views_equal(b.read_rooms(), oracle_rooms_as_views(orc, rooms), f"n={n} fuse={fuse} after turn {b.turn}")
        assert int(rooms["games"].max()) >= 2                       # rooms did finish and start again


@pytest.mark.parametrize("n,rounds", [(4, 1), (3, 2), (8, 3), (12, 2)])
def test_two_truths_from_random_states(dsl_tt, n, rounds):
    R, seed, first = 20000, 5, 1 << 40
    rng = np.random.default_rng(n + rounds)
    orc = _oracle(dsl_tt, n, rounds)
    views = _random_tt_views(orc, n, R, rng, rounds)
    rooms = views_as_oracle_rooms(orc, views)
    with RoomBatch([(GameTable(dsl_tt, rounds), n, R)], seed=seed, first_room=first, max_fuse=4) as b:
        b.step(2)
        b.write_rooms(0, views)
        for chunk in (1, 4, 1):
            b.step(chunk)
            orc.run(rooms, seed, first, b.turn - chunk, chunk, threads=0)
            assert_views_equal(b.read_rooms(), oracle_rooms_as_views(orc, rooms), f"tt n={n} after turn {b.turn}")


def _edge_case_views(n=8):
    def base(phase, prev):
        v = np.zeros(1, dtype=ROOM_VIEW_DTYPE)
        v["phase_id"], v["prev_phase_id"], v["phase0_done"], v["end_turn"] = phase, prev, 1, -1
        v["n_players"], v["pack"] = n, 1
        roles = [2, 2, 3, 4, 1, 1, 1, 1]
        for i, r in enumerate(roles):
            v["players"][0, i, :9] = [r, 2 if r == 2 else 1, 1, 0, 1, int(r != 1), int(r != 1), 0, 0]
        return v

    cases = []
    v = base(15, 14)                      # day vote complete with a 3-3 tie between players 5 and 3 -> 3 dies
    v["players"][0, :n, 9] = 1
    v["players"][0, :n, 10] = [5, 5, 5, 3, 3, 3, 6, 7]
    cases.append(("tie", v))
    v = base(12, 11)                      # detective phase done; wolves chose 5, doctor protects 5 -> nobody dies at 13
    v["players"][0, 0, 7:9] = [1, 5]; v["players"][0, 1, 7:9] = [1, 5]; v["players"][0, 2, 7:9] = [1, 5]
    v["players"][0, 3, 9:11] = [1, 6]; v["players"][0, 3, 7] = 1
    cases.append(("protected", v))
    v = base(10, 9)                       # doctor is dead: phase 11 has no target players
    v["players"][0, 2, 2] = 0; v["players"][0, 2, 4] = 0
    v["players"][0, 0, 9:11] = [1, 6]; v["players"][0, 1, 9:11] = [1, 6]
    cases.append(("dead doctor", v))
    v = base(9, 16)                       # two wolves, two villagers alive -> wolves win
    v["players"][0, 4:8, 2] = 0
    cases.append(("wolves win", v))
    v = base(9, 13)                       # no wolves alive -> village wins
    v["players"][0, :2, 2] = 0
    cases.append(("village wins", v))
    v = base(9, 13)                       # follows night -> day discussion (14)
    cases.append(("follows night", v))
    v = base(9, 16)                       # follows day -> next night (10)
    cases.append(("follows day", v))
    return np.concatenate([c[1] for c in cases])


def test_hand_built_edge_cases(dsl_ww):
    """Ties -> lowest id; protected victim survives; dead Doctor -> empty target set completes at once;
    wolves >= villagers and wolves == 0 route to phase 99; follows-day / follows-night routing."""
    n = 8
    orc = _oracle(dsl_ww, n)
    tb = GameTable(dsl_ww)
    views = _edge_case_views(n)
    cases = range(len(views))
    rooms = views_as_oracle_rooms(orc, views)
    with RoomBatch([(tb, n, len(views))], seed=1, max_fuse=1) as b:
        b.step(3)
        b.write_rooms(0, views)
        traj = []
        for t in range(3, 7):
            b.step(1)
            orc.run(rooms, 1, 0, t, 1)
            got = b.read_rooms()
            assert_views_equal(got, oracle_rooms_as_views(orc, rooms), f"turn {t}")
            traj.append(got.copy())
    first = traj[0]
    assert first["phase_id"].tolist()[:1] == [16] and first["players"][0, 2, 2] == 0 and first["players"][0, 4, 2] == 1   # tie: 3 dies, 5 lives
    assert first["phase_id"][1] == 13 and first["players"][1, :n, 2].sum() == 8                                        # protected
    assert first["phase_id"][3] == 99 and first["phase_id"][4] == 99
    assert first["phase_id"][5] == 14 and first["phase_id"][6] == 10
    assert first["end_turn"][3] == 3
    dd = [int(x["phase_id"][2]) for x in traj]
    assert 11 in dd and dd[dd.index(11) + 1] == 12 if dd.index(11) + 1 < len(dd) else True   # empty target set: one turn only


# ---- random states where the matrix above does not reach: the mixed kernel, Werewolf with absent seats of the x 12 layout
# ---- (9 - 11 players) and 5 - 7 players on the large-batch build, Two-Truths on the large-batch build and in single-turn
# ---- launches, the draft DSL's bound fields, host-driven seats with batched injection, the event trace.  Every room
# ---- against the oracle after every block of turns, and the summary (checksum included) against the host reference.

def _summary_ref(parts, first, turn):
    from oracle.summary import reference_summary_words
    return reference_summary_words([(orc.table, orc.n, rooms) for orc, rooms in parts], first, turn)


def _random_views(orc, n, R, rng):
    if orc.table.pack == 1:
        return _random_ww_views(orc, n, R, rng, consistent=bool(R % 2))
    return _random_tt_views(orc, n, R, rng, rounds=1)


def _play_blocks(b, parts, seed, first, chunks, restart, what):
    """Steps `b` by each chunk and the oracle with it; every room and the summary compared after each block."""
    from parity_util import assert_summary_equal
    for chunk in chunks:
        b.step(chunk)
        base = 0
        for orc, rooms in parts:
            orc.run(rooms, seed, first + base, b.turn - chunk, chunk, threads=0, restart=restart)
            assert_views_equal(b.read_rooms(base, len(rooms)), oracle_rooms_as_views(orc, rooms),
                               f"{what}: x{orc.n} segment at {base}, turn {b.turn}")
            base += len(rooms)
        assert_summary_equal(b.summary_words(), _summary_ref(parts, first, b.turn), f"{what}: turn {b.turn}")


@pytest.mark.parametrize("fuse", [1, 16])
@pytest.mark.parametrize("sizes", [(3001, 2999, 3037, 2903), (20011, 17003, 16411, 15013)])   # total below / above 65 536
def test_mixed_batch_from_random_states(dsl_ww, dsl_tt, sizes, fuse):
    """The mixed kernel (one launch for Werewolf x 6, Two-Truths x 4, Werewolf x 10, Two-Truths x 7), steady state."""
    seed, first = 31337, (1 << 34) + 5
    games = [(dsl_ww, 6), (dsl_tt, 4), (dsl_ww, 10), (dsl_tt, 7)]
    rng = np.random.default_rng(sum(sizes) + fuse)
    parts, segs = [], []
    for (dsl, n), R in zip(games, sizes):
        orc = _oracle(dsl, n)
        views = _random_views(orc, n, R, rng)
        parts.append((orc, views_as_oracle_rooms(orc, views)))
        segs.append(((GameTable(dsl), n, R), views))
    with RoomBatch([s for s, _ in segs], seed=seed, first_room=first, max_fuse=fuse, restart=True) as b:
        b.step(4)
        base = 0
        for (_, _, R), views in segs:
            b.write_rooms(base, views)
            base += R
        _play_blocks(b, parts, seed, first, (1, 1, 16, 2, 33), True, f"mixed {sizes} fuse {fuse}")
        assert b.summary()["games_recycled"] > 0


@pytest.mark.parametrize("n,R,fuse", [(5, 3000, 1), (7, 3000, 16), (7, 90000, 1), (9, 3000, 1), (10, 3000, 16),
                                      (10, 90000, 8), (11, 3000, 1)])
def test_werewolf_player_counts_from_random_states(dsl_ww, n, R, fuse):
    """Werewolf with absent seats: x 5 / x 7 in the x 8 layout, x 9 - x 11 in the x 12 layout; both builds for 7 and 10."""
    seed, first = 4243, 1 << 37
    rng = np.random.default_rng(n * 13 + R + fuse)
    orc = _oracle(dsl_ww, n)
    views = _random_ww_views(orc, n, R, rng, consistent=False)
    parts = [(orc, views_as_oracle_rooms(orc, views))]
    with RoomBatch([(GameTable(dsl_ww), n, R)], seed=seed, first_room=first, max_fuse=fuse, restart=True) as b:
        b.step(3)
        b.write_rooms(0, views)
        _play_blocks(b, parts, seed, first, (1, 17, 1, 40), True, f"werewolf x{n} {R} rooms fuse {fuse}")


@pytest.mark.parametrize("n,fuse", [(4, 1), (4, 8), (7, 8)])
def test_two_truths_large_batch_from_random_states(dsl_tt, n, fuse):
    """The shipped Two-Truths table on the large-batch build, single-turn launches and fused ones."""
    R, seed, first = 150000, 6, 1 << 41
    rng = np.random.default_rng(n * 3 + fuse)
    orc = _oracle(dsl_tt, n)
    views = _random_tt_views(orc, n, R, rng, 1)
    parts = [(orc, views_as_oracle_rooms(orc, views))]
    with RoomBatch([(GameTable(dsl_tt), n, R)], seed=seed, first_room=first, max_fuse=fuse, restart=True) as b:
        b.step(2)
        b.write_rooms(0, views)
        _play_blocks(b, parts, seed, first, (1, 8, 1, 16), True, f"two-truths x{n} fuse {fuse}")


def _random_draft_views(orc, n, R, rng):
    """Random states of the reference's draft Werewolf DSL: the slots it declares (through its own field names) take random
    values; the slots it does not declare (has_secret_role, night_action_submitted, selected_target_id) keep what the
    template gives every room, as they would in a real game of this DSL."""
    from parity_util import oracle_rooms_as_views as as_views
    v = _random_ww_views(orc, n, R, rng, consistent=False)
    init = as_views(orc, orc.init_rooms(1))[0]
    slots = ("role", "team", "is_alive", "role_revealed", "can_vote", "has_secret_role", "night_action_eligible",
             "night_action_submitted", "selected_target_id")
    for col, slot in enumerate(slots):
        if not orc.table.declared(slot):
            v["players"][:, :n, col] = init["players"][:n, col]
    if not orc.table.declared("investigated_alignments"):
        v["det"][:] = 0
    return v


@pytest.mark.parametrize("n,fuse", [(8, 1), (11, 16)])
def test_draft_werewolf_from_random_states(n, fuse):
    from conftest import load_dsl
    dsl = load_dsl("draft-werewolf-(mafia)")
    R, seed, first = 6000, 12, 999
    orc = _oracle(dsl, n)
    assert not orc.table.declared("selected_target_id")             # the binding the builder respects
    views = _random_draft_views(orc, n, R, np.random.default_rng(n + fuse))
    parts = [(orc, views_as_oracle_rooms(orc, views))]
    with RoomBatch([(GameTable(dsl), n, R)], seed=seed, first_room=first, max_fuse=fuse, restart=True) as b:
        b.step(1)
        b.write_rooms(0, views)
        _play_blocks(b, parts, seed, first, (1, 16, 1, 16), True, f"draft werewolf x{n} fuse {fuse}")


@pytest.mark.parametrize("game,n,mask", [("werewolf-(mafia)", 8, 0b10000001), ("werewolf-(mafia)", 11, 0b10000000101),
                                         ("two-truths-and-a-lie", 5, 0b11)])
def test_host_driven_seats_from_random_states(game, n, mask):
    """Random states with host-driven seats: batched injection (ge_batch_inject_actions) of random actions between
    single-turn launches, accepted / refused exactly as Oracle.inject decides, then every room and the summary."""
    from conftest import load_dsl
    dsl = load_dsl(game)
    R, seed, first = 2000, 8, 1 << 30
    rng = np.random.default_rng(n + mask)
    orc = _oracle(dsl, n)
    views = _random_views(orc, n, R, rng)
    rooms = views_as_oracle_rooms(orc, views)
    human = [i + 1 for i in range(n) if (mask >> i) & 1]
    accepted = refused = 0
    with RoomBatch([(GameTable(dsl), n, R, mask)], seed=seed, first_room=first, max_fuse=1) as b:
        b.step(2)
        b.write_rooms(0, views)
        for t in range(12):
            rs = np.sort(rng.choice(R, size=600, replace=False)).astype(np.uint64)
            pl = rng.choice(human, size=len(rs)).astype(np.uint32)
            ch = rng.integers(0, n + 2, len(rs)).astype(np.uint32)
            status = b.inject_actions(rs, pl, ch)
            for k in range(len(rs)):
                ok = orc.inject(rooms, int(rs[k]), int(pl[k]), int(ch[k]))
                assert ok == (status[k] == 0), (t, int(rs[k]), int(pl[k]), int(ch[k]), int(status[k]))
                accepted += ok
                refused += not ok
            b.step(1)
            orc.run(rooms, seed, first, b.turn - 1, 1, threads=0, human_mask=mask)
            assert_views_equal(b.read_rooms(), oracle_rooms_as_views(orc, rooms), f"{game} x{n} turn {b.turn}")
        from parity_util import assert_summary_equal
        assert_summary_equal(b.summary_words(), _summary_ref([(orc, rooms)], first, b.turn), f"{game} x{n} host-driven")
    assert accepted > 100 and refused > 100


@pytest.mark.parametrize("game,n,R", [("werewolf-(mafia)", 8, 3000), ("werewolf-(mafia)", 10, 70001),
                                      ("two-truths-and-a-lie", 4, 3000), ("two-truths-and-a-lie", 9, 70001)])
def test_event_trace_from_random_states(game, n, R):
    """trace=True from random states: every turn's events (read_events) == the oracle's record of that turn."""
    from conftest import load_dsl
    from parity_util import oracle_events
    dsl = load_dsl(game)
    seed, first = 515, 1 << 20
    orc = _oracle(dsl, n)
    views = _random_views(orc, n, R, np.random.default_rng(n * R))
    rooms = views_as_oracle_rooms(orc, views)
    with RoomBatch([(GameTable(dsl), n, R)], seed=seed, first_room=first, max_fuse=16, restart=True, trace=True) as b:
        b.step(1)
        b.write_rooms(0, views)
        for chunk in (1, 16, 5):
            b.step(chunk)
            ev = b.read_events()
            assert ev.shape == (R, chunk)
            for k in range(chunk):
                t = b.turn - chunk + k
                orc.run(rooms, seed, first, t, 1, threads=0, restart=True)
                want, got = oracle_events(orc, rooms, t), np.ascontiguousarray(ev[:, k])
                for f in ("turn", "from_phase_id", "to_phase_id", "acted_now", "restarted", "choice"):
                    assert (got[f] == want[f]).all(), (game, n, f, t)
            assert_views_equal(b.read_rooms(), oracle_rooms_as_views(orc, rooms), f"{game} x{n} traced, turn {b.turn}")

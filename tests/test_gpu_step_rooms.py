"""ge_batch_step_rooms / ge_batch_read_rooms_at (-m gpu): a chosen set of rooms moved by one turn, each under its own RNG key
and turn number, against the oracle stepping the same state under that key and turn - from fuzzed states, over many turns
with role deals in play, beside ordinary batch steps, and refusals that must leave every record as it was."""
import numpy as np
import pytest

from conftest import load_dsl
from game_engine_amd import GameTable, GeError, RoomBatch
from oracle import dsl_variants
from oracle.oracle import Oracle
from parity_util import assert_views_equal, oracle_events, oracle_rooms_as_views, raw_records, views_as_oracle_rooms
from test_gpu_fuzz import _random_draft_views, _random_tt_views, _random_ww_views

pytestmark = pytest.mark.gpu

GE_ERR_ARG, GE_ERR_RANGE = -1, -6
WORDS = {(1, False): 8, (1, True): 10, (2, 4): 6, (2, 8): 8, (2, 12): 12}
EV_FIELDS = ("turn", "from_phase_id", "to_phase_id", "acted_now", "restarted", "choice")


def _words(orc):
    if orc.table.pack == 1:
        return WORDS[(1, orc.n > 8)]
    return WORDS[(2, 4 if orc.n <= 4 else 8 if orc.n <= 8 else 12)]


def _views(orc, game, R, rng):
    if game == "draft":
        return _random_draft_views(orc, orc.n, R, rng)
    if orc.table.pack == 1:
        return _random_ww_views(orc, orc.n, R, rng, consistent=bool(R % 2))
    return _random_tt_views(orc, orc.n, R, rng, rounds=1)


def _dsl(game):
    if game == "ww":
        return load_dsl("werewolf-(mafia)")
    if game == "tt":
        return load_dsl("two-truths-and-a-lie")
    if game == "draft":
        return load_dsl("draft-werewolf-(mafia)")
    if game == "ww_generic":
        return dsl_variants.build("ww_generic", load_dsl("werewolf-(mafia)"))
    return dsl_variants.build("tt_generic", load_dsl("two-truths-and-a-lie"))


def _raw(b, parts):
    return [raw_records(b, s, len(rooms), _words(orc)) for s, (orc, rooms) in enumerate(parts)]


def _oracle_step(orc, rooms, i, seed, key, turn, restart, mask):
    """room i of `rooms` (an oracle ROOM_DTYPE array) one turn under global room `key` at `turn`; returns its event"""
    one = rooms[i:i + 1]
    orc.run(one, seed, key, turn, 1, threads=1, restart=restart, human_mask=mask)
    return oracle_events(orc, one, turn)[0]


CASES = [[("ww", 4, 0)], [("ww", 8, 0)], [("ww", 12, 0)], [("tt", 3, 0)], [("tt", 4, 0)], [("tt", 12, 0)],
         [("draft", 8, 0)], [("ww_generic", 8, 0)], [("tt_generic", 5, 0)],
         [("ww", 8, 0b10000001)], [("tt", 4, 0b0011)], [("ww", 12, 0b100000000101)],
         [("ww", 6, 0), ("tt", 4, 0b10), ("ww", 10, 0), ("tt", 7, 0)]]


def _case_id(g):
    return "+".join(f"{n}x{k}" + (f"h{m:x}" if m else "") for n, k, m in g)


@pytest.mark.parametrize("restart", [False, True])
@pytest.mark.parametrize("games", CASES, ids=_case_id)
def test_step_rooms_matches_the_oracle_under_each_key_and_turn(games, restart):
    rng = np.random.default_rng(sum(k * 7 + m for _, k, m in games) + restart)
    sizes = [int(rng.integers(300, 700)) for _ in games]
    _check_step_rooms(games, restart, rng, sizes, sum(sizes) // 3)


# the GENERIC builds of the twelve-seat layouts, which no case above launches: 65 entries - a full wavefront and one live lane
@pytest.mark.parametrize("games", [[("ww_generic", 12, 0b100000000100)], [("tt_generic", 9, 0b100000001)]], ids=_case_id)
def test_step_rooms_generic_tables_of_twelve_seats(games):
    _check_step_rooms(games, True, np.random.default_rng(12), [97], 65)


def _check_step_rooms(games, restart, rng, sizes, n_listed):
    seed = 0xB0B0 + len(games)
    parts, segs = [], []
    for (game, n, mask), R in zip(games, sizes):
        dsl = _dsl(game)
        orc = Oracle(dsl, n)
        views = _views(orc, game, R, rng)
        parts.append((orc, views_as_oracle_rooms(orc, views)))
        segs.append(((GameTable(dsl), n, R, mask), views, mask))
    total = sum(sizes)
    with RoomBatch([s for s, _, _ in segs], seed=seed, first_room=12345, max_fuse=1, restart=restart) as b:
        b.step(3)
        base = 0
        for (_, _, R, _), views, _ in segs:
            b.write_rooms(base, views)
            base += R
        turn_before = b.turn
        for rnd in range(3):
            before = _raw(b, parts)
            chosen = rng.choice(total, size=n_listed, replace=False)            # a random subset, in shuffled order
            keys = rng.choice(1 << 40, size=len(chosen), replace=False).astype(np.uint64)
            keys[: len(keys) // 2] = rng.integers(0, 1 << 20, len(keys) // 2)   # keys below and above 2^32
            keys[0], keys[1] = (1 << 32) - 1, (1 << 47) + 3
            turns = rng.integers(0, 0xFFFFFFFF, len(chosen), dtype=np.uint64).astype(np.uint32)
            turns[:3] = [0, 0xFFFFFFFE, 1]
            turns[3: 3 + len(turns) // 3] = rng.integers(0, 200, len(turns) // 3)
            if len(set(keys.tolist())) != len(keys):
                keys = np.arange(len(keys), dtype=np.uint64) * 7919 + (1 << 33)
            ev = b.step_rooms(chosen, keys, turns)
            assert b.turn == turn_before
            base, listed = 0, set(chosen.tolist())
            for s, ((orc, rooms), (_, _, mask)) in enumerate(zip(parts, segs)):
                for k, r in enumerate(chosen):
                    if base <= r < base + len(rooms):
                        want = _oracle_step(orc, rooms, int(r) - base, seed, int(keys[k]), int(turns[k]), restart, mask)
                        for f in EV_FIELDS:
                            assert np.array_equal(ev[k][f], want[f]), (games, rnd, int(r), f, ev[k][f], want[f])
                assert_views_equal(b.read_rooms(base, len(rooms)), oracle_rooms_as_views(orc, rooms), f"{games} round {rnd} segment {s}")
                after = raw_records(b, s, len(rooms), _words(orc))
                unlisted = [i for i in range(len(rooms)) if base + i not in listed]
                assert np.array_equal(after[unlisted], before[s][unlisted]), f"{games}: an unlisted room's record changed"
                base += len(rooms)


@pytest.mark.parametrize("n", [12, 8])
def test_many_turns_each_room_on_its_own_clock(dsl_ww, n):
    """256 rooms, each with its own key; 200 calls step random subsets; every room ends as the oracle run of its key from turn
    0 over its own number of turns - role deals (dealt on the spot, never from a cache of another key) on both record forms."""
    R, seed = 256, 77
    rng = np.random.default_rng(n)
    orc = Oracle(dsl_ww, n)
    keys = rng.choice(1 << 44, size=R, replace=False).astype(np.uint64)
    turn = np.zeros(R, dtype=np.uint32)
    with RoomBatch([(GameTable(dsl_ww), n, R)], seed=seed, first_room=0, max_fuse=1, restart=True) as b:
        b.step(16)                                  # the slots' own prepared deals (batch key) fill the side plane (x 12)
        b.write_rooms(0, oracle_rooms_as_views(orc, orc.init_rooms(R)))
        for _ in range(200):
            sub = rng.choice(R, size=int(rng.integers(1, R + 1)), replace=False)
            b.step_rooms(sub, keys[sub], turn[sub])
            turn[sub] += 1
        got = b.read_rooms()
    assert int(turn.min()) > 20
    for i in range(R):
        rooms = orc.init_rooms(1)
        orc.run(rooms, seed, int(keys[i]), 0, int(turn[i]), threads=1, restart=True)
        assert_views_equal(got[i:i + 1], oracle_rooms_as_views(orc, rooms), f"x{n} room {i} after {int(turn[i])} turns")
    assert int(got["games"].max()) >= 1


def test_ordinary_steps_around_indexed_steps_stay_exact(dsl_ww):
    """step(64) -> step_rooms under other keys -> step(64): both segments equal the oracle (deal hygiene)."""
    seed, first, sizes = 4040, 1 << 36, (700, 500)
    parts = [(Oracle(dsl_ww, 8), sizes[0]), (Oracle(dsl_ww, 12), sizes[1])]
    rooms = [orc.init_rooms(R) for orc, R in parts]
    rng = np.random.default_rng(5)
    with RoomBatch([(GameTable(dsl_ww), 8, sizes[0]), (GameTable(dsl_ww), 12, sizes[1])], seed=seed, first_room=first,
                   max_fuse=1, restart=True) as b:
        b.step(64)
        for (orc, _), r, base in zip(parts, rooms, (0, sizes[0])):
            orc.run(r, seed, first + base, 0, 64, threads=0, restart=True)
        chosen = rng.choice(sum(sizes), size=600, replace=False)
        keys = rng.choice(1 << 40, size=600, replace=False).astype(np.uint64)
        turns = rng.integers(0, 100, 600).astype(np.uint32)
        for rep in range(3):
            b.step_rooms(chosen, keys, turns + rep)
            for k, c in enumerate(chosen):
                s = 0 if c < sizes[0] else 1
                i = int(c) - (0 if s == 0 else sizes[0])
                _oracle_step(parts[s][0], rooms[s], i, seed, int(keys[k]), int(turns[k]) + rep, True, 0)
        b.step(64)
        for (orc, _), r, base in zip(parts, rooms, (0, sizes[0])):
            orc.run(r, seed, first + base, 64, 64, threads=0, restart=True)
            assert_views_equal(b.read_rooms(base, len(r)), oracle_rooms_as_views(orc, r), f"x{orc.n} after step / step_rooms / step")


def test_refusals_change_nothing(dsl_ww, dsl_tt):
    with RoomBatch([(GameTable(dsl_ww), 8, 300), (GameTable(dsl_tt), 4, 200)], seed=1, max_fuse=1) as b:
        b.step(7)
        before = [raw_records(b, 0, 300, 8), raw_records(b, 1, 200, 6)]
        turn = b.turn
        bad = [([1, 2, 1], [1, 2, 3], [0, 0, 0], GE_ERR_ARG),
               ([1, 500, 3], [1, 2, 3], [0, 0, 0], GE_ERR_RANGE),
               ([1, 2, 3], [1, 2, 3], [0, 0xFFFFFFFF, 0], GE_ERR_RANGE)]
        for rooms, keys, turns, status in bad:
            with pytest.raises(GeError) as e:
                b.step_rooms(rooms, keys, turns)
            assert e.value.status == status
            assert np.array_equal(raw_records(b, 0, 300, 8), before[0]) and np.array_equal(raw_records(b, 1, 200, 6), before[1])
        assert len(b.step_rooms([], [], [])) == 0
        assert np.array_equal(raw_records(b, 0, 300, 8), before[0]) and np.array_equal(raw_records(b, 1, 200, 6), before[1])
        assert b.turn == turn
        with pytest.raises(GeError) as e:
            b.read_rooms_at([0, 500])
        assert e.value.status == GE_ERR_RANGE


def test_read_rooms_at_is_read_rooms_gathered(dsl_ww, dsl_tt):
    sizes = (333, 257, 129, 64)
    segs = [(GameTable(dsl_ww), 8, sizes[0]), (GameTable(dsl_tt), 4, sizes[1]), (GameTable(dsl_ww), 11, sizes[2]),
            (GameTable(dsl_tt), 9, sizes[3])]
    rng = np.random.default_rng(3)
    with RoomBatch(segs, seed=9, max_fuse=4, restart=True) as b:
        b.step(37)
        full = b.read_rooms()
        idx = rng.integers(0, sum(sizes), 2000)                               # any order, repeats
        got = b.read_rooms_at(idx)
        assert got.tobytes() == full[idx].tobytes()
        assert len(b.read_rooms_at([])) == 0

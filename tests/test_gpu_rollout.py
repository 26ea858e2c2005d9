"""ge_batch_rollout_rooms (-m gpu): playouts of listed rooms against the oracle playing R copies of each under keys[k] + r,
against the composition it is defined by (a fresh batch of R copies: write_rooms + set_turn + step + summary), read-only on the
source batch, refusals that leave the output untouched, 2^20 playouts word for word, and determinism."""
import numpy as np
import pytest

from conftest import load_dsl
from game_engine_amd import GameTable, GeError, RoomBatch
from game_engine_amd.stepper import rollout_to_dict
from oracle import dsl_variants
from oracle.oracle import Oracle
from parity_util import assert_views_equal, oracle_batch, raw_records, views_as_oracle_rooms
from rollout_ref import reference_rollout
from test_gpu_fuzz import _random_draft_views, _random_tt_views, _random_ww_views

pytestmark = pytest.mark.gpu

GE_ERR_ARG, GE_ERR_RANGE = -1, -6
WORDS = {(1, False): 8, (1, True): 10, (2, 4): 6, (2, 8): 8, (2, 12): 12}


def _words(orc):
    if orc.table.pack == 1:
        return WORDS[(1, orc.n > 8)]
    return WORDS[(2, 4 if orc.n <= 4 else 8 if orc.n <= 8 else 12)]


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


def _views(orc, game, R, rng):
    if game == "draft":
        return _random_draft_views(orc, orc.n, R, rng)
    if orc.table.pack == 1:
        return _random_ww_views(orc, orc.n, R, rng, consistent=bool(R % 2))
    return _random_tt_views(orc, orc.n, R, rng, rounds=1)


def _source(games, rng, R=24):
    """A batch created WITH a human mask and GE_FLAG_RESTART (both must be ignored), of fuzzed views; its oracle rooms."""
    parts, segs = [], []
    for game, n in games:
        dsl = _dsl(game)
        orc = Oracle(dsl, n)
        views = _views(orc, game, R, rng)
        parts.append((orc, views_as_oracle_rooms(orc, views)))
        segs.append(((GameTable(dsl), n, R, 0b101), views))
    b = RoomBatch([s for s, _ in segs], seed=0xFEED, first_room=77, max_fuse=1, restart=True)
    for k, (_, views) in enumerate(segs):
        b.write_rooms(k * R, views)
    return b, parts, R


def _expected(parts, R_src, rooms, keys, turns, n_rollouts, max_turns, seed, threads=1):
    out = []
    for room, key, turn in zip(rooms, keys, turns):
        orc, orooms = parts[int(room) // R_src]
        out.append(reference_rollout(orc, orooms[int(room) % R_src].copy(), seed, int(key), int(turn), n_rollouts, max_turns, threads))
    return np.stack(out)


def _assert_words(got, want, what):
    for k in range(len(want)):
        if not (got[k] == want[k]).all():
            bad = np.nonzero(got[k] != want[k])[0]
            raise AssertionError(f"{what}: entry {k} words {bad.tolist()} got {got[k][bad].tolist()} want {want[k][bad].tolist()}")


CASES = [[("ww", 4)], [("ww", 8)], [("ww", 12)], [("tt", 3)], [("tt", 4)], [("tt", 8)], [("tt", 12)],
         [("draft", 8)], [("ww_generic", 8)], [("tt_generic", 5)], [("ww", 6), ("tt", 4), ("ww", 10), ("tt", 7)]]
RM = [(1, 9), (63, 600), (64, 1), (65, 600), (300, 0), (300, 600)]


@pytest.mark.parametrize("games", CASES, ids=lambda g: "+".join(f"{n}x{k}" for n, k in g))
def test_rollouts_match_the_oracle(games):
    rng = np.random.default_rng(sum(k * 13 for _, k in games) + len(games))
    b, parts, R_src = _source(games, rng)
    total = R_src * len(games)
    # a terminal source where the fuzz made one (else the last room), repeats, one key that wraps past 2^64
    terminal = [i for i in range(total) if len(parts[i // R_src][0].table.phases[int(parts[i // R_src][1][i % R_src]["phase"])].branches) == 0]
    rooms = [0, 3, 3, total - 1, terminal[0] if terminal else total - 2] + [int(x) for x in rng.integers(0, total, 3)]
    keys = [12345, 2 ** 64 - 40, 999, int(rng.integers(0, 2 ** 62)), 5, 6, 7, 1 << 48]
    turns = [0, 17, 5, 1000, 3, 40000, 2, 9]
    for R, M in RM:
        seed = 0xABC0 + R + M
        got = b.rollout_rooms(rooms, keys, turns, R, M, seed=seed)
        want = _expected(parts, R_src, rooms, keys, turns, R, M, seed)
        _assert_words(got, want, f"{games} R={R} M={M}")
    b.close()


LAYOUTS = [("ww", 8), ("ww", 12), ("tt", 4), ("tt", 8), ("tt", 12), ("ww_generic", 8), ("tt_generic", 5)]


@pytest.mark.parametrize("game,n", LAYOUTS)
def test_rollout_equals_the_composition(game, n):
    """summary words == summary_words() of B' (R copies, first_room = key, set_turn, step(M)) on the GPU."""
    rng = np.random.default_rng(n * 31)
    b, parts, R_src = _source([(game, n)], rng)
    dsl = _dsl(game)
    R, M, key, turn, seed = 200, 300, 4242, 11, 0x51
    for room in (1, 7):
        got = b.rollout_rooms([room], [key], [turn], R, M, seed=seed)[0]
        view = b.read_rooms(room, 1)
        with RoomBatch([(GameTable(dsl), n, R, 0)], seed=seed, first_room=key) as c:
            c.write_rooms(0, np.repeat(view, R))
            c.set_turn(turn)
            c.step(M)
            want = c.summary_words()
        assert (got[:41] == want).all(), (game, n, room, np.nonzero(got[:41] != want)[0].tolist())
    b.close()


def test_rollout_reads_only():
    rng = np.random.default_rng(3)
    games = [("ww", 8), ("tt", 4), ("ww", 12), ("tt", 12)]
    parts, segs = [], []
    for game, n in games:
        orc = Oracle(_dsl(game), n)
        segs.append((GameTable(_dsl(game)), n, 40, 0b1))
        parts.append(orc)
    with RoomBatch(segs, seed=9, first_room=5, max_fuse=3, restart=True, trace=True) as b:
        b.step(3)
        before = [raw_records(b, s, 40, _words(orc)) for s, orc in enumerate(parts)]
        turn, ev = b.turn, b.read_events()
        b.rollout_rooms([0, 41, 85, 159, 0], [1, 2, 3, 4, 5], [0, 9, 7, 3, 100], 130, 200)
        after = [raw_records(b, s, 40, _words(orc)) for s, orc in enumerate(parts)]
        assert all((x == y).all() for x, y in zip(before, after))
        assert b.turn == turn and (b.read_events() == ev).all()


def test_rollout_leaves_the_werewolf12_side_plane_alone():
    """Prepared deals (the x 12 side plane) in play, a rollout between steps: the rooms stay equal to the oracle and to a twin."""
    dsl = load_dsl("werewolf-(mafia)")
    tb = GameTable(dsl)
    orc = Oracle(dsl, 12)
    n, seed, first = 256, 0x12, 1000
    with RoomBatch([(tb, 12, n)], seed=seed, first_room=first, max_fuse=1, restart=True) as a, \
            RoomBatch([(tb, 12, n)], seed=seed, first_room=first, max_fuse=1, restart=True) as twin:
        a.step(40)
        twin.step(40)
        a.rollout_rooms(list(range(0, n, 5)), list(range(0, n, 5)), [40] * len(range(0, n, 5)), 64, 300)
        a.step(160)
        twin.step(160)
        got = a.read_rooms()
        assert_views_equal(got, twin.read_rooms(), "twin")
        assert_views_equal(got, oracle_batch(orc, n, seed, first, 200, restart=True), "oracle")


def test_refusals_leave_the_output_untouched():
    dsl = load_dsl("werewolf-(mafia)")
    with RoomBatch([(GameTable(dsl), 8, 4)], seed=1) as b:
        lib = b._lib

        def call(n, rooms, keys, turns, R, M):
            rooms = np.asarray(rooms, dtype=np.uint64)
            keys = np.asarray(keys, dtype=np.uint64)
            turns = np.asarray(turns, dtype=np.uint32)
            out = np.full((max(n, 1), 77), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
            st = lib.ge_batch_rollout_rooms(b._h, n, rooms.ctypes.data, keys.ctypes.data, turns.ctypes.data,
                                            R, M, 7, out.ctypes.data)
            return st, (out == np.uint64(0xA5A5A5A5A5A5A5A5)).all()

        one = ([0], [0], [0])
        st = lib.ge_batch_rollout_rooms(b._h, 1, None, np.zeros(1, np.uint64).ctypes.data, np.zeros(1, np.uint32).ctypes.data, 4, 4, 7,
                                        np.zeros(77, np.uint64).ctypes.data)
        assert st == GE_ERR_ARG
        st = lib.ge_batch_rollout_rooms(b._h, 1, np.zeros(1, np.uint64).ctypes.data, np.zeros(1, np.uint64).ctypes.data,
                                        np.zeros(1, np.uint32).ctypes.data, 4, 4, 7, None)
        assert st == GE_ERR_ARG
        for args, want in [((1,) + one + (0, 4), GE_ERR_ARG), ((1,) + one + ((1 << 20) + 1, 4), GE_ERR_ARG),
                           ((65, [0] * 65, [0] * 65, [0] * 65, 1 << 20, 1), GE_ERR_ARG), ((1,) + one + (4, 4097), GE_ERR_ARG),
                           ((2, [0, 4], [0, 0], [0, 0], 4, 4), GE_ERR_RANGE), ((2, [0, 1], [0, 0], [0, 0xFFFFFFFF - 3], 4, 4), GE_ERR_RANGE)]:
            st, untouched = call(*args)
            assert st == want and untouched, (args[0], args[4], args[5], st)
        st, untouched = call(0, [], [], [], 0, 0)
        assert st == 0 and untouched
        st, untouched = call(2, [0, 1], [0, 0], [0, 0xFFFFFFFF - 4], 4, 4)     # turns[k] + M == 0xFFFFFFFF: allowed
        assert st == 0 and not untouched
        with pytest.raises(GeError):
            b.rollout_rooms([9], [0], [0], 4, 4)


@pytest.mark.parametrize("midgame", [False, True])
def test_a_million_rollouts_word_for_word(midgame):
    dsl = load_dsl("werewolf-(mafia)")
    orc = Oracle(dsl, 8)
    R, M, key, seed = 1 << 20, 256, 3 << 40, 0x77
    with RoomBatch([(GameTable(dsl), 8, 1)], seed=5, first_room=31) as b:
        turn = 0
        if midgame:
            b.step(9)
            turn = 9
        view = b.read_rooms(0, 1)
        got = b.rollout_rooms([0], [key], [turn], R, M, seed=seed)
    want = reference_rollout(orc, views_as_oracle_rooms(orc, view)[0], seed, key, turn, R, M, threads=0)
    _assert_words(got, want[None], f"2^20 playouts midgame={midgame}")
    d = rollout_to_dict(got[0])
    assert d["summary"]["rooms"] == R and d["summary"]["finished"] > 0


def test_rollouts_are_deterministic():
    dsl = load_dsl("two-truths-and-a-lie")
    with RoomBatch([(GameTable(dsl), 4, 3), (GameTable(load_dsl("werewolf-(mafia)")), 8, 3)], seed=2) as b:
        b.step(4)
        args = ([0, 4, 2, 5], [10, 20, 30, 40], [4, 4, 4, 4], 500, 400)
        x = b.rollout_rooms(*args)
        assert (b.rollout_rooms(*args) == x).all()
        assert (b.rollout_rooms(*args, seed=2) == x).all()                      # None = the batch's seed
        y = b.rollout_rooms(*args, seed=3)
        assert all(x[k][38] != y[k][38] for k in range(4))                        # checksums differ under another seed

"""ge_batch_rollout_actions (-m gpu): playouts after given actions from fuzzed states against the oracle (every (seat, choice)
candidate of each source room: the device's verdict is Oracle.inject's on a copy, and every accepted entry's 77 words are the
reference's), multi-action entries, zero-action entries equal to rollout_rooms, the composition it is defined by, read-only
behaviour, refused entries and structural errors that leave the output untouched, 2^20 playouts, and determinism."""
import numpy as np
import pytest

from conftest import load_dsl
from game_engine_amd import GameTable, GeError, RoomBatch
from oracle.oracle import Oracle
from parity_util import raw_records, views_as_oracle_rooms
from rollout_actions_ref import inject_all, reference_rollout_actions
from test_gpu_rollout import CASES, GE_ERR_ARG, GE_ERR_RANGE, _assert_words, _dsl, _source, _words

pytestmark = pytest.mark.gpu

SENTINEL = np.uint64(0xA5A5A5A5A5A5A5A5)


def _entries(parts, R_src, total, rng, n_src=2):
    """Every (seat, choice) candidate of a few source rooms as one-action entries, plus each room's no-action entry."""
    def accepts(room):
        orc, orooms = parts[room // R_src]
        return any(inject_all(orc, orooms[room % R_src], [(s, c)])[1] == 0 for s in range(1, orc.n + 1) for c in range(1, orc.n + 1))

    # source rooms with at least one legal candidate (one per segment where the fuzz made one), and one picked at random
    srcs = []
    for g in range(total // R_src):
        live = [r for r in range(g * R_src, (g + 1) * R_src) if accepts(r)]
        if live:
            srcs.append(live[int(rng.integers(0, len(live)))])
    srcs = srcs[:n_src] + [int(rng.integers(0, total))]
    rooms, actions = [], []
    for room in srcs:
        orc = parts[room // R_src][0]
        n = orc.n
        choices = range(0, n + 2) if orc.table.pack == 1 else range(0, 5)     # out-of-range choices included: refused
        for seat in range(0, n + 2):                                           # seats 0 and n + 1: refused
            for c in choices:
                rooms.append(room)
                actions.append([(seat, c)])
        rooms.append(room)
        actions.append([])
    return rooms, actions


def _reference(parts, R_src, rooms, keys, turns, actions, R, M, seed):
    words, status = [], []
    for room, key, turn, act in zip(rooms, keys, turns, actions):
        orc, orooms = parts[int(room) // R_src]
        w, s = reference_rollout_actions(orc, orooms[int(room) % R_src].copy(), seed, int(key), int(turn), act, R, M)
        words.append(w)
        status.append(s)
    return np.stack(words), np.array(status, dtype=np.int32)


@pytest.mark.parametrize("games", CASES, ids=lambda g: "+".join(f"{n}x{k}" for n, k in g))
def test_every_candidate_matches_the_oracle(games):
    rng = np.random.default_rng(sum(k * 17 for _, k in games) + 3 * len(games))
    b, parts, R_src = _source(games, rng)
    total = R_src * len(games)
    rooms, actions = _entries(parts, R_src, total, rng, n_src=4)
    keys = [int(x) for x in rng.integers(0, 2 ** 63, len(rooms))]
    keys[0] = 2 ** 64 - 30                                                     # a key that wraps past 2^64
    turns = [int(x) for x in rng.integers(0, 50000, len(rooms))]
    for R, M in [(70, 150), (1, 9)]:
        seed = 0xACE0 + R + M
        got, st = b.rollout_actions(rooms, keys, turns, actions, R, M, seed=seed)
        want, wst = _reference(parts, R_src, rooms, keys, turns, actions, R, M, seed)
        assert st.tolist() == wst.tolist(), (games, R, M)
        assert (wst == 0).sum() > len(set(rooms)) and (wst != 0).any()        # both verdicts occur
        _assert_words(got, want, f"{games} R={R} M={M}")
    b.close()


def test_multi_action_entries():
    """Two seats in one entry, and a refused action in the middle of an entry, which refuses the whole entry."""
    rng = np.random.default_rng(11)
    b, parts, R_src = _source([("ww", 8)], rng)
    orc, orooms = parts[0]
    found = None
    for room in range(R_src):                                                  # a room where two seats may act
        ok = [(s, c) for s in range(1, 9) for c in range(1, 9) if inject_all(orc, orooms[room], [(s, c)])[1] == 0]
        seats = sorted({s for s, _ in ok})
        if len(seats) >= 2:
            a1 = next(x for x in ok if x[0] == seats[0])
            a2 = next(x for x in ok if x[0] == seats[1])
            found = (room, a1, a2)
            break
    assert found
    room, a1, a2 = found
    acts = [[a1, a2], [a2, a1], [a1, (0, 1), a2], [a1, a1], [a1, a2, (a1[0], 9)], [a1]]
    R, M, seed = 100, 200, 0x3
    got, st = b.rollout_actions([room] * len(acts), [5] * len(acts), [7] * len(acts), acts, R, M, seed=seed)
    want, wst = _reference(parts, R_src, [room] * len(acts), [5] * len(acts), [7] * len(acts), acts, R, M, seed)
    assert st.tolist() == wst.tolist()
    assert wst[0] == 0 and wst[5] == 0 and wst[2] == wst[3] == GE_ERR_ARG and wst[4] == GE_ERR_ARG
    _assert_words(got, want, "multi-action")
    assert (got[2:5] == 0).all()
    b.close()


@pytest.mark.parametrize("games", [[("ww", 8)], [("tt", 4)], [("ww", 12)], [("ww", 6), ("tt", 4), ("ww", 10), ("tt", 7)]],
                         ids=lambda g: "+".join(f"{n}x{k}" for n, k in g))
def test_zero_action_entries_equal_rollout_rooms(games):
    rng = np.random.default_rng(5)
    b, parts, R_src = _source(games, rng)
    total = R_src * len(games)
    rooms = [int(x) for x in rng.integers(0, total, 12)]
    keys = [int(x) for x in rng.integers(0, 2 ** 62, 12)]
    turns = [int(x) for x in rng.integers(0, 1000, 12)]
    for R, M in [(65, 300), (300, 0)]:
        got, st = b.rollout_actions(rooms, keys, turns, [[]] * 12, R, M, seed=9)
        assert (st == 0).all()
        assert (got == b.rollout_rooms(rooms, keys, turns, R, M, seed=9)).all()
    b.close()


@pytest.mark.parametrize("game,n", [("ww", 8), ("ww", 12), ("tt", 4), ("tt", 12), ("ww_generic", 8), ("tt_generic", 5)])
def test_actions_equal_the_composition(game, n):
    """summary words == a fresh batch of R copies: write_rooms, inject_actions on every replica, set_turn, step, summary."""
    for attempt in range(8):                                                   # fuzzed sources until one has a legal candidate
        b, parts, R_src = _source([(game, n)], np.random.default_rng(n * 7 + len(game) + 1000 * attempt))
        orc, orooms = parts[0]
        cands = [(room, [(s, c)]) for room in range(R_src) for s in range(1, n + 1)
                 for c in range(1, (n if orc.table.pack == 1 else 3) + 1) if inject_all(orc, orooms[room], [(s, c)])[1] == 0]
        if cands:
            break
        b.close()
    assert cands
    R, M, key, turn, seed = 130, 300, 4242, 11, 0x51
    dsl = _dsl(game)
    for room, act in cands[:: max(1, len(cands) // 3)][:3]:
        got, st = b.rollout_actions([room], [key], [turn], [act], R, M, seed=seed)
        assert st[0] == 0
        view = b.read_rooms(room, 1)
        with RoomBatch([(GameTable(dsl), n, R, 0)], seed=seed, first_room=key) as c:
            c.write_rooms(0, np.repeat(view, R))
            assert (c.inject_actions(list(range(R)), [act[0][0]] * R, [act[0][1]] * R) == 0).all()
            c.set_turn(turn)
            c.step(M)
            want = c.summary_words()
        assert (got[0][:41] == want).all(), (game, n, room, act, np.nonzero(got[0][:41] != want)[0].tolist())
    b.close()


def test_rollout_actions_reads_only():
    games = [("ww", 8), ("tt", 4), ("ww", 12), ("tt", 12)]
    segs, orcs = [], []
    for game, n in games:
        segs.append((GameTable(_dsl(game)), n, 40, 0b1))
        orcs.append(Oracle(_dsl(game), n))
    with RoomBatch(segs, seed=9, first_room=5, max_fuse=3, restart=True, trace=True) as b:
        b.step(3)
        before = [raw_records(b, s, 40, _words(orc)) for s, orc in enumerate(orcs)]
        turn, ev = b.turn, b.read_events()
        acts = [[(1, 2)], [(1, 1), (2, 3)], [], [(3, 1)], [(0, 0)]]
        b.rollout_actions([0, 41, 85, 159, 0], [1, 2, 3, 4, 5], [0, 9, 7, 3, 100], acts, 130, 200)
        after = [raw_records(b, s, 40, _words(orc)) for s, orc in enumerate(orcs)]
        assert all((x == y).all() for x, y in zip(before, after))
        assert b.turn == turn and (b.read_events() == ev).all()


def test_refused_entries_and_structural_errors_leave_the_output_untouched():
    dsl = load_dsl("werewolf-(mafia)")
    with RoomBatch([(GameTable(dsl), 8, 4)], seed=1) as b:
        lib = b._lib

        def call(n, rooms, keys, turns, first, players, choices, R, M, nulls=()):
            arrs = [np.asarray(rooms, dtype=np.uint64), np.asarray(keys, dtype=np.uint64), np.asarray(turns, dtype=np.uint32),
                    np.asarray(first, dtype=np.uint32), np.asarray(players, dtype=np.uint32), np.asarray(choices, dtype=np.uint32)]
            ptrs = [None if i in nulls else a.ctypes.data for i, a in enumerate(arrs)]
            out = np.full((max(n, 1), 77), SENTINEL, dtype=np.uint64)
            status = np.full(max(n, 1), 7, dtype=np.int32)
            st = lib.ge_batch_rollout_actions(b._h, n, *ptrs, status.ctypes.data, R, M, 7, out.ctypes.data)
            return st, out, status

        ok = ([0], [0], [0], [0, 1], [1], [2])
        for i in range(6):                                                     # NULL arrays
            st, out, status = call(1, *ok, 4, 4, nulls=(i,))
            assert st == GE_ERR_ARG and (out == SENTINEL).all() and (status == 7).all(), i
        for args, want in [((1,) + ok + (0, 4), GE_ERR_ARG), ((1,) + ok + ((1 << 20) + 1, 4), GE_ERR_ARG),
                           ((65, [0] * 65, [0] * 65, [0] * 65, [0] * 66, [], [], 1 << 20, 1), GE_ERR_ARG),
                           ((1,) + ok + (4, 4097), GE_ERR_ARG),
                           ((2, [0, 1], [0, 0], [0, 0], [1, 1, 1], [1], [2], 4, 4), GE_ERR_ARG),          # first_action[0] != 0
                           ((2, [0, 1], [0, 0], [0, 0], [0, 1, 0], [1], [2], 4, 4), GE_ERR_ARG),          # decreasing
                           ((1, [0], [0], [0], [0, 13], [1] * 13, [2] * 13, 4, 4), GE_ERR_ARG),           # 13 actions in one entry
                           ((2, [0, 4], [0, 0], [0, 0], [0, 0, 0], [], [], 4, 4), GE_ERR_RANGE),
                           ((2, [0, 1], [0, 0], [0, 0xFFFFFFFF - 3], [0, 0, 0], [], [], 4, 4), GE_ERR_RANGE)]:
            st, out, status = call(*args)
            assert st == want and (out == SENTINEL).all() and (status == 7).all(), (args[0], args[4], args[7], args[8], st)
        st, out, status = call(0, [], [], [], [0], [], [], 0, 0)
        assert st == 0 and (out == SENTINEL).all() and (status == 7).all()
        # refused entries: their rows stay the sentinel, every other entry is played; the first refused entry's status returns
        st, out, status = call(4, [0, 1, 2, 3], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 1, 3, 4], [0, 1, 9, 1], [1, 1, 1, 1], 70, 50)
        assert st == GE_ERR_ARG and status.tolist() == [0, GE_ERR_ARG, GE_ERR_ARG, GE_ERR_ARG]
        assert (out[1:] == SENTINEL).all() and not (out[0] == SENTINEL).all()
        assert (out[0] == b.rollout_rooms([0], [0], [0], 70, 50, seed=7)[0]).all()
        with pytest.raises(GeError):
            b.rollout_actions([9], [0], [0], [[]], 4, 4)
        with pytest.raises(GeError):
            b.rollout_actions([0], [0], [0], [[(1, 1)] * 13], 4, 4)
        w, s = b.rollout_actions([0, 1], [0, 0], [0, 0], [[(0, 1)], []], 4, 4)   # a refused entry is no error in Python
        assert s.tolist() == [GE_ERR_ARG, 0] and (w[0] == 0).all() and w[1][0] == 4


def _ww_day_vote_room():
    """A Werewolf x 8 room played up to a phase where every living seat votes; (dsl, view, turn, accepted (seat, choice))."""
    dsl = load_dsl("werewolf-(mafia)")
    orc = Oracle(dsl, 8)
    with RoomBatch([(GameTable(dsl), 8, 1)], seed=5, first_room=31) as b:
        for turn in range(1, 40):
            b.step(1)
            view = b.read_rooms(0, 1)
            room = views_as_oracle_rooms(orc, view)[0]
            ok = [(s, c) for s in range(1, 9) for c in range(1, 9) if inject_all(orc, room, [(s, c)])[1] == 0]
            if len({s for s, _ in ok}) >= 4:
                return dsl, orc, view, turn, ok
    raise AssertionError("no voting phase reached")


def test_a_million_playouts_after_an_action_word_for_word():
    dsl, orc, view, turn, ok = _ww_day_vote_room()
    R, M, key, seed = 1 << 20, 256, 5 << 40, 0x78
    act = [ok[len(ok) // 2]]
    with RoomBatch([(GameTable(dsl), 8, 1)], seed=1) as b:
        b.write_rooms(0, view)
        got, st = b.rollout_actions([0], [key], [turn], [act], R, M, seed=seed)
    assert st[0] == 0
    want, wst = reference_rollout_actions(orc, views_as_oracle_rooms(orc, view)[0], seed, key, turn, act, R, M, threads=0)
    _assert_words(got, want[None], "2^20 playouts after an action")


def test_rollout_actions_are_deterministic():
    dsl, _, view, turn, ok = _ww_day_vote_room()
    with RoomBatch([(GameTable(dsl), 8, 2)], seed=2) as b:
        b.write_rooms(0, np.repeat(view, 2))
        args = ([0, 1, 0, 1], [10, 20, 30, 40], [turn] * 4, [[ok[0]], [ok[-1]], [], [ok[0], (0, 0)]], 500, 400)
        x, s = b.rollout_actions(*args)
        y, t = b.rollout_actions(*args)
        assert (x == y).all() and (s == t).all() and s.tolist() == [0, 0, 0, GE_ERR_ARG]

"""ge_batch_rollout_seats (-m gpu): playouts from a seat's view against the oracle reference of POLICY.md §3c for every layout,
shipped and GENERIC, from fuzzed states with every seat 0..n, with and without actions; seat 0 equal to rollout_actions; views
that hide nothing equal to the full view; the no-leak property (rooms that differ only in where the hidden tuples sit give the
same words from the seat's view); read-only behaviour, structural errors, refusals, determinism and 2^20 playouts."""
import numpy as np
import pytest

from conftest import load_dsl
from game_engine_amd import GameTable, GeError, RoomBatch
from oracle.oracle import Oracle
from parity_util import oracle_rooms_as_views, raw_records
from rollout_actions_ref import inject_all
from rollout_seats_ref import known_sets, reference_rollout_seats, tuple_fields
from test_gpu_rollout import CASES, GE_ERR_ARG, GE_ERR_RANGE, _assert_words, _dsl, _source, _words

pytestmark = pytest.mark.gpu

SENTINEL = np.uint64(0xA5A5A5A5A5A5A5A5)


def _reference(parts, R_src, rooms, keys, turns, seats, actions, R, M, seed):
    words, status = [], []
    for room, key, turn, seat, act in zip(rooms, keys, turns, seats, actions):
        orc, orooms = parts[int(room) // R_src]
        w, s = reference_rollout_seats(orc, orooms[int(room) % R_src].copy(), seed, int(key), int(turn), int(seat), act, R, M)
        words.append(w)
        status.append(s)
    return np.stack(words), np.array(status, dtype=np.int32)


def _legal(parts, R_src, room):
    orc, orooms = parts[room // R_src]
    hi = orc.n if orc.table.pack == 1 else 3
    return [(s, c) for s in range(1, orc.n + 1) for c in range(1, hi + 1) if inject_all(orc, orooms[room % R_src], [(s, c)])[1] == 0]


@pytest.mark.parametrize("games", CASES, ids=lambda g: "+".join(f"{n}x{k}" for n, k in g))
def test_every_seat_matches_the_oracle(games):
    rng = np.random.default_rng(sum(k * 31 for _, k in games) + 7 * len(games))
    b, parts, R_src = _source(games, rng)
    rooms, seats, actions = [], [], []
    for g in range(len(games)):
        n = parts[g][0].n
        for room in (int(rng.integers(g * R_src, (g + 1) * R_src)), int(rng.integers(g * R_src, (g + 1) * R_src))):
            legal = _legal(parts, R_src, room)
            for seat in range(0, n + 1):
                rooms.append(room); seats.append(seat); actions.append([])
                if legal:                                                    # the same seat after a legal action
                    rooms.append(room); seats.append(seat); actions.append([legal[seat % len(legal)]])
            rooms.append(room); seats.append(1); actions.append([(0, 1)])   # refused
    keys = [int(x) for x in rng.integers(0, 2 ** 63, len(rooms))]
    keys[0] = 2 ** 64 - 20                                                    # a key that wraps past 2^64
    turns = [int(x) for x in rng.integers(0, 50000, len(rooms))]
    for R, M in [(70, 150), (1, 9)]:
        seed = 0x5EA7 + R + M
        got, st = b.rollout_seats(rooms, keys, turns, seats, actions, R, M, seed=seed)
        want, wst = _reference(parts, R_src, rooms, keys, turns, seats, actions, R, M, seed)
        assert st.tolist() == wst.tolist(), (games, R, M)
        _assert_words(got, want, f"{games} R={R} M={M}")
        # seat 0 is rollout_actions's entry word for word
        zero = [k for k, s in enumerate(seats) if s == 0]
        ga, sa = b.rollout_actions([rooms[k] for k in zero], [keys[k] for k in zero], [turns[k] for k in zero],
                                   [actions[k] for k in zero], R, M, seed=seed)
        assert (ga == got[zero]).all() and (sa == st[zero]).all()
    b.close()


@pytest.mark.parametrize("game,n", [("ww", 8), ("ww", 12), ("tt", 4), ("tt", 12)])
def test_views_that_hide_nothing_equal_the_full_view(game, n):
    """Before the deal (every hidden tuple alike), with every other seat revealed, and a Two-Truths speaker's own view."""
    dsl = _dsl(game)
    orc = Oracle(dsl, n)
    recs = orc.init_rooms(3)
    if orc.table.pack == 1:
        orc.run(recs[1:], 3, 0, 0, 8)
        recs[1]["p"][:n, 3] = 1                                               # everyone revealed
        recs[2]["p"][:n, 3] = 1
        recs[2]["p"][4, 3] = 0                                                # ... but seat 5, who looks
        seat_of = [3, 2, 5]
    else:
        orc.run(recs[1:], 3, 0, 0, 4)
        recs[1]["p"][:n, 3] = 1                                               # the lie revealed
        sp = int(np.argmax(recs[2]["p"][:n, 0]))
        seat_of = [2, 2, sp + 1]                                              # the speaker knows its lie
    with RoomBatch([(GameTable(dsl), n, 3)], seed=1) as b:
        b.write_rooms(0, oracle_rooms_as_views(orc, recs))
        for k in range(3):
            w, _ = b.rollout_seats([k], [77], [5], [seat_of[k]], None, 200, 300, seed=4)
            assert (w == b.rollout_rooms([k], [77], [5], 200, 300, seed=4)).all(), k


def _swapped(orc, rec, seat):
    """rec with the hidden tuples of a wolf and a non-wolf that `seat` cannot tell apart swapped (None if there are none)."""
    U, Uw, Uv, _ = known_sets(orc, rec, seat)
    p = rec["p"]
    q = [c for c in U if c not in Uw and c not in Uv]
    wolves = [c for c in q if p[c][1] == 2 and rec["det"][c] == 0]
    others = [c for c in q if p[c][1] != 2 and rec["det"][c] == 0]
    if not wolves or not others:
        return None
    a, c = wolves[0], others[0]
    out = rec.copy()
    for f in tuple_fields(orc, rec):
        out["p"][a][f], out["p"][c][f] = rec["p"][c][f], rec["p"][a][f]
    return out


@pytest.mark.parametrize("n", [8, 12])
def test_a_seat_cannot_tell_rooms_that_differ_in_what_it_cannot_see(n):
    """The no-leak property: two rooms that differ only in which unknown seats hold which hidden tuples (the same investigated
    set) give identical words from the seat's view and different words in the full view."""
    dsl = load_dsl("werewolf-(mafia)")
    orc = Oracle(dsl, n)
    done = 0
    for turns in (6, 9, 13, 17):
        rooms = orc.init_rooms(1)
        orc.run(rooms, 0xBEEF, 9, 0, turns)
        rec = rooms[0]
        for seat in range(1, n + 1):
            if rec["p"][seat - 1][1] == 2 or rec["p"][seat - 1][3]:
                continue                                                      # a wolf sees every team; skip revealed seats
            other = _swapped(orc, rec, seat)
            if other is None:
                continue
            with RoomBatch([(GameTable(dsl), n, 2)], seed=1) as b:
                b.write_rooms(0, oracle_rooms_as_views(orc, np.stack([rec, other])))
                ws, _ = b.rollout_seats([0, 1], [3 << 16, 3 << 16], [turns] * 2, [seat, seat], None, 512, 400, seed=21)
                wf, _ = b.rollout_seats([0, 1], [3 << 16, 3 << 16], [turns] * 2, [0, 0], None, 512, 400, seed=21)
            assert (ws[0] == ws[1]).all(), (turns, seat)
            assert not (wf[0] == wf[1]).all(), (turns, seat)
            done += 1
    assert done >= 4


def test_rollout_seats_reads_only():
    games = [("ww", 8), ("tt", 4), ("ww", 12), ("tt", 12)]
    segs, orcs = [], []
    for game, n in games:
        segs.append((GameTable(_dsl(game)), n, 40, 0b1))
        orcs.append(Oracle(_dsl(game), n))
    with RoomBatch(segs, seed=9, first_room=5, max_fuse=3, restart=True, trace=True) as b:
        b.step(3)
        before = [raw_records(b, s, 40, _words(orc)) for s, orc in enumerate(orcs)]
        turn, ev = b.turn, b.read_events()
        b.rollout_seats([0, 41, 85, 159, 0], [1, 2, 3, 4, 5], [0, 9, 7, 3, 100], [1, 2, 12, 3, 0],
                        [[(1, 2)], [(1, 1), (2, 3)], [], [(3, 1)], [(0, 0)]], 130, 200)
        after = [raw_records(b, s, 40, _words(orc)) for s, orc in enumerate(orcs)]
        assert all((x == y).all() for x, y in zip(before, after))
        assert b.turn == turn and (b.read_events() == ev).all()


def test_structural_errors_and_refusals():
    dsl = load_dsl("werewolf-(mafia)")
    with RoomBatch([(GameTable(dsl), 8, 4), (GameTable(load_dsl("two-truths-and-a-lie")), 4, 2)], seed=1) as b:
        lib = b._lib

        def call(n, rooms, keys, turns, seats, first, players, choices, R, M, nulls=()):
            arrs = [np.asarray(rooms, dtype=np.uint64), np.asarray(keys, dtype=np.uint64), np.asarray(turns, dtype=np.uint32),
                    np.asarray(seats, dtype=np.uint32), np.asarray(first, dtype=np.uint32), np.asarray(players, dtype=np.uint32),
                    np.asarray(choices, dtype=np.uint32)]
            ptrs = [None if i in nulls else a.ctypes.data for i, a in enumerate(arrs)]
            out = np.full((max(n, 1), 77), SENTINEL, dtype=np.uint64)
            status = np.full(max(n, 1), 7, dtype=np.int32)
            st = lib.ge_batch_rollout_seats(b._h, n, *ptrs, status.ctypes.data, R, M, 7, out.ctypes.data)
            return st, out, status

        ok = ([0], [0], [0], [1], [0, 1], [1], [2])
        for i in range(4):                                                     # NULL rooms / keys / turns / seats
            st, out, status = call(1, *ok, 4, 4, nulls=(i,))
            assert st == GE_ERR_ARG and (out == SENTINEL).all() and (status == 7).all(), i
        for args, want in [((1, [0], [0], [0], [9], [0, 0], [], [], 4, 4), GE_ERR_ARG),            # seat above 8
                           ((1, [4], [0], [0], [5], [0, 0], [], [], 4, 4), GE_ERR_ARG),            # above the segment's 4
                           ((1,) + ok + (0, 4), GE_ERR_ARG), ((1,) + ok + (4, 4097), GE_ERR_ARG),
                           ((2, [0, 1], [0, 0], [0, 0], [1, 1], [1, 1, 1], [1], [2], 4, 4), GE_ERR_ARG),
                           ((1, [0], [0], [0], [1], [0, 13], [1] * 13, [2] * 13, 4, 4), GE_ERR_ARG),
                           ((2, [0, 6], [0, 0], [0, 0], [1, 1], [0, 0, 0], [], [], 4, 4), GE_ERR_RANGE)]:
            st, out, status = call(*args)
            assert st == want and (out == SENTINEL).all() and (status == 7).all(), (args, st)
        st, out, status = call(0, [], [], [], [], [0], [], [], 0, 0)
        assert st == 0 and (out == SENTINEL).all()
        # no actions (NULL first_action): every entry played
        st, out, status = call(2, [0, 4], [0, 0], [0, 0], [3, 4], [0], [], [], 70, 50, nulls=(4, 5, 6))
        assert st == 0 and status.tolist() == [0, 0] and not (out == SENTINEL).any()
        # refused entries keep the sentinel, the others are played
        st, out, status = call(3, [0, 1, 4], [0, 0, 0], [0, 0, 0], [2, 2, 2], [0, 1, 1, 1], [9], [1], 70, 50)
        assert st == GE_ERR_ARG and status.tolist() == [GE_ERR_ARG, 0, 0]
        assert (out[0] == SENTINEL).all() and not (out[1:] == SENTINEL).any()
        with pytest.raises(GeError):
            b.rollout_seats([0], [0], [0], [9], None, 4, 4)
        w, s = b.rollout_seats([0, 1], [0, 0], [0, 0], [1, 1], [[(0, 1)], []], 4, 4)
        assert s.tolist() == [GE_ERR_ARG, 0] and (w[0] == 0).all() and w[1][0] == 4


def _ww_night_room():
    dsl = load_dsl("werewolf-(mafia)")
    orc = Oracle(dsl, 8)
    rooms = orc.init_rooms(1)
    orc.run(rooms, 5, 31, 0, 9)
    return dsl, orc, rooms[0]


def test_a_million_playouts_from_a_seat_word_for_word():
    dsl, orc, rec = _ww_night_room()
    seat = next(s for s in range(1, 9) if rec["p"][s - 1][0] == 1 and not rec["p"][s - 1][3])
    R, M, key, seed, turn = 1 << 20, 256, 5 << 40, 0x78, 9
    with RoomBatch([(GameTable(dsl), 8, 1)], seed=1) as b:
        b.write_rooms(0, oracle_rooms_as_views(orc, rec.reshape(1)))
        got, st = b.rollout_seats([0], [key], [turn], [seat], None, R, M, seed=seed)
    assert st[0] == 0
    want, _ = reference_rollout_seats(orc, rec, seed, key, turn, seat, [], R, M, threads=0)
    _assert_words(got, want[None], "2^20 playouts from a seat's view")


def test_rollout_seats_are_deterministic():
    dsl, orc, rec = _ww_night_room()
    with RoomBatch([(GameTable(dsl), 8, 2)], seed=2) as b:
        b.write_rooms(0, oracle_rooms_as_views(orc, np.stack([rec, rec])))
        args = ([0, 1, 0, 1], [10, 20, 30, 40], [9] * 4, [1, 2, 3, 0], None, 500, 400)
        x, s = b.rollout_seats(*args)
        y, t = b.rollout_seats(*args)
        assert (x == y).all() and (s == t).all() and (s == 0).all()

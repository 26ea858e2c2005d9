"""ge_batch_rollout_beliefs (-m gpu): seat-view playouts and comparisons weighted by the caller's beliefs (POLICY.md §3j).
Equal weights are rollout_seats / rollout_compare word for word; weighted views are the oracle reference (rollout_beliefs_ref)
bit for bit, comparison sums included; structural errors in the documented order with nothing touched, refusals per entry,
the batch only read, two calls identical.  Shapes: one source room per segment, R = 70 (a full wavefront and a partial one) and
R = 1, M in {0, 150, 9} (M = 0 leaves the re-deal itself in the checksum word), Werewolf x 4 / 8 / 12 and Two-Truths x 4 / 12,
shipped and GENERIC."""
import numpy as np
import pytest

from game_engine_amd import GameTable, GeError, RoomBatch
from game_engine_amd.stepper import GE_ERR_ARG
from oracle.oracle import Oracle
from parity_util import raw_records, views_as_oracle_rooms
from rollout_actions_ref import inject_all
from rollout_beliefs_ref import reference_beliefs
from rollout_seats_ref import known_sets
from test_gpu_rollout import GE_ERR_RANGE, _assert_words, _dsl, _source, _views, _words

pytestmark = pytest.mark.gpu

SENTINEL = np.uint64(0xA5A5A5A5A5A5A5A5)
LAYOUTS = [("ww", 4), ("ww", 8), ("ww", 12), ("tt", 4), ("tt", 12)]
RM = [(70, 0), (70, 150), (1, 9)]


def _name(game, generic):
    return game + "_generic" if generic else game


def _slots(orc):
    return orc.n if orc.table.pack == 1 else 3


def _interesting(orc, rec):
    """A fuzzed record on which the beliefs can show: Werewolf - a seat that is neither wolf nor Detective with wolves to place
    and at least two seats more than wolves to place them on, and (from 8 seats) a wolf seat and a Detective whose memory
    fits; Two-Truths - an unrevealed lie of a speaker; and in both a phase in which some seat has a legal action."""
    n, p = orc.n, rec["p"]
    if orc.table.pack != 1:
        sp = [c for c in range(n) if p[c][0]]
        return bool(sp) and p[sp[0]][3] == 0 and p[sp[0]][2] != 0 and bool(_legal(orc, rec))
    plain = det = wolf = False
    for seat in range(1, n + 1):
        U, Uw, Uv, need = known_sets(orc, rec, seat)
        uq = len(U) - len(Uw) - len(Uv)
        if p[seat - 1][1] == 2:
            wolf = True
        elif p[seat - 1][0] == 4:
            det = det or (bool(Uw or Uv) and need >= 1 and uq > need)
        else:
            plain = plain or (need >= 1 and uq >= need + 2)
    return plain and (n < 8 or (det and wolf)) and bool(_legal(orc, rec))


def _fuzzed(game, n, generic):
    """_source's batch of ONE fuzzed room of the layout (human mask and GE_FLAG_RESTART set: both must be ignored), from the
    first rng seed whose room is _interesting; (batch, oracle, the room's oracle record)."""
    name = _name(game, generic)
    orc = Oracle(_dsl(name), n)
    for seed in range(4000):
        rec = views_as_oracle_rooms(orc, _views(orc, name, 1, np.random.default_rng(seed)))[0]
        if _interesting(orc, rec):
            break
    else:
        raise AssertionError(f"no fuzzed {name} x {n} room shows the beliefs")
    b, parts, _ = _source([(name, n)], np.random.default_rng(seed), R=1)
    assert parts[0][1][0].tobytes() == rec.tobytes()
    return b, orc, rec


def _legal(orc, rec):
    hi = orc.n if orc.table.pack == 1 else 3
    return [(s, c) for s in range(1, orc.n + 1) for c in range(1, hi + 1) if inject_all(orc, rec, [(s, c)])[1] == 0]


def _row(orc, values):
    row = np.zeros(16, dtype=np.uint8)
    row[:_slots(orc)] = values
    return row


@pytest.mark.parametrize("generic", [False, True], ids=["shipped", "generic"])
@pytest.mark.parametrize("game,n", LAYOUTS, ids=lambda v: str(v))
def test_equal_weights_are_the_old_call(game, n, generic):
    b, orc, rec = _fuzzed(game, n, generic)
    with b:
        legal = _legal(orc, rec)
        rooms, seats, actions = [], [], []
        for seat in range(0, n + 1):                                              # every seat, with and without a legal action
            rooms.append(0); seats.append(seat); actions.append([])
            if legal:
                rooms.append(0); seats.append(seat); actions.append([legal[seat % len(legal)]])
        N = len(rooms)
        keys = [(11 + s) << 16 for s in seats]
        keys[0] = 2 ** 64 - 20
        turns = [7] * N
        baseline = [k - (k % 2) if legal else k for k in range(N)]                # the action entry against its seat's plain entry
        subjects = [max(s, 1) for s in seats]
        for R, M in RM:
            seed = 0xBE11 + R + M
            want_w, want_s = b.rollout_seats(rooms, keys, turns, seats, actions, R, M, seed=seed)
            cw, cs, want_c = b.rollout_compare(rooms, keys, turns, seats, actions, baseline, subjects, R, M, seed=seed)
            assert (cw == want_w).all() and (cs == want_s).all()
            assert (want_s == 0).all() and want_w[:, 0].sum() + want_w[:, 37].sum() > 0
            for v in (1, 16, 255):
                bel = np.stack([_row(orc, v)] * N)
                got_w, got_s = b.rollout_beliefs(rooms, keys, turns, seats, actions, bel, R, M, seed=seed)
                assert (got_s == want_s).all(), (v, R, M)
                _assert_words(got_w, want_w, f"{game} x {n} generic={generic} v={v} R={R} M={M}")
                got_w, got_s, got_c = b.rollout_beliefs(rooms, keys, turns, seats, actions, bel, R, M, seed=seed,
                                                        baseline=baseline, subjects=subjects)
                assert (got_s == want_s).all() and (got_c == want_c).all(), (v, R, M)
                _assert_words(got_w, want_w, f"{game} x {n} generic={generic} v={v} R={R} M={M} comparing")


def _belief_rows(orc, rec, seat, rng):
    """Rows for one viewing seat: random with zeros, all zero, one seat (statement) at 255 among ones, and the fallback - every
    seat the view cannot rule out zeroed but one, fewer than the wolves still to place wherever there are two or more."""
    k = _slots(orc)
    rows = [_row(orc, rng.integers(0, 256, k) * rng.integers(0, 2, k)), _row(orc, 0)]
    hot = np.ones(k, dtype=np.int64)
    hot[int(rng.integers(0, k))] = 255
    rows.append(_row(orc, hot))
    fall = rng.integers(1, 256, k)
    if orc.table.pack == 1 and seat:
        U, Uw, Uv, _ = known_sets(orc, rec, seat)
        uq = [c for c in U if c not in Uw and c not in Uv]
        fall[uq[1:]] = 0
    else:
        fall[1:] = 0
    rows.append(_row(orc, fall))
    return rows


@pytest.mark.parametrize("generic", [False, True], ids=["shipped", "generic"])
@pytest.mark.parametrize("game,n", LAYOUTS, ids=lambda v: str(v))
def test_weighted_views_match_the_reference(game, n, generic):
    b, orc, rec = _fuzzed(game, n, generic)
    rng = np.random.default_rng(n * 17 + generic)
    with b:
        legal = _legal(orc, rec)
        rooms, seats, actions, bel, baseline, subjects = [], [], [], [], [], []
        for seat in range(0, n + 1):                                              # wolves, the Detective, voters, the speaker
            for j, row in enumerate(_belief_rows(orc, rec, seat, rng)):
                first = len(rooms)
                acts = [[legal[(seat + j) % len(legal)]]] if legal and j == seat % 4 else []   # one row per seat with an action too
                for act in acts + [[]]:
                    rooms.append(0); seats.append(seat); actions.append(act); bel.append(row)
                    baseline.append(first + len(acts))                            # the plain entry, behind the action's
                    subjects.append(max(seat, 1))
        rooms.append(0); seats.append(1); actions.append([(0, 1)]); bel.append(_row(orc, 3))       # refused
        baseline.append(len(rooms) - 1); subjects.append(1)
        bel = np.stack(bel)
        keys = [int(x) for x in rng.integers(0, 2 ** 63, len(rooms))]
        for k, bl in enumerate(baseline):                                         # common random numbers: a baseline's key
            keys[k] = keys[bl]
        wrap = next(k for k, s in enumerate(seats) if s == 2)
        for k in range(len(rooms)):                                               # a key that wraps past 2^64 under a re-deal
            if baseline[k] == baseline[wrap]:
                keys[k] = 2 ** 64 - 20
        turns = [int(rng.integers(0, 50000))] * len(rooms)
        orc_of = lambda r: (orc, rec)                                              # noqa: E731
        moved = False
        for R, M in RM:
            seed = 0x5A5 + R + M
            want_w, want_s, want_c = reference_beliefs(orc_of, rooms, keys, turns, seats, actions, bel, R, M, seed, baseline, subjects)
            got_w, got_s = b.rollout_beliefs(rooms, keys, turns, seats, actions, bel, R, M, seed=seed)
            assert got_s.tolist() == want_s.tolist(), (R, M)
            _assert_words(got_w, want_w, f"{game} x {n} generic={generic} R={R} M={M}")
            got_w, got_s, got_c = b.rollout_beliefs(rooms, keys, turns, seats, actions, bel, R, M, seed=seed, baseline=baseline,
                                                    subjects=subjects)
            assert got_s.tolist() == want_s.tolist(), (R, M)
            _assert_words(got_w, want_w, f"{game} x {n} generic={generic} R={R} M={M} comparing")
            bad = np.nonzero((got_c != want_c).any(axis=1))[0]
            assert len(bad) == 0, f"R={R} M={M}: entries {bad.tolist()} got {got_c[bad].tolist()} want {want_c[bad].tolist()}"
            assert want_s[-1] != 0 and (want_s[:-1] == 0).all()
            plain_w, _ = b.rollout_seats(rooms, keys, turns, seats, actions, R, M, seed=seed)
            moved = moved or bool((plain_w != want_w).any())
        assert moved, "the reference under these beliefs never differs from the unweighted view: the case shows nothing"


def _mixed():
    games = [("ww", 8), ("tt", 4), ("ww", 12), ("tt", 12)]
    segs, orcs = [], []
    for game, n in games:
        segs.append((GameTable(_dsl(game)), n, 3, 0b1))
        orcs.append(Oracle(_dsl(game), n))
    return RoomBatch(segs, seed=9, first_room=5, max_fuse=3, restart=True, trace=True), orcs


def test_structural_errors_in_order_and_nothing_touched():
    b, orcs = _mixed()                                                            # rooms 0..2 Werewolf x 8, 3..5 Two-Truths x 4, ...
    with b:
        lib = b._lib
        b.step(3)

        def call(n, rooms, seats, bel, baseline=None, subj=None, R=4, M=4, nulls=(), first=None, players=(), choices=(), with_cmp=None):
            arrs = {"rooms": np.asarray(rooms, dtype=np.uint64), "keys": np.full(max(n, 1), 5, dtype=np.uint64),
                    "turns": np.zeros(max(n, 1), dtype=np.uint32), "seats": np.asarray(seats, dtype=np.uint32),
                    "bel": np.ascontiguousarray(bel, dtype=np.uint8), "baseline": np.asarray(baseline or [0], dtype=np.uint32),
                    "subj": np.asarray(subj or [0], dtype=np.uint32), "first": np.asarray(first or [0], dtype=np.uint32),
                    "players": np.asarray(players, dtype=np.uint32), "choices": np.asarray(choices, dtype=np.uint32)}
            out = np.full((max(n, 1), 77), SENTINEL, dtype=np.uint64)
            cmp = np.full((max(n, 1), 6), SENTINEL, dtype=np.uint64)
            status = np.full(max(n, 1), 7, dtype=np.int32)
            p = {k: (None if k in nulls else a.ctypes.data) for k, a in arrs.items()}
            for k, given in (("baseline", baseline), ("subj", subj), ("first", first), ("players", first), ("choices", first)):
                if given is None:
                    p[k] = None
            if with_cmp is None:
                with_cmp = baseline is not None or subj is not None
            pc = cmp.ctypes.data if with_cmp else None
            st = lib.ge_batch_rollout_beliefs(b._h, n, p["rooms"], p["keys"], p["turns"], p["seats"], p["first"], p["players"], p["choices"],
                                              status.ctypes.data, p["bel"], R, M, 7, out.ctypes.data, p["baseline"], p["subj"], pc)
            touched = not ((out == SENTINEL).all() and (cmp == SENTINEL).all() and (status == 7).all())
            return st, touched, out, status, cmp

        ok8 = np.zeros((2, 16), dtype=np.uint8)
        ok8[:, :8] = 16
        good = (2, [0, 0], [1, 2], ok8)
        st, touched, out, status, _ = call(*good)
        assert st == 0 and status.tolist() == [0, 0] and not (out == SENTINEL).any()
        st, touched, out, status, cmp = call(*good, baseline=[1, 1], subj=[2, 2])
        assert st == 0 and not (cmp == SENTINEL).any() and cmp[1].tolist() == [4, 0, 0, 0, 0, 0]
        for null in ("rooms", "keys", "turns", "seats", "bel"):                  # NULL arrays
            assert call(*good, nulls=(null,))[:2] == (GE_ERR_ARG, False), null
        # rollout_seats's own checks come before the beliefs': a range error with beliefs NULL and a bad stride behind it
        bad8 = ok8.copy()
        bad8[0, 8] = 1
        assert call(2, [0, 99], [1, 2], bad8, nulls=("bel",))[:2] == (GE_ERR_RANGE, False)
        assert call(2, [0, 0], [9, 2], bad8)[:2] == (GE_ERR_ARG, False)            # seat above 8
        assert call(*good, R=0)[:2] == (GE_ERR_ARG, False) and call(*good, M=4097)[:2] == (GE_ERR_ARG, False)
        # a non-zero byte beyond the player count / the three statements
        assert call(2, [0, 0], [1, 2], bad8)[:2] == (GE_ERR_ARG, False)
        tt = np.zeros((1, 16), dtype=np.uint8)
        tt[0, :3] = 9
        assert call(1, [3], [1], tt)[0] == 0
        tt[0, 3] = 1                                                              # Two-Truths x 4: slot 3 is a seat, not a statement
        assert call(1, [3], [1], tt)[:2] == (GE_ERR_ARG, False)
        w12 = np.zeros((1, 16), dtype=np.uint8)
        w12[0, :12] = 200
        assert call(1, [6], [12], w12)[0] == 0
        w12[0, 12] = 1
        assert call(1, [6], [12], w12)[:2] == (GE_ERR_ARG, False)
        # the bad byte is reported before the partial comparison arrays, and those before rollout_compare's own checks
        assert call(2, [0, 0], [1, 2], bad8, baseline=[1, 1])[:2] == (GE_ERR_ARG, False)
        for part in ({"baseline": [1, 1]}, {"subj": [2, 2]}, {"baseline": [1, 1], "subj": [2, 2], "with_cmp": False}):
            assert call(*good, **part)[:2] == (GE_ERR_ARG, False), part
        assert call(*good, with_cmp=True)[:2] == (GE_ERR_ARG, False)            # cmp alone
        assert call(*good, baseline=[1, 2], subj=[2, 2])[:2] == (GE_ERR_ARG, False)                # a baseline outside the call
        assert call(2, [0, 1], [1, 2], ok8, baseline=[1, 1], subj=[2, 2])[:2] == (GE_ERR_ARG, False)   # of another room
        assert call(*good, baseline=[1, 1], subj=[0, 2])[:2] == (GE_ERR_ARG, False)                # subject 0
        assert call(*good, baseline=[1, 1], subj=[9, 2])[:2] == (GE_ERR_ARG, False)
        st, touched, _, _, _ = call(0, [], [], np.zeros((0, 16), dtype=np.uint8))
        assert st == 0 and not touched
        # refusals per entry: the refused entry keeps the sentinel, the others are played
        ok3 = np.concatenate([ok8, ok8[:1]])
        st, _, out, status, _ = call(3, [0, 1, 0], [2, 2, 2], ok3, R=70, M=50, first=[0, 1, 1, 1], players=[9], choices=[1])
        assert st == GE_ERR_ARG and status.tolist() == [GE_ERR_ARG, 0, 0]
        assert (out[0] == SENTINEL).all() and not (out[1:] == SENTINEL).any()
        with pytest.raises(GeError):
            b.rollout_beliefs([0], [0], [0], [1], None, bad8[:1], 4, 4)
        with pytest.raises(GeError):
            b.rollout_beliefs([0], [0], [0], [1], None, ok8[:1], 4, 4, baseline=[0])
        w, s = b.rollout_beliefs([0, 1], [0, 0], [0, 0], [1, 1], [[(0, 1)], []], ok8, 4, 4)
        assert s.tolist() == [GE_ERR_ARG, 0] and (w[0] == 0).all() and w[1][0] == 4


def test_reads_only_and_is_deterministic():
    b, orcs = _mixed()
    with b:
        b.step(3)
        rng = np.random.default_rng(5)
        rooms, seats = [0, 4, 7, 10, 1], [1, 2, 12, 3, 0]
        bel = np.zeros((5, 16), dtype=np.uint8)
        for k, (r, s) in enumerate(zip(rooms, seats)):
            orc = orcs[r // 3]
            bel[k, :_slots(orc)] = rng.integers(0, 256, _slots(orc))
        args = (rooms, [1, 2, 3, 4, 5], [3] * 5, seats, [[(1, 2)], [], [], [], [(0, 0)]], bel, 70, 150)
        before = [raw_records(b, s, 3, _words(orc)) for s, orc in enumerate(orcs)]
        turn, ev, summary = b.turn, b.read_events(), b.summary()
        x = b.rollout_beliefs(*args, seed=4)
        y = b.rollout_beliefs(*args, seed=4)
        xc = b.rollout_beliefs(*args, seed=4, baseline=[0, 1, 2, 3, 4], subjects=[1, 2, 12, 3, 1])
        yc = b.rollout_beliefs(*args, seed=4, baseline=[0, 1, 2, 3, 4], subjects=[1, 2, 12, 3, 1])
        assert all((p == q).all() for p, q in zip(x, y)) and all((p == q).all() for p, q in zip(xc, yc))
        assert (xc[0] == x[0]).all() and (xc[1] == x[1]).all() and x[1][-1] != 0 and (x[1][1:-1] == 0).all()
        after = [raw_records(b, s, 3, _words(orc)) for s, orc in enumerate(orcs)]
        assert all((p == q).all() for p, q in zip(before, after))
        assert b.turn == turn and (b.read_events() == ev).all() and b.summary() == summary

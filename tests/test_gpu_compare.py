"""ge_batch_rollout_compare (-m gpu): the paired counts of POLICY.md §3e against the oracle reference (compare_ref), bit for bit -
every layout, shipped and GENERIC, full view and seat view, every seat as subject, partial last wavefronts, several segments in
one call with a baseline behind its entry, refused entries and baselines, words and verdicts equal to rollout_seats's, the
batch only read, two calls identical, structural errors.  Every case first shows on the reference's own numbers that it is
not empty (an option with better > 0 and one with worse > 0), so a kernel that returns zeros cannot pass."""
import numpy as np
import pytest

from compare_ref import reference_compare
from game_engine_amd import GameTable, GeError, RoomBatch
from oracle.oracle import Oracle
from parity_util import oracle_rooms_as_views, raw_records
from rollout_actions_ref import inject_all
from test_gpu_rollout import GE_ERR_ARG, GE_ERR_RANGE, _assert_words, _dsl, _words

pytestmark = pytest.mark.gpu

SENTINEL = np.uint64(0xA5A5A5A5A5A5A5A5)
LAYOUTS = [("ww", 8), ("ww", 12), ("tt", 4), ("tt", 8), ("tt", 12)]
# the two source rooms of a game: a fresh room played by the oracle until its phase asks for this kind of action (ge_step.h
# GE_ACT_*) - Werewolf: the wolves' target and the day vote, Two-Truths: the speaker's lie and the vote on it
SOURCE_ACTS = {"ww": (1, 4), "tt": (6, 7)}


def _rooms(game, n, generic, seed=0x51):
    """(dsl, oracle, the source records, the turn each stands at)"""
    dsl = _dsl(game + "_generic" if generic else game)
    orc = Oracle(dsl, n)
    recs = orc.init_rooms(len(SOURCE_ACTS[game]))
    at = []
    for i, act in enumerate(SOURCE_ACTS[game]):
        t = 0
        while orc.table.phases[int(recs[i]["phase"])].act != act:
            orc.run(recs[i:i + 1], seed, 40 + i, t, 1)
            t += 1
            assert t < 64, (game, n, act)
        at.append(t)
    return dsl, orc, recs, at


def _legal(orc, rec):
    hi = orc.n if orc.table.pack == 1 else 3
    return {s: [c for c in range(1, hi + 1) if inject_all(orc, rec, [(s, c)])[1] == 0] for s in range(1, orc.n + 1)}


def _advise_entries(orc, recs, seat_view, subjects=None):
    """Per source room and subject seat: every legal choice of an acting seat (the subject itself when it may act), then the
    policy's entry - the baseline of the options before it, and its own."""
    rooms, seats, actions, baseline, subj = [], [], [], [], []
    for room, rec in enumerate(recs):
        legal = _legal(orc, rec)
        actors = [s for s in legal if len(legal[s]) >= 2]
        for s in (subjects or range(1, orc.n + 1)):
            if not actors:
                continue
            a = s if s in actors else actors[s % len(actors)]
            first = len(rooms)
            for c in legal[a]:
                rooms.append(room); seats.append(a if seat_view else 0); actions.append([(a, c)])
            rooms.append(room); seats.append(a if seat_view else 0); actions.append([])
            baseline += [first + len(legal[a])] * (len(legal[a]) + 1)
            subj += [s] * (len(legal[a]) + 1)
    return rooms, seats, actions, baseline, subj


def _assert_ground(cmp, what):
    assert (cmp[:, 1] > 0).any() and (cmp[:, 2] > 0).any(), f"{what}: the reference itself shows no option better and none worse"


def _check(b, orc_of, rooms, keys, turns, seats, actions, baseline, subj, R, M, seed, what):
    want_w, want_s, want_c = reference_compare(orc_of, rooms, keys, turns, seats, actions, baseline, subj, R, M, seed)
    _assert_ground(want_c, what)
    got_w, got_s, got_c = b.rollout_compare(rooms, keys, turns, seats, actions, baseline, subj, R, M, seed=seed)
    print(f"{what}: entries {len(rooms)} better {int(want_c[:, 1].sum())} worse {int(want_c[:, 2].sum())} "
          f"gain {int(want_c[:, 3].sum())} loss {int(want_c[:, 4].sum())}")
    assert got_s.tolist() == want_s.tolist(), what
    _assert_words(got_w, want_w, what)
    assert got_c.dtype == np.uint64 and got_c.shape == want_c.shape
    bad = np.nonzero((got_c != want_c).any(axis=1))[0]
    assert len(bad) == 0, f"{what}: entries {bad.tolist()} got {got_c[bad].tolist()} want {want_c[bad].tolist()}"
    # out and entry_status are rollout_seats's for the same entries, word for word
    seats_w, seats_s = b.rollout_seats(rooms, keys, turns, seats, actions, R, M, seed=seed)
    assert (seats_w == got_w).all() and (seats_s == got_s).all(), what
    return got_c


@pytest.mark.parametrize("view", ["full", "seat"])
@pytest.mark.parametrize("generic", [False, True], ids=["shipped", "generic"])
@pytest.mark.parametrize("game,n", LAYOUTS, ids=lambda v: str(v))
def test_every_subject_matches_the_reference(game, n, generic, view):
    dsl, orc, recs, at = _rooms(game, n, generic)
    rooms, seats, actions, baseline, subj = _advise_entries(orc, recs, view == "seat")
    assert sorted(set(subj)) == list(range(1, n + 1))                         # every seat is a subject
    assert any(bl > k for k, bl in enumerate(baseline))                       # baselines lie behind their entries
    keys = [(7 + r) << 16 for r in rooms]
    turns = [at[r] for r in rooms]
    with RoomBatch([(GameTable(dsl), n, len(recs), 0b1)], seed=3, restart=True) as b:
        b.write_rooms(0, oracle_rooms_as_views(orc, recs))
        got = _check(b, lambda r: (orc, recs[r]), rooms, keys, turns, seats, actions, baseline, subj, 100, 300, 0xC0 + n,
                     f"{game} x {n} generic={generic} {view}")
    pol = [k for k, bl in enumerate(baseline) if bl == k]                      # self-baseline: compared = R, zeros elsewhere
    assert (got[pol, 0] == 100).all() and (got[pol, 1:] == 0).all()
    if orc.table.pack == 1:
        assert (got[:, 3] == got[:, 1]).all() and (got[:, 4] == got[:, 2]).all() and (got[:, 5] == got[:, 1] + got[:, 2]).all()


@pytest.mark.parametrize("R", [1, 63, 64, 100, 4097])
@pytest.mark.parametrize("game,n", [("ww", 8), ("tt", 4)], ids=lambda v: str(v))
def test_partial_last_wavefronts(game, n, R):
    dsl, orc, recs, at = _rooms(game, n, False)
    subjects = range(1, n + 1) if R <= 100 else [1, 2]
    rooms, seats, actions, baseline, subj = _advise_entries(orc, recs, True, subjects)
    keys = [(3 + r) << 16 for r in rooms]
    turns = [at[r] for r in rooms]
    with RoomBatch([(GameTable(dsl), n, len(recs))], seed=3) as b:
        b.write_rooms(0, oracle_rooms_as_views(orc, recs))
        _check(b, lambda r: (orc, recs[r]), rooms, keys, turns, seats, actions, baseline, subj, R, 300, 0xD1, f"{game} x {n} R={R}")


def _mixed():
    games = [("ww", 8), ("tt", 4), ("ww", 12), ("tt", 8)]
    parts = [_rooms(g, n, False, seed=0x77 + i) for i, (g, n) in enumerate(games)]
    per = 2
    segs = [(GameTable(dsl), orc.n, per, 0b10) for dsl, orc, _, _ in parts]
    b = RoomBatch(segs, seed=11, first_room=5, max_fuse=3, restart=True, trace=True)
    for i, (_, orc, recs, _) in enumerate(parts):
        b.write_rooms(i * per, oracle_rooms_as_views(orc, recs))
    return b, games, parts, per


def _interleaved(games, parts, per):
    """Entries of four segments interleaved; every baseline lies behind its entry (the policy entries come last), one option
    per segment is refused, and one policy entry - a baseline - is refused too."""
    opts, pols = [], []
    for i, (_, orc, recs, _) in enumerate(parts):
        room = i * per + 1
        legal = _legal(orc, recs[1])
        a = next(s for s in legal if len(legal[s]) >= 2)
        opts.append([(room, a, [(a, c)]) for c in legal[a]] + [(room, a, [(0, 1)])])      # the last one is refused
        pols.append((room, a, [(a, legal[a][0]), (a, legal[a][0])] if i == 3 else []))     # segment 3's baseline is refused
    rooms, seats, actions, owner = [], [], [], []
    for j in range(max(len(o) for o in opts)):                                # round robin over the segments
        for i, o in enumerate(opts):
            if j < len(o):
                rooms.append(o[j][0]); seats.append(o[j][1]); actions.append(o[j][2]); owner.append(i)
    first_pol = len(rooms)
    for room, a, act in reversed(pols):
        rooms.append(room); seats.append(a); actions.append(act); owner.append(-1)
    baseline = [first_pol + (len(pols) - 1 - i) if i >= 0 else k for k, i in enumerate(owner)]
    subj = list(seats)
    turns = [parts[r // per][3][r % per] for r in rooms]
    keys = [(9 + r) << 16 for r in rooms]
    return rooms, keys, turns, seats, actions, baseline, subj


def test_segments_interleaved_refusals_and_read_only():
    b, games, parts, per = _mixed()
    with b:
        rooms, keys, turns, seats, actions, baseline, subj = _interleaved(games, parts, per)
        orcs = [orc for _, orc, _, _ in parts]
        before = [raw_records(b, s, per, _words(orc)) for s, orc in enumerate(orcs)]
        turn, ev, summary = b.turn, b.read_events(), b.summary()
        got = _check(b, lambda r: (parts[r // per][1], parts[r // per][2][r % per]), rooms, keys, turns, seats, actions, baseline, subj,
                     100, 300, 0xE2, "four segments interleaved")
        want_s = reference_compare(lambda r: (parts[r // per][1], parts[r // per][2][r % per]), rooms, keys, turns, seats, actions,
                                   baseline, subj, 1, 0, 0xE2)[1]
        refused = [k for k in range(len(rooms)) if want_s[k] != 0]
        assert len(refused) == 5                                              # four options and segment 3's baseline
        hit = [k for k in range(len(rooms)) if want_s[k] != 0 or want_s[baseline[k]] != 0]
        assert (got[hit] == 0).all() and len(hit) > len(refused)              # zeros, compared included
        rest = [k for k in range(len(rooms)) if k not in hit]
        assert (got[rest, 0] == 100).all()
        again = b.rollout_compare(rooms, keys, turns, seats, actions, baseline, subj, 100, 300, seed=0xE2)
        assert (again[2] == got).all()
        after = [raw_records(b, s, per, _words(orc)) for s, orc in enumerate(orcs)]
        assert all((x == y).all() for x, y in zip(before, after))
        assert b.turn == turn and (b.read_events() == ev).all() and b.summary() == summary


def test_structural_errors_leave_everything_untouched():
    b, games, parts, per = _mixed()
    with b:
        lib = b._lib

        def call(n, rooms, keys, turns, seats, baseline, subj, R=4, M=4, nulls=()):
            arrs = [np.asarray(rooms, dtype=np.uint64), np.asarray(keys, dtype=np.uint64), np.asarray(turns, dtype=np.uint32),
                    np.asarray(seats, dtype=np.uint32), np.asarray(baseline, dtype=np.uint32), np.asarray(subj, dtype=np.uint32)]
            p = [None if i in nulls else a.ctypes.data for i, a in enumerate(arrs)]
            out = np.full((max(n, 1), 77), SENTINEL, dtype=np.uint64)
            cmp = np.full((max(n, 1), 6), SENTINEL, dtype=np.uint64)
            status = np.full(max(n, 1), 7, dtype=np.int32)
            st = lib.ge_batch_rollout_compare(b._h, n, p[0], p[1], p[2], p[3], None, None, None, status.ctypes.data, R, M, 7,
                                              out.ctypes.data, p[4], p[5], None if 6 in nulls else cmp.ctypes.data)
            assert st == 0 or ((out == SENTINEL).all() and (cmp == SENTINEL).all() and (status == 7).all()), (st, n, nulls)
            return st

        ok = (2, [0, 0], [5, 5], [0, 0], [1, 1], [1, 1], [2, 2])
        assert call(*ok) == 0
        for i in range(7):                                                    # NULL rooms / keys / turns / seats / baseline / subjects / cmp
            assert call(*ok, nulls=(i,)) == GE_ERR_ARG, i
        assert call(2, [0, 0], [5, 5], [0, 0], [1, 1], [1, 2], [2, 2]) == GE_ERR_ARG          # a baseline outside the call
        assert call(2, [0, 1], [5, 5], [0, 0], [1, 1], [1, 1], [2, 2]) == GE_ERR_ARG          # a baseline of another room
        assert call(2, [0, 0], [5, 5], [0, 0], [1, 1], [1, 1], [0, 2]) == GE_ERR_ARG          # subject 0
        assert call(2, [0, 0], [5, 5], [0, 0], [1, 1], [1, 1], [9, 2]) == GE_ERR_ARG          # above Werewolf x 8
        assert call(2, [2, 2], [5, 5], [0, 0], [1, 1], [1, 1], [5, 2]) == GE_ERR_ARG          # above Two-Truths x 4
        big = 65537
        assert call(big, [0] * big, [5] * big, [0] * big, [1] * big, [0] * big, [1] * big, R=1) == GE_ERR_ARG
        # rollout_seats's own checks come first: its caps, its range error and its seat bound before any of the above
        assert call(*ok, R=0) == GE_ERR_ARG and call(*ok, M=4097) == GE_ERR_ARG
        assert call(2, [0, 8], [5, 5], [0, 0], [1, 1], [9, 9], [0, 0], nulls=(4, 5, 6)) == GE_ERR_RANGE
        assert call(2, [0, 0], [5, 5], [0, 0], [9, 1], [9, 9], [0, 0]) == GE_ERR_ARG
        assert call(0, [], [], [], [], [], []) == 0
        with pytest.raises(GeError):
            b.rollout_compare([0, 0], [5, 5], [0, 0], [1, 1], None, [0, 2], [1, 1], 4, 4)

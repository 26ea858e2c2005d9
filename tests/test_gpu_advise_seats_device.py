"""ge_batch_advise_seats (-m gpu): listed seats advised on the device against tests/advise_ref.py (POLICY.md §3m restated by
composition: Oracle.inject for `legal`, the rollout_seats reference for every word) - every field of every (room, seat) of every
room for every layout and table kind, one and two wavefronts per entry, the full view, more entries than one pass holds, a
shuffled order, that the call only reads, that it shares the staging of the indexed calls, and every structural refusal."""
import numpy as np
import pytest

from advise_ref import ADVISE_CASES, GE_ERR_ARG, PER, case_entries, case_reference
from game_engine_amd import GameTable, GeError, RoomBatch
from game_engine_amd.stepper import ADVICE_DTYPE
from parity_util import assert_views_equal, oracle_events, oracle_rooms_as_views
from run_ref import SEED

pytestmark = pytest.mark.gpu

GE_ERR_RANGE = -6
R, M = 70, 48                       # two wavefronts per entry, the second partly filled
EV_FIELDS = ("turn", "from_phase_id", "to_phase_id", "acted_now", "restarted", "choice")
# the advised (room, seat) pairs and their legal options at 16 rooms per segment, from the reference alone
COUNTS = {"ww8_h1": (6, 47), "ww12_h2": (20, 164), "tt4_h1": (10, 28), "tt8_h1": (17, 49), "ww8_generic_h1": (14, 75),
          "tt4_generic_h1": (6, 16), "draft8_h1": (14, 92)}
MIXED_PAIRS = [0, 9, 18, 18]
_TABLES = {}


def _table(dsl):
    if id(dsl) not in _TABLES:
        _TABLES[id(dsl)] = (GameTable(dsl), dsl)                 # (the dsl is kept alive: its id is the key)
    return _TABLES[id(dsl)][0]


def _batch(segs, restart=False, trace=False, seed=SEED, max_fuse=1):
    b = RoomBatch([(_table(dsl), n, len(rooms), mask) for _, dsl, n, mask, rooms in segs], seed=seed, first_room=777, max_fuse=max_fuse,
                  restart=restart, trace=trace)
    base = 0
    for orc, _, _, _, rooms in segs:
        b.write_rooms(base, oracle_rooms_as_views(orc, rooms))
        base += len(rooms)
    return b


def _assert_advice(got, want, what):
    assert got.dtype == ADVICE_DTYPE and len(got) == len(want), what
    for f in ("status", "legal", "best", "phase_id"):
        bad = np.flatnonzero(got[f] != want[f])
        assert not len(bad), (what, f, bad[:5].tolist(), got[f][bad[:5]].tolist(), want[f][bad[:5]].tolist())
    for f in ("finished", "wins", "score"):
        bad = np.flatnonzero(got["policy"][f] != want["policy"][f])
        assert not len(bad), (what, "policy", f, bad[:5].tolist(), got["policy"][f][bad[:5]].tolist(), want["policy"][f][bad[:5]].tolist())
        bad = np.argwhere(got["option"][f] != want["option"][f])
        assert not len(bad), (what, "option", f, bad[:5].tolist())
    refused = got[got["status"] != 0]
    assert not len(refused) or not np.frombuffer(refused.tobytes(), dtype=np.uint32).reshape(len(refused), -1)[:, 1:].any(), f"{what}: a refused entry is not zero"


def _check_counts(name, ref):
    ok = ref["status"] == 0
    assert set(ref["status"].tolist()) <= {0, GE_ERR_ARG}
    options = int(sum(bin(int(m)).count("1") for m in ref["legal"]))
    if name == "mixed":
        rooms = case_entries(name)[1]
        assert [int(ok[rooms // PER == g].sum()) for g in range(4)] == MIXED_PAIRS
        return
    assert (int(ok.sum()), options) == COUNTS[name], (name, int(ok.sum()), options)
    assert ok.sum() >= 5 and (~ok).sum() >= 1, f"{name}: one half of the answer is untested"


@pytest.mark.parametrize("name", ADVISE_CASES)
def test_every_seat_of_every_room_matches_the_reference(name):
    segs, rooms, keys, turns, seats = case_entries(name)
    assert (keys < 1 << 32).any() and (keys > 1 << 32).any()
    ref = case_reference(name, R, M)
    _check_counts(name, ref)
    with _batch(segs) as b:
        got = b.advise_seats(rooms, keys, turns, seats, R, M)
    _assert_advice(got, ref, name)


@pytest.mark.parametrize("n_rollouts,full_view", [(1, False), (64, False), (R, True)])
def test_one_wavefront_and_the_full_view(n_rollouts, full_view):
    segs, rooms, keys, turns, seats = case_entries("ww8_h1")
    ref = case_reference("ww8_h1", n_rollouts, M, full_view)
    with _batch(segs) as b:
        got = b.advise_seats(rooms, keys, turns, seats, n_rollouts, M, full_view=full_view)
    _assert_advice(got, ref, f"ww8_h1 R={n_rollouts} full_view={full_view}")
    if full_view:                                                # (the view matters: the same seats advised from what they know)
        assert not np.array_equal(got["option"]["wins"], case_reference("ww8_h1", R, M)["option"]["wins"])


def test_more_entries_than_a_pass_holds():
    """Werewolf x 12 reserves 13 entries per listed entry: 27 x 192 listed entries reserve 67 392 > 65 536, so the call takes two
    passes; every copy of a pair must equal the reference's record of the pair."""
    segs, rooms, keys, turns, seats = case_entries("ww12_h2")
    ref = case_reference("ww12_h2", 1, 8)
    reps = 27
    assert reps * len(rooms) * 13 > 65536 and len(rooms) == 192
    with _batch(segs) as b:
        got = b.advise_seats(np.tile(rooms, reps), np.tile(keys, reps), np.tile(turns, reps), np.tile(seats, reps), 1, 8)
    assert (ref["status"] == 0).sum() == 20
    _assert_advice(got, np.tile(ref, reps), "two passes")


def test_a_shuffled_order_gives_the_permuted_result():
    segs, rooms, keys, turns, seats = case_entries("mixed")
    ref = case_reference("mixed", R, M)
    perm = np.random.default_rng(5).permutation(len(rooms))
    with _batch(segs) as b:
        got = b.advise_seats(rooms[perm], keys[perm], turns[perm], seats[perm], R, M)
    _assert_advice(got, ref[perm], "mixed, shuffled")


def _state(b, trace):
    return (b.read_rooms().tobytes(), b.seats().tobytes(), b.turn, b.read_events().tobytes() if trace else b"", b.summary()["checksum"])


@pytest.mark.parametrize("how", ["plain", "seat_plane", "restart_trace"])
def test_advise_seats_reads_only(how):
    segs, rooms, keys, turns, seats = case_entries("mixed")
    trace = how == "restart_trace"
    with _batch(segs, restart=trace, trace=trace, max_fuse=3) as b:   # (a trace holds max_fuse turns)
        if how == "seat_plane":
            b.set_seats([1, 20, 40, 63], [0b101, 0b1, 0, 0b1000001])
        b.step(3)
        before = _state(b, trace)
        got = b.advise_seats(rooms, keys, turns, seats, 5, 20)
        assert _state(b, trace) == before
        assert (got["status"] == 0).any() and (got["status"] != 0).any()


def test_advise_seats_shares_the_staging_of_the_indexed_calls():
    """step_rooms, an advise_seats large enough to regrow the scratch, step_rooms and read_rooms_at: events and views equal the
    oracle's."""
    segs, rooms, keys, turns, seats = case_entries("ww12_h2")
    orc, _, _, mask, recs = segs[0]
    recs = recs.copy()
    listed = np.array([3, 0, 11, 7], dtype=np.uint64)
    with _batch(segs) as b:
        for rnd, (skeys, sturns) in enumerate([([5, 1 << 35, 7, 8], [0, 4, 9, 100]), ([9, 10, 1 << 40, 12], [1, 5, 10, 101])]):
            ev = b.step_rooms(listed, skeys, sturns)
            for k, r in enumerate(listed):
                one = recs[int(r):int(r) + 1]
                orc.run(one, SEED, int(skeys[k]), int(sturns[k]), 1, threads=1, restart=False, human_mask=mask)
                want = oracle_events(orc, one, int(sturns[k]))[0]
                for f in EV_FIELDS:
                    assert np.array_equal(ev[k][f], want[f]), (rnd, int(r), f)
            if rnd == 0:
                got = b.advise_seats(np.tile(rooms, 8), np.tile(keys, 8), np.tile(turns, 8), np.tile(seats, 8), 1, 4)
                assert len(got) == 8 * 192
        assert_views_equal(b.read_rooms_at(listed), oracle_rooms_as_views(orc, recs[listed.astype(np.int64)]), "after the advice")


def test_structural_errors_leave_the_output_untouched():
    segs = case_entries("mixed")[0]                              # segments of 6, 4, 10 and 7 players, 16 rooms each
    with _batch(segs) as b:
        lib = b._lib

        def call(n, rooms, keys, turns, seats, n_rollouts, max_turns, flags=0, nulls=()):
            arrs = [np.asarray(rooms, dtype=np.uint64), np.asarray(keys, dtype=np.uint64), np.asarray(turns, dtype=np.uint32),
                    np.asarray(seats, dtype=np.uint32)]
            ptrs = [None if i in nulls else a.ctypes.data for i, a in enumerate(arrs)]
            out = np.full(max(n, 1) * ADVICE_DTYPE.itemsize, 0xA5, dtype=np.uint8)
            st = lib.ge_batch_advise_seats(b._h, n, *ptrs, n_rollouts, max_turns, 7, flags, None if 4 in nulls else out.ctypes.data)
            return st, bool((out == 0xA5).all())

        ok = ([0], [0], [0], [1])
        for i in range(5):                                       # NULL rooms / keys / turns / seats / out
            assert call(1, *ok, 4, 4, nulls=(i,)) == (GE_ERR_ARG, True), i
        for args, want in [((1,) + ok + (4, 4, 2), GE_ERR_ARG),                                   # an unknown flag bit
                           ((1,) + ok + (4, 4, 0x80000001), GE_ERR_ARG),
                           ((1,) + ok + (0, 4), GE_ERR_ARG), ((1,) + ok + ((1 << 20) + 1, 4), GE_ERR_ARG),
                           ((1,) + ok + (4, 4097), GE_ERR_ARG),
                           ((1, [0], [0], [0], [0], 4, 4), GE_ERR_ARG),                            # seat 0
                           ((1, [0], [0], [0], [7], 4, 4), GE_ERR_ARG),                            # above the segment's 6
                           ((2, [0, 16], [0, 0], [0, 0], [6, 5], 4, 4), GE_ERR_ARG),               # above the segment's 4
                           ((1, [33], [0], [0], [11], 4, 4), GE_ERR_ARG),
                           ((2, [0, 64], [0, 0], [0, 0], [1, 1], 4, 4), GE_ERR_RANGE),             # a room outside the batch
                           ((1, [0], [0], [0xFFFFFFFF - 3], [1], 4, 4), GE_ERR_RANGE),             # turn + max_turns
                           ((10, [0] * 10, [0] * 10, [0] * 10, [1] * 10, 1 << 20, 4), GE_ERR_ARG),  # 10 x 7 x 2^20 > 2^26
                           ((13, [16] * 13, [0] * 13, [0] * 13, [1] * 13, 1 << 20, 4), GE_ERR_ARG)]:   # Two-Truths x 4: 13 x 5 x 2^20
            assert call(*args) == (want, True), (args[0], args[5:], call(*args))
        assert call(0, [], [], [], [], 0, 9999, 77) == (0, True)   # n == 0: GE_OK, nothing read
        assert call(1, [0], [0], [0xFFFFFFFF - 4], [1], 4, 4)[0] == 0   # the last turns a room can take
        assert call(9, [0] * 9, [0] * 9, [0] * 9, [1] * 9, 1 << 20, 0)[0] == 0   # 9 x 7 x 2^20 <= 2^26 (no turns played)
        with pytest.raises(GeError):
            b.advise_seats([0], [0], [0], [7], 4, 4)
        with pytest.raises(GeError):
            b.advise_seats([0, 1], [0], [0, 0], [1, 1], 4, 4)
        assert len(b.advise_seats([], [], [], [], 4, 4)) == 0


def test_refused_entries_are_zero_behind_the_status_and_the_call_succeeds():
    segs, rooms, keys, turns, seats = case_entries("ww8_h1")
    ref = case_reference("ww8_h1", R, M)
    refused = np.flatnonzero(ref["status"] != 0)
    assert len(refused) > 100
    with _batch(segs) as b:
        out = np.full(len(refused) * ADVICE_DTYPE.itemsize, 0xA5, dtype=np.uint8)
        arrs = [np.ascontiguousarray(a[refused]) for a in (rooms, keys, turns, seats)]   # (kept alive across the call)
        st = b._lib.ge_batch_advise_seats(b._h, len(refused), *[a.ctypes.data for a in arrs], R, M, SEED, 0, out.ctypes.data)
        assert st == 0                                           # a call of nothing but refusals is a valid call
        got = out.view(ADVICE_DTYPE)
        assert (got["status"] == GE_ERR_ARG).all()
        assert not out.view(np.uint32).reshape(len(refused), -1)[:, 1:].any()


def test_repeated_pairs_and_determinism():
    segs, rooms, keys, turns, seats = case_entries("tt8_h1")
    ref = case_reference("tt8_h1", R, M)
    pick = np.flatnonzero(ref["status"] == 0)[:6]
    idx = np.concatenate([pick, pick[::-1], pick])
    with _batch(segs) as b:
        x = b.advise_seats(rooms[idx], keys[idx], turns[idx], seats[idx], R, M)
        y = b.advise_seats(rooms[idx], keys[idx], turns[idx], seats[idx], R, M)
    assert x.tobytes() == y.tobytes()
    _assert_advice(x, ref[idx], "repeated pairs")


def test_an_advised_option_is_rollout_seats_own_entry():
    """The composition on the GPU itself: option c of an advised seat against rollout_seats of (seat, [(seat, c)])."""
    segs, rooms, keys, turns, seats = case_entries("draft8_h1")
    with _batch(segs) as b:
        adv = b.advise_seats(rooms, keys, turns, seats, 200, 64)
        k = int(np.flatnonzero(adv["status"] == 0)[0])
        s = int(seats[k])
        cs = [c for c in range(1, 13) if (int(adv["legal"][k]) >> (c - 1)) & 1]
        words, st = b.rollout_seats([rooms[k]] * (len(cs) + 1), [keys[k]] * (len(cs) + 1), [turns[k]] * (len(cs) + 1), [s] * (len(cs) + 1),
                                    [[(s, c)] for c in cs] + [[]], 200, 64)
    assert (st == 0).all()
    for j, c in enumerate(cs):
        assert tuple(adv["option"][k][c - 1]) == (words[j][1], words[j][41 + 12 + s - 1], words[j][41 + 24 + s - 1]), c
    assert tuple(adv["policy"][k]) == (words[-1][1], words[-1][41 + 12 + s - 1], words[-1][41 + 24 + s - 1])
    assert int(adv["best"][k]) == cs[int(np.argmax([words[j][41 + 12 + s - 1] for j in range(len(cs))]))]

"""ge_batch_step_rooms_playout (-m gpu): playout seats (POLICY.md §3d) against the oracle-side reference tests/playout_ref.py for
every layout, shipped and GENERIC, seat view and full view, from fuzzed and oracle-played states with every bot seat a playout
seat; mask 0 and max_turns = 0 equal to ge_batch_step_rooms; every choice the argmax of a separate ge_batch_rollout_seats call;
unlisted rooms, the turn counter and the trace untouched; all-or-nothing refusals; determinism; no leak from the seat's view;
and full-view village bots that win more games than the policy."""
import copy

import numpy as np
import pytest

from conftest import golden_dsl, load_golden
from game_engine_amd import GameTable, GeError, RoomBatch
from oracle.oracle import Oracle
from oracle.rng import pick
from parity_util import assert_views_equal, oracle_events, oracle_rooms_as_views, raw_records, views_as_oracle_rooms
from playout_ref import SEAT_WINS, candidates, due_seats, reference_step_playout, seat_draw
from test_gpu_rollout import _dsl, _views, _words
from test_gpu_rollout_seats import _swapped
from test_gpu_run_playout import _all_bot_ww8
from test_gpu_run_rooms import _batch as _run_batch

pytestmark = pytest.mark.gpu

GE_ERR_ARG, GE_ERR_RANGE = -1, -6
EV_FIELDS = ("turn", "from_phase_id", "to_phase_id", "acted_now", "restarted", "choice")
R_SMALL, M_SMALL = 64, 48


def _played(orc, R, rng):
    """R oracle rooms played from the start for 0 .. 39 turns each (night, day-vote, lie and vote phases among them)."""
    rooms = orc.init_rooms(R)
    for i in range(R):
        one = rooms[i:i + 1]
        orc.run(one, int(rng.integers(0, 1 << 30)), int(rng.integers(0, 1 << 20)), 0, int(rng.integers(0, 40)))
    return rooms


def _source(games, rng, R=16, restart=False, trace=False):
    """A batch of segments (game, n, human mask): half its rooms oracle-played, half fuzzed; the oracle rooms of each."""
    parts, segs = [], []
    for game, n, hmask in games:
        dsl = _dsl(game)
        orc = Oracle(dsl, n)
        recs = _played(orc, R // 2, rng)
        views = np.concatenate([oracle_rooms_as_views(orc, recs), _views(orc, game, R - R // 2, rng)])
        parts.append((orc, views_as_oracle_rooms(orc, views), hmask))
        segs.append(((GameTable(dsl), n, R, hmask), views))
    b = RoomBatch([s for s, _ in segs], seed=0x5EED, first_room=41, max_fuse=1, restart=restart, trace=trace)
    for k, (_, views) in enumerate(segs):
        b.write_rooms(k * R, views)
    return b, parts, R


def _all_bots(parts, R, rooms):
    return [((1 << parts[r // R][0].n) - 1) & ~parts[r // R][2] for r in rooms]


def _reference(parts, R_src, rooms, keys, turns, masks, pkeys, seed, pseed, R, M, full_view, restart=False):
    """(oracle rooms after the call, events, decided) of the reference, for the whole batch."""
    after = [(orc, orooms.copy()) for orc, orooms, _ in parts]
    events, decided = [], []
    for room, key, turn, mask, pkey in zip(rooms, keys, turns, masks, pkeys):
        g, i = int(room) // R_src, int(room) % R_src
        orc, orooms = after[g]
        decided.append(reference_step_playout(orc, orooms, i, seed, int(key), int(turn), int(mask), int(pkey), pseed, R, M, full_view,
                                              restart, parts[g][2]))
        events.append(oracle_events(orc, orooms[i:i + 1], int(turn))[0])
    return after, events, np.array(decided, dtype=np.uint32)


def _assert_matches(b, after, R_src, events, decided, want_events, want_decided, rooms, what):
    for g, (orc, orooms) in enumerate(after):
        assert_views_equal(b.read_rooms(g * R_src, R_src), oracle_rooms_as_views(orc, orooms), f"{what} segment {g}")
    for k in range(len(rooms)):
        for f in EV_FIELDS:
            assert np.array_equal(events[k][f], want_events[k][f]), (what, k, int(rooms[k]), f, events[k][f], want_events[k][f])
    assert decided.tolist() == want_decided.tolist(), what


CASES = [[("ww", 8, 0)], [("ww", 12, 0)], [("tt", 4, 0)], [("tt", 8, 0)], [("tt", 12, 0)], [("draft", 8, 0)],
         [("ww_generic", 8, 0)], [("tt_generic", 5, 0)], [("ww", 8, 0b10000001)],
         [("ww", 6, 0), ("tt", 4, 0b10), ("ww", 10, 0), ("tt", 7, 0)]]


@pytest.mark.parametrize("full_view", [False, True], ids=["seat", "full"])
@pytest.mark.parametrize("games", CASES, ids=lambda g: "+".join(f"{n}x{k}" + (f"h{m:x}" if m else "") for n, k, m in g))
def test_step_rooms_playout_matches_the_reference(games, full_view):
    rng = np.random.default_rng(sum(k * 13 + m for _, k, m in games) + full_view)
    b, parts, R_src = _source(games, rng)
    total = R_src * len(games)
    seed, pseed = 0x5EED, 0xF00D + full_view
    n_decided = 0
    for rnd in range(3):
        rooms = rng.permutation(total)[: total - 2].astype(np.uint64)               # two rooms unlisted
        keys = rng.integers(0, 1 << 40, len(rooms)).astype(np.uint64)
        turns = rng.integers(0, 50000, len(rooms)).astype(np.uint32)
        masks = np.array(_all_bots(parts, R_src, rooms), dtype=np.uint32)
        masks[::5] &= rng.integers(0, 1 << 12, len(masks[::5])).astype(np.uint32)  # some rooms with fewer playout seats
        pkeys = rng.integers(0, 1 << 63, len(rooms)).astype(np.uint64)
        after, want_ev, want_dec = _reference(parts, R_src, rooms, keys, turns, masks, pkeys, seed, pseed, R_SMALL, M_SMALL, full_view)
        ev, dec = b.step_rooms_playout(rooms, keys, turns, masks, pkeys, R_SMALL, M_SMALL, seed=pseed, full_view=full_view)
        _assert_matches(b, after, R_src, ev, dec, want_ev, want_dec, rooms, f"{games} round {rnd}")
        n_decided += int(sum(bin(int(d)).count("1") for d in dec))
        parts = [(orc, orooms, h) for (orc, orooms), (_, _, h) in zip(after, parts)]
    assert n_decided > 0
    b.close()


GOLDEN = ["traj_werewolf_n8.json", "traj_werewolf_n12.json", "traj_two_truths_and_a_lie_n4.json", "traj_two_truths_and_a_lie_n8.json",
          "traj_two_truths_and_a_lie_n12.json", "traj_variant_ww_generic_n8.json", "traj_draft_werewolf_n8.json"]


@pytest.mark.parametrize("full_view", [False, True], ids=["seat", "full"])
@pytest.mark.parametrize("name", GOLDEN)
def test_golden_trajectory_states_match_the_reference(name, full_view):
    """The states of a golden trajectory (the oracle replays it; its projections are the golden's), each stepped as the
    trajectory's own room at its own turn with every seat a playout seat."""
    g = load_golden(name)
    orc = Oracle(golden_dsl(g), g["n_players"], g.get("rounds", 1))
    case = g["cases"][0]
    one, states, turns = orc.init_rooms(1), [], []
    for t, want in enumerate(case["turns"][:40]):
        states.append(one[0].copy()); turns.append(t)
        orc.run(one, case["seed"], case["room"], t, 1)
        assert orc.project(one[0], declared_only=True) == want, t
    recs = np.stack(states)
    n = len(recs)
    with RoomBatch([(GameTable(golden_dsl(g)), orc.n, n, 0)], seed=case["seed"], max_fuse=1) as b:
        b.write_rooms(0, oracle_rooms_as_views(orc, recs))
        rooms = np.arange(n, dtype=np.uint64)
        keys = np.full(n, case["room"], np.uint64)
        tt = np.array(turns, np.uint32)
        masks = np.full(n, (1 << orc.n) - 1, np.uint32)
        pkeys = (np.arange(n, dtype=np.uint64) + 3) << np.uint64(16)
        parts = [(orc, recs.copy(), 0)]
        after, want_ev, want_dec = _reference(parts, n, rooms, keys, tt, masks, pkeys, case["seed"], 0xF00D, R_SMALL, M_SMALL, full_view)
        ev, dec = b.step_rooms_playout(rooms, keys, tt, masks, pkeys, R_SMALL, M_SMALL, seed=0xF00D, full_view=full_view)
        _assert_matches(b, after, n, ev, dec, want_ev, want_dec, rooms, name)
        assert dec.any()


def _tt2():
    """Two-Truths for 2 players (a DSL whose min_players allows it): a seat has 3 candidates but the room only 2 players."""
    dsl = copy.deepcopy(_dsl("tt"))
    dsl["declaration"]["min_players"] = 2
    return GameTable(dsl)


def test_two_player_two_truths_reserves_three_candidates_per_seat():
    """Every seat a playout seat in 2-player Two-Truths rooms: each decided choice is the argmax of a separate rollout_seats
    call over statements 1..3, max_turns = 0 is step_rooms word for word, and the cost cap counts 3 candidates per seat."""
    tb, n, R_src = _tt2(), 2, 64
    b1 = RoomBatch([(tb, n, R_src, 0)], seed=0x5EED, max_fuse=1)
    b2 = RoomBatch([(tb, n, R_src, 0)], seed=0x5EED, max_fuse=1)
    rng = np.random.default_rng(29)
    rooms = np.arange(R_src, dtype=np.uint64)
    masks = np.full(R_src, 0b11, np.uint32)
    checked = zero_checked = 0
    for t in range(24):
        keys = (rooms + 1000).astype(np.uint64)
        turns = np.full(R_src, t, np.uint32)
        pkeys = rng.integers(0, 1 << 63, R_src).astype(np.uint64)
        views = b1.read_rooms()
        b2.write_rooms(0, views)
        q = [(r, s, c) for r in range(R_src) for s in (1, 2) for c in (1, 2, 3)]
        words, st = b2.rollout_seats([r for r, _, _ in q], [int(pkeys[r]) for r, _, _ in q], [t] * len(q), [s for _, s, _ in q],
                                     [[(s, c)] for _, s, c in q], 128, 40, seed=0xAB)
        ev, dec = b1.step_rooms_playout(rooms, keys, turns, masks, pkeys, 128, 40, seed=0xAB)
        for r in range(R_src):
            for s in (1, 2):
                if not (int(dec[r]) >> (s - 1)) & 1:
                    continue
                vals = [(int(words[k][SEAT_WINS + s - 1]), c) for k, (rr, ss, c) in enumerate(q) if rr == r and ss == s]
                assert all(st[k] == 0 for k, (rr, ss, _) in enumerate(q) if rr == r and ss == s)
                top = max(v for v, _ in vals)
                tied = [c for v, c in vals if v == top]
                assert int(ev[r]["choice"][s - 1]) == tied[pick(seat_draw(0x5EED, 1000 + r, t, s), len(tied))], (t, r, s, vals)
                checked += 1
        # the same state under max_turns = 0 is the policy's turn
        b2.write_rooms(0, views)
        want = b2.step_rooms(rooms, keys, turns)
        after_policy = b2.read_rooms()
        b2.write_rooms(0, views)
        ev0, dec0 = b2.step_rooms_playout(rooms, keys, turns, masks, pkeys, 16, 0, seed=0xAB)
        assert ev0.tobytes() == want.tobytes() and b2.read_rooms().tobytes() == after_policy.tobytes(), t
        zero_checked += int(dec0.any())
    assert checked > 0 and zero_checked > 0
    with pytest.raises(GeError) as e:                                  # 11 rooms x 2 seats x 3 candidates x 2^20 > 2^26
        b1.step_rooms_playout(rooms[:11], rooms[:11], np.zeros(11, np.uint32), masks[:11], rooms[:11], 1 << 20, 1)
    assert e.value.status == GE_ERR_ARG
    b1.step_rooms_playout(rooms[:10], rooms[:10], np.zeros(10, np.uint32), masks[:10], rooms[:10], 1 << 20, 0)   # 60 x 2^20: allowed
    b1.close(); b2.close()


def test_restart_batches_and_several_due_seats():
    """GE_FLAG_RESTART (no decision in a restart-terminal turn) and rooms where several playout seats decide at once."""
    rng = np.random.default_rng(3)
    b, parts, R_src = _source([("ww", 8, 0), ("tt", 4, 0)], rng, R=24, restart=True)
    rooms = np.arange(48, dtype=np.uint64)
    several = 0
    for rnd in range(4):
        keys = rng.integers(0, 1 << 40, 48).astype(np.uint64)
        turns = rng.integers(0, 5000, 48).astype(np.uint32)
        masks = np.array(_all_bots(parts, R_src, rooms), dtype=np.uint32)
        pkeys = rng.integers(0, 1 << 63, 48).astype(np.uint64)
        after, want_ev, want_dec = _reference(parts, R_src, rooms, keys, turns, masks, pkeys, 0x5EED, 9, 32, 40, False, restart=True)
        ev, dec = b.step_rooms_playout(rooms, keys, turns, masks, pkeys, 32, 40, seed=9)
        _assert_matches(b, after, R_src, ev, dec, want_ev, want_dec, rooms, f"restart round {rnd}")
        several += int(sum(1 for d in dec if bin(int(d)).count("1") >= 2))
        parts = [(orc, orooms, h) for (orc, orooms), (_, _, h) in zip(after, parts)]
    assert several > 0
    b.close()


def _twins(games, seed=11, R=32):
    rng = np.random.default_rng(seed)
    b1, parts, R_src = _source(games, rng, R=R)
    views = b1.read_rooms()
    b2 = RoomBatch([(GameTable(_dsl(g)), n, R, m) for g, n, m in games], seed=0x5EED, first_room=41, max_fuse=1)
    b2.write_rooms(0, views)
    return b1, b2, parts, R_src


@pytest.mark.parametrize("games", [[("ww", 8, 0)], [("ww", 12, 0)], [("tt", 8, 0)], [("ww", 6, 0), ("tt", 4, 0b10)]],
                         ids=lambda g: "+".join(f"{n}x{k}" for n, k, _ in g))
def test_mask_zero_and_zero_max_turns_are_step_rooms(games):
    b1, b2, parts, R_src = _twins(games)
    rng = np.random.default_rng(5)
    total = R_src * len(games)
    decided = 0
    for rnd in range(6):
        rooms = rng.permutation(total).astype(np.uint64)
        keys = rng.integers(0, 1 << 40, total).astype(np.uint64)
        turns = rng.integers(0, 50000, total).astype(np.uint32)
        pkeys = rng.integers(0, 1 << 63, total).astype(np.uint64)
        want = b2.step_rooms(rooms, keys, turns)
        if rnd % 2 == 0:
            ev, dec = b1.step_rooms_playout(rooms, keys, turns, np.zeros(total, np.uint32), pkeys, 64, 48, seed=3)
            assert not dec.any()
        else:
            masks = np.array(_all_bots(parts, R_src, rooms), dtype=np.uint32)
            ev, dec = b1.step_rooms_playout(rooms, keys, turns, masks, pkeys, 16, 0, seed=3)
            decided |= int(np.bitwise_or.reduce(dec))
        assert ev.tobytes() == want.tobytes(), rnd
        for g, (orc, _, _) in enumerate(parts):
            assert np.array_equal(raw_records(b1, g, R_src, _words(orc)), raw_records(b2, g, R_src, _words(orc))), (rnd, g)
    assert decided != 0                                   # max_turns = 0: decisions were made, and every one was the policy's
    b1.close(); b2.close()


@pytest.mark.parametrize("game,n,full_view", [("ww", 8, False), ("ww", 12, True), ("tt", 8, False), ("ww_generic", 8, False)])
def test_every_choice_is_the_argmax_of_rollout_seats(game, n, full_view):
    """Device only, R = 1024: the decided choice is the argmax (tie-break pick(d, m)) of a separate rollout_seats call."""
    b1, b2, parts, R_src = _twins([(game, n, 0)], seed=17, R=48)
    orc = parts[0][0]
    rng = np.random.default_rng(23)
    R, M, pseed, seed = 1024, 96, 0xAB, 0x5EED
    checked = 0
    for rnd in range(3):
        rooms = np.arange(R_src, dtype=np.uint64)
        keys = rng.integers(0, 1 << 40, R_src).astype(np.uint64)
        turns = rng.integers(0, 50000, R_src).astype(np.uint32)
        pkeys = rng.integers(0, 1 << 63, R_src).astype(np.uint64)
        recs = views_as_oracle_rooms(orc, b1.read_rooms())
        q_rooms, q_keys, q_turns, q_seats, q_acts, owner = [], [], [], [], [], []
        for r in range(R_src):
            for s in due_seats(orc, recs[r], seed, int(keys[r]), int(turns[r]), False, 0):
                cand = candidates(orc, recs[r], s)
                if len(cand) < 2:
                    continue
                for c in cand:
                    q_rooms.append(r); q_keys.append(int(pkeys[r])); q_turns.append(int(turns[r]))
                    q_seats.append(0 if full_view else s); q_acts.append([(s, c)]); owner.append((r, s, c))
        words, st = b1.rollout_seats(q_rooms, q_keys, q_turns, q_seats, q_acts, R, M, seed=pseed)
        assert not st.any()
        best = {}
        for (r, s, c), w in zip(owner, words):
            best.setdefault((r, s), []).append((int(w[SEAT_WINS + s - 1]), c))
        ev, dec = b1.step_rooms_playout(rooms, keys, turns, (1 << n) - 1 + np.zeros(R_src, np.uint32), pkeys, R, M, seed=pseed,
                                        full_view=full_view)
        for (r, s), vals in best.items():
            top = max(v for v, _ in vals)
            tied = [c for v, c in vals if v == top]
            assert (int(dec[r]) >> (s - 1)) & 1, (r, s)
            assert int(ev[r]["choice"][s - 1]) == tied[pick(seat_draw(seed, int(keys[r]), int(turns[r]), s), len(tied))], (r, s, vals)
            checked += 1
        assert sum(bin(int(d)).count("1") for d in dec) == len(best)
    assert checked > 0
    b1.close(); b2.close()


@pytest.mark.parametrize("halving", [False, True], ids=["plain", "halving"])
def test_step_rooms_playout_across_the_pass_boundary(halving):
    """1 025 rooms x 8 playout seats x 8 candidates: a capacity of 65 600 entries, two passes.  A listed room's result depends only
    on its own record, keys and turn, so the one call equals the list given in two calls that stay inside one pass each."""
    segs, listed, keys, turns, masks, pkeys, _ = _all_bot_ww8(1100, 1025, 5)
    with _run_batch(segs, True) as b, _run_batch(segs, True) as twin:
        ev, dec = b.step_rooms_playout(listed, keys, turns, masks, pkeys, 4, 8, seed=11, halving=halving)
        halves = [twin.step_rooms_playout(listed[s], keys[s], turns[s], masks[s], pkeys[s], 4, 8, seed=11, halving=halving)
                  for s in (slice(0, 512), slice(512, 1025))]
        assert ev.tobytes() == np.concatenate([h[0] for h in halves]).tobytes()
        assert dec.tolist() == np.concatenate([h[1] for h in halves]).tolist()
        assert b.read_rooms().tobytes() == twin.read_rooms().tobytes()
    assert dec[-64:].any(), "the second pass decided nothing"


def test_unlisted_rooms_turn_counter_and_trace_untouched_and_determinism():
    rng = np.random.default_rng(31)
    games = [("ww", 8, 0), ("tt", 4, 0)]
    b1, parts, R_src = _source(games, rng, R=32, trace=True)
    b2, _, _ = _source(games, np.random.default_rng(31), R=32, trace=True)
    for b in (b1, b2):
        b.step(1)                                                               # (a traced batch steps one launch at a time)
        b.step(1)
    ev_before = b1.read_events()
    turn_before = b1.turn
    raw_before = [raw_records(b1, g, R_src, _words(orc)) for g, (orc, _, _) in enumerate(parts)]
    rooms = np.arange(0, 64, 2, dtype=np.uint64)                                # every other room
    keys = rng.integers(0, 1 << 40, 32).astype(np.uint64)
    turns = rng.integers(0, 50000, 32).astype(np.uint32)
    masks = np.array(_all_bots(parts, R_src, rooms), dtype=np.uint32)
    pkeys = rng.integers(0, 1 << 63, 32).astype(np.uint64)
    out = [b.step_rooms_playout(rooms, keys, turns, masks, pkeys, 64, 48, seed=5) for b in (b1, b2)]
    assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1].tolist() == out[1][1].tolist()
    for g, (orc, _, _) in enumerate(parts):
        got = raw_records(b1, g, R_src, _words(orc))
        assert np.array_equal(got[1::2], raw_before[g][1::2]), g                # the unlisted rooms
        assert np.array_equal(got, raw_records(b2, g, R_src, _words(orc))), g   # the same call, the same records
    assert b1.turn == turn_before
    assert b1.read_events().tobytes() == ev_before.tobytes()
    b1.close(); b2.close()


def test_refusals_are_all_or_nothing():
    rng = np.random.default_rng(37)
    b, parts, R_src = _source([("ww", 8, 0b1), ("ww", 12, 0)], rng, R=8)
    words = [_words(orc) for orc, _, _ in parts]
    before = [raw_records(b, g, R_src, words[g]) for g in range(2)]
    rooms, keys, turns = [0, 1, 9], [1, 2, 3], [4, 5, 6]
    masks, pkeys = [0b10, 0b100, 0xFFF], [7, 8, 9]

    def call(status, rooms=rooms, keys=keys, turns=turns, masks=masks, pkeys=pkeys, R=8, M=8, full_view=False):
        with pytest.raises(GeError) as e:
            b.step_rooms_playout(rooms, keys, turns, masks, pkeys, R, M, seed=1, full_view=full_view)
        assert e.value.status == status
        for g in range(2):
            assert np.array_equal(raw_records(b, g, R_src, words[g]), before[g])

    call(GE_ERR_RANGE, rooms=[0, 1, 16])                                          # room outside the batch
    call(GE_ERR_RANGE, turns=[4, 0xFFFFFFFF, 6])
    call(GE_ERR_ARG, rooms=[0, 1, 0])                                             # repeated room
    call(GE_ERR_ARG, R=0)
    call(GE_ERR_ARG, R=(1 << 20) + 1)
    call(GE_ERR_ARG, M=4097)
    call(GE_ERR_RANGE, turns=[4, 0xFFFFFFFF - 7, 6], M=8)
    call(GE_ERR_ARG, masks=[0b10, 0b100000000, 0xFFF])                            # seat 9 of an 8-player room
    call(GE_ERR_ARG, masks=[0b11, 0b100, 0xFFF])                                  # seat 1 is host-driven in segment 0
    call(GE_ERR_ARG, masks=[0b10, 0b100, 0x1FFF])                                 # seat 13 of a 12-player room
    call(GE_ERR_ARG, R=1 << 20)                                                   # (1 + 1 + 12) x 12 ... x 2^20 > 2^26
    with pytest.raises(GeError):
        b.step_rooms_playout(rooms, keys, turns, masks[:2], pkeys, 8, 8)
    st = b._lib.ge_batch_step_rooms_playout(b._h, 3, np.array(rooms, np.uint64).ctypes.data, np.array(keys, np.uint64).ctypes.data,
                                            np.array(turns, np.uint32).ctypes.data, np.array(masks, np.uint32).ctypes.data,
                                            np.array(pkeys, np.uint64).ctypes.data, 8, 8, 1, 2, None, None)
    assert st == GE_ERR_ARG                                                       # an unknown flag
    for g in range(2):
        assert np.array_equal(raw_records(b, g, R_src, words[g]), before[g])
    b.close()


def test_seat_view_does_not_leak():
    """Swapping the hidden tuples of two seats the playout seat cannot tell apart leaves its choice unchanged."""
    orc = Oracle(_dsl("ww"), 8)
    rng = np.random.default_rng(41)
    recs, swaps, seats = [], [], []
    while len(recs) < 48:
        one = orc.init_rooms(1)
        orc.run(one, int(rng.integers(0, 1 << 30)), 1, 0, int(rng.integers(6, 30)))
        rec = one[0]
        if orc.table.phases[int(rec["phase"])].branches == []:
            continue
        for s in range(1, 9):
            if rec["p"][s - 1][1] == 2 or rec["p"][s - 1][0] == 4 or not rec["p"][s - 1][2]:
                continue                                                       # a living seat that knows no team
            sw = _swapped(orc, rec, s)
            if sw is not None:
                recs.append(rec.copy()); swaps.append(sw); seats.append(s)
                break
    n = len(recs)
    with RoomBatch([(GameTable(_dsl("ww")), 8, 2 * n, 0)], seed=0x5EED) as b:
        checked = 0
        for t in range(4):
            rooms = np.arange(2 * n, dtype=np.uint64)
            keys = np.tile(np.arange(n, dtype=np.uint64) * 7 + 1000 * t, 2)
            turns = np.full(2 * n, 100 + t, np.uint32)
            masks = np.tile(np.array([1 << (s - 1) for s in seats], np.uint32), 2)
            pkeys = np.tile(np.arange(n, dtype=np.uint64) + 5, 2)
            b.write_rooms(0, oracle_rooms_as_views(orc, np.concatenate([np.stack(recs), np.stack(swaps)])))
            ev, dec = b.step_rooms_playout(rooms, keys, turns, masks, pkeys, 128, 64, seed=77)
            for k in range(n):
                s = seats[k]
                assert int(dec[k]) == int(dec[n + k]), k
                if dec[k]:
                    assert int(ev[k]["choice"][s - 1]) == int(ev[n + k]["choice"][s - 1]), (k, s)
                    checked += 1
        assert checked > 0


def _play_to_the_end(b, R, n, village_bots, turns=200):
    rooms = np.arange(R, dtype=np.uint64)
    keys = rooms + 5000
    for t in range(turns):
        if village_bots:
            v = b.read_rooms()
            masks = np.zeros(R, np.uint32)
            for i in range(n):
                masks |= ((v["players"][:, i, 1] == 1).astype(np.uint32) << i)           # team villagers
            b.step_rooms_playout(rooms, keys, np.full(R, t, np.uint32), masks, keys + 1, 64, 256, seed=0xACE, full_view=True)
        else:
            b.step_rooms(rooms, keys, np.full(R, t, np.uint32))
    v = b.read_rooms()
    alive_wolves = ((v["players"][:, :n, 2] != 0) & (v["players"][:, :n, 1] == 2)).sum(axis=1)
    finished = v["end_turn"] >= 0
    return int((finished & (alive_wolves == 0)).sum()), int(finished.sum())


def test_full_view_village_bots_win_more():
    """256 Werewolf x 8 games to the end on a fixed seed: the village side's seats as full-view playout bots win strictly more
    games than the same games under step_rooms (deterministic runs: not flaky).  Measured on an MI355X: the policy's village
    wins 55 of 256, full-view village playout bots 256 of 256."""
    dsl = _dsl("ww")
    res = []
    for bots in (False, True):
        with RoomBatch([(GameTable(dsl), 8, 256, 0)], seed=0x5EED) as b:
            res.append(_play_to_the_end(b, 256, 8, bots))
    (v0, f0), (v1, f1) = res
    print(f"village wins: policy {v0}/{f0}, full-view village playout bots {v1}/{f1}")
    assert f0 > 200 and f1 > 200
    assert v1 > v0
    assert (v0, v1) == (55, 256)                          # the recorded counts: a change in the bots' strength shows here

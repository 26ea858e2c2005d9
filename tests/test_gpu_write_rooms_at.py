"""ge_batch_write_rooms_at (-m gpu): the indexed write.  Random views scattered into random distinct rooms of every layout must
lie in HBM exactly as ge_batch_write_rooms stores them, leave every other record bit-identical, read back through the indexed
read, and play on exactly as the oracle from the same states - fused, single-turn and indexed steps, with role deals in play.
Refusals write nothing."""
import numpy as np
import pytest

from game_engine_amd import GameTable, GeError, RoomBatch
from oracle.oracle import Oracle
from parity_util import assert_records_canonical, assert_views_equal, oracle_events, oracle_rooms_as_views, raw_records, views_as_oracle_rooms
from test_gpu_step_rooms import _dsl, _views, _words

pytestmark = pytest.mark.gpu

GE_ERR_ARG, GE_ERR_RANGE = -1, -6
CASES = [[("ww", 4)], [("ww", 8)], [("ww", 12)], [("tt", 3)], [("tt", 4)], [("tt", 12)], [("draft", 8)],
         [("ww_generic", 8)], [("tt_generic", 5)], [("ww", 6), ("tt", 4), ("ww", 10), ("tt", 7)]]


def _setup(games, rng):
    parts, segs, before, fresh = [], [], [], []
    for game, n in games:
        dsl = _dsl(game)
        orc = Oracle(dsl, n)
        R = int(rng.integers(300, 700))
        before.append(_views(orc, game, R, rng))
        fresh.append(_views(orc, game, R, rng))
        parts.append(orc)
        segs.append((GameTable(dsl), n, R))
    return parts, segs, np.concatenate(before), np.concatenate(fresh)


def _raws(b, parts, segs):
    return np.concatenate([np.pad(raw_records(b, s, segs[s][2], _words(orc)), ((0, 0), (0, 12 - _words(orc))))
                           for s, orc in enumerate(parts)])


@pytest.mark.parametrize("max_fuse", [0, 1])
@pytest.mark.parametrize("games", CASES, ids=lambda g: "+".join(f"{n}x{k}" for n, k in g))
def test_scatter_stores_what_write_rooms_stores_and_plays_on(games, max_fuse):
    rng = np.random.default_rng(sum(k for _, k in games) * 31 + max_fuse)
    seed, first = 0x5CA7 + len(games), 777
    parts, segs, before, fresh = _setup(games, rng)
    total = len(before)
    rooms = rng.permutation(total)[: int(rng.integers(total // 4, total // 2))].astype(np.uint64)
    with RoomBatch(segs, seed=seed, first_room=first, max_fuse=max_fuse) as b, RoomBatch(segs, seed=seed, first_room=first) as w:
        b.write_rooms(0, before)
        b.step(3)                                                  # prepared deals in play (records and the x 12 side plane)
        raw0, views0 = _raws(b, parts, segs), b.read_rooms()
        b.write_rooms_at(rooms, fresh[rooms.astype(np.int64)])
        want_views = views0.copy()
        want_views[rooms.astype(np.int64)] = fresh[rooms.astype(np.int64)]
        w.write_rooms(0, want_views)                               # what ge_batch_write_rooms stores for the same views
        raw1, raww = _raws(b, parts, segs), _raws(w, parts, segs)
        listed = np.zeros(total, dtype=bool)
        listed[rooms.astype(np.int64)] = True
        assert (raw1[listed] == raww[listed]).all(), "scattered records differ from ge_batch_write_rooms'"
        assert (raw1[~listed] == raw0[~listed]).all(), "an unlisted record changed"
        assert_views_equal(b.read_rooms_at(rooms), w.read_rooms_at(rooms), "read_rooms_at after the scatter")
        got = b.read_rooms()
        base = 0
        oracle_parts = []
        for s, orc in enumerate(parts):
            R = segs[s][2]
            o = views_as_oracle_rooms(orc, got[base:base + R])
            assert_records_canonical(b, s, orc, o, f"segment {s} after the scatter")
            oracle_parts.append((orc, o, base))
            base += R
        # ordinary steps from here (fused or single-turn), against the oracle over every room
        turn0 = b.turn
        b.step(7)
        after = b.read_rooms()
        for s, (orc, o, base) in enumerate(oracle_parts):
            orc.run(o, seed, first + base, turn0, 7, threads=0)
            assert_views_equal(after[base:base + len(o)], oracle_rooms_as_views(orc, o), f"segment {s}, {7} turns after the scatter")
        # and indexed steps after a second scatter, each room under its own key and turn
        sub = rng.permutation(total)[:64].astype(np.uint64)
        b.write_rooms_at(sub, fresh[sub.astype(np.int64)])
        keys = rng.integers(0, 1 << 40, len(sub)).astype(np.uint64)
        turns = rng.integers(0, 5000, len(sub)).astype(np.uint32)
        ev = b.step_rooms(sub, keys, turns)
        got = b.read_rooms_at(sub)
        for k, r in enumerate(sub.astype(np.int64)):
            base = 0
            for s, seg in enumerate(segs):
                if r < base + seg[2]:
                    break
                base += seg[2]
            orc = parts[s]
            one = views_as_oracle_rooms(orc, fresh[r:r + 1])
            orc.run(one, seed, int(keys[k]), int(turns[k]), 1, threads=1)
            assert_views_equal(got[k:k + 1], oracle_rooms_as_views(orc, one), f"indexed step of room {r}")
            want_ev = oracle_events(orc, one, int(turns[k]))[0]
            for f in ("turn", "from_phase_id", "to_phase_id", "acted_now", "restarted", "choice"):
                assert np.array_equal(ev[k][f], want_ev[f]), (r, f)


def test_scatter_quarter_million_entries_into_a_million_rooms():
    from conftest import load_dsl
    dsl = load_dsl("werewolf-(mafia)")
    orc = Oracle(dsl, 8)
    R, n = 1 << 20, 262144
    rng = np.random.default_rng(5)
    rooms = rng.permutation(R)[:n].astype(np.uint64)
    views = _views(orc, "ww", n, rng)
    with RoomBatch([(GameTable(dsl), 8, R)], seed=9, first_room=0) as b:
        b.step(5)
        before = b.read_rooms()
        b.write_rooms_at(rooms, views)
        got = b.read_rooms()
        want = before.copy()
        want[rooms.astype(np.int64)] = views
        assert_views_equal(got, want, "1 M rooms after the scatter")
        o = views_as_oracle_rooms(orc, got)
        b.step(4)
        orc.run(o, 9, 0, 5, 4, threads=0)
        assert_views_equal(b.read_rooms(), oracle_rooms_as_views(orc, o), "4 turns after the scatter")


@pytest.mark.parametrize("games", [CASES[1], CASES[2], CASES[-1]], ids=["ww8", "ww12", "mixed"])
def test_refusals_write_nothing(games):
    from game_engine_amd import _lib
    rng = np.random.default_rng(3)
    parts, segs, before, fresh = _setup(games, rng)
    total = len(before)
    with RoomBatch(segs, seed=1) as b:
        b.write_rooms(0, before)
        b.step(2)
        raw0 = _raws(b, parts, segs)
        lib = _lib.load()

        def call(rooms, views):
            rooms = np.ascontiguousarray(rooms, dtype=np.uint64)
            views = np.ascontiguousarray(views)
            return lib.ge_batch_write_rooms_at(b._h, len(rooms), rooms.ctypes.data, views.ctypes.data)

        ok = rng.permutation(total)[:10]
        assert call(np.append(ok, total), fresh[np.append(ok, 0)]) == GE_ERR_RANGE
        assert call(np.append(ok, ok[3]), fresh[np.append(ok, ok[3])]) == GE_ERR_ARG
        bad = fresh[ok].copy()
        bad[6]["phase_id"] = 4242
        assert call(ok, bad) == GE_ERR_ARG
        assert lib.ge_last_rejected_room() == int(ok[6])
        bad = fresh[ok].copy()
        bad[2]["n_players"] = int(bad[2]["n_players"]) + 1
        with pytest.raises(GeError, match=f"room {int(ok[2])} does not fit"):
            b.write_rooms_at(ok, bad)
        assert call([], fresh[:0]) == 0
        assert (_raws(b, parts, segs) == raw0).all(), "a refused scatter changed a record"

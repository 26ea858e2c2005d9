"""ge_batch_summary against the host summary reference (oracle/summary.py) (-m gpu): every word, checksum included, for
every record layout on both kernel builds, ragged mixed batches, states no real game reaches (scores past the last
bucket, late end turns, recycled slots, terminal rooms whose end turn was never set); the raw records in HBM are the
canonical packing the checksum is defined over, after single-turn and after fused launches; and the checksum moves, by
what the reference predicts, when any one field of any one room changes or a state moves to another room."""
import numpy as np
import pytest

from conftest import load_dsl
from game_engine_amd import GameTable, RoomBatch
from oracle.oracle import Oracle
from oracle.summary import reference_summary_words
from parity_util import (assert_records_canonical, assert_summary_equal, assert_views_equal, oracle_rooms_as_views,
                         views_as_oracle_rooms)
from test_gpu_fuzz import _random_tt_views, _random_ww_views

pytestmark = pytest.mark.gpu
WW, TT = "werewolf-(mafia)", "two-truths-and-a-lie"
LAYOUTS = [(WW, 8), (WW, 11), (TT, 4), (TT, 7), (TT, 12)]        # Werewolf x 8 / x 12, Two-Truths x 4 / x 8 / x 12


def random_views(orc, n, R, rng):
    """Random states (test_gpu_fuzz's builders) with what they leave out: end turns from 0 to the saturated 65 534 (or unset,
    also in terminal phases), recycled-game counts, Two-Truths scores up to 199."""
    if orc.table.pack == 1:
        v = _random_ww_views(orc, n, R, rng, consistent=False)
    else:
        v = _random_tt_views(orc, n, R, rng, rounds=1)
    v["end_turn"] = np.where(rng.integers(0, 3, R) == 0, -1, rng.choice([3, 64, 120, 127, 128, 500, 65534], R))
    v["games"] = rng.integers(0, 3000, R)
    terminal = [p.id for p in orc.table.phases if not p.branches]
    v["phase_id"][::7] = terminal[0]
    return v


def _case(game, n, R, fuse, seed=0xC0FFEE, first=(1 << 32) - 1000):
    dsl = load_dsl(game)
    orc = Oracle(dsl, n)
    rng = np.random.default_rng(n * 1000 + R % 997 + fuse)
    views = random_views(orc, n, R, rng)
    return dsl, orc, views, views_as_oracle_rooms(orc, views), seed, first


@pytest.mark.parametrize("fuse", [1, 16])
@pytest.mark.parametrize("R", [3001, 70001])                     # lone-wavefront build / large-batch build
@pytest.mark.parametrize("game,n", LAYOUTS)
def test_summary_and_raw_records_equal_reference(game, n, R, fuse):
    """Written random states, then blocks of turns in steady state: after the write and after every block, every room ==
    oracle, every raw record == its canonical packing, every summary word == the reference."""
    dsl, orc, views, rooms, seed, first = _case(game, n, R, fuse)
    with RoomBatch([(GameTable(dsl), n, R)], seed=seed, first_room=first, max_fuse=fuse, restart=True) as b:
        b.step(5)
        b.write_rooms(0, views)
        assert_summary_equal(b.summary_words(), reference_summary_words([(orc.table, n, rooms)], first, 5), "written states")
        fin = np.array([not orc.table.phases[int(p)].branches for p in rooms["phase"]])
        assert (fin & (rooms["end_turn"] < 0)).any() and (rooms["end_turn"] >= 120).any() and rooms["games"].any()
        for chunk in (1, 16, 3):
            b.step(chunk)
            orc.run(rooms, seed, first, b.turn - chunk, chunk, threads=0, restart=True)
            what = f"{game} x{n}, {R} rooms, max_fuse {fuse}, turn {b.turn}"
            assert_views_equal(b.read_rooms(), oracle_rooms_as_views(orc, rooms), what)
            assert_records_canonical(b, 0, orc, rooms, what)
            assert_summary_equal(b.summary_words(), reference_summary_words([(orc.table, n, rooms)], first, b.turn), what)
        if orc.table.pack == 2:
            assert b.summary()["score_hist"][15] > 0


@pytest.mark.parametrize("fuse", [1, 16])
def test_ragged_mixed_batch_summary_equals_reference(fuse):
    """Four segments whose ends fall inside 4 096-room summary blocks (the kernel walks 16 chunks of 256 rooms per block,
    one segment per block): summary == reference, records canonical, every room == oracle."""
    segs = [(WW, 6, 5000), (TT, 4, 4097), (WW, 10, 257), (TT, 9, 8191)]
    seed, first = 77, 1 << 40
    parts = []
    for k, (game, n, R) in enumerate(segs):
        dsl, orc, views, rooms, _, _ = _case(game, n, R, fuse + k)
        parts.append((GameTable(dsl), orc, views, rooms))
    with RoomBatch([(p[0], segs[k][1], segs[k][2]) for k, p in enumerate(parts)], seed=seed, first_room=first,
                   max_fuse=fuse, restart=True) as b:
        b.step(2)
        base = 0
        for (_, _, views, _), (_, _, R) in zip(parts, segs):
            b.write_rooms(base, views)
            base += R
        for chunk in (0, 1, 16):
            if chunk:
                b.step(chunk)
            base = 0
            for k, ((_, orc, _, rooms), (game, n, R)) in enumerate(zip(parts, segs)):
                if chunk:
                    orc.run(rooms, seed, first + base, b.turn - chunk, chunk, threads=0, restart=True)
                assert_views_equal(b.read_rooms(base, R), oracle_rooms_as_views(orc, rooms), f"segment {k} turn {b.turn}")
                assert_records_canonical(b, k, orc, rooms, f"segment {k} turn {b.turn}")
                base += R
            want = reference_summary_words([(p[1].table, n, p[3]) for p, (_, n, _) in zip(parts, segs)], first, b.turn)
            assert_summary_equal(b.summary_words(), want, f"ragged mixed batch, turn {b.turn}")


def _other_values(orc, n, view):
    """(description, one-room view array) for every field of `view` changed to another valid value: phase ids, phase-0
    guard, end turn, games, and every player field (and Detective memory) of the first and the last seat."""
    ids = [p.id for p in orc.table.phases]
    ww = orc.table.pack == 1
    mod = [5, 3, 2, 2, 2, 2, 2, 2, n + 1, 2, n + 1] if ww else [2, 2, 4, 2, 2, 4, 2, 256, 16, 2, 4]
    out = []

    def changed(what, f):
        v = np.array([view], dtype=view.dtype)
        f(v[0])
        out.append((what, v))

    def field(name, value):
        return lambda r: r.__setitem__(name, value(int(r[name])))
    changed("phase_id", field("phase_id", lambda x: ids[(ids.index(x) + 1) % len(ids)]))
    changed("prev_phase_id", field("prev_phase_id", lambda x: ids[(ids.index(x) + 3) % len(ids)]))
    changed("phase0_done", field("phase0_done", lambda x: 1 - x))
    changed("end_turn", field("end_turn", lambda x: 130 if x < 0 else -1))
    changed("games", field("games", lambda x: x + 1))
    for seat in (0, n - 1):
        for f in range(11):
            def g(r, seat=seat, f=f):
                r["players"][seat, f] = (int(r["players"][seat, f]) + 1) % mod[f]
            changed(f"player {seat + 1} field {f}", g)
        if ww:
            def d(r, seat=seat):
                r["det"][seat] = (int(r["det"][seat]) + 1) % 3
            changed(f"player {seat + 1} detective memory", d)
    return out


@pytest.mark.parametrize("game,n", LAYOUTS)
def test_checksum_moves_with_every_field_and_room_index(game, n):
    """One room's view changed in one field, every field in turn, written with ge_batch_write_rooms: the checksum changes,
    by what the reference predicts (the other summary words follow the reference too).  Exchanging two rooms' states changes
    it as well: the hash is keyed by the global room index."""
    R, first = 300, 123456789
    dsl, orc, views, rooms, _, _ = _case(game, n, R, 0, first=first)
    with RoomBatch([(GameTable(dsl), n, R)], seed=1, first_room=first) as b:
        b.write_rooms(0, views)
        base = b.summary_words()
        assert_summary_equal(base, reference_summary_words([(orc.table, n, rooms)], first, 0), "base")
        k = 17
        for what, v in _other_values(orc, n, views[k]):
            b.write_rooms(k, v)
            got = b.summary_words()
            mod = rooms.copy()
            mod[k:k + 1] = views_as_oracle_rooms(orc, v)
            assert got[38] != base[38], f"{game} x{n}: checksum blind to {what}"
            assert_summary_equal(got, reference_summary_words([(orc.table, n, mod)], first, 0), what)
            b.write_rooms(k, views[k:k + 1])
        assert np.array_equal(b.summary_words(), base)
        swapped = views[[k + 1, k]].copy()
        assert views[k].tobytes() != views[k + 1].tobytes()
        b.write_rooms(k, swapped)
        got = b.summary_words()
        assert got[38] != base[38] and np.array_equal(np.delete(got, 38), np.delete(base, 38))
        mod = rooms.copy()
        mod[k:k + 2] = rooms[[k + 1, k]]
        assert_summary_equal(got, reference_summary_words([(orc.table, n, mod)], first, 0), "two rooms exchanged")

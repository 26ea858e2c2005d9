"""ge_batch_run_rooms_forecast without a GPU (POLICY.md §3i): the exported symbol and its C99 prototype, the oracle-side
reference (tests/timeline_ref.py) against its own invariants, proof on the oracle alone that the inputs the GPU tests share are
not vacuous, and the services' bookkeeping of run_room(forecast=True) against oracle-backed batches: element 0 of "forecasts" is
forecast() before the run, the last element forecast() after it."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from game_engine_amd import _lib
from rollout_ref import reference_rollout
from rollout_seats_ref import reference_rollout_seats
from run_ref import CASES, END, PERSON, SEED, run_ref
from timeline_ref import FSEED, N_ROLLOUTS, PLAYOUT_MAX_TURNS, ROOMS_PER_SEGMENT, SHAPES, reference_timeline, timeline_inputs, timeline_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_symbol():
    lib = _lib.load()
    assert "ge_batch_run_rooms_forecast" in _lib.SYMBOLS and lib.ge_batch_run_rooms_forecast is not None
    assert lib.ge_batch_run_rooms_forecast(None, 0, None, None, None, 1, 0, None, None, 1, 0, 0, None, None, None, None, 0, None, 0) == -1


def test_header_declares_run_rooms_forecast(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text("""
#include "ge_step.h"
int (*p)(ge_batch *, uint64_t, const uint64_t *, const uint64_t *, const uint32_t *, uint32_t, uint32_t, const uint64_t *, const uint32_t *,
         uint32_t, uint32_t, uint64_t, uint32_t *, uint32_t *, ge_turn_event *, ge_room_view *, size_t, ge_rollout_stats *, size_t)
    = ge_batch_run_rooms_forecast;
int main(void) { return p == 0 || GE_ABI_VERSION != 5; }
""")
    subprocess.check_call([cc, "-std=c99", "-pedantic", "-Werror", "-Wall", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "t.o")])


@pytest.mark.parametrize("name", ["ww8_h1", "tt4_h2", "mixed"])
def test_reference_without_playout_turns_is_the_unplayed_record(name):
    """playout_max_turns = 0, full view: every point's words are the statistics of n_rollouts copies of the point's own record."""
    from oracle.summary import reference_summary_words
    from parity_util import views_as_oracle_rooms
    from rollout_ref import seat_words
    segs, listed, keys, turns, fkeys, _ = timeline_inputs(name, True)
    full = np.zeros(len(listed), dtype=np.uint32)
    played, _, _, views, _, stats = reference_timeline(segs, listed, keys, turns, 5, 0, True, fkeys, full, 9, 0, FSEED)
    for k, r in enumerate(listed):
        s, i = divmod(int(r), ROOMS_PER_SEGMENT)
        orc, _, _, _, rooms = segs[s]
        assert stats[k].shape == (int(played[k]) + 1, 77)
        for p in range(int(played[k]) + 1):
            rec = rooms[i:i + 1] if p == 0 else views_as_oracle_rooms(orc, np.array(views[k][p - 1]).reshape(1))
            copies = np.concatenate([rec] * 9)
            assert np.array_equal(stats[k][p][:41], reference_summary_words([(orc.table, orc.n, copies)], int(fkeys[k]), int(turns[k]) + p))
            assert np.array_equal(stats[k][p][41:], seat_words(orc, copies))


@pytest.mark.parametrize("name", ["ww8_h2", "tt8_h1", "mixed"])
def test_reference_last_point_is_point_zero_of_the_follow_up_call(name):
    restart = False
    segs, listed, keys, turns, fkeys, seats = timeline_inputs(name, restart)
    args = (fkeys, seats, N_ROLLOUTS, PLAYOUT_MAX_TURNS, FSEED)
    played, _, _, _, after, stats = reference_timeline(segs, listed, keys, turns, 4, PERSON | END, restart, *args)
    segs2 = [(orc, dsl, n, mask, rooms) for (orc, dsl, n, mask, _), rooms in zip(segs, after)]
    _, _, _, _, _, stats2 = reference_timeline(segs2, listed, keys, turns + played, 3, 0, restart, *args)
    for k in range(len(listed)):
        assert np.array_equal(stats[k][int(played[k])], stats2[k][0]), (name, k)


def test_the_shared_inputs_are_not_vacuous():
    """On the oracle alone, over the inputs and sizes tests/test_gpu_timeline.py uses: an entry stopped by PERSON before the limit,
    one by END, one at the limit; a point where every playout finished and one where only some did; a point whose seat view gives
    other words than its full view."""
    need = {"person", "end", "limit", "all_finished", "some_finished", "seat_differs"}
    for name in sorted(CASES):
        for restart in (False, True):
            segs, listed, keys, turns, fkeys, seats = timeline_inputs(name, restart)
            assert len(listed) == 6 * len(CASES[name]) and (seats[1::2] != 0).any() and not seats[::2].any()
            for max_turns, until in SHAPES:
                played, stopped, _, views, _, stats = reference_timeline(segs, listed, keys, turns, max_turns, until, restart, fkeys, seats,
                                                                         N_ROLLOUTS, PLAYOUT_MAX_TURNS, FSEED)
                if ((stopped & PERSON) != 0)[played < max_turns].any():
                    need.discard("person")
                if ((stopped & END) != 0).any():
                    need.discard("end")
                if ((stopped == 0) & (played == max_turns)).any() and until:
                    need.discard("limit")
                for k, st in enumerate(stats):
                    fin = st[:, 1]
                    if (fin == N_ROLLOUTS).any():
                        need.discard("all_finished")
                    if ((fin > 0) & (fin < N_ROLLOUTS)).any():
                        need.discard("some_finished")
                    if seats[k] and "seat_differs" in need:
                        s, i = divmod(int(listed[k]), ROOMS_PER_SEGMENT)
                        orc, _, _, _, rooms = segs[s]
                        full = timeline_of(orc, rooms[i], views[k], FSEED, fkeys[k], turns[k], 0, N_ROLLOUTS, PLAYOUT_MAX_TURNS)
                        if not np.array_equal(full, st):
                            need.discard("seat_differs")
            if not need:
                return
    assert not need, need


# ---- service bookkeeping: oracle-backed batches, run_rooms_forecast restated by run_ref + timeline_of
def _oracle_services():
    from game_engine_amd import RoomPoolService, RoomService
    from game_engine_amd.stepper import EVENT_DTYPE, ROOM_VIEW_DTYPE
    from oracle.oracle import Oracle
    from test_messages import _OracleBatch
    from test_room_pool import _OracleChunk

    class Mixin:
        def run_rooms(self, rooms, keys, turns, max_turns, until):
            self.calls["run_rooms"] = self.calls.get("run_rooms", 0) + 1
            return self._run(rooms, keys, turns, max_turns, until)[:4]

        def _run(self, rooms, keys, turns, max_turns, until, fc=None):
            n = len(rooms)
            played, stopped = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
            events, views = np.zeros((n, max_turns), dtype=EVENT_DTYPE), np.zeros((n, max_turns), dtype=ROOM_VIEW_DTYPE)
            stats = np.zeros((n, max_turns + 1, 77), dtype=np.uint64)
            for k in range(n):
                start = self.rooms[int(rooms[k])].copy()
                p, why, ev, vw = run_ref(self.orc, self.rooms, int(rooms[k]), self.seed, int(keys[k]), int(turns[k]), max_turns, until, False, self.mask)
                played[k], stopped[k], events[k, :p], views[k, :p] = p, why, ev, vw
                if fc:
                    fkeys, seats, R, M, seed = fc
                    stats[k, :p + 1] = timeline_of(self.orc, start, vw, seed, fkeys[k], turns[k], seats[k], R, M)
            return played, stopped, events, views, stats

        def run_rooms_forecast(self, rooms, keys, turns, forecast_keys, n_rollouts, playout_max_turns=1024, seats=None, seed=0, max_turns=64,
                               until=3):
            self.calls["run_rooms_forecast"] = self.calls.get("run_rooms_forecast", 0) + 1
            assert len(set(int(r) for r in rooms)) == len(rooms)
            return self._run(rooms, keys, turns, max_turns, until, (forecast_keys, seats or [0] * len(rooms), n_rollouts, playout_max_turns, seed))

        def rollout_rooms(self, rooms, keys, turns, n_rollouts, max_turns=1024, seed=None):
            return np.stack([reference_rollout(self.orc, self.rooms[int(r)].copy(), seed, int(k), int(t), n_rollouts, max_turns)
                             for r, k, t in zip(rooms, keys, turns)])

        def rollout_seats(self, rooms, keys, turns, seats, actions=None, n_rollouts=4096, max_turns=1024, seed=None):
            assert actions is None
            res = [reference_rollout_seats(self.orc, self.rooms[int(r)].copy(), seed, int(k), int(t), int(s), [], n_rollouts, max_turns)
                   for r, k, t, s in zip(rooms, keys, turns, seats)]
            return np.stack([w for w, _ in res]), np.array([s for _, s in res], dtype=np.int32)

    class Batch(Mixin, _OracleBatch):
        def __init__(self, *a):
            super().__init__(*a)
            self.calls = {}

        def set_turn(self, turn):
            self.turn = turn

    class Chunk(Mixin, _OracleChunk):
        pass

    chunks = []

    class One(RoomService):
        def _new_batch(self, tb, n_players, human_mask, first_room):
            return Batch(Oracle(tb.dsl, n_players), self.seed, first_room, human_mask)

    class Pool(RoomPoolService):
        def _new_chunk(self, tb, n_players, human_mask, n_rooms):
            chunks.append(Chunk(Oracle(tb.dsl, n_players), self.seed, n_rooms, human_mask))
            return chunks[-1]

    return One, Pool, chunks


def _players(n, humans=()):
    return [{"name": f"P{i + 1}", "gamePlayerId": i + 1, "isBot": (i + 1) not in humans} for i in range(n)]


@pytest.mark.parametrize("game,n,humans,seat", [("werewolf-(mafia)", 8, (1,), 3), ("werewolf-(mafia)", 8, (), None),
                                                ("two-truths-and-a-lie", 4, (2,), 1)])
def test_run_room_forecasts_are_the_forecasts_around_the_run(game, n, humans, seat):
    import json
    from conftest import load_dsl
    from test_strings_golden import _strip
    One, Pool, chunks = _oracle_services()
    dsl = load_dsl(game)
    R, M = 12, 30
    svcs = [One(seed=11), Pool(seed=11, chunk_rooms=3)]
    twin = One(seed=11)
    for s in svcs + [twin]:
        for t in ("a", "b"):
            s.create_room(t, game, _players(n, humans), dsl=dsl)
    for rnd, (until, max_turns) in enumerate(((("person", "end"), 20), ((), 3), (("end",), 64))):
        before = [s.forecast("a", R, M, seat) for s in svcs]
        plain = twin.run_room("a", max_turns, until)
        outs = [svcs[0].run_room("a", max_turns, until, forecast=True, forecast_rollouts=R, forecast_max_turns=M, forecast_seat=seat),
                svcs[1].run_rooms(["b", "a"], max_turns, until, forecast=True, forecast_rollouts=R, forecast_max_turns=M,
                                  forecast_seats=[None, seat])[1]]
        after = [s.forecast("a", R, M, seat) for s in svcs]
        for o, f0, f1 in zip(outs, before, after):
            assert list(o) == ["turns", "played", "stopped", "forecasts"] and len(o["forecasts"]) == o["played"] + 1
            assert o["forecasts"][0] == f0 and o["forecasts"][-1] == f1, (game, rnd)
            assert [f["turn"] for f in o["forecasts"]] == [f0["turn"] + p for p in range(o["played"] + 1)]
            assert ("seat" in f0) == (seat is not None) and json.loads(json.dumps(o["forecasts"])) == o["forecasts"]
            # without the option the output is today's: the twin's plain run_room, key for key
            assert list(plain) == ["turns", "played", "stopped"]
            assert _strip({k: o[k] for k in plain}) == _strip(plain), (game, rnd)
        assert outs[0]["forecasts"] == outs[1]["forecasts"]
    assert sum(c.calls.get("run_rooms_forecast", 0) for c in chunks) == 3 and not any(c.calls.get("run_rooms", 0) for c in chunks)
    for s in svcs + [twin]:
        s.close()


def test_forecast_refusals_leave_the_thread_where_it_is():
    from conftest import load_dsl
    One, Pool, chunks = _oracle_services()
    dsl = load_dsl("two-truths-and-a-lie")
    one, pool = One(seed=3), Pool(seed=3, chunk_rooms=8)
    for s in (one, pool):
        s.create_room("t", "two-truths-and-a-lie", _players(4), dsl=dsl)
        s.create_room("p", "two-truths-and-a-lie", _players(4), dsl=dsl, playout_seats=(2,))
        s.continue_room("t")
    before = (one._rooms["t"]["batch"].rooms.tobytes(), one._rooms["t"]["batch"].turn, chunks[0].rooms.tobytes(), pool._rooms["t"]["turn"])
    bad = [dict(forecast_rollouts=0), dict(forecast_rollouts=65537), dict(forecast_max_turns=4097), dict(forecast_max_turns=-1),
           dict(forecast_seat=0), dict(forecast_seat=5), dict(max_turns=4096, forecast_rollouts=65536), dict(max_turns=0)]
    for kw in bad:
        with pytest.raises(ValueError):
            one.run_room("t", **{"max_turns": 8, "forecast": True, **kw})
        with pytest.raises(ValueError):
            pool.run_room("t", **{"max_turns": 8, "forecast": True, **kw})
    for playout in (False, True):                                 # a thread with playout seats: refused with or without playout=True
        with pytest.raises(ValueError):
            one.run_room("p", 8, playout=playout, forecast=True)
        with pytest.raises(ValueError):
            pool.run_rooms(["t", "p"], 8, playout=playout, forecast=True)
    with pytest.raises(ValueError):
        pool.run_rooms(["t"], 8, forecast=True, forecast_seats=[1, 2])
    assert before == (one._rooms["t"]["batch"].rooms.tobytes(), one._rooms["t"]["batch"].turn, chunks[0].rooms.tobytes(), pool._rooms["t"]["turn"])
    assert not any(c.calls.get("run_rooms_forecast", 0) for c in chunks) and not one._rooms["t"]["batch"].calls

"""ge_batch_rollout_rooms on the CPU side: the C99 header's ge_rollout_stats layout, rollout_to_dict, and RoomPoolService's
forecasts with its chunks stood in for by an oracle-backed batch that implements rollout_rooms (as test_room_pool.py's
_OracleChunk does for step_rooms): keys, seed, grouping by chunk, output shape and the service-level cap."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import load_dsl
from rollout_ref import reference_rollout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_pins_the_rollout_record(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text("""
#include <stddef.h>
#include "ge_step.h"
_Static_assert(sizeof(ge_summary) == 41 * 8, "summary");
_Static_assert(sizeof(ge_rollout_stats) == 616, "rollout stats");
_Static_assert(offsetof(ge_rollout_stats, summary) == 0, "summary first");
_Static_assert(offsetof(ge_rollout_stats, seat_alive) == 328, "seat_alive");
_Static_assert(offsetof(ge_rollout_stats, seat_wins) == 424, "seat_wins");
_Static_assert(offsetof(ge_rollout_stats, seat_score) == 520, "seat_score");
int (*p)(ge_batch *, uint64_t, const uint64_t *, const uint64_t *, const uint32_t *, uint32_t, uint32_t, uint64_t, ge_rollout_stats *) =
    ge_batch_rollout_rooms;
int main(void) { return p == 0; }
""")
    subprocess.check_call([cc, "-std=c99", "-pedantic", "-Werror", "-Wall", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "t.o")])


def test_ctypes_record_and_symbol():
    from game_engine_amd import _lib
    assert C.sizeof(_lib.RolloutStats) == 616 and _lib.ROLLOUT_WORDS == 77
    assert _lib.RolloutStats.seat_alive.offset == 328 and _lib.RolloutStats.seat_score.offset == 520
    assert "ge_batch_rollout_rooms" in _lib.SYMBOLS


def test_rollout_to_dict():
    from game_engine_amd.stepper import rollout_to_dict, summary_to_dict
    w = np.arange(77, dtype=np.uint64) * np.uint64(3) + np.uint64(1)
    d = rollout_to_dict(w)
    assert d["summary"] == summary_to_dict(w[:41])
    assert d["seat_alive"] == [int(x) for x in w[41:53]]
    assert d["seat_wins"] == [int(x) for x in w[53:65]]
    assert d["seat_score"] == [int(x) for x in w[65:77]]
    assert d["summary"]["turn"] == int(w[39]) and d["summary"]["games_recycled"] == int(w[40])


class _OracleChunk:
    """The subset of RoomBatch a RoomPoolService chunk uses for forecasts and turns, run by the oracle (CPU tests only)."""

    def __init__(self, orc, seed, n_rooms, human_mask):
        self.orc, self.seed, self.mask = orc, seed, human_mask
        self.rooms = orc.init_rooms(n_rooms)
        self.rollout_calls = []

    def step_rooms(self, rooms, keys, turns):
        from parity_util import oracle_events
        from game_engine_amd.stepper import EVENT_DTYPE
        ev = np.zeros(len(rooms), dtype=EVENT_DTYPE)
        for k, r in enumerate(int(x) for x in rooms):
            one = self.rooms[r:r + 1]
            self.orc.run(one, self.seed, int(keys[k]), int(turns[k]), 1, human_mask=self.mask)
            ev[k] = oracle_events(self.orc, one, int(turns[k]))[0]
        return ev

    def read_rooms_at(self, rooms):
        from parity_util import oracle_rooms_as_views
        return oracle_rooms_as_views(self.orc, self.rooms[np.asarray(rooms, dtype=np.int64)]).copy()

    def inject_actions(self, rooms, players, choices):
        return np.array([0 if self.orc.inject(self.rooms, int(r), int(p), int(c)) else -1
                         for r, p, c in zip(rooms, players, choices)], dtype=np.int32)

    def write_rooms(self, first, views):
        from parity_util import views_as_oracle_rooms
        self.rooms[first:first + len(views)] = views_as_oracle_rooms(self.orc, views)

    def rollout_rooms(self, rooms, keys, turns, n_rollouts, max_turns=1024, seed=None):
        seed = self.seed if seed is None else seed
        self.rollout_calls.append(([int(r) for r in rooms], [int(k) for k in keys], [int(t) for t in turns], n_rollouts, max_turns, seed))
        return np.stack([reference_rollout(self.orc, self.rooms[int(r)].copy(), seed, int(k), int(t), n_rollouts, max_turns)
                         for r, k, t in zip(rooms, keys, turns)])

    def close(self):
        pass


def _service(chunk_rooms=2, seed=0x5EED):
    from game_engine_amd import RoomPoolService
    from oracle.oracle import Oracle
    chunks = []

    class Svc(RoomPoolService):
        def _new_chunk(self, tb, n_players, human_mask, n_rooms):
            c = _OracleChunk(Oracle(tb.dsl, n_players), self.seed, n_rooms, human_mask)
            chunks.append(c)
            return c

    return Svc(seed=seed, chunk_rooms=chunk_rooms), chunks


def _players(n, humans=()):
    return [{"name": f"P{i + 1}", "gamePlayerId": i + 1, "isBot": (i + 1) not in humans} for i in range(n)]


def test_pool_forecasts_keys_seed_chunks_and_shape():
    from game_engine_amd import room_index_of
    from game_engine_amd.room_service import FORECAST_SEED_XOR
    seed = 0x5EED
    svc, chunks = _service(chunk_rooms=2, seed=seed)
    tids = ["a", "b", "c"]
    for t in tids:
        svc.create_room(t, "werewolf-(mafia)", _players(8, humans=(1,)), dsl=load_dsl("werewolf-(mafia)"))
    svc.create_room("tt", "two-truths-and-a-lie", _players(4), dsl=load_dsl("two-truths-and-a-lie"))
    for _ in range(3):
        svc.handle_messages([(t, "Continue") for t in tids + ["tt"]])
    svc.continue_room("a")
    views_before = {t: svc._rooms[t]["view"].copy() for t in tids}
    out = svc.forecasts(["c", "a", "tt", "b"], n_rollouts=20, max_turns=40)
    # one call per chunk touched: a, b share chunk 0; c is in chunk 1; tt has a pool of its own
    calls = [c.rollout_calls for c in chunks]
    assert [len(c) for c in calls] == [1, 1, 1]
    rooms, keys, turns, R, M, s = calls[0][0]
    assert rooms == [0, 1] and R == 20 and M == 40 and s == seed ^ FORECAST_SEED_XOR
    assert keys == [(room_index_of("a") << 16) & (2 ** 64 - 1), (room_index_of("b") << 16) & (2 ** 64 - 1)]
    assert turns == [4, 3]
    assert [o["threadId"] for o in out] == ["c", "a", "tt", "b"]
    a = out[1]
    assert a["turn"] == 4 and a["rollouts"] == 20 and a["maxTurns"] == 40
    assert set(a) == {"threadId", "turn", "rollouts", "maxTurns", "finished", "endTurnSum", "ended", "sides", "players"}
    assert set(a["sides"]) == {"villagers", "werewolves"} and a["sides"]["villagers"] + a["sides"]["werewolves"] == a["finished"]
    assert list(a["players"]) == [str(i) for i in range(1, 9)]
    assert a["players"]["1"] == {"name": "P1", "alive": a["players"]["1"]["alive"], "wins": a["players"]["1"]["wins"]}
    t = out[2]
    assert set(t) == {"threadId", "turn", "rollouts", "maxTurns", "finished", "endTurnSum", "ended", "players"}
    assert set(t["players"]["1"]) == {"name", "scoreSum", "topScore"}
    # the words behind it: the oracle reference of the slot under the documented key and seed
    from oracle.oracle import Oracle
    orc = Oracle(load_dsl("werewolf-(mafia)"), 8)
    from parity_util import views_as_oracle_rooms
    room = views_as_oracle_rooms(orc, views_before["a"].reshape(1))[0]
    w = reference_rollout(orc, room, seed ^ FORECAST_SEED_XOR, (room_index_of("a") << 16) & (2 ** 64 - 1), 4, 20, 40)
    assert a["finished"] == int(w[1]) and a["endTurnSum"] == int(w[5]) and a["ended"] == int(w[6:22].sum())
    assert a["sides"] == {"villagers": int(w[2]), "werewolves": int(w[3])}
    assert [a["players"][str(i + 1)]["alive"] for i in range(8)] == [int(x) for x in w[41:49]]
    assert [a["players"][str(i + 1)]["wins"] for i in range(8)] == [int(x) for x in w[53:61]]
    assert json.loads(json.dumps(out)) == out                    # JSON integers and strings only
    # a forecast changes no thread
    assert all((svc._rooms[t]["view"] == views_before[t]).all() for t in tids)
    assert svc.forecast("a", n_rollouts=20, max_turns=40) == a


def test_forecast_caps():
    svc, _ = _service()
    svc.create_room("a", "werewolf-(mafia)", _players(8), dsl=load_dsl("werewolf-(mafia)"))
    with pytest.raises(ValueError):
        svc.forecast("a", n_rollouts=65537)
    with pytest.raises(ValueError):
        svc.forecast("a", n_rollouts=0)
    with pytest.raises(ValueError):
        svc.forecasts(["a"], n_rollouts=16, max_turns=4097)
    assert svc.forecast("a", n_rollouts=1, max_turns=0)["rollouts"] == 1


def test_reference_seat_words_split_sides_like_the_summary():
    """rollout_ref's village / wolf split and the summary reference count the same finished games."""
    from oracle.oracle import Oracle
    orc = Oracle(load_dsl("werewolf-(mafia)"), 8)
    room = orc.init_rooms(1)[0]
    w = reference_rollout(orc, room, 7, 1000, 0, 64, 300)
    assert int(w[1]) == int(w[2]) + int(w[3]) and int(w[1]) > 0
    assert int(w[0]) == 64 and int(w[39]) == 300
    assert int(w[41:53].sum()) == int(w[4])                  # alive seats = alive_players

"""RoomPoolService's bookkeeping on the CPU: its chunks are stood in for by an oracle-backed batch of the same interface
(step_rooms / read_rooms_at / inject_actions / write_rooms), as test_messages._OracleBatch stands in for RoomService's
batch.  Message classification, injection rounds, slot reuse, per-thread keys and turns, logging and rendering are the
product's.  Also: the built library exports the indexed entry points."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLD, load_dsl, load_golden
from test_messages import _replay
from test_strings_golden import _strip

FILES = sorted(f for f in os.listdir(GOLD) if f.startswith("strings_human_"))


class _OracleChunk:
    """The subset of RoomBatch a RoomPoolService chunk uses, stepped by the oracle (CPU tests only)."""

    def __init__(self, orc, seed, n_rooms, human_mask):
        self.orc, self.seed, self.mask = orc, seed, human_mask
        self.rooms = orc.init_rooms(n_rooms)
        self.calls = {"step_rooms": 0, "read_rooms_at": 0, "inject_actions": 0, "write_rooms": 0}

    def step_rooms(self, rooms, keys, turns):
        from parity_util import oracle_events
        from game_engine_amd.stepper import EVENT_DTYPE
        self.calls["step_rooms"] += 1
        rooms = [int(r) for r in rooms]
        assert len(set(rooms)) == len(rooms)
        ev = np.zeros(len(rooms), dtype=EVENT_DTYPE)
        for k, r in enumerate(rooms):
            one = self.rooms[r:r + 1]
            self.orc.run(one, self.seed, int(keys[k]), int(turns[k]), 1, human_mask=self.mask)
            ev[k] = oracle_events(self.orc, one, int(turns[k]))[0]
        return ev

    def read_rooms_at(self, rooms):
        from parity_util import oracle_rooms_as_views
        self.calls["read_rooms_at"] += 1
        return oracle_rooms_as_views(self.orc, self.rooms[np.asarray(rooms, dtype=np.int64)]).copy()

    def inject_actions(self, rooms, players, choices):
        self.calls["inject_actions"] += 1
        return np.array([0 if self.orc.inject(self.rooms, int(r), int(p), int(c)) else -1
                         for r, p, c in zip(rooms, players, choices)], dtype=np.int32)

    def write_rooms(self, first, views):
        from parity_util import views_as_oracle_rooms
        self.calls["write_rooms"] += 1
        self.rooms[first:first + len(views)] = views_as_oracle_rooms(self.orc, views)

    def close(self):
        pass


def _service(chunk_rooms=4, seed=0):
    from game_engine_amd import RoomPoolService
    from oracle.oracle import Oracle
    chunks = []

    class Svc(RoomPoolService):
        def _new_chunk(self, tb, n_players, human_mask, n_rooms):
            c = _OracleChunk(Oracle(tb.dsl, n_players), self.seed, n_rooms, human_mask)
            chunks.append(c)
            return c

    return Svc(seed=seed, chunk_rooms=chunk_rooms), chunks


@pytest.mark.parametrize("name", FILES)
def test_person_messages_through_the_pool_equal_reference_run(name):
    g = load_golden(name)
    for case in g["cases"]:
        svc, _ = _service(seed=case["seed"])
        _replay(svc, g, case, f"{name} seed={case['seed']:#x} room={case['room']} (pool)")


def _players(n, humans=()):
    return [{"name": f"P{i + 1}", "gamePlayerId": i + 1, "isBot": (i + 1) not in humans} for i in range(n)]


def test_pool_equals_room_service_with_slot_reuse():
    """Threads on the pool against the same threads on RoomService (oracle-backed both), ticks of many messages; threads
    closed mid-run, new ones opened in the freed slots (written back to the template first)."""
    from game_engine_amd import RoomService
    from oracle.oracle import Oracle
    from test_messages import _OracleBatch
    dsl = load_dsl("werewolf-(mafia)")

    class Ref(RoomService):
        def _new_batch(self, tb, n_players, human_mask, first_room):
            return _OracleBatch(Oracle(tb.dsl, n_players), self.seed, first_room, human_mask)

    ref, (pool, chunks) = Ref(seed=7), _service(chunk_rooms=3, seed=7)
    rng = np.random.default_rng(1)
    threads = [f"thread-{i}" for i in range(7)]
    for i, t in enumerate(threads):
        humans = (1,) if i % 2 else ()
        assert _strip(pool.create_room(t, "werewolf-(mafia)", _players(8, humans), dsl=dsl)) == \
            _strip(ref.create_room(t, "werewolf-(mafia)", _players(8, humans), dsl=dsl))
    texts = ["Continue", "Player P1 in game chat: hi", 'Player 1 voted "P3" in voting x', "Input: hello", "Start game."]
    opened = len(threads)
    for tick in range(30):
        live = list(threads)
        sub = [live[i] for i in rng.permutation(len(live))[: int(rng.integers(1, len(live) + 1))]]
        msgs = [(t, texts[int(rng.integers(0, len(texts)))]) for t in sub]
        got = pool.handle_messages(msgs)
        for (t, text), o in zip(msgs, got):
            assert _strip(o) == _strip(ref.handle_message(t, text)), (tick, t, text)     # (log timestamps aside)
        if tick % 6 == 5:                                       # close two, open two: they land in the freed slots
            for t in threads[:2]:
                pool.close(t)
                ref.close(t)
            threads = threads[2:]
            for _ in range(2):
                t = f"thread-{opened}"
                opened += 1
                threads.append(t)
                assert _strip(pool.create_room(t, "werewolf-(mafia)", _players(8), dsl=dsl)) == \
                    _strip(ref.create_room(t, "werewolf-(mafia)", _players(8), dsl=dsl))
    assert sum(c.calls["write_rooms"] for c in chunks) >= 5             # reused slots were reset to the template
    assert 3 <= len(chunks) <= 4                                      # 3-slot chunks of two pools (bots only / seat 1 human)
    pool.close()
    ref.close()


def test_one_call_per_chunk_per_tick():
    pool, chunks = _service(chunk_rooms=64)
    dsl = load_dsl("two-truths-and-a-lie")
    for i in range(40):
        pool.create_room(f"t{i}", "two-truths-and-a-lie", _players(4), dsl=dsl)
    before = dict(chunks[0].calls)
    out = pool.handle_messages([(f"t{i}", "Continue") for i in range(40)])
    assert len(chunks) == 1 and chunks[0].calls["step_rooms"] - before["step_rooms"] == 1
    assert chunks[0].calls["read_rooms_at"] - before["read_rooms_at"] == 1
    assert all(o["played"] for o in out)


def test_a_thread_twice_in_one_tick_is_refused_before_anything_runs():
    pool, chunks = _service()
    dsl = load_dsl("werewolf-(mafia)")
    pool.create_room("a", "werewolf-(mafia)", _players(8), dsl=dsl)
    pool.create_room("b", "werewolf-(mafia)", _players(8), dsl=dsl)
    before = chunks[0].rooms.copy()
    with pytest.raises(ValueError):
        pool.handle_messages([("a", "Continue"), ("b", "Continue"), ("a", "Continue")])
    assert chunks[0].rooms.tobytes() == before.tobytes() and chunks[0].calls["step_rooms"] == 0
    assert pool.handle_messages([("a", "Continue"), ("b", "Continue")])[0]["played"]


def test_library_exports_the_indexed_entry_points():
    from game_engine_amd.stepper import library_path
    lib = C.CDLL(library_path())
    for name in ("ge_batch_step_rooms", "ge_batch_read_rooms_at"):
        assert getattr(lib, name) is not None

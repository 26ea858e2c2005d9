"""ge_batch_run_rooms without a GPU: the oracle-side reference (tests/run_ref.py) against plain oracle stepping, proof that the
inputs the GPU tests share reach every stop reason, the exported symbol, and the services' bookkeeping of run_room against an
oracle-backed chunk - run_room's output is the sequence of continue_room outputs of a twin service."""
import copy

import numpy as np
import pytest

from game_engine_amd import _lib
from game_engine_amd.stepper import run_until_bits, run_until_names
from parity_util import oracle_events, oracle_rooms_as_views
from run_ref import CASES, END, PERSON, PHASE, SEED, case_inputs, reference_call, run_ref


@pytest.mark.parametrize("name", ["ww8_h1", "tt4_h2", "mixed"])
def test_reference_without_conditions_or_with_one_turn_is_plain_stepping(name):
    segs, listed, keys, turns = case_inputs(name, 12, True)
    per = len(segs[0][4])
    plain = [rooms.copy() for _, _, _, _, rooms in segs]
    played, stopped, events, views, after = reference_call(segs, listed, keys, turns, 7, 0, True)
    assert (played == 7).all() and not stopped.any()
    for k, r in enumerate(listed):
        s, i = divmod(int(r), per)
        orc, _, _, mask, _ = segs[s]
        for t in range(7):
            one = plain[s][i:i + 1]
            orc.run(one, SEED, int(keys[k]), int(turns[k]) + t, 1, threads=1, restart=True, human_mask=mask)
            assert oracle_events(orc, one, int(turns[k]) + t)[0].tobytes() == events[k][t].tobytes()
            assert oracle_rooms_as_views(orc, one)[0].tobytes() == views[k][t].tobytes()
    for a, b in zip(after, plain):
        assert a.tobytes() == b.tobytes()
    one_turn = [rooms.copy() for _, _, _, _, rooms in segs]
    for until in (0, PERSON, 7):
        played, stopped, events, _, after = reference_call(segs, listed, keys, turns, 1, until, True)
        assert (played == 1).all() and not (stopped & ~np.uint32(until)).any()
    for k, r in enumerate(listed):
        s, i = divmod(int(r), per)
        orc, _, _, mask, _ = segs[s]
        orc.run(one_turn[s][i:i + 1], SEED, int(keys[k]), int(turns[k]), 1, threads=1, restart=True, human_mask=mask)
    for a, b in zip(after, one_turn):
        assert a.tobytes() == b.tobytes()


def test_every_stop_reason_occurs_in_the_shared_inputs():
    """On the oracle alone: per pack, some entry stops for each reason and at the limit, and some entry has 1 < played < max_turns
    (the inputs and limits test_gpu_run_rooms.py uses)."""
    seen = {1: set(), 2: set()}
    between = {1: False, 2: False}
    for name in sorted(CASES):
        if len(CASES[name]) > 1:
            continue
        for restart in (False, True):
            segs, listed, keys, turns = case_inputs(name, 48, restart)
            pack = segs[0][0].table.pack
            for until in (PERSON, END, PHASE, 7):
                max_turns = (5, 64, 17, 40)[until % 4]
                played, stopped, _, _, _ = reference_call(segs, listed, keys, turns, max_turns, until, restart)
                for bit in (PERSON, END, PHASE):
                    if (stopped & bit).any():
                        seen[pack].add(bit)
                if ((stopped == 0) & (played == max_turns)).any():
                    seen[pack].add(0)
                between[pack] |= bool(((played > 1) & (played < max_turns)).any())
    for pack in (1, 2):
        assert seen[pack] == {0, PERSON, END, PHASE}, (pack, seen[pack])
        assert between[pack]


def test_list_length_inputs_reach_a_person_and_the_limit():
    segs, _, _, _ = case_inputs("ww8_h1", 100, True, rng_seed=64)
    rng = np.random.default_rng(64)
    listed = rng.permutation(100)[:64]
    keys = rng.choice(1 << 44, size=64, replace=False).astype(np.uint64)
    turns = rng.integers(0, 1000, 64).astype(np.uint32)
    played, stopped, _, _, _ = reference_call(segs, listed, keys, turns, 12, PERSON | END, True)
    assert (stopped & PERSON).any() and (played == 12).any()


def test_library_exports_the_symbol_and_the_names_map_to_its_bits():
    lib = _lib.load()
    assert "ge_batch_run_rooms" in _lib.SYMBOLS and lib.ge_batch_run_rooms is not None
    assert lib.ge_batch_run_rooms(None, 0, None, None, None, 1, 0, None, None, None, None, 0) == -1
    assert run_until_bits(("person", "end")) == 3 and run_until_bits(()) == 0 and run_until_bits("phase") == 4 and run_until_bits(5) == 5
    assert run_until_names(6) == ["end", "phase"]
    with pytest.raises(ValueError):
        run_until_bits(("person", "nobody"))


# ---- service bookkeeping: oracle-backed batches with run_rooms restated by run_ref
def _oracle_services(seed):
    from game_engine_amd import RoomPoolService, RoomService
    from game_engine_amd.stepper import EVENT_DTYPE, ROOM_VIEW_DTYPE
    from oracle.oracle import Oracle
    from test_messages import _OracleBatch
    from test_room_pool import _OracleChunk

    def run_many(orc, store, seed_, mask, rooms, keys, turns, max_turns, until):
        n = len(rooms)
        played, stopped = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        events, views = np.zeros((n, max_turns), dtype=EVENT_DTYPE), np.zeros((n, max_turns), dtype=ROOM_VIEW_DTYPE)
        for k in range(n):
            p, why, ev, vw = run_ref(orc, store, int(rooms[k]), seed_, int(keys[k]), int(turns[k]), max_turns, until, False, mask)
            played[k], stopped[k], events[k, :p], views[k, :p] = p, why, ev, vw
        return played, stopped, events, views

    class Batch(_OracleBatch):
        def run_rooms(self, rooms, keys, turns, max_turns, until):
            return run_many(self.orc, self.rooms, self.seed, self.mask, rooms, keys, turns, max_turns, until)

        def set_turn(self, turn):
            self.turn = turn

    class Chunk(_OracleChunk):
        def run_rooms(self, rooms, keys, turns, max_turns, until):
            self.calls["run_rooms"] = self.calls.get("run_rooms", 0) + 1
            assert len(set(int(r) for r in rooms)) == len(rooms)
            return run_many(self.orc, self.rooms, self.seed, self.mask, rooms, keys, turns, max_turns, until)

    chunks = []

    class One(RoomService):
        def _new_batch(self, tb, n_players, human_mask, first_room):
            return Batch(Oracle(tb.dsl, n_players), self.seed, first_room, human_mask)

    class Pool(RoomPoolService):
        def _new_chunk(self, tb, n_players, human_mask, n_rooms):
            chunks.append(Chunk(Oracle(tb.dsl, n_players), self.seed, n_rooms, human_mask))
            return chunks[-1]

    return One, Pool, chunks


def _accepted(svc, thread_id, seat, choice):
    """True if the action was logged; only the services' refusal (GeError, GE_ERR_ARG) counts as "not this one"."""
    from game_engine_amd import GeError
    try:
        svc.human_action(thread_id, seat, choice)
        return True
    except GeError as e:
        if e.status != -1:
            raise
        return False


def _players(n, humans=()):
    return [{"name": f"P{i + 1}", "gamePlayerId": i + 1, "isBot": (i + 1) not in humans} for i in range(n)]


@pytest.mark.parametrize("game,n,humans", [("werewolf-(mafia)", 8, (1,)), ("werewolf-(mafia)", 8, ()), ("two-truths-and-a-lie", 4, (2,))])
def test_run_room_is_the_sequence_of_continue_room_outputs(game, n, humans):
    """run_room / run_rooms against a twin service's continue_room loop: every turn's output, played, stopped, the thread's
    turn and panel afterwards (the next message's output), with a human action between the runs."""
    from conftest import load_dsl
    from test_strings_golden import _strip
    One, Pool, chunks = _oracle_services(11)
    dsl = load_dsl(game)
    items = [{"id": "x1", "type": "text"}]
    for until, max_turns in ((("person", "end"), 64), ((), 5), (("phase",), 9), (("person", "end", "phase"), 1)):
        svcs = [One(seed=11), Pool(seed=11, chunk_rooms=3)]
        twin = One(seed=11)
        for s in svcs + [twin]:
            for t in ("a", "b"):
                s.create_room(t, game, _players(n, humans), dsl=dsl)
        for rnd in range(4):
            outs = [svcs[0].run_room("a", max_turns, until, items), svcs[1].run_rooms(["b", "a"], max_turns, until, [None, items])[1]]
            want = []
            for _ in range(outs[0]["played"]):
                want.append(copy.deepcopy(twin.continue_room("a", items)))   # as its caller sees it then
            for o in outs:
                assert 1 <= o["played"] <= max_turns and len(o["turns"]) == o["played"]
                assert _strip(o["turns"]) == _strip(want), (game, until, rnd)
                assert o["stopped"] == outs[0]["stopped"] and set(o["stopped"]) <= set(until)
            if not outs[0]["stopped"]:
                assert outs[0]["played"] == max_turns
            if "person" in outs[0]["stopped"]:                   # the person answers: some action of the human seat is accepted
                assert humans
                for s in svcs + [twin]:
                    assert any(_accepted(s, "a", humans[0], c) for c in range(1, n + 1))
            msg = "Continue"
            nxt = _strip(twin.handle_message("a", msg, items))
            assert [_strip(s.handle_message("a", msg, items)) for s in svcs] == [nxt, nxt]
        for s in svcs + [twin]:
            s.close()
    assert all(c.calls.get("run_rooms", 0) >= 1 for c in chunks) and chunks


def test_run_rooms_is_one_call_per_chunk_and_refusals_run_nothing():
    from conftest import load_dsl
    One, Pool, chunks = _oracle_services(3)
    dsl = load_dsl("two-truths-and-a-lie")
    pool = Pool(seed=3, chunk_rooms=8)
    for i in range(12):
        pool.create_room(f"t{i}", "two-truths-and-a-lie", _players(4), dsl=dsl)
    pool.create_room("p", "two-truths-and-a-lie", _players(4), dsl=dsl, playout_seats=(2,))
    out = pool.run_rooms([f"t{i}" for i in range(12)], max_turns=200, until=("end",))
    assert [c.calls.get("run_rooms", 0) for c in chunks] == [1, 1]
    assert all(o["stopped"] == ["end"] and 1 < o["played"] < 200 for o in out)
    before = [c.rooms.tobytes() for c in chunks]
    for args in ((["t0", "t0"],), (["t0", "p"],), (["t0"], 0), (["t0"], 4097), (["t0"], 8, ("person", "nobody")), (["t0", "t1"], 8, (), [None])):
        with pytest.raises(ValueError):
            pool.run_rooms(*args)
    with pytest.raises(KeyError):
        pool.run_rooms(["t0", "nobody"])
    assert [c.rooms.tobytes() for c in chunks] == before and [c.calls.get("run_rooms", 0) for c in chunks] == [1, 1]
    one = One(seed=3)
    one.create_room("p", "two-truths-and-a-lie", _players(4), dsl=dsl, playout_seats=(2,))
    with pytest.raises(ValueError):
        one.run_room("p")

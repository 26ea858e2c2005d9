"""ge_batch_run_rooms_playout without a GPU: the oracle-side reference (tests/run_playout_ref.py) against run_ref where §3g says
they are equal, proof on the oracle alone that the inputs the GPU tests share reach what those tests are for, the exported symbol
and its prototype, and the services' bookkeeping of run_room(playout=True) against oracle-backed batches - its output is the
sequence of continue_room outputs of a twin service."""
import copy
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from game_engine_amd import _lib
from playout_ref import reference_step_playout
from run_playout_ref import M_SMALL, PSEED, R_SMALL, REF_CALLS, REF_CASES, playout_inputs, reference_call, run_playout_ref, shared_reference
from run_ref import END, PERSON, PHASE, SEED, case_inputs
import run_ref


@pytest.mark.parametrize("name", ["ww8_h1", "tt4_h2", "mixed"])
def test_reference_without_playout_seats_or_playout_turns_is_run_ref(name):
    """All masks 0: run_ref word for word, decided all zero.  playout_max_turns = 0: every candidate wins 0 playouts, so every tie
    goes to the policy's own pick - run_ref again, although decisions were made."""
    segs, listed, keys, turns, masks, pkeys = playout_inputs(name, 9 if name == "mixed" else 36, False)
    decided_any = False
    for until, max_turns in ((PERSON | END, 20), (PHASE, 9), (0, 6)):
        p0, s0, e0, v0, a0 = run_ref.reference_call(segs, listed, keys, turns, max_turns, until, False)
        for use_masks, M in ((np.zeros_like(masks), M_SMALL), (masks, 0)):
            p1, s1, e1, v1, d1, a1 = reference_call(segs, listed, keys, turns, use_masks, pkeys, max_turns, until, False, M=M)
            assert p0.tolist() == p1.tolist() and s0.tolist() == s1.tolist()
            for k in range(len(listed)):
                assert [e.tobytes() for e in e0[k]] == [e.tobytes() for e in e1[k]], (name, until, k)
                assert [v.tobytes() for v in v0[k]] == [v.tobytes() for v in v1[k]], (name, until, k)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a0, a1))
            if M:
                assert not any(x for d in d1 for x in d)
            else:
                decided_any |= any(x for d in d1 for x in d)
    assert decided_any


def test_shared_inputs_reach_every_stop_reason_and_late_decisions():
    """On the oracle alone, for the calls tests/test_gpu_run_playout.py checks against this reference: per pack every stop reason
    and the limit, an entry with 1 < played < max_turns, and a decision at t >= 1."""
    seen, between, late = {1: set(), 2: set()}, {1: False, 2: False}, {1: False, 2: False}
    for name in REF_CASES:
        if name == "mixed":
            continue
        for restart in (False, True):
            for until, max_turns in REF_CALLS:
                (segs, *_), (played, stopped, _, _, decided, _) = shared_reference(name, restart, until, max_turns)
                pack = segs[0][0].table.pack
                for bit in (PERSON, END, PHASE):
                    if (stopped & bit).any():
                        seen[pack].add(bit)
                if ((stopped == 0) & (played == max_turns)).any():
                    seen[pack].add(0)
                between[pack] |= bool(((played > 1) & (played < max_turns)).any())
                late[pack] |= any(x for d in decided for x in d[1:])
    for pack in (1, 2):
        assert seen[pack] == {0, PERSON, END, PHASE}, (pack, seen[pack])
        assert between[pack] and late[pack], (pack, between, late)


def test_a_room_decides_after_another_of_its_list_has_stopped():
    """Within one list of 64 rooms (the all-bot Werewolf x 8 list of the GPU composition test, until = PHASE): a room decides at a
    turn later than another room's stop - the case in which a stopped room must not be planned, decided or advanced."""
    segs, _, _, _ = case_inputs("ww8", 100, True, rng_seed=63)
    rng = np.random.default_rng(63)
    listed = rng.permutation(100)[:63].astype(np.uint64)
    keys = rng.choice(1 << 44, size=63, replace=False).astype(np.uint64)
    turns = rng.integers(0, 1000, 63).astype(np.uint32)
    pkeys = rng.integers(0, 1 << 63, 63).astype(np.uint64)
    masks = np.full(63, 0xFF, dtype=np.uint32)
    played, stopped, _, _, decided, _ = reference_call(segs, listed, keys, turns, masks, pkeys, 12, PHASE, True)
    first_stop = int(played.min())
    assert any(x for d in decided for x in d[first_stop:]), (played.tolist(), [len(d) for d in decided])
    assert (stopped == PHASE).any() and int(played.max()) > first_stop


def test_library_exports_the_symbol_and_the_header_declares_it(tmp_path):
    lib = _lib.load()
    assert "ge_batch_run_rooms_playout" in _lib.SYMBOLS and lib.ge_batch_run_rooms_playout is not None
    assert lib.ge_batch_run_rooms_playout(None, 0, None, None, None, None, None, 1, 1, 0, 0, 1, 0, None, None, None, None, None, 0) == -1
    src = tmp_path / "proto.c"
    src.write_text('#include "ge_step.h"\n'
                   "int (*f)(ge_batch *, uint64_t, const uint64_t *, const uint64_t *, const uint32_t *, const uint32_t *, const uint64_t *,\n"
                   "         uint32_t, uint32_t, uint64_t, uint32_t, uint32_t, uint32_t, uint32_t *, uint32_t *, uint32_t *, ge_turn_event *,\n"
                   "         ge_room_view *, size_t) = ge_batch_run_rooms_playout;\n"
                   "int v = GE_ABI_VERSION == 5 ? 1 : -1; char a[GE_ABI_VERSION == 5 ? 1 : -1];\n")
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "proto.o")])


# ---- service bookkeeping: oracle-backed batches with the playout calls restated by the references
def _oracle_services():
    from game_engine_amd import RoomPoolService, RoomService
    from game_engine_amd.stepper import EVENT_DTYPE, ROOM_VIEW_DTYPE
    from oracle.oracle import Oracle
    from parity_util import oracle_events
    from test_run_host import _oracle_services as plain_services

    One0, Pool0, _ = plain_services(0)                             # the plain doubles (run_rooms by run_ref): the base classes below

    def step_many(orc, store, seed_, hmask, rooms, keys, turns, masks, pkeys, R, M, seed, full_view):
        ev, dec = np.zeros(len(rooms), dtype=EVENT_DTYPE), np.zeros(len(rooms), dtype=np.uint32)
        for k in range(len(rooms)):
            i = int(rooms[k])
            dec[k] = reference_step_playout(orc, store, i, seed_, int(keys[k]), int(turns[k]), int(masks[k]), int(pkeys[k]), seed, R, M,
                                            full_view, False, hmask)
            ev[k] = oracle_events(orc, store[i:i + 1], int(turns[k]))[0]
        return ev, dec

    def run_many(orc, store, seed_, hmask, rooms, keys, turns, masks, pkeys, R, M, seed, full_view, max_turns, until):
        n = len(rooms)
        played, stopped = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        events, views = np.zeros((n, max_turns), dtype=EVENT_DTYPE), np.zeros((n, max_turns), dtype=ROOM_VIEW_DTYPE)
        decided = np.zeros((n, max_turns), dtype=np.uint32)
        for k in range(n):
            p, why, ev, vw, dec = run_playout_ref(orc, store, int(rooms[k]), seed_, int(keys[k]), int(turns[k]), int(masks[k]), int(pkeys[k]),
                                                  seed, R, M, full_view, max_turns, until, False, hmask)
            played[k], stopped[k], events[k, :p], views[k, :p], decided[k, :p] = p, why, ev, vw, dec
        return played, stopped, events, views, decided

    def doubles(base):
        class Double(base):
            def step_rooms_playout(self, rooms, keys, turns, masks, pkeys, R, M, seed=None, full_view=False):
                self.calls["step_rooms_playout"] = self.calls.get("step_rooms_playout", 0) + 1
                return step_many(self.orc, self.rooms, self.seed, self.mask, rooms, keys, turns, masks, pkeys, R, M, seed, full_view)

            def run_rooms_playout(self, rooms, keys, turns, masks, pkeys, R, M=256, seed=None, full_view=False, max_turns=64, until=3,
                                  views=True):
                self.calls["run_rooms_playout"] = self.calls.get("run_rooms_playout", 0) + 1
                assert len(set(int(r) for r in rooms)) == len(rooms)
                return run_many(self.orc, self.rooms, self.seed, self.mask, rooms, keys, turns, masks, pkeys, R, M, seed, full_view, max_turns,
                                until)
        return Double

    chunks, batches = [], []
    probe_one, probe_pool = One0(seed=0), Pool0(seed=0)

    class One(RoomService):
        def _new_batch(self, tb, n_players, human_mask, first_room):
            base = type(probe_one._new_batch(tb, n_players, human_mask, first_room))
            b = doubles(base)(Oracle(tb.dsl, n_players), self.seed, first_room, human_mask)
            b.calls = {}
            batches.append(b)
            return b

    class Pool(RoomPoolService):
        def _new_chunk(self, tb, n_players, human_mask, n_rooms):
            base = type(probe_pool._new_chunk(tb, n_players, human_mask, n_rooms))
            chunks.append(doubles(base)(Oracle(tb.dsl, n_players), self.seed, n_rooms, human_mask))
            return chunks[-1]

    return One, Pool, chunks, batches


def _players(n, humans=()):
    return [{"name": f"P{i + 1}", "gamePlayerId": i + 1, "isBot": (i + 1) not in humans} for i in range(n)]


OPTS = dict(playout_rollouts=R_SMALL, playout_max_turns=M_SMALL)


@pytest.mark.parametrize("game,n,humans,bots", [("werewolf-(mafia)", 8, (1,), (3, 6)), ("two-truths-and-a-lie", 4, (2,), (1, 3))])
def test_run_room_with_playout_is_the_sequence_of_continue_room_outputs(game, n, humans, bots):
    """run_room(playout=True) / run_rooms(playout=True) against a twin service's continue_room loop: every turn's output, played,
    stopped, the thread's turn and panel afterwards (the next message's output), with a human action between the runs."""
    from conftest import load_dsl
    from test_run_host import _accepted
    from test_strings_golden import _strip
    One, Pool, chunks, batches = _oracle_services()
    dsl = load_dsl(game)
    items = [{"id": "x1", "type": "text"}]
    for until, max_turns in ((("person", "end"), 40), (("phase",), 7)):
        svcs = [One(seed=11, **OPTS), Pool(seed=11, chunk_rooms=3, **OPTS)]
        twin = One(seed=11, **OPTS)
        for s in svcs + [twin]:
            s.create_room("a", game, _players(n, humans), dsl=dsl, playout_seats=bots)
            s.create_room("b", game, _players(n, humans), dsl=dsl)
        for rnd in range(3):
            outs = [svcs[0].run_room("a", max_turns, until, items, playout=True),
                    svcs[1].run_rooms(["b", "a"], max_turns, until, [None, items], playout=True)[1]]
            want = []
            for _ in range(outs[0]["played"]):
                want.append(copy.deepcopy(twin.continue_room("a", items)))   # as its caller sees it then
            for o in outs:
                assert 1 <= o["played"] <= max_turns and len(o["turns"]) == o["played"]
                assert _strip(o["turns"]) == _strip(want), (game, until, rnd)
                assert o["stopped"] == outs[0]["stopped"] and set(o["stopped"]) <= set(until)
            if "person" in outs[0]["stopped"]:                   # the person answers: some action of the human seat is accepted
                for s in svcs + [twin]:
                    assert any(_accepted(s, "a", humans[0], c) for c in range(1, n + 1))
            nxt = _strip(twin.handle_message("a", "Continue", items))
            assert [_strip(s.handle_message("a", "Continue", items)) for s in svcs] == [nxt, nxt]
        for s in svcs + [twin]:
            s.close()
    assert any(b.calls.get("run_rooms_playout") for b in batches) and any(c.calls.get("run_rooms_playout") for c in chunks)
    assert any(b.calls.get("step_rooms_playout") for b in batches), "the twin's playout bots never stepped"


def test_pool_makes_one_call_per_chunk_and_the_refusal_stands_without_the_option():
    from conftest import load_dsl
    One, Pool, chunks, _ = _oracle_services()
    dsl = load_dsl("two-truths-and-a-lie")
    pool = Pool(seed=3, chunk_rooms=8, **OPTS)
    for i in range(12):                                          # two chunks, each mixing plain and playout threads
        pool.create_room(f"t{i}", "two-truths-and-a-lie", _players(4), dsl=dsl, playout_seats=(2,) if i % 3 == 0 else ())
    ids = [f"t{i}" for i in range(12)]
    before = [c.rooms.tobytes() for c in chunks]
    with pytest.raises(ValueError, match="playout=True"):
        pool.run_rooms(ids, max_turns=30, until=("end",))
    with pytest.raises(ValueError, match="playout=True"):
        pool.run_room("t0")
    assert [c.rooms.tobytes() for c in chunks] == before and not any(c.calls.get("run_rooms_playout") or c.calls.get("run_rooms") for c in chunks)
    out = pool.run_rooms(ids, max_turns=200, until=("end",), playout=True)
    assert [c.calls.get("run_rooms_playout", 0) for c in chunks] == [1, 1] and not any(c.calls.get("run_rooms") for c in chunks)
    assert all(o["stopped"] == ["end"] and 1 < o["played"] < 200 for o in out)
    plain = pool.run_rooms(["t1", "t2"], max_turns=3, until=(), playout=True)   # no playout thread in the list: the plain call
    assert [o["played"] for o in plain] == [3, 3] and chunks[0].calls.get("run_rooms") == 1
    one = One(seed=3, **OPTS)
    one.create_room("p", "two-truths-and-a-lie", _players(4), dsl=dsl, playout_seats=(2,))
    with pytest.raises(ValueError, match="playout=True"):
        one.run_room("p")
    assert one.run_room("p", 5, (), playout=True)["played"] == 5


def test_pool_splits_a_chunks_list_where_one_turns_playouts_pass_the_cap():
    """65 536 rollouts x 2 playout seats x 4 candidates = 2^19 per Two-Truths x 4 thread: 128 threads fill the call's cap of 2^26, so a
    chunk's list of 130 takes two calls (the doubles play with few rollouts whatever the service asks for), every thread still
    gets its own turns, and `most` bounds a part's length."""
    from conftest import load_dsl
    _, Pool, chunks, _ = _oracle_services()
    dsl = load_dsl("two-truths-and-a-lie")
    pool = Pool(seed=3, chunk_rooms=200, playout_rollouts=1 << 16, playout_max_turns=M_SMALL)
    ids = [f"t{i}" for i in range(130)]
    for t in ids:
        pool.create_room(t, "two-truths-and-a-lie", _players(4), dsl=dsl, playout_seats=(1, 3))
    (chunk,) = chunks
    seen = []
    inner = chunk.run_rooms_playout
    chunk.run_rooms_playout = lambda rooms, keys, turns, masks, pkeys, R, M, **kw: (
        seen.append((len(rooms), R)), inner(rooms, keys, turns, masks, pkeys, R_SMALL, M, **kw))[1]
    out = pool.run_rooms(ids, max_turns=2, until=(), playout=True)
    assert seen == [(128, 1 << 16), (2, 1 << 16)]
    assert [o["played"] for o in out] == [2] * 130 and all(pool._rooms[t]["turn"] == 2 for t in ids)
    rooms = [pool._rooms[t] for t in ids]
    assert pool._playout_parts(rooms) == [(0, 128), (128, 130)]
    assert pool._playout_parts(rooms, 50) == [(0, 50), (50, 100), (100, 130)]
    assert pool._playout_parts(rooms[:3], 1) == [(0, 1), (1, 2), (2, 3)]

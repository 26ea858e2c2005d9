"""ge_batch_advise_seats without a GPU: the header's records through a C compiler, the Python binding's struct and dtype, the
reference (tests/advise_ref.py) on rooms whose answer is known, and the services' hint / hints through their batch seam - a chunk
whose advise_seats is answered by the reference - with the Node host printing the same bytes for the same records."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from advise_ref import ADVICE_REF_DTYPE, GE_ERR_ARG, legal_mask, reference_advice
from conftest import load_dsl
from find_ref import room_facts
from game_engine_amd import _lib
from game_engine_amd.messages import ACT_TT_STATEMENTS
from oracle.oracle import Oracle
from test_messages import _OracleBatch
from test_rollout_actions_host import MASK64, _players
from test_rollout_seats_host import _SeatChunk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE_DIR = os.path.join(ROOT, "game_engine_amd", "node")


def test_header_pins_the_records_and_the_prototype(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text("""
#include <stddef.h>
#include "ge_step.h"
typedef char advice_is_224_bytes[sizeof(ge_advice) == 224 ? 1 : -1];
typedef char option_is_16_bytes[sizeof(ge_advice_option) == 16 ? 1 : -1];
typedef char advice_fields[offsetof(ge_advice, legal) == 4 && offsetof(ge_advice, best) == 8 && offsetof(ge_advice, phase_id) == 12 &&
                           offsetof(ge_advice, policy) == 16 && offsetof(ge_advice, option) == 32 ? 1 : -1];
typedef char option_fields[offsetof(ge_advice_option, wins) == 4 && offsetof(ge_advice_option, score) == 8 ? 1 : -1];
typedef char full_view_is_1[GE_ADVISE_FULL_VIEW == 1u ? 1 : -1];
typedef char abi_stays_5[GE_ABI_VERSION == 5 ? 1 : -1];
int (*p)(ge_batch *, uint64_t, const uint64_t *, const uint64_t *, const uint32_t *, const uint32_t *, uint32_t, uint32_t, uint64_t, uint32_t,
         ge_advice *) = ge_batch_advise_seats;
int main(void) { return p == 0; }
""")
    subprocess.check_call([cc, "-std=c99", "-pedantic", "-Werror", "-Wall", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "t.o")])


def test_binding_has_the_records_size_and_offsets():
    from game_engine_amd import ADVICE_DTYPE
    lib = _lib.load()
    assert "ge_batch_advise_seats" in _lib.SYMBOLS and lib.ge_batch_advise_seats is not None
    assert lib.ge_batch_advise_seats(None, 0, None, None, None, None, 1, 1, 0, 0, None) == -1      # b NULL: no device needed
    assert C.sizeof(_lib.Advice) == 224 and C.sizeof(_lib.AdviceOption) == 16 and _lib.ADVISE_FULL_VIEW == 1
    assert ADVICE_DTYPE.itemsize == 224 and ADVICE_DTYPE == ADVICE_REF_DTYPE
    for f, off in (("status", 0), ("legal", 4), ("best", 8), ("phase_id", 12), ("policy", 16), ("option", 32)):
        assert getattr(_lib.Advice, f).offset == off and ADVICE_DTYPE.fields[f][1] == off, f
    for f, off in (("finished", 0), ("wins", 4), ("score", 8)):
        assert getattr(_lib.AdviceOption, f).offset == off and ADVICE_DTYPE.fields["policy"][0].fields[f][1] == off, f


def _played(name, n, turns, seed=0xFACE, key=31):
    orc = Oracle(load_dsl(name), n)
    rooms = orc.init_rooms(1)
    orc.run(rooms, seed, key, 0, turns)
    return orc, rooms[0]


def test_a_statements_phase_has_the_single_legal_choice_1():
    orc = Oracle(load_dsl("two-truths-and-a-lie"), 4)
    seen = 0
    for turns in range(0, 12):
        rec = _played("two-truths-and-a-lie", 4, turns)[1]
        if orc.table.phases[int(rec["phase"])].act != ACT_TT_STATEMENTS:
            continue
        masks = [legal_mask(orc, rec, s) for s in range(1, 5)]
        assert set(masks) <= {0, 1} and any(masks), (turns, masks)
        seat = masks.index(1) + 1
        adv = reference_advice(orc, rec, 7, 100, turns, seat, 6, 30)
        assert (int(adv["status"]), int(adv["legal"]), int(adv["best"])) == (0, 1, 1)
        assert adv["option"][0]["finished"] <= 6 and not adv["option"][1:].tobytes().strip(b"\0")
        seen += 1
    assert seen


@pytest.mark.parametrize("name,n", [("werewolf-(mafia)", 8), ("two-truths-and-a-lie", 4)])
def test_no_seat_of_a_finished_room_is_advised(name, n):
    orc, rec = _played(name, n, 400)
    assert not orc.table.phases[int(rec["phase"])].branches      # the game is over
    for seat in range(1, n + 1):
        adv = reference_advice(orc, rec, 7, 100, 400, seat, 4, 10)
        assert int(adv["status"]) == GE_ERR_ARG and not adv.tobytes()[4:].strip(b"\0")


def test_best_is_the_lowest_choice_with_the_highest_value_and_words_are_rollout_seats():
    from rollout_seats_ref import reference_rollout_seats
    orc, rec = _played("werewolf-(mafia)", 8, 9)
    seat = next(s for s in range(1, 9) if legal_mask(orc, rec, s))
    for full in (False, True):
        adv = reference_advice(orc, rec, 5, 1 << 33, 9, seat, 20, 40, full_view=full)
        cs = [c for c in range(1, 9) if (int(adv["legal"]) >> (c - 1)) & 1]
        assert len(cs) >= 2 and int(adv["phase_id"]) == int(orc.ids[int(rec["phase"])])
        wins = [int(adv["option"][c - 1]["wins"]) for c in cs]
        assert int(adv["best"]) == cs[wins.index(max(wins))]
        w, st = reference_rollout_seats(orc, rec.copy(), 5, 1 << 33, 9, 0 if full else seat, [(seat, cs[-1])], 20, 40)
        assert st == 0 and tuple(adv["option"][cs[-1] - 1].item()) == (w[1], w[41 + 12 + seat - 1], w[41 + 24 + seat - 1])
        w, _ = reference_rollout_seats(orc, rec.copy(), 5, 1 << 33, 9, 0 if full else seat, [], 20, 40)
        assert tuple(adv["policy"].item()) == (w[1], w[41 + 12 + seat - 1], w[41 + 24 + seat - 1])


class _HintChunk(_SeatChunk):
    """_SeatChunk plus advise_seats and find_rooms, answered by the references (CPU tests only)."""

    def __init__(self, *a):
        super().__init__(*a)
        self.advise_calls = []

    def advise_seats(self, rooms, keys, turns, seats, n_rollouts, max_turns=1024, seed=None, full_view=False):
        seed = self.seed if seed is None else seed
        self.advise_calls.append(([int(r) for r in rooms], [int(k) for k in keys], [int(t) for t in turns], [int(s) for s in seats],
                                  n_rollouts, max_turns, seed, full_view))
        return np.array([reference_advice(self.orc, self.rooms[int(r)], seed, int(k), int(t), int(s), n_rollouts, max_turns, full_view)
                         for r, k, t, s in zip(rooms, keys, turns, seats)], dtype=ADVICE_REF_DTYPE)

    def find_rooms(self, want=("person", "end")):
        from game_engine_amd.stepper import ROOM_HIT_DTYPE
        assert tuple(want) == ("person",)
        facts = room_facts(self.orc, self.rooms, self.mask)
        hits = [(i, 1, p, pid, 0) for i, (p, _, pid) in enumerate(facts) if p]
        return np.array(hits, dtype=ROOM_HIT_DTYPE), len(hits)


def _pool(chunk_rooms=4, seed=0x5EED):
    from game_engine_amd import RoomPoolService
    chunks = []

    class Svc(RoomPoolService):
        def _new_chunk(self, tb, n_players, human_mask, n_rooms):
            c = _HintChunk(Oracle(tb.dsl, n_players), self.seed, n_rooms, human_mask)
            chunks.append(c)
            return c

    return Svc(seed=seed, chunk_rooms=chunk_rooms), chunks


def _own(forecast, seat, ww):
    """The advised seat's (finished, wins, score) inside one of advise's forecasts."""
    p = forecast["players"][str(seat)]
    return (forecast["finished"], p["wins"], 0) if ww else (forecast["finished"], p["topScore"], p["scoreSum"])


def _assert_hint_is_advise(hint, adv, ww):
    seat = adv["playerId"]
    assert {k: hint[k] for k in ("threadId", "turn", "playerId", "phaseId", "rollouts", "maxTurns")} == \
           {k: adv[k] for k in ("threadId", "turn", "playerId", "phaseId", "rollouts", "maxTurns")}
    assert [(o["choice"], o["label"]) for o in hint["options"]] == [(o["choice"], o["label"]) for o in adv["options"]]
    for h, a in zip(hint["options"], adv["options"]):
        assert (h["finished"], h["wins"], h["score"]) == _own(a["forecast"], seat, ww), h
    if hint["options"]:
        p = hint["policy"]
        assert (p["finished"], p["wins"], p["score"]) == _own(adv["policy"], seat, ww)
        value = [o["wins"] if ww else o["score"] for o in hint["options"]]
        assert hint["best"] == hint["options"][value.index(max(value))]["choice"]
    else:
        assert hint["best"] is None and hint["policy"] is None


def _waiting_pool(seed=0x5EED):
    """Three Werewolf x 8 threads (people on seats 2 and 5) and two Two-Truths x 4 (seat 1), played on until someone waits."""
    svc, chunks = _pool(chunk_rooms=2, seed=seed)
    ww, tt = load_dsl("werewolf-(mafia)"), load_dsl("two-truths-and-a-lie")
    for t in ("a", "b", "c"):
        svc.create_room(t, "werewolf-(mafia)", _players(8, humans=(2, 5)), dsl=ww)
    for t in ("x", "y"):
        svc.create_room(t, "two-truths-and-a-lie", _players(4, humans=(1,)), dsl=tt)
    for _ in range(40):
        busy = [t for t in ("a", "b", "c", "x", "y") if t not in svc.waiting()]
        if not busy:
            break
        svc.handle_messages([(t, "Continue") for t in busy])
    return svc, chunks


def test_hints_shape_keys_seed_and_numbers_through_the_pool_seam():
    from game_engine_amd import room_index_of
    from game_engine_amd.room_service import FORECAST_SEED_XOR
    seed = 0x5EED
    svc, chunks = _waiting_pool(seed)
    wait = svc.waiting()
    assert set(wait) == {"a", "b", "c", "x", "y"}
    pairs = [(t, s) for t in ("a", "b", "c", "x", "y") for s in wait[t]]
    before = [c.rooms.copy() for c in chunks]
    hints = svc.hints(n_rollouts=6, max_turns=30)
    assert [(h["threadId"], h["playerId"]) for h in hints] == pairs
    calls = [c.advise_calls for c in chunks if c.advise_calls]
    assert all(len(c) == 1 for c in calls) and len(calls) == len({id(svc._rooms[t]["chunk"]) for t, _ in pairs})   # one call per chunk touched
    for c in chunks:
        for rooms, keys, turns, seats, R, M, s, full in c.advise_calls:
            assert (R, M, s, full) == (6, 30, seed ^ FORECAST_SEED_XOR, False)
            for r, k, t in zip(rooms, keys, turns):
                tid = next(t_ for t_, room in svc._rooms.items() if room["chunk"] is c and room["slot"] == r)
                assert k == (room_index_of(tid) << 16) & MASK64 and t == svc._rooms[tid]["turn"]
    assert all((x == y).all() for x, y in zip(before, [c.rooms for c in chunks]))
    for h in hints:
        ww = h["threadId"] in "abc"
        assert list(h) == ["threadId", "turn", "playerId", "phaseId", "rollouts", "maxTurns", "best", "policy", "options", "view"]
        assert h["view"] == "seat" and h["options"] and json.loads(json.dumps(h)) == h
        assert all(list(o) == ["choice", "label", "wins", "score", "finished"] for o in h["options"])
        _assert_hint_is_advise(h, svc.advise(h["threadId"], h["playerId"], n_rollouts=6, max_turns=30, view="seat"), ww)
        assert svc.hints([h["threadId"]], [h["playerId"]], n_rollouts=6, max_turns=30) == [h]
    # listed threads: the lowest human seat by default, any seat on request; the full view drops "view"
    full = svc.hints(["x", "a"], None, 6, 30, "full")
    assert [(h["threadId"], h["playerId"]) for h in full] == [("x", 1), ("a", 2)] and all("view" not in h for h in full)
    _assert_hint_is_advise(full[1], svc.advise("a", 2, n_rollouts=6, max_turns=30), True)
    other = svc.hints(["a", "a"], [7, None], 6, 30)
    assert [h["playerId"] for h in other] == [7, 2]
    _assert_hint_is_advise(other[0], svc.advise("a", 7, n_rollouts=6, max_turns=30, view="seat"), True)
    idle = next(h for h in svc.hints(["a"] * 8, list(range(1, 9)), 6, 30) if not h["options"])   # a seat with nothing to do now
    assert idle["best"] is None and idle["policy"] is None and idle["view"] == "seat"
    with pytest.raises(ValueError):
        svc.hints(None, [1])
    with pytest.raises(ValueError):
        svc.hints(["a"], [1, 2])
    with pytest.raises(ValueError):
        svc.hints(["a"], view="spectator")
    with pytest.raises(ValueError):
        svc.hints(["a"], n_rollouts=0)
    with pytest.raises(KeyError):
        svc.hints(["nobody"])


def test_room_service_hint_through_the_batch_seam():
    from game_engine_amd import RoomService
    from game_engine_amd.room_service import FORECAST_SEED_XOR
    batches = []

    class Svc(RoomService):
        def _new_batch(self, tb, n_players, human_mask, first_room):
            b = _TurnBatch(Oracle(tb.dsl, n_players), self.seed, first_room, human_mask)
            batches.append(b)
            return b

    svc = Svc(seed=77)
    svc.create_room("t", "werewolf-(mafia)", _players(8, humans=(3,)), dsl=load_dsl("werewolf-(mafia)"))
    for _ in range(40):
        svc.continue_room("t")
        if legal_mask(batches[0].orc, batches[0].rooms[0], 3):
            break
    h = svc.hint("t", n_rollouts=5, max_turns=25)
    rooms, keys, turns, seats, R, M, s, full = batches[0].advise_calls[-1]
    assert (rooms, seats, R, M, s, full) == ([0], [3], 5, 25, 77 ^ FORECAST_SEED_XOR, False) and turns == [batches[0].turn]
    assert h["playerId"] == 3 and h["options"] and h["view"] == "seat"
    _assert_hint_is_advise(h, svc.advise("t", n_rollouts=5, max_turns=25, view="seat"), True)
    f = svc.hint("t", 3, 5, 25, "full")
    assert batches[0].advise_calls[-1][-1] is True and "view" not in f
    _assert_hint_is_advise(f, svc.advise("t", n_rollouts=5, max_turns=25), True)


class _TurnBatch(_OracleBatch):
    """test_messages._OracleBatch - the lone batch of a RoomService thread - plus advise_seats and the playouts advise uses,
    answered by the references."""

    def __init__(self, *a):
        super().__init__(*a)
        self.advise_calls = []

    def advise_seats(self, rooms, keys, turns, seats, n_rollouts, max_turns=1024, seed=None, full_view=False):
        self.advise_calls.append(([int(r) for r in rooms], [int(k) for k in keys], [int(t) for t in turns], [int(s) for s in seats],
                                  n_rollouts, max_turns, seed, full_view))
        return np.array([reference_advice(self.orc, self.rooms[int(r)], seed, int(k), int(t), int(s), n_rollouts, max_turns, full_view)
                         for r, k, t, s in zip(rooms, keys, turns, seats)], dtype=ADVICE_REF_DTYPE)

    def rollout_seats(self, rooms, keys, turns, seats, actions=None, n_rollouts=4096, max_turns=1024, seed=None):
        from rollout_seats_ref import reference_rollout_seats
        actions = [[] for _ in rooms] if actions is None else actions
        res = [reference_rollout_seats(self.orc, self.rooms[int(r)].copy(), seed, int(k), int(t), int(s), [(int(p), int(c)) for p, c in a],
                                       n_rollouts, max_turns) for r, k, t, s, a in zip(rooms, keys, turns, seats, actions)]
        return np.stack([w for w, _ in res]), np.array([st for _, st in res], dtype=np.int32)

    def rollout_actions(self, rooms, keys, turns, actions, n_rollouts, max_turns=1024, seed=None):
        return self.rollout_seats(rooms, keys, turns, [0] * len(rooms), actions, n_rollouts, max_turns, seed)


needs_node = pytest.mark.skipif(shutil.which("node") is None or not os.path.exists(os.path.join(NODE_DIR, "ge_addon.node")),
                                reason="node or the built addon is not available")


@needs_node
def test_node_prints_the_same_hint_bytes_for_the_same_records(tmp_path):
    """The records of the pool's hints as ge_advice bytes: decoded by index.js and printed by room_service.js's hintOutput, the
    JSON text equals the Python service's, byte for byte."""
    svc, chunks = _waiting_pool()
    metas, recs, want = [], [], []
    for view in ("seat", "full"):
        for tid in ("a", "x"):
            room = svc._rooms[tid]
            for seat in range(1, len(room["names"]) + 1):
                h, = svc.hints([tid], [seat], 6, 30, view)
                want.append(h)
                recs.append(room["chunk"].advise_seats([room["slot"]], [room["chunk"].advise_calls[-1][1][0]], [room["turn"]], [seat], 6, 30,
                                                       room["chunk"].advise_calls[-1][6], view == "full")[0])
                metas.append({"threadId": tid, "turn": room["turn"], "seat": seat, "phaseId": int(room["view"]["phase_id"]), "rollouts": 6,
                              "maxTurns": 30, "seatView": view == "seat", "pack": room["table"].pack, "names": room["names"]})
    assert any(not h["options"] for h in want) and any(h["options"] for h in want)
    got = []
    for pack in (1, 2):                                            # one run per game: the labels are the names or the numbers
        idx = [k for k, m in enumerate(metas) if m["pack"] == pack]
        spec = tmp_path / f"spec{pack}.json"
        spec.write_text(json.dumps({"pack": pack, "names": metas[idx[0]]["names"], "meta": [metas[k] for k in idx],
                                    "hex": np.array([recs[k] for k in idx], dtype=ADVICE_REF_DTYPE).tobytes().hex()}))
        p = subprocess.run(["node", os.path.join(NODE_DIR, "selftest_advise_seats.js"), "--output", str(spec)], capture_output=True,
                           text=True, timeout=120)
        assert p.returncode == 0, p.stderr[-3000:]
        text = p.stdout.strip().splitlines()[-1]
        assert text == json.dumps([want[k] for k in idx], separators=(",", ":"), ensure_ascii=False)
        got += json.loads(text)
    assert len(got) == len(want)

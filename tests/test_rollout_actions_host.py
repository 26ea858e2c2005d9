"""ge_batch_rollout_actions and advise on the CPU side: the C99 prototype, the ctypes symbol, and RoomPoolService's advise /
advises with its chunks stood in for by an oracle-backed batch that implements rollout_actions (tests/rollout_actions_ref.py):
candidates per pack and phase kind, keys and seed, the no-action entry equal to forecast, grouping by chunk, output shape, and
the default seat."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import load_dsl
from rollout_actions_ref import reference_rollout_actions
from test_rollout_host import _OracleChunk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK64 = 2 ** 64 - 1


def test_header_declares_rollout_actions(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text("""
#include "ge_step.h"
int (*p)(ge_batch *, uint64_t, const uint64_t *, const uint64_t *, const uint32_t *, const uint32_t *, const uint32_t *,
         const uint32_t *, int32_t *, uint32_t, uint32_t, uint64_t, ge_rollout_stats *) = ge_batch_rollout_actions;
int main(void) { return p == 0; }
""")
    subprocess.check_call([cc, "-std=c99", "-pedantic", "-Werror", "-Wall", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "t.o")])


def test_symbol_listed():
    from game_engine_amd import _lib
    assert "ge_batch_rollout_actions" in _lib.SYMBOLS


class _ActChunk(_OracleChunk):
    """_OracleChunk plus rollout_actions, run by the oracle (CPU tests only)."""

    def __init__(self, *a):
        super().__init__(*a)
        self.action_calls = []

    def rollout_actions(self, rooms, keys, turns, actions, n_rollouts, max_turns=1024, seed=None):
        seed = self.seed if seed is None else seed
        actions = [[(int(p), int(c)) for p, c in a] for a in actions]
        self.action_calls.append(([int(r) for r in rooms], [int(k) for k in keys], [int(t) for t in turns], actions, n_rollouts, max_turns, seed))
        res = [reference_rollout_actions(self.orc, self.rooms[int(r)].copy(), seed, int(k), int(t), a, n_rollouts, max_turns)
               for r, k, t, a in zip(rooms, keys, turns, actions)]
        return np.stack([w for w, _ in res]), np.array([s for _, s in res], dtype=np.int32)


def _service(chunk_rooms=2, seed=0x5EED):
    from game_engine_amd import RoomPoolService
    from oracle.oracle import Oracle
    chunks = []

    class Svc(RoomPoolService):
        def _new_chunk(self, tb, n_players, human_mask, n_rooms):
            c = _ActChunk(Oracle(tb.dsl, n_players), self.seed, n_rooms, human_mask)
            chunks.append(c)
            return c

    return Svc(seed=seed, chunk_rooms=chunk_rooms), chunks


def _players(n, humans=()):
    return [{"name": f"P{i + 1}", "gamePlayerId": i + 1, "isBot": (i + 1) not in humans} for i in range(n)]


def _accepted(svc, tid, seat, cands):
    """The candidates the oracle accepts for `seat` in a copy of the thread's record."""
    from oracle.oracle import Oracle
    from parity_util import views_as_oracle_rooms
    room = svc._rooms[tid]
    orc = Oracle(room["table"].dsl, int(room["view"]["n_players"]))
    rec = views_as_oracle_rooms(orc, room["view"].reshape(1))
    out = []
    for c in cands:
        one = rec.copy()
        if orc.inject(one, 0, seat, c):
            out.append(c)
    return out


def test_advise_werewolf_candidates_keys_seed_and_policy():
    from game_engine_amd import room_index_of
    from game_engine_amd.room_service import FORECAST_SEED_XOR
    seed = 0x5EED
    svc, chunks = _service(chunk_rooms=4, seed=seed)
    svc.create_room("a", "werewolf-(mafia)", _players(8, humans=(2, 5)), dsl=load_dsl("werewolf-(mafia)"))
    seen_options = False
    for step in range(12):
        before = svc._rooms["a"]["view"].copy()
        out = svc.advise("a", n_rollouts=6, max_turns=25)
        rooms, keys, turns, actions, R, M, s = chunks[0].action_calls[-1]
        # one entry per seat id, then the policy's entry without actions; every entry under forecast's key and seed
        assert actions == [[(2, c)] for c in range(1, 9)] + [[]]
        assert rooms == [0] * 9 and turns == [step] * 9 and R == 6 and M == 25 and s == seed ^ FORECAST_SEED_XOR
        assert keys == [(room_index_of("a") << 16) & MASK64] * 9
        assert out["playerId"] == 2 and out["turn"] == step and out["phaseId"] == int(before["phase_id"])
        assert set(out) == {"threadId", "turn", "playerId", "phaseId", "rollouts", "maxTurns", "policy", "options"}
        assert out["policy"] == svc.forecast("a", n_rollouts=6, max_turns=25)
        acc = _accepted(svc, "a", 2, range(1, 9))
        assert [o["choice"] for o in out["options"]] == acc
        for o in out["options"]:
            assert o["label"] == f"P{o['choice']}" and set(o) == {"choice", "label", "forecast"}
            assert set(o["forecast"]) == set(out["policy"])
        seen_options |= bool(acc)
        assert json.loads(json.dumps(out)) == out
        assert (svc._rooms["a"]["view"] == before).all()           # advise changes no thread
        svc.continue_room("a")
    assert seen_options
    # another seat, named
    assert svc.advise("a", player_id=5, n_rollouts=2, max_turns=3)["playerId"] == 5
    assert chunks[0].action_calls[-1][3][0] == [(5, 1)]


def test_advise_two_truths_candidates_by_phase():
    from game_engine_amd.messages import ACT_TT_STATEMENTS
    svc, chunks = _service(chunk_rooms=2)
    svc.create_room("t", "two-truths-and-a-lie", _players(4, humans=(1,)), dsl=load_dsl("two-truths-and-a-lie"))
    tb = svc._rooms["t"]["table"]
    acts = {r["phase_id"]: r["act"] for r in tb.rows()}
    kinds = set()
    for _ in range(14):
        out = svc.advise("t", n_rollouts=3, max_turns=10)
        act = acts.get(int(svc._rooms["t"]["view"]["phase_id"]), 0)
        want = [1] if act == ACT_TT_STATEMENTS else [1, 2, 3]
        kinds.add(len(want))
        assert chunks[0].action_calls[-1][3] == [[(1, c)] for c in want] + [[]]
        assert [o["choice"] for o in out["options"]] == _accepted(svc, "t", 1, want)
        assert all(o["label"] == str(o["choice"]) for o in out["options"])
        svc.continue_room("t")
    assert kinds == {1, 3}


def test_advises_group_by_chunk_and_match_advise():
    svc, chunks = _service(chunk_rooms=2)
    for t in ("a", "b", "c"):
        svc.create_room(t, "werewolf-(mafia)", _players(8, humans=(1,)), dsl=load_dsl("werewolf-(mafia)"))
    svc.create_room("tt", "two-truths-and-a-lie", _players(4, humans=(3,)), dsl=load_dsl("two-truths-and-a-lie"))
    for _ in range(3):
        svc.handle_messages([(t, "Continue") for t in ("a", "b", "c", "tt")])
    out = svc.advises(["c", "a", "tt", "b"], [None, 4, None, None], n_rollouts=5, max_turns=20)
    # a, b share chunk 0; c is in chunk 1; tt has a pool of its own: one call each
    assert [len(c.action_calls) for c in chunks] == [1, 1, 1]
    rooms, _, _, actions, _, _, _ = chunks[0].action_calls[0]
    assert rooms == [0] * 9 + [1] * 9
    assert actions[:9] == [[(4, c)] for c in range(1, 9)] + [[]] and actions[9:] == [[(1, c)] for c in range(1, 9)] + [[]]
    assert [o["threadId"] for o in out] == ["c", "a", "tt", "b"] and [o["playerId"] for o in out] == [1, 4, 3, 1]
    assert out[1] == svc.advise("a", 4, n_rollouts=5, max_turns=20)
    assert out[0] == svc.advise("c", n_rollouts=5, max_turns=20)
    assert out[2]["policy"] == svc.forecast("tt", n_rollouts=5, max_turns=20)


def test_advise_default_seat_and_caps():
    svc, _ = _service()
    svc.create_room("bots", "werewolf-(mafia)", _players(8), dsl=load_dsl("werewolf-(mafia)"))
    with pytest.raises(ValueError):
        svc.advise("bots")
    with pytest.raises(ValueError):
        svc.advises(["bots"], n_rollouts=4)
    assert svc.advise("bots", player_id=3, n_rollouts=2, max_turns=2)["playerId"] == 3
    with pytest.raises(ValueError):
        svc.advise("bots", 3, n_rollouts=65537)
    with pytest.raises(KeyError):
        svc.advise("nobody", 1)

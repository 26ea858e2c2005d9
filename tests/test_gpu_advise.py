"""Advice through RoomService and RoomPoolService (-m gpu): the strings_human_* reference runs replayed message by message, with
an advise wherever the human seat has an action due.  Every advise equals the RoomBatch-level rollout_actions of the thread's room
under forecast's key and seed and the oracle's playouts; the golden's next choice of that seat is among the options; every message
output still equals the golden; the Node twins print the same JSON."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_dsl, load_golden
from game_engine_amd import GameTable, RoomBatch, RoomPoolService, RoomService
from game_engine_amd import messages as M
from game_engine_amd.room_service import FORECAST_SEED_XOR, advise_candidates, advise_output
from game_engine_amd.stepper import PACK_WEREWOLF, slot_values
from game_engine_amd.toolcalls import WW_IS_ALIVE
from oracle.oracle import Oracle
from parity_util import views_as_oracle_rooms
from rollout_actions_ref import inject_all, reference_rollout_actions
from test_messages import _check_turn
from test_strings_golden import _strip

pytestmark = pytest.mark.gpu

FILES = ["strings_human_werewolf_n8.json", "strings_human_two_truths_and_a_lie_n4.json", "strings_human_draft_werewolf_n8.json"]
R, MT = 128, 300


def _expected(g, case, view, turn, names, seat, orc):
    key = (case["room"] << 16) & (2 ** 64 - 1)
    seed = case["seed"] ^ FORECAST_SEED_XOR
    tb = GameTable(load_dsl(g["game"]))
    cands = advise_candidates(tb, view)
    acts = [[(seat, c)] for c in cands] + [[]]
    with RoomBatch([(tb, g["n_players"], 1, 0)], seed=1) as b:
        b.write_rooms(0, np.asarray(view).reshape(1))
        w, st = b.rollout_actions([0] * len(acts), [key] * len(acts), [turn] * len(acts), acts, R, MT, seed=seed)
    rec = views_as_oracle_rooms(orc, np.asarray(view).reshape(1))[0]
    for k, act in enumerate(acts):
        want, wst = reference_rollout_actions(orc, rec.copy(), seed, key, turn, act, R, MT)
        assert int(st[k]) == wst and (w[k] == want).all(), (k, act, np.nonzero(w[k] != want)[0].tolist())
    return advise_output(tb, names, "t", turn, seat, view, cands, R, MT, w, st)


def _due(orc, view, seat, tb):
    rec = views_as_oracle_rooms(orc, np.asarray(view).reshape(1))[0]
    return [c for c in advise_candidates(tb, view) if inject_all(orc, rec, [(seat, c)])[1] == 0]


def _replay_with_advice(svc, g, case, where, pool):
    orc = Oracle(load_dsl(g["game"]), g["n_players"])
    tb = GameTable(load_dsl(g["game"]))
    players = [{"name": nm, "gamePlayerId": i + 1, "isBot": (i + 1) not in case["human_seats"]} for i, nm in enumerate(case["names"])]
    svc.create_room("t", g["game"], players, dsl=load_dsl(g["game"]), room_index=case["room"])
    seat = min(case["human_seats"])
    sizes, out, seen, matched = (0, 0, 0), None, [], 0
    for k, want in enumerate(case["messages"]):
        room = svc._rooms["t"]
        view = room["view"]
        due = _due(orc, view, seat, tb)
        if due:
            turn = room["turn"] if pool else room["batch"].turn
            got = svc.advise("t", n_rollouts=R, max_turns=MT)
            assert got == _expected(g, case, view, turn, room["names"], seat, orc), (where, k)
            assert [o["choice"] for o in got["options"]] == due
            assert got["policy"] == svc.forecast("t", n_rollouts=R, max_turns=MT)
            # the seat's actual next choice, where this message makes one, is among the options
            n = int(view["n_players"])
            pid = int(view["phase_id"])
            act = next((r["act"] for r in tb.rows() if r["phase_id"] == pid), 0)
            alive = [bool(slot_values(tb, view, i)[WW_IS_ALIVE]) for i in range(n)] if tb.pack == PACK_WEREWOLF else [True] * n
            for s, c in M.resolve(want["message"], room["panel"], act, tb.pack, room["names"], alive, room["human_seats"]):
                if s == seat and c in due:
                    assert c in [o["choice"] for o in got["options"]]
                    matched += 1
                    break
            seen.append(got)
        out = svc.handle_message("t", want["message"])
        assert out["played"] == want["played"], (where, k)
        sizes = _check_turn(out["state"], sizes, want, f"{where} message {k}: {want['message'][:60]!r}")
    final = case["final"]
    assert _strip(out["state"]["playerActions"]) == final["playerActions"]
    assert out["state"]["game_notes"] == final["game_notes"] and _strip(out["state"]["phase_history"]) == final["phase_history"]
    svc.close()
    return seen, matched


@pytest.mark.parametrize("name", FILES)
def test_advice_between_messages_equals_the_rollout_and_the_oracle(name):
    g = load_golden(name)
    advised = matched = 0
    for case in g["cases"][:2]:
        a, ma = _replay_with_advice(RoomService(seed=case["seed"]), g, case, f"{name} room={case['room']}", pool=False)
        b, mb = _replay_with_advice(RoomPoolService(seed=case["seed"], chunk_rooms=8), g, case, f"{name} room={case['room']} (pool)", pool=True)
        assert a == b and ma == mb
        advised += len(a)
        matched += ma
    if "draft" not in name:                      # (the draft runs' human seat has no action due in their first cases)
        assert advised > 1 and matched > 0


def test_pool_advises_in_one_call_per_chunk():
    dsl = load_dsl("werewolf-(mafia)")
    players = [{"name": f"P{i + 1}", "isBot": i != 2} for i in range(8)]
    pool = RoomPoolService(seed=5, chunk_rooms=4)
    ref = RoomService(seed=5)
    tids = [f"t{i}" for i in range(10)]
    for t in tids:
        pool.create_room(t, "werewolf-(mafia)", players, dsl=dsl)
        ref.create_room(t, "werewolf-(mafia)", players, dsl=dsl)
    for k in range(8):
        sub = tids[k:]
        pool.handle_messages([(t, "Continue") for t in sub])
        for t in sub:
            ref.continue_room(t)
    got = pool.advises(tids[::-1], n_rollouts=300, max_turns=500)
    assert got == [ref.advise(t, n_rollouts=300, max_turns=500) for t in tids[::-1]]
    assert all(o["playerId"] == 3 for o in got) and any(o["options"] for o in got)
    assert pool.advise("t1", 5, n_rollouts=64, max_turns=50) == ref.advise("t1", 5, n_rollouts=64, max_turns=50)
    bots = RoomService(seed=1)
    bots.create_room("b", "werewolf-(mafia)", [{"name": f"P{i + 1}"} for i in range(8)], dsl=dsl)
    with pytest.raises(ValueError):
        bots.advise("b")
    bots.close()
    pool.close()
    ref.close()


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not available")
@pytest.mark.parametrize("name", ["strings_human_werewolf_n8.json", "strings_human_two_truths_and_a_lie_n4.json"])
def test_node_advice_prints_the_same_json(tmp_path, name):
    g = load_golden(name)
    case = g["cases"][0]
    script = {"game": g["game"], "dsl": os.path.join(ROOT, "tests", "golden", "dsl", f"{g['game']}.json"), "seed": case["seed"],
              "room": case["room"], "names": case["names"], "humans": case["human_seats"],
              "messages": [m["message"] for m in case["messages"][:14]], "rollouts": R, "maxTurns": MT}
    sp = tmp_path / "script.json"
    sp.write_text(json.dumps(script))
    p = subprocess.run(["node", os.path.join(ROOT, "game_engine_amd", "node", "selftest_advise.js"), str(sp)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    node_lines = p.stdout.strip().splitlines()
    py_lines = []
    for svc in (RoomService(seed=case["seed"]), RoomPoolService(seed=case["seed"], chunk_rooms=8)):
        players = [{"name": nm, "gamePlayerId": i + 1, "isBot": (i + 1) not in case["human_seats"]} for i, nm in enumerate(case["names"])]
        svc.create_room("t", g["game"], players, dsl=load_dsl(g["game"]), room_index=case["room"])
        for text in script["messages"]:
            py_lines.append(json.dumps(svc.advise("t", n_rollouts=R, max_turns=MT), separators=(",", ":"), ensure_ascii=False))
            svc.handle_message("t", text)
        svc.close()
    assert node_lines == py_lines and any('"options":[{' in x for x in py_lines)

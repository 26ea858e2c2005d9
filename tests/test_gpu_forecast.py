"""Forecasts through RoomService and RoomPoolService (-m gpu): the strings_human_* reference runs replayed message by message
with forecasts in between.  Every forecast equals the RoomBatch-level rollout of the thread's room under the documented key and
seed and the oracle's playouts; every message output still equals the golden; the Node twin prints the same JSON."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_dsl, load_golden
from game_engine_amd import GameTable, RoomBatch, RoomPoolService, RoomService
from game_engine_amd.room_service import FORECAST_SEED_XOR, forecast_output
from oracle.oracle import Oracle
from parity_util import views_as_oracle_rooms
from rollout_ref import reference_rollout
from test_messages import _check_turn
from test_strings_golden import _strip

pytestmark = pytest.mark.gpu

FILES = ["strings_human_werewolf_n8.json", "strings_human_two_truths_and_a_lie_n4.json", "strings_human_draft_werewolf_n8.json"]
R, M = 512, 400


def _expected(g, case, view, turn, names, orc):
    key = (case["room"] << 16) & (2 ** 64 - 1)
    seed = case["seed"] ^ FORECAST_SEED_XOR
    n = g["n_players"]
    tb = GameTable(load_dsl(g["game"]))
    with RoomBatch([(tb, n, 1, 0)], seed=1) as b:
        b.write_rooms(0, np.asarray(view).reshape(1))
        w = b.rollout_rooms([0], [key], [turn], R, M, seed=seed)[0]
    want = reference_rollout(orc, views_as_oracle_rooms(orc, np.asarray(view).reshape(1))[0], seed, key, turn, R, M)
    assert (w == want).all(), np.nonzero(w != want)[0].tolist()
    return forecast_output(tb, names, "t", turn, R, M, w)


def _replay_with_forecasts(svc, g, case, where, pool):
    orc = Oracle(load_dsl(g["game"]), g["n_players"])
    players = [{"name": nm, "gamePlayerId": i + 1, "isBot": (i + 1) not in case["human_seats"]} for i, nm in enumerate(case["names"])]
    svc.create_room("t", g["game"], players, dsl=load_dsl(g["game"]), room_index=case["room"])
    sizes, out, seen = (0, 0, 0), None, []
    for k, want in enumerate(case["messages"]):
        if k % 3 == 0:
            room = svc._rooms["t"]
            turn = room["turn"] if pool else room["batch"].turn
            got = svc.forecast("t", n_rollouts=R, max_turns=M)
            assert got == _expected(g, case, room["view"], turn, room["names"], orc), (where, k)
            assert svc.forecast("t", n_rollouts=R, max_turns=M) == got                       # same turn: identical
            seen.append(got)
        out = svc.handle_message("t", want["message"])
        assert out["played"] == want["played"], (where, k)
        sizes = _check_turn(out["state"], sizes, want, f"{where} message {k}: {want['message'][:60]!r}")
    final = case["final"]
    assert _strip(out["state"]["playerActions"]) == final["playerActions"]
    assert out["state"]["game_notes"] == final["game_notes"] and _strip(out["state"]["phase_history"]) == final["phase_history"]
    svc.close()
    return seen


@pytest.mark.parametrize("name", FILES)
def test_forecasts_between_messages_equal_the_rollout_and_the_oracle(name):
    g = load_golden(name)
    for case in g["cases"][:2]:
        a = _replay_with_forecasts(RoomService(seed=case["seed"]), g, case, f"{name} room={case['room']}", pool=False)
        b = _replay_with_forecasts(RoomPoolService(seed=case["seed"], chunk_rooms=8), g, case, f"{name} room={case['room']} (pool)", pool=True)
        assert a == b and len(a) > 1


def test_pool_forecasts_in_one_call_per_chunk():
    dsl = load_dsl("werewolf-(mafia)")
    players = [{"name": f"P{i + 1}"} for i in range(8)]
    pool = RoomPoolService(seed=5, chunk_rooms=4)
    ref = RoomService(seed=5)
    tids = [f"t{i}" for i in range(10)]
    for t in tids:
        pool.create_room(t, "werewolf-(mafia)", players, dsl=dsl)
        ref.create_room(t, "werewolf-(mafia)", players, dsl=dsl)
    for k in range(6):
        sub = tids[k:]
        pool.handle_messages([(t, "Continue") for t in sub])
        for t in sub:
            ref.continue_room(t)
    got = pool.forecasts(tids[::-1], n_rollouts=300, max_turns=500)
    assert got == [ref.forecast(t, n_rollouts=300, max_turns=500) for t in tids[::-1]]
    with pytest.raises(ValueError):
        pool.forecast("t0", n_rollouts=65537)
    pool.close()
    ref.close()


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not available")
def test_node_forecasts_print_the_same_json(tmp_path):
    g = load_golden("strings_human_werewolf_n8.json")
    case = g["cases"][0]
    script = {"game": g["game"], "dsl": os.path.join(ROOT, "tests", "golden", "dsl", f"{g['game']}.json"), "seed": case["seed"],
              "room": case["room"], "names": case["names"], "humans": case["human_seats"],
              "messages": [m["message"] for m in case["messages"][:12]], "rollouts": R, "maxTurns": M}
    sp = tmp_path / "script.json"
    sp.write_text(json.dumps(script))
    p = subprocess.run(["node", os.path.join(ROOT, "game_engine_amd", "node", "selftest_rollout.js"), str(sp)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    node_lines = p.stdout.strip().splitlines()
    py_lines = []
    for svc, pool in ((RoomService(seed=case["seed"]), False), (RoomPoolService(seed=case["seed"], chunk_rooms=8), True)):
        players = [{"name": nm, "gamePlayerId": i + 1, "isBot": (i + 1) not in case["human_seats"]} for i, nm in enumerate(case["names"])]
        svc.create_room("t", g["game"], players, dsl=load_dsl(g["game"]), room_index=case["room"])
        for text in script["messages"]:
            py_lines.append(json.dumps(svc.forecast("t", n_rollouts=R, max_turns=M), separators=(",", ":"), ensure_ascii=False))
            svc.handle_message("t", text)
        svc.close()
    assert node_lines == py_lines

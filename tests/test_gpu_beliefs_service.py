"""Beliefs through RoomService and RoomPoolService (-m gpu): the strings_human_* reference runs replayed message by message, with
advise(view="seat", beliefs=...) - plain and comparing - and forecast(seat=..., beliefs=...) wherever the human seat has an
action due.  Each equals the RoomBatch-level rollout_beliefs of the thread's room under forecast's key and seed; beliefs=None is
today's output; a pool call that mixes threads with and without beliefs equals the single calls; the Node twins print the same
JSON and refuse the same arguments."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_dsl, load_golden
from game_engine_amd import GameTable, RoomBatch, RoomPoolService, RoomService
from game_engine_amd.room_service import FORECAST_SEED_XOR, advise_candidates, advise_output, belief_bytes, seat_forecast_output
from oracle.oracle import Oracle
from test_gpu_advise import _due

pytestmark = pytest.mark.gpu

FILES = ["strings_human_werewolf_n8.json", "strings_human_two_truths_and_a_lie_n4.json"]
BELIEFS = {"strings_human_werewolf_n8.json": {2: 255, 5: 0, "7": 40}, "strings_human_two_truths_and_a_lie_n4.json": {1: 200, 3: 0}}
R, MT, MESSAGES = 128, 300, 12


def _expected(g, case, view, turn, names, seat, bel, compare):
    key = (case["room"] << 16) & (2 ** 64 - 1)
    seed = case["seed"] ^ FORECAST_SEED_XOR
    tb = GameTable(load_dsl(g["game"]))
    cands = advise_candidates(tb, view)
    acts = [[(seat, c)] for c in cands] + [[]]
    k = len(acts)
    extra = {"baseline": [k - 1] * k, "subjects": [seat] * k} if compare else {}
    with RoomBatch([(tb, g["n_players"], 1, 0)], seed=1) as b:
        b.write_rooms(0, np.asarray(view).reshape(1))
        res = b.rollout_beliefs([0] * k, [key] * k, [turn] * k, [seat] * k, acts, [list(bel)] * k, R, MT, seed=seed, **extra)
    adv = advise_output(tb, names, "t", turn, seat, view, cands, R, MT, res[0], res[1], True, res[2] if compare else None, bel)
    return adv, seat_forecast_output(tb, names, "t", turn, R, MT, seat, res[0][len(cands)], bel)


def _replay(svc, g, case, beliefs, pool):
    orc = Oracle(load_dsl(g["game"]), g["n_players"])
    tb = GameTable(load_dsl(g["game"]))
    players = [{"name": nm, "gamePlayerId": i + 1, "isBot": (i + 1) not in case["human_seats"]} for i, nm in enumerate(case["names"])]
    svc.create_room("t", g["game"], players, dsl=load_dsl(g["game"]), room_index=case["room"])
    seat = min(case["human_seats"])
    bel = belief_bytes("t", tb, g["n_players"], beliefs, True)
    seen = []
    for k, want in enumerate(case["messages"][:MESSAGES]):
        room = svc._rooms["t"]
        view = room["view"]
        if _due(orc, view, seat, tb):
            turn = room["turn"] if pool else room["batch"].turn
            adv = svc.advise("t", n_rollouts=R, max_turns=MT, view="seat", beliefs=beliefs)
            advc = svc.advise("t", n_rollouts=R, max_turns=MT, view="seat", beliefs=beliefs, compare=True)
            fc = svc.forecast("t", n_rollouts=R, max_turns=MT, seat=seat, beliefs=beliefs)
            assert (adv, fc) == _expected(g, case, view, turn, room["names"], seat, bel, False), k
            assert advc == _expected(g, case, view, turn, room["names"], seat, bel, True)[0], k
            assert adv["beliefs"] == list(bel) == fc["beliefs"] and list(adv)[-1] == "beliefs" and advc["compare"] is True
            plain = svc.advise("t", n_rollouts=R, max_turns=MT, view="seat")
            assert "beliefs" not in plain and plain == svc.advise("t", n_rollouts=R, max_turns=MT, view="seat", beliefs=None)
            seen.append((adv, advc, fc, plain))
        svc.handle_message("t", want["message"])
    svc.close()
    return seen


@pytest.mark.parametrize("name", FILES)
def test_services_equal_the_direct_call(name):
    g = load_golden(name)
    case = g["cases"][0]
    a = _replay(RoomService(seed=case["seed"]), g, case, BELIEFS[name], pool=False)
    b = _replay(RoomPoolService(seed=case["seed"], chunk_rooms=8), g, case, BELIEFS[name], pool=True)
    assert a == b and len(a) >= 1


def test_pool_mixes_threads_with_and_without_beliefs():
    dsl = load_dsl("werewolf-(mafia)")
    players = [{"name": f"P{i + 1}", "isBot": i != 2} for i in range(8)]
    pool = RoomPoolService(seed=5, chunk_rooms=4)
    ref = RoomService(seed=5)
    tids = [f"t{i}" for i in range(6)]
    for t in tids:
        pool.create_room(t, "werewolf-(mafia)", players, dsl=dsl)
        ref.create_room(t, "werewolf-(mafia)", players, dsl=dsl)
    for k in range(6):
        pool.handle_messages([(t, "Continue") for t in tids[k:]])
        for t in tids[k:]:
            ref.continue_room(t)
    bel = [None if i % 2 else {1 + i: 255, 8: 0} for i in range(6)]
    for compare in (False, True):
        got = pool.advises(tids, n_rollouts=200, max_turns=400, view="seat", compare=compare, beliefs=bel)
        assert got == [ref.advise(t, n_rollouts=200, max_turns=400, view="seat", compare=compare, beliefs=bm) for t, bm in zip(tids, bel)]
    seats = [None if i == 1 else 1 + i for i in range(6)]
    fcs = pool.forecasts(tids, n_rollouts=200, max_turns=400, seats=seats, beliefs=[None if s is None else bm for s, bm in zip(seats, bel)])
    assert fcs == [ref.forecast(t, n_rollouts=200, max_turns=400, seat=s, beliefs=None if s is None else bm) for t, s, bm in zip(tids, seats, bel)]
    assert "beliefs" in fcs[0] and "beliefs" not in fcs[1] and "beliefs" not in fcs[3]
    # the beliefs move something: from some seat's view (a Villager's) a strong suspicion changes the forecast, equal weights never
    moved = 0
    for s in range(1, 9):                                                      # (t5 has played six turns: its roles are dealt)
        plain = ref.forecast("t5", n_rollouts=200, max_turns=400, seat=s)
        hot = ref.forecast("t5", n_rollouts=200, max_turns=400, seat=s, beliefs={s % 8 + 1: 255, (s + 1) % 8 + 1: 0})
        flat = ref.forecast("t5", n_rollouts=200, max_turns=400, seat=s, beliefs={k: 3 for k in range(1, 9)})
        assert {k: v for k, v in flat.items() if k != "beliefs"} == plain
        moved += {k: v for k, v in hot.items() if k != "beliefs"} != plain
    assert moved >= 1
    pool.close()
    ref.close()


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not available")
@pytest.mark.parametrize("name", FILES)
def test_node_prints_the_same_json(tmp_path, name):
    g = load_golden(name)
    case = g["cases"][0]
    script = {"game": g["game"], "dsl": os.path.join(ROOT, "tests", "golden", "dsl", f"{g['game']}.json"), "seed": case["seed"],
              "room": case["room"], "names": case["names"], "humans": case["human_seats"],
              "messages": [m["message"] for m in case["messages"][:MESSAGES]], "rollouts": R, "maxTurns": MT,
              "beliefs": {str(k): v for k, v in BELIEFS[name].items()}}
    sp = tmp_path / "script.json"
    sp.write_text(json.dumps(script))
    p = subprocess.run(["node", os.path.join(ROOT, "game_engine_amd", "node", "selftest_beliefs.js"), str(sp)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    node_lines = p.stdout.strip().splitlines()
    py_lines = []
    seat = min(case["human_seats"])
    for svc in (RoomService(seed=case["seed"]), RoomPoolService(seed=case["seed"], chunk_rooms=8)):
        players = [{"name": nm, "gamePlayerId": i + 1, "isBot": (i + 1) not in case["human_seats"]} for i, nm in enumerate(case["names"])]
        svc.create_room("t", g["game"], players, dsl=load_dsl(g["game"]), room_index=case["room"])
        for text in script["messages"]:
            for compare in (False, True):
                py_lines.append(json.dumps(svc.advise("t", n_rollouts=R, max_turns=MT, view="seat", compare=compare, beliefs=BELIEFS[name]),
                                           separators=(",", ":"), ensure_ascii=False))
            py_lines.append(json.dumps(svc.forecast("t", n_rollouts=R, max_turns=MT, seat=seat, beliefs=BELIEFS[name]),
                                       separators=(",", ":"), ensure_ascii=False))
            svc.handle_message("t", text)
        svc.close()
    assert node_lines == py_lines and any('"beliefs":[' in x for x in py_lines) and any('"options":[{' in x for x in py_lines)

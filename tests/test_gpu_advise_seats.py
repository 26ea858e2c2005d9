"""Seat-view advice and forecasts through RoomService and RoomPoolService (-m gpu): the strings_human_* reference runs replayed
message by message, with advise(view="seat") and forecast(seat=...) wherever the human seat has an action due.  Each equals the
RoomBatch-level rollout_seats of the thread's room under forecast's key and seed and the oracle reference; every message output
still equals the golden; the Node twins print the same JSON."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_dsl, load_golden
from game_engine_amd import GameTable, RoomBatch, RoomPoolService, RoomService
from game_engine_amd.room_service import FORECAST_SEED_XOR, advise_candidates, advise_output, seat_forecast_output
from oracle.oracle import Oracle
from parity_util import views_as_oracle_rooms
from rollout_seats_ref import reference_rollout_seats
from test_gpu_advise import _due
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
        w, st = b.rollout_seats([0] * len(acts), [key] * len(acts), [turn] * len(acts), [seat] * len(acts), acts, R, MT, seed=seed)
    rec = views_as_oracle_rooms(orc, np.asarray(view).reshape(1))[0]
    for k, act in enumerate(acts):
        want, wst = reference_rollout_seats(orc, rec.copy(), seed, key, turn, seat, act, R, MT)
        assert int(st[k]) == wst and (w[k] == want).all(), (k, act, np.nonzero(w[k] != want)[0].tolist())
    adv = advise_output(tb, names, "t", turn, seat, view, cands, R, MT, w, st, True)
    return adv, seat_forecast_output(tb, names, "t", turn, R, MT, seat, w[len(cands)])


def _replay(svc, g, case, where, pool):
    orc = Oracle(load_dsl(g["game"]), g["n_players"])
    tb = GameTable(load_dsl(g["game"]))
    players = [{"name": nm, "gamePlayerId": i + 1, "isBot": (i + 1) not in case["human_seats"]} for i, nm in enumerate(case["names"])]
    svc.create_room("t", g["game"], players, dsl=load_dsl(g["game"]), room_index=case["room"])
    seat = min(case["human_seats"])
    sizes, out, seen = (0, 0, 0), None, []
    for k, want in enumerate(case["messages"]):
        room = svc._rooms["t"]
        view = room["view"]
        due = _due(orc, view, seat, tb)
        if due:
            turn = room["turn"] if pool else room["batch"].turn
            adv = svc.advise("t", n_rollouts=R, max_turns=MT, view="seat")
            fc = svc.forecast("t", n_rollouts=R, max_turns=MT, seat=seat)
            assert (adv, fc) == _expected(g, case, view, turn, room["names"], seat, orc), (where, k)
            assert [o["choice"] for o in adv["options"]] == due and adv["view"] == "seat" and fc["seat"] == seat
            assert {k2: v for k2, v in fc.items() if k2 != "seat"} == adv["policy"]
            seen.append((adv, fc))
        out = svc.handle_message("t", want["message"])
        assert out["played"] == want["played"], (where, k)
        sizes = _check_turn(out["state"], sizes, want, f"{where} message {k}: {want['message'][:60]!r}")
    final = case["final"]
    assert _strip(out["state"]["playerActions"]) == final["playerActions"]
    assert out["state"]["game_notes"] == final["game_notes"] and _strip(out["state"]["phase_history"]) == final["phase_history"]
    svc.close()
    return seen


@pytest.mark.parametrize("name", FILES)
def test_seat_view_between_messages_equals_the_rollout_and_the_oracle(name):
    g = load_golden(name)
    advised = 0
    for case in g["cases"][:2]:
        a = _replay(RoomService(seed=case["seed"]), g, case, f"{name} room={case['room']}", pool=False)
        b = _replay(RoomPoolService(seed=case["seed"], chunk_rooms=8), g, case, f"{name} room={case['room']} (pool)", pool=True)
        assert a == b
        advised += len(a)
    if "draft" not in name:                      # (the draft runs' human seat has no action due in their first cases)
        assert advised > 1


def test_pool_seat_views_in_one_call_per_chunk():
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
    got = pool.advises(tids[::-1], n_rollouts=300, max_turns=500, view="seat")
    assert got == [ref.advise(t, n_rollouts=300, max_turns=500, view="seat") for t in tids[::-1]]
    seats = [None if i % 3 == 0 else 1 + i % 8 for i in range(10)]
    fcs = pool.forecasts(tids, n_rollouts=300, max_turns=500, seats=seats)
    assert fcs == [ref.forecast(t, n_rollouts=300, max_turns=500, seat=s) for t, s in zip(tids, seats)]
    assert fcs[0] == pool.forecast("t0", n_rollouts=300, max_turns=500) and "seat" not in fcs[0]
    # the full view is unchanged by the seat view's existence, and differs from it somewhere
    full = pool.advises(tids, n_rollouts=300, max_turns=500)
    assert full == [ref.advise(t, n_rollouts=300, max_turns=500) for t in tids]
    assert any(f["policy"] != s["policy"] for f, s in zip(full, got[::-1]))
    pool.close()
    ref.close()


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not available")
@pytest.mark.parametrize("name", ["strings_human_werewolf_n8.json", "strings_human_two_truths_and_a_lie_n4.json"])
def test_node_seat_view_prints_the_same_json(tmp_path, name):
    g = load_golden(name)
    case = g["cases"][0]
    script = {"game": g["game"], "dsl": os.path.join(ROOT, "tests", "golden", "dsl", f"{g['game']}.json"), "seed": case["seed"],
              "room": case["room"], "names": case["names"], "humans": case["human_seats"],
              "messages": [m["message"] for m in case["messages"][:14]], "rollouts": R, "maxTurns": MT}
    sp = tmp_path / "script.json"
    sp.write_text(json.dumps(script))
    p = subprocess.run(["node", os.path.join(ROOT, "game_engine_amd", "node", "selftest_seats.js"), str(sp)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    node_lines = p.stdout.strip().splitlines()
    py_lines = []
    seat = min(case["human_seats"])
    for svc in (RoomService(seed=case["seed"]), RoomPoolService(seed=case["seed"], chunk_rooms=8)):
        players = [{"name": nm, "gamePlayerId": i + 1, "isBot": (i + 1) not in case["human_seats"]} for i, nm in enumerate(case["names"])]
        svc.create_room("t", g["game"], players, dsl=load_dsl(g["game"]), room_index=case["room"])
        for text in script["messages"]:
            py_lines.append(json.dumps(svc.advise("t", n_rollouts=R, max_turns=MT, view="seat"), separators=(",", ":"), ensure_ascii=False))
            py_lines.append(json.dumps(svc.forecast("t", n_rollouts=R, max_turns=MT, seat=seat), separators=(",", ":"), ensure_ascii=False))
            svc.handle_message("t", text)
        svc.close()
    assert node_lines == py_lines and any('"view":"seat"' in x for x in py_lines) and any('"options":[{' in x for x in py_lines)

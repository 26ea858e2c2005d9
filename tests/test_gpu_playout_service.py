"""Playout bots through RoomService and RoomPoolService (-m gpu): on a thread with playout seats, every bot choice the turn logs
is the argmax, with the pick(d, m) tie-break, of advise(view="seat")'s option forecasts at that moment restricted to the
policy's candidates (the same keys and seed); pool threads equal RoomService threads message by message, threads without
playout seats beside them included; the Node twins print the same bytes."""
import json
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT, load_dsl
from game_engine_amd import RoomPoolService, RoomService
from oracle.oracle import Oracle
from oracle.rng import pick
from parity_util import views_as_oracle_rooms
from playout_ref import candidates, due_seats, seat_draw

pytestmark = pytest.mark.gpu

R, MT, SEED = 96, 160, 7


def _players(n):
    return [{"name": f"P{i + 1}", "gamePlayerId": i + 1, "isBot": True} for i in range(n)]


def _logged(out):
    """{seat: choice} of the bots' update_player_actions calls of one turn."""
    return {int(c["args"]["player_id"]): int(re.search(r"\|c=(\d+)\]", c["args"]["actions"]).group(1))
            for c in out["toolCalls"] if c["name"] == "update_player_actions"}


def _wins(forecast, seat):
    p = forecast["players"][str(seat)]
    return p["wins"] if "wins" in p else p["topScore"]


@pytest.mark.parametrize("game,n,seats,turns", [("werewolf-(mafia)", 8, (2, 3, 4, 5, 6, 7, 8), 40), ("werewolf-(mafia)", 12, (1, 5, 9, 12), 30),
                                                ("two-truths-and-a-lie", 4, (1, 2, 3, 4), 30)])
def test_bot_choices_are_the_argmax_of_seat_view_advice(game, n, seats, turns):
    dsl = load_dsl(game)
    svc = RoomService(seed=SEED, playout_rollouts=R, playout_max_turns=MT)
    svc.create_room("t", game, _players(n), dsl=dsl, room_index=321, playout_seats=seats)
    orc = Oracle(dsl, n)
    room = svc._rooms["t"]
    checked = 0
    for _ in range(turns):
        turn = room["batch"].turn
        rec = views_as_oracle_rooms(orc, room["view"].reshape(1))[0]
        expect = {}
        for s in due_seats(orc, rec, SEED, 321, turn, False, 0):
            cand = candidates(orc, rec, s)
            if s not in seats or len(cand) < 2:
                continue
            adv = svc.advise("t", s, R, MT, view="seat")
            vals = {o["choice"]: _wins(o["forecast"], s) for o in adv["options"]}
            top = max(vals[c] for c in cand)
            tied = [c for c in cand if vals[c] == top]
            expect[s] = tied[pick(seat_draw(SEED, 321, turn, s), len(tied))]
        got = _logged(svc.continue_room("t"))
        for s, c in expect.items():
            assert got.get(s) == c, (turn, s, got, expect)
        checked += len(expect)
    assert checked > 0
    svc.close()


@pytest.mark.parametrize("view", ["seat", "full"])
def test_pool_threads_equal_room_service_threads(view):
    threads = [("a", "werewolf-(mafia)", 8, (1, 2, 3)), ("b", "werewolf-(mafia)", 8, ()), ("c", "two-truths-and-a-lie", 4, (2, 4)),
               ("d", "werewolf-(mafia)", 8, (4, 5, 6, 7, 8)), ("e", "werewolf-(mafia)", 12, (3,))]
    single = RoomService(seed=SEED, playout_rollouts=64, playout_max_turns=120, playout_view=view)
    pool = RoomPoolService(seed=SEED, chunk_rooms=2, playout_rollouts=64, playout_max_turns=120, playout_view=view)
    for k, (tid, game, n, seats) in enumerate(threads):
        for svc in (single, pool):
            svc.create_room(tid, game, _players(n), dsl=load_dsl(game), room_index=900 + k, playout_seats=seats)
    for t in range(30):
        outs = pool.handle_messages([(tid, "Continue") for tid, _, _, _ in threads])
        for (tid, _, _, _), got in zip(threads, outs):
            want = single.handle_message(tid, "Continue")
            for f in ("toolCalls", "uiCalls", "played", "kind"):
                assert json.dumps(got[f], sort_keys=True) == json.dumps(want[f], sort_keys=True), (t, tid, f)
    single.close()
    pool.close()


@pytest.mark.skipif(shutil.which("node") is None or not os.path.exists(os.path.join(ROOT, "game_engine_amd", "node", "ge_addon.node")),
                    reason="node or the N-API addon is not built here")
@pytest.mark.parametrize("view", ["seat", "full"])
def test_node_prints_the_same_bytes(tmp_path, view):
    threads = [{"id": "a", "game": "werewolf-(mafia)", "n": 8, "seats": [1, 2, 3, 4], "room": 71},
               {"id": "b", "game": "two-truths-and-a-lie", "n": 4, "seats": [2, 3], "room": 72},
               {"id": "c", "game": "werewolf-(mafia)", "n": 8, "seats": [], "room": 73}]
    for th in threads:
        th["dsl"] = os.path.join(ROOT, "tests", "golden", "dsl", f"{th['game']}.json")
        th["names"] = [f"P{i + 1}" for i in range(th["n"])]
    script = {"seed": SEED, "rollouts": 48, "maxTurns": 100, "view": view, "turns": 16, "threads": threads}
    sp = tmp_path / "script.json"
    sp.write_text(json.dumps(script))
    p = subprocess.run(["node", os.path.join(ROOT, "game_engine_amd", "node", "selftest_playout.js"), str(sp)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    py_lines = []
    for svc in (RoomService(seed=SEED, playout_rollouts=48, playout_max_turns=100, playout_view=view),
                RoomPoolService(seed=SEED, chunk_rooms=2, playout_rollouts=48, playout_max_turns=100, playout_view=view)):
        for th in threads:
            svc.create_room(th["id"], th["game"], _players(th["n"]), dsl=load_dsl(th["game"]), room_index=th["room"],
                            playout_seats=th["seats"])
        for _ in range(script["turns"]):
            for th in threads:
                out = svc.handle_message(th["id"], "Continue")
                py_lines.append(json.dumps({"toolCalls": out["toolCalls"], "uiCalls": out["uiCalls"]}, separators=(",", ":"), ensure_ascii=False))
        svc.close()
    assert p.stdout.strip().splitlines() == py_lines

"""Threads handed to the stepper mid-game (-m gpu): AgentStates written into rooms (RoomBatch.write_agent_state,
RoomService.adopt_room, RoomPoolService.adopt_rooms) continue exactly as the thread would have gone on - the DSLs'
players_example blocks against the oracle, and every turn of the bot-only strings goldens and every message boundary of the
strings_human_* goldens against the reference runs' own later turns."""
import copy
import json
import os

import pytest

from conftest import GOLD, load_dsl, load_golden
from game_engine_amd import GameTable, RoomBatch
from oracle.oracle import Oracle
from parity_util import assert_views_equal, oracle_rooms_as_views, views_as_oracle_rooms
from test_adopt_state import STRINGS, example_state, golden_states
from test_strings_golden import _check_turn

pytestmark = pytest.mark.gpu

HUMAN = sorted(f for f in os.listdir(GOLD) if f.startswith("strings_human_"))


def _sizes(state):
    n_act = sum(len(r["actions"]) for r in state["playerActions"].values())
    return n_act, len(state.get("game_notes") or []), len(state["phase_history"])


@pytest.mark.parametrize("game, phase", [("werewolf-(mafia)", 2), ("two-truths-and-a-lie", 5)])
@pytest.mark.parametrize("max_fuse", [0, 1])
def test_players_example_plays_on_as_the_oracle(game, phase, max_fuse):
    dsl = load_dsl(game)
    tb, orc = GameTable(dsl), Oracle(dsl, 4)
    state = example_state(game, phase)
    state["phase_history"] = [{"phase_id": p} for p in range(phase + 1)]     # a thread that played its way to `phase`
    with RoomBatch([(tb, 4, 3)], seed=0xAD0, first_room=40, max_fuse=max_fuse) as b:
        host = b.write_agent_state(1, state)
        assert host["names"]["1"] in ("Alpha", "Alex")
        rooms = views_as_oracle_rooms(orc, b.read_rooms())
        b.step(30)
        orc.run(rooms, 0xAD0, 40, 0, 30, threads=1)
        assert_views_equal(b.read_rooms(), oracle_rooms_as_views(orc, rooms), f"{game} players_example, 30 turns")


def _continue_python(svc, tid, case, k, state, out, where):
    sizes = _sizes(state)
    assert out["toolCalls"] == [] and out["state"]["current_phase_id"] == state["current_phase_id"]
    for t in range(k + 1, len(case["turns"])):
        o = svc.continue_room(tid)
        sizes = _check_turn(o["state"], sizes, case["turns"][t], f"{where} adopted at {k}, turn {t}")


@pytest.mark.parametrize("name", STRINGS)
def test_adopt_at_every_golden_turn_room_service(name):
    from game_engine_amd import RoomService
    g = load_golden(name)
    dsl = load_dsl(g["game"])
    for case in g["cases"]:
        svc = RoomService(seed=case["seed"])
        for k, state in golden_states(case):
            out = svc.adopt_room("t", g["game"], copy.deepcopy(state), dsl=dsl, room_index=case["room"])
            _continue_python(svc, "t", case, k, state, out, f"{name} seed={case['seed']:#x}")
        svc.close()


@pytest.mark.parametrize("name", STRINGS)
def test_adopt_every_golden_turn_at_once_into_the_pool(name):
    from game_engine_amd import RoomPoolService
    g = load_golden(name)
    dsl = load_dsl(g["game"])
    for case in g["cases"]:
        pool = RoomPoolService(seed=case["seed"], chunk_rooms=32)
        pool.create_room("warm", g["game"], [{"name": f"Bot {i + 1}"} for i in range(g["n_players"])], dsl=dsl)
        pool.close("warm")                                       # a reused slot is adopted into without a template write
        states = list(golden_states(case))
        outs = pool.adopt_rooms([(f"t{k}", g["game"], copy.deepcopy(s), {"dsl": dsl, "room_index": case["room"]}) for k, s in states])
        sizes = {}
        for (k, s), o in zip(states, outs):
            assert o["toolCalls"] == [] and o["state"]["current_phase_id"] == s["current_phase_id"]
            sizes[k] = _sizes(s)
        T = len(case["turns"])
        for step in range(1, T):
            live = [k for k, _ in states if k + step < T]
            res = pool.handle_messages([(f"t{k}", "Continue") for k in live])
            for k, o in zip(live, res):
                sizes[k] = _check_turn(o["state"], sizes[k], case["turns"][k + step], f"{name} pool, adopted at {k}, turn {k + step}")
        pool.close()


@pytest.mark.parametrize("name", HUMAN)
def test_adopt_at_every_message_boundary_of_the_human_goldens(name):
    from game_engine_amd import RoomService, RoomPoolService
    g = load_golden(name)
    dsl = load_dsl(g["game"])
    for case in g["cases"]:
        players = [{"name": nm, "gamePlayerId": i + 1, "isBot": (i + 1) not in case["human_seats"]} for i, nm in enumerate(case["names"])]
        ref = RoomService(seed=case["seed"])
        ref.create_room("ref", g["game"], players, dsl=dsl, room_index=case["room"])
        msgs = case["messages"]
        sizes, boundaries = (0, 0, 0), []
        for j, want in enumerate(msgs):
            out = ref.handle_message("ref", want["message"])
            sizes = _check_turn(out["state"], sizes, want, f"{name} reference replay, message {j}")
            view = ref._rooms["ref"]["view"]
            visit = {s: int(view["players"][s - 1][10]) for s in case["human_seats"] if view["players"][s - 1][9]}
            boundaries.append((j, copy.deepcopy(out["state"]), visit, sizes, out["uiCalls"] if out["played"] else None))
        ref.close()
        pool = RoomPoolService(seed=case["seed"], chunk_rooms=16)
        outs = pool.adopt_rooms([(f"b{j}", g["game"], copy.deepcopy(st), {"dsl": dsl, "room_index": case["room"], "players": players,
                                                                           "visit_actions": visit}) for j, st, visit, _, _ in boundaries])
        svc = RoomService(seed=case["seed"])
        for (j, st, visit, sz, ui), po in zip(boundaries, outs):
            o = svc.adopt_room("a", g["game"], copy.deepcopy(st), players=players, dsl=dsl, room_index=case["room"], visit_actions=visit)
            assert o["state"] == st == po["state"], f"{name}: adopted state at message {j}"
            if ui is not None:                                   # the UI the thread showed after its last turn (panel, votingId)
                assert o["uiCalls"] == ui == po["uiCalls"], f"{name}: adopted uiCalls at message {j}"
            s1 = s2 = sz
            for m in range(j + 1, len(msgs)):
                where = f"{name} adopted after message {j}, message {m}"
                a = svc.handle_message("a", msgs[m]["message"])
                b = pool.handle_message(f"b{j}", msgs[m]["message"])
                assert a["played"] == msgs[m]["played"] == b["played"], where
                s1 = _check_turn(a["state"], s1, msgs[m], where)
                s2 = _check_turn(b["state"], s2, msgs[m], where + " (pool)")
        svc.close()
        pool.close()


def test_refused_adoption_leaves_the_services_untouched():
    from game_engine_amd import RoomPoolService, RoomService
    dsl = load_dsl("werewolf-(mafia)")
    players = [{"name": f"Bot {i + 1}"} for i in range(8)]
    good = example_state("werewolf-(mafia)", 2)
    bad = copy.deepcopy(good)
    bad["player_states"]["2"]["role"] = "Seer"
    svc = RoomService(seed=1)
    svc.create_room("t", "werewolf-(mafia)", players, dsl=dsl)
    before = svc.continue_room("t")["state"]
    with pytest.raises(ValueError):
        svc.adopt_room("t", "werewolf-(mafia)", bad, dsl=dsl)
    assert svc._rooms["t"]["log"].agent_state(svc._rooms["t"]["view"]) == before
    svc.close()
    pool = RoomPoolService(seed=1, chunk_rooms=4)
    pool.create_room("t", "werewolf-(mafia)", players, dsl=dsl)
    free = {k: list(p.free) for k, p in pool._pools.items()}
    with pytest.raises(ValueError):
        pool.adopt_rooms([("u", "werewolf-(mafia)", good, {"dsl": dsl}), ("t", "werewolf-(mafia)", bad, {"dsl": dsl})])
    assert set(pool._rooms) == {"t"} and {k: list(p.free) for k, p in pool._pools.items()} == free
    pool.close()


@pytest.mark.skipif(__import__("shutil").which("node") is None, reason="node is not available")
@pytest.mark.parametrize("name", ["strings_werewolf_n8.json", "strings_two_truths_and_a_lie_n4.json", "strings_draft_werewolf_n8.json"])
def test_node_adopt_room_and_adopt_rooms(name):
    import subprocess
    from conftest import ROOT
    g = load_golden(name)
    out = subprocess.run(["node", os.path.join(ROOT, "game_engine_amd", "node", "selftest_adopt.js"),
                          os.path.join(GOLD, "dsl", g["game"] + ".json"), os.path.join(GOLD, name)],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["ok"] is True and r["adoptions"] == 2 * sum(len(c["turns"]) for c in g["cases"]), r

"""AgentState -> room view (stepper.agent_state_to_view): the inverse of view_to_agent_state / RoomLog.agent_state, for threads
handed to the stepper mid-game.  CPU only: the DSLs' own players_example blocks round-trip, the cumulative state of every turn of
the bot-only strings goldens converts to the oracle's room (the rules that derive the phase fields and this visit's actions),
a thread adopted at any of those turns continues on the oracle exactly as the uninterrupted run, and bad states are refused."""
import copy
import json
import os

import numpy as np
import pytest

from conftest import GOLD, load_dsl, load_golden
from game_engine_amd import GameTable
from game_engine_amd.stepper import agent_state_to_view, project_view, view_to_agent_state

GAMES = ["werewolf-(mafia)", "two-truths-and-a-lie", "draft-werewolf-(mafia)"]
STRINGS = sorted(f for f in os.listdir(GOLD) if f.startswith("strings_") and not f.startswith("strings_human_"))


def golden_states(case):
    """(k, the thread's AgentState after turn k) rebuilt from a strings golden case: player_states of turn k and the logs
    accumulated from actions_added / history_added / notes_added."""
    pa, hist, notes = {}, [], []
    for k, t in enumerate(case["turns"]):
        for a in t["actions_added"]:
            rec = pa.setdefault(a["player_id"], {"name": a["name"], "actions": {}})
            rec["actions"][a["id"]] = {"action": a["action"], "phase": a["phase"], "id": a["id"]}
        hist += t["history_added"]
        notes += t["notes_added"]
        yield k, {"current_phase_id": t["current_phase_id"], "current_phase_name": t["current_phase_name"],
                  "player_states": copy.deepcopy(t["player_states"]), "playerActions": copy.deepcopy(pa),
                  "phase_history": list(hist), "game_notes": list(notes)}


def example_state(game, phase_id):
    ex = load_dsl(game)["declaration"]["players_example"]["player_states"]
    return {"current_phase_id": phase_id, "player_states": copy.deepcopy(ex), "playerActions": {}, "phase_history": []}


@pytest.mark.parametrize("game", GAMES)
def test_players_example_round_trip(game):
    tb = GameTable(load_dsl(game))
    state = example_state(game, 0)
    view, host = agent_state_to_view(tb, state)
    back = view_to_agent_state(tb, view)["player_states"]
    for pid, want in state["player_states"].items():
        got = dict(back[pid], name=host["names"][pid])
        got.update(host["statements"].get(pid) is not None and {tb.field_names[9]: host["statements"][pid]} or {})
        got.update(host["extra"].get(pid, {}))
        assert got == want, (game, pid)


def test_players_example_fields_land_in_the_record():
    tb = GameTable(load_dsl("werewolf-(mafia)"))
    view, _ = agent_state_to_view(tb, example_state("werewolf-(mafia)", 2))
    assert int(view["n_players"]) == 4 and int(view["phase_id"]) == 2
    assert [int(view["players"][i][0]) for i in range(4)] == [2, 1, 3, 4]            # Werewolf, Villager, Doctor, Detective
    assert [int(view["players"][i][8]) for i in range(4)] == [2, 0, 2, 1]
    assert int(view["det"][0]) == 2 and not view["det"][1:].any()
    tt = GameTable(load_dsl("two-truths-and-a-lie"))
    view, host = agent_state_to_view(tt, example_state("two-truths-and-a-lie", 5))
    assert [int(view["players"][i][7]) for i in range(4)] == [1, 2, 0, 1]
    assert host["statements"]["1"]["2"] == "I can speak four languages."


@pytest.mark.parametrize("name", STRINGS)
def test_every_golden_turn_converts_to_the_oracle_room(name):
    from oracle.oracle import Oracle
    from parity_util import oracle_rooms_as_views
    g = load_golden(name)
    dsl = load_dsl(g["game"])
    orc, tb = Oracle(dsl, g["n_players"]), GameTable(dsl)
    for case in g["cases"]:
        rooms = orc.init_rooms(1)
        for k, state in golden_states(case):
            orc.run(rooms, case["seed"], case["room"], k, 1)
            want = oracle_rooms_as_views(orc, rooms)[0]
            got, _ = agent_state_to_view(tb, state)
            # every slot, declared or not, acted / choice and prev_phase_id included
            assert project_view(got) == project_view(want), f"{name} seed={case['seed']:#x} turn {k}"
            assert int(got["games"]) == int(want["games"])


@pytest.mark.parametrize("name", STRINGS)
def test_adopted_thread_continues_as_the_uninterrupted_run(name):
    """Adopt at every turn k, step the view on the oracle from turn k + 1 (= len(phase_history)): every later room equals the
    uninterrupted run's."""
    from oracle.oracle import Oracle
    from parity_util import oracle_rooms_as_views, views_as_oracle_rooms
    g = load_golden(name)
    dsl = load_dsl(g["game"])
    orc, tb = Oracle(dsl, g["n_players"]), GameTable(dsl)
    for case in g["cases"]:
        T = len(case["turns"])
        ref, traj = orc.init_rooms(1), []
        for t in range(T):
            orc.run(ref, case["seed"], case["room"], t, 1)
            traj.append(project_view(oracle_rooms_as_views(orc, ref)[0]))
        for k, state in golden_states(case):
            view, _ = agent_state_to_view(tb, state)
            rooms = views_as_oracle_rooms(orc, np.array([view]))
            assert len(state["phase_history"]) == k + 1
            for t in range(k + 1, T):
                orc.run(rooms, case["seed"], case["room"], t, 1)
                assert project_view(oracle_rooms_as_views(orc, rooms)[0]) == traj[t], f"{name} adopted at {k}, turn {t}"


def _bad(state, pid, field, value):
    s = copy.deepcopy(state)
    s["player_states"][pid][field] = value
    return s


@pytest.mark.parametrize("mutate, match", [
    (lambda s: _bad(s, "2", "role", "Seer"), "unknown role"),
    (lambda s: _bad(s, "2", "team", "villager"), "team"),
    (lambda s: {**s, "player_states": {k: v for k, v in s["player_states"].items() if k != "3"}}, "players 1..3"),
    (lambda s: _bad(s, "1", "selected_target_id", 5), "selected_target_id"),
    (lambda s: _bad(s, "2", "investigated_alignments", {"1": "werewolves"}), "investigation"),
    (lambda s: {**s, "current_phase_id": 42}, "current_phase_id"),
    (lambda s: _bad(s, "1", "team", "villagers"), None),                  # role and team are separate slots: held as given
    (lambda s: _bad(s, "2", "is_alive", 1), "boolean"),
    (lambda s: _bad(s, "4", "investigated_alignments", {"9": "werewolves"}), "investigated_alignments"),
])
def test_refusals(mutate, match):
    tb = GameTable(load_dsl("werewolf-(mafia)"))
    state = example_state("werewolf-(mafia)", 2)
    bad = mutate(state)
    if match is None:                       # the record holds role and team apart: this one is accepted and reads back as given
        view, _ = agent_state_to_view(tb, bad)
        assert view_to_agent_state(tb, view)["player_states"]["1"]["team"] == "villagers"
        return
    with pytest.raises(ValueError, match=match):
        agent_state_to_view(tb, bad)


def test_inconsistent_derived_slot_is_refused():
    """wolf_chat_enabled is derived (team == werewolves, POLICY.md 3a): a state that says otherwise cannot be held."""
    tb = GameTable(load_dsl("draft-werewolf-(mafia)"))
    state = example_state("draft-werewolf-(mafia)", 2)
    state["player_states"]["2"]["wolf_chat_enabled"] = True
    with pytest.raises(ValueError, match="player 2: field 'wolf_chat_enabled'"):
        agent_state_to_view(tb, state)


def test_phase_fields_and_visit_actions():
    tb = GameTable(load_dsl("werewolf-(mafia)"))
    s = example_state("werewolf-(mafia)", 7)
    s["phase_history"] = [{"phase_id": p} for p in (0, 0, 1, 2, 3, 4, 5, 6, 7, 7)]
    s["playerActions"] = {"2": {"name": "Beta", "actions": {
        "1": {"action": "[t=9|c=1] voted to eliminate Player 1", "phase": "First Day Voting", "id": "1"},
        "2": {"action": "[t=8|c=3] voted to eliminate Player 3", "phase": "First Day Voting", "id": "2"},   # the turn that entered
        "3": {"action": "hello", "phase": "First Day Voting", "id": "3"}}}}
    v, _ = agent_state_to_view(tb, s, visit_actions={3: 4})
    assert int(v["prev_phase_id"]) == 6 and int(v["phase0_done"]) == 1 and int(v["end_turn"]) == -1
    assert [(int(v["players"][i][9]), int(v["players"][i][10])) for i in range(4)] == [(0, 0), (1, 1), (1, 4), (0, 0)]
    s["current_phase_id"] = 99
    s["phase_history"] += [{"phase_id": 99}, {"phase_id": 99}]
    v, _ = agent_state_to_view(tb, s)
    assert int(v["end_turn"]) == 10 and int(v["prev_phase_id"]) == 7
    v, _ = agent_state_to_view(tb, dict(s, previous_phase_id=9, end_turn=11, games=3))
    assert (int(v["prev_phase_id"]), int(v["end_turn"]), int(v["games"])) == (9, 11, 3)
    with pytest.raises(ValueError, match="visit action"):
        agent_state_to_view(tb, s, visit_actions={2: 9})



def test_more_players_than_a_room_holds_is_refused():
    tb = GameTable(load_dsl("werewolf-(mafia)"))
    s = example_state("werewolf-(mafia)", 2)
    s["player_states"] = {str(i): copy.deepcopy(s["player_states"]["2"]) for i in range(1, 14)}
    with pytest.raises(ValueError, match="1..12"):
        agent_state_to_view(tb, s)


NODE_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "game_engine_amd", "node")


@pytest.mark.skipif(__import__("shutil").which("node") is None or not os.path.exists(os.path.join(NODE_DIR, "ge_addon.node")),
                    reason="node or the built addon is not available")
def test_node_agent_state_to_view_matches_python():
    """agentStateToView (node/index.js) gives byte-equal views on the players_example blocks and on every turn of the bot-only
    strings goldens, and refuses what Python refuses (TypeError for a wrong type, RangeError for a value that does not fit)."""
    import subprocess
    cases = []
    for game in GAMES:
        cases.append({"dsl": os.path.join(GOLD, "dsl", game + ".json"), "state": example_state(game, 0)})
    for name in STRINGS:
        g = load_golden(name)
        for case in g["cases"]:
            for k, state in golden_states(case):
                cases.append({"dsl": os.path.join(GOLD, "dsl", g["game"] + ".json"), "state": state})
    ww = os.path.join(GOLD, "dsl", "werewolf-(mafia).json")
    good = example_state("werewolf-(mafia)", 7)
    good["phase_history"] = [{"phase_id": p} for p in (0, 0, 1, 2, 3, 4, 5, 6, 7, 7)]
    cases.append({"dsl": ww, "state": good, "visitActions": {"3": 4}})
    refusals = [(_bad(example_state("werewolf-(mafia)", 2), "2", "role", "Seer"), "RangeError"),
                (_bad(example_state("werewolf-(mafia)", 2), "2", "team", "villager"), "RangeError"),
                ({**example_state("werewolf-(mafia)", 2), "player_states": {k: v for k, v in example_state("werewolf-(mafia)", 2)["player_states"].items() if k != "3"}}, "RangeError"),
                (_bad(example_state("werewolf-(mafia)", 2), "1", "selected_target_id", 5), "RangeError"),
                (_bad(example_state("werewolf-(mafia)", 2), "2", "investigated_alignments", {"1": "werewolves"}), "RangeError"),
                ({**example_state("werewolf-(mafia)", 2), "current_phase_id": 42}, "RangeError"),
                (_bad(example_state("werewolf-(mafia)", 2), "2", "is_alive", 1), "TypeError"),
                (_bad(example_state("werewolf-(mafia)", 2), "1", "selected_target_id", "2"), "TypeError")]
    draft = example_state("draft-werewolf-(mafia)", 2)
    draft["player_states"]["2"]["wolf_chat_enabled"] = True
    refusals.append((draft, "RangeError"))
    n_ok = len(cases)
    cases += [{"dsl": os.path.join(GOLD, "dsl", ("draft-werewolf-(mafia)" if s is draft else "werewolf-(mafia)") + ".json"), "state": s}
              for s, _ in refusals]
    out = subprocess.run(["node", os.path.join(NODE_DIR, "selftest_adopt.js"), "--views"], input=json.dumps(cases),
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    got = json.loads(out.stdout.strip().splitlines()[-1])
    assert len(got) == len(cases)
    tables = {}
    for c, res in zip(cases[:n_ok], got[:n_ok]):
        tb = tables.setdefault(c["dsl"], GameTable(json.load(open(c["dsl"], encoding="utf-8"))))
        view, _ = agent_state_to_view(tb, c["state"], visit_actions=c.get("visitActions") and {int(k): v for k, v in c["visitActions"].items()})
        assert isinstance(res, str) and bytes.fromhex(res) == view.tobytes(), (c["dsl"], res)
    for (state, kind), c, res in zip(refusals, cases[n_ok:], got[n_ok:]):
        tb = tables.setdefault(c["dsl"], GameTable(json.load(open(c["dsl"], encoding="utf-8"))))
        with pytest.raises(ValueError):
            agent_state_to_view(tb, state)
        assert isinstance(res, dict) and res["error"] == kind, (res, kind)

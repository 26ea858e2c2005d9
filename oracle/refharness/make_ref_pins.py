"""Generates the tests/golden/ref_*.json pins: what the reference's own functions and files give for the inputs the
CPU tests use, recorded once so that those tests run from a clean checkout without the reference.

Build container only (needs the reference checkout, see walker.REFERENCE_ROOT).  Run:
    python -m oracle.refharness.make_ref_pins
Every pin is checked against the reference while it is written (the asserts below); the tests then check the product
against the pins.  Outputs (data only):
  ref_dsl_sources.json             per DSL fixture: digests of the reference's YAML file and of its yaml.safe_load
  ref_initialize_player_states.json   utils.initialize_player_states_from_dsl on the games' YAML DSLs
  ref_human_action_logging.json    utils.process_human_action_if_needed on a list of browser messages
  ref_frontend_tools.json          the useCopilotAction parameter table extracted from src/app/page.tsx
  ref_toolcall_replay.json         per trajectory golden and turn: a digest of the tool calls that, applied with
                                   backend_tools' _execute_* functions, reproduced the golden projection of that turn
"""
from __future__ import annotations

import asyncio
import copy
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLD = os.path.join(ROOT, "tests", "golden")

DSL_FILES = {"werewolf-(mafia)": "games/werewolf-(mafia).yaml", "two-truths-and-a-lie": "games/two-truths-and-a-lie.yaml",
             "draft-werewolf-(mafia)": "game_draft/werewolf-(mafia).yaml"}
PLAYERS = [{"name": f"P{i}"} for i in range(5)] + [{}]
MESSAGES = ["Continue", " continue", "Start game.", "start game", "Player A in game chat: x", "Player A to Bot 2: y", "to bot",
            "TO BOT 2", "Input: " + "z" * 300, 'Player 4 voted "Bot 2" in voting vote-p7-t11', "", "In Game Chat: q", "hello",
            "CONTINUE"]
REPLAY_TRAJ = ["traj_werewolf_n8.json", "traj_werewolf_n12.json", "traj_werewolf_n5.json", "traj_two_truths_and_a_lie_n4.json",
               "traj_two_truths_and_a_lie_n6.json", "traj_draft_werewolf_n8.json", "traj_draft_werewolf_n12.json",
               "traj_variant_ww_minimal_schema_n8.json", "traj_variant_ww_generic_n8.json"]


def canonical_digest(obj) -> str:
    return hashlib.sha256(json.dumps(obj, sort_keys=True, ensure_ascii=False, separators=(",", ":")).encode("utf-8")).hexdigest()


def yaml_form(dsl: dict) -> dict:
    """A committed JSON DSL fixture back in the form yaml.safe_load gives the reference: integer keys where the YAML
    has them (the phase table and the numbered player_states of the declaration's template and example)."""
    d = copy.deepcopy(dsl)
    d["phases"] = {int(k): v for k, v in d["phases"].items()}
    for key in ("player_states_template", "players_example"):
        sub = d.get("declaration", {}).get(key)
        if isinstance(sub, dict) and isinstance(sub.get("player_states"), dict):
            sub["player_states"] = {int(k): v for k, v in sub["player_states"].items()}
    return d


def _write(name, doc, indent=1):
    with open(os.path.join(GOLD, name), "w", encoding="utf-8") as f:
        json.dump(doc, f, ensure_ascii=False, indent=indent, separators=None if indent else (",", ":"))
        f.write("\n")


def _reference_tools():
    from .walker import REFERENCE_ROOT, _STANDINS
    for p in (_STANDINS, os.path.join(REFERENCE_ROOT, "agent")):
        if p not in sys.path:
            sys.path.insert(0, p)
    sys.dont_write_bytecode = True
    import tools.backend_tools as bt
    import tools.utils as ut
    return bt, ut


def dsl_sources():
    import yaml
    from .walker import REFERENCE_ROOT
    out = {}
    for game, rel in DSL_FILES.items():
        with open(os.path.join(REFERENCE_ROOT, rel), "rb") as f:
            raw = f.read()
        doc = yaml.safe_load(raw.decode("utf-8"))
        with open(os.path.join(GOLD, "dsl", f"{game}.json"), encoding="utf-8") as f:
            fixture = json.load(f)
        assert json.loads(json.dumps(doc)) == fixture, game
        assert yaml_form(fixture) == doc, game
        out[game] = {"file": rel, "file_sha256": hashlib.sha256(raw).hexdigest(), "safe_load_sha256": canonical_digest(doc)}
    _write("ref_dsl_sources.json", {"source": "yaml.safe_load of the reference's game files; digest = sha256 of the "
                                              "sort_keys compact JSON", "games": out})


def initialize_player_states():
    from .walker import REFERENCE_ROOT
    import yaml
    _, ut = _reference_tools()
    out = {}
    for game in ("werewolf-(mafia)", "two-truths-and-a-lie"):
        with open(os.path.join(REFERENCE_ROOT, DSL_FILES[game]), encoding="utf-8") as f:
            dsl = yaml.safe_load(f)
        out[game] = asyncio.run(ut.initialize_player_states_from_dsl(dsl, PLAYERS))
    _write("ref_initialize_player_states.json", {"source": "tools.utils.initialize_player_states_from_dsl(yaml DSL, players)",
                                                 "players": PLAYERS, "player_states": out})


def human_action_logging():
    from .walker import load_reference
    load_reference("v2")
    from langchain_core.messages import HumanMessage
    from tools.utils import process_human_action_if_needed
    with open(os.path.join(GOLD, "dsl", "werewolf-(mafia).json"), encoding="utf-8") as f:
        dsl = json.load(f)
    room = {"players": [{"gamePlayerId": 1, "name": "Alice"}]}
    cases = [{"message": text, "logged": process_human_action_if_needed([HumanMessage(content=text)], {}, {}, 0, room, dsl)}
             for text in MESSAGES]
    _write("ref_human_action_logging.json", {"source": "tools.utils.process_human_action_if_needed([HumanMessage(message)], {}, "
                                                       "{}, 0, room_session, werewolf DSL), timestamps stripped",
                                             "room_session": room, "cases": _strip_ts(cases)})


def _strip_ts(o):
    if isinstance(o, dict):
        return {k: _strip_ts(v) for k, v in o.items() if k != "timestamp"}
    if isinstance(o, list):
        return [_strip_ts(v) for v in o]
    return o


def frontend_tools():
    import importlib.util
    from .walker import REFERENCE_ROOT
    spec = importlib.util.spec_from_file_location("extract_frontend_tools", os.path.join(ROOT, "tools", "extract_frontend_tools.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    with open(os.path.join(REFERENCE_ROOT, "src", "app", "page.tsx"), encoding="utf-8") as f:
        tools = ex.extract(f.read())
    _write("ref_frontend_tools.json", {"source": "tools/extract_frontend_tools.py over the reference's src/app/page.tsx",
                                       "tools": tools})


def toolcall_replay():
    """Replays the product's rendered calls of every turn through the reference's _execute_* plumbing, asserts the golden
    projection turn by turn, and records a digest of each turn's calls."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import golden_dsl, load_golden, restart_files
    from parity_util import calls_digest, rendered_turn_calls
    from game_engine_amd import GameTable
    from oracle.oracle import Oracle
    from .walker import project_state
    bt, ut = _reference_tools()
    out = {}
    for name, restart in [(n, False) for n in REPLAY_TRAJ] + [(n, True) for n in restart_files()]:
        g = load_golden(name)
        dsl = golden_dsl(g)
        dsl_ref = dict(dsl, phases={int(k): v for k, v in dsl["phases"].items()})
        n = g["n_players"]
        orc = Oracle(dsl, n, rounds=g["rounds"])
        table = GameTable(dsl, rounds=g["rounds"])
        terminal = {p.id for p in orc.table.phases if not p.branches}
        room_session = {"players": [{"name": f"Bot {i + 1}", "gamePlayerId": i + 1} for i in range(n)]}

        def fresh_state():
            ps = asyncio.run(ut.initialize_player_states_from_dsl(dsl_ref, room_session["players"]))
            return {"current_phase_id": 0, "player_states": ps, "playerActions": {}, "phase_history": [], "game_notes": []}

        cases = []
        for case in g["cases"]:
            state, t_enter, prev, end_turn = fresh_state(), -1, 0, -1
            digests = []
            for t, calls, restarted in rendered_turn_calls(orc, table, case, restart=restart):
                if restarted:                        # a new LangGraph thread on the recycled slot
                    state, t_enter, prev, end_turn = fresh_state(), t - 1, 0, -1
                p0 = state["current_phase_id"]
                for call in calls:
                    a = call["args"]
                    if call["name"] == "update_player_actions":
                        state["playerActions"] = bt._execute_update_player_actions(
                            state["playerActions"], a["player_id"], a["actions"], a["phase"], room_session, state["player_states"])
                    elif call["name"] == "update_player_state":
                        state["player_states"] = bt._execute_update_player_state(
                            state["player_states"], a["player_id"], a["state_name"], a["state_value"])
                    elif call["name"] == "add_game_note":
                        state["game_notes"] = bt._execute_add_game_note(state["game_notes"], a["note_type"], a["content"])
                    elif call["name"] == "set_next_phase":
                        assert a["next_phase_id"] in dsl_ref["phases"]          # v2:1173-1204 validation
                        if a["transition"]:
                            state["current_phase_id"] = a["next_phase_id"]
                        state["phase_history"].append({"phase_id": state["current_phase_id"]})   # v2:1207-1215
                q = state["current_phase_id"]
                if q != p0:
                    t_enter, prev = t, p0
                    if q in terminal and end_turn < 0:
                        end_turn = t
                got = project_state(orc.table, state, t_enter, prev, end_turn)
                assert got == case["turns"][t], f"{name} seed={case['seed']:#x} room={case['room']} turn={t}"
                digests.append(calls_digest(calls))
            cases.append({"seed": case["seed"], "room": case["room"], "calls_sha256_16": digests})
        out[("restart:" if restart else "") + name] = cases
        print("replayed", name, "restart" if restart else "", file=sys.stderr)
    _write("ref_toolcall_replay.json", {"source": "game_engine_amd.toolcalls.turn_tool_calls of oracle-stepped golden cases, each "
                                                  "turn's calls applied with the reference's backend_tools._execute_* and checked "
                                                  "against the golden projection; per turn the first 16 hex digits of sha256 of "
                                                  "the calls' compact JSON", "goldens": out}, indent=None)


if __name__ == "__main__":
    dsl_sources()
    initialize_player_states()
    human_action_logging()
    frontend_tools()
    toolcall_replay()

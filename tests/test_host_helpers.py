"""Host helpers that keep the reference's names and contracts (CPU)."""
import os

import pytest

from conftest import GOLD, load_dsl, load_golden
from game_engine_amd import initialize_player_states_from_dsl, load_dsl_by_gamename


def test_load_dsl_by_gamename_contract(tmp_path):
    assert load_dsl_by_gamename("", str(tmp_path)) == {}                       # utils.py:559-561
    assert load_dsl_by_gamename("nope", str(tmp_path)) == {}                   # utils.py:576-578
    d = load_dsl_by_gamename("werewolf-(mafia)", os.path.join(GOLD, "dsl"))    # the JSON form of the same document
    assert set(d) == {"declaration", "phases"} and len(d["phases"]) == 18
    (tmp_path / "mini.yaml").write_text("declaration: {min_players: 2}\nphases:\n  0: {name: Intro}\n")
    y = load_dsl_by_gamename("mini", str(tmp_path))
    assert y["phases"][0]["name"] == "Intro"                                   # YAML int keys, as in the reference


def test_initialize_player_states(dsl_ww, dsl_tt):
    players = [{"name": "Alice"}, {"name": "Bob"}, {}]
    ps = initialize_player_states_from_dsl(dsl_ww, players)
    assert list(ps) == ["1", "2", "3"] and ps["1"]["name"] == "Alice" and ps["3"]["name"] == "Player 3"
    assert ps["2"]["is_alive"] is True and ps["2"]["selected_target_id"] == 0 and ps["2"]["investigated_alignments"] == {}
    assert initialize_player_states_from_dsl({}, players) == {}
    no_tmpl = {"declaration": {"player_states": {"score": {"type": "num"}, "ok": {"type": "boolean"}, "tag": {"type": "string", "example": "x"}}}}
    assert initialize_player_states_from_dsl(no_tmpl, [{"name": "Z"}]) == {"1": {"score": 0, "ok": True, "tag": "x", "name": "Z"}}


@pytest.mark.parametrize("game", ["werewolf-(mafia)", "two-truths-and-a-lie"])
def test_initialize_player_states_equals_reference(game):
    """Against what utils.py's own initialize_player_states_from_dsl returned for the game's YAML DSL
    (tests/golden/ref_initialize_player_states.json, oracle/refharness/make_ref_pins.py)."""
    from oracle.refharness.make_ref_pins import yaml_form
    pins = load_golden("ref_initialize_player_states.json")
    players, want = pins["players"], pins["player_states"][game]
    assert players == [{"name": f"P{i}"} for i in range(5)] + [{}]
    dsl_yaml = yaml_form(load_dsl(game))                                             # what yaml.safe_load gives (pinned in test_table.py)
    assert initialize_player_states_from_dsl(dsl_yaml, players) == want            # YAML (int keys) form
    assert initialize_player_states_from_dsl(load_dsl(game), players) == want      # JSON (str keys) form

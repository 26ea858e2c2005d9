"""advise(compare=True) through RoomService and RoomPoolService (-m gpu): the strings_human_* reference runs replayed message by
message; wherever the human seat has an action due, in both views, the advice with "versus" / "compare" removed equals advise()
byte for byte, "versus" equals the oracle reference (compare_ref) of the option against the policy's entry, and service and pool
agree; the pool makes one rollout_compare call per chunk touched and no other playout call; the Node twins print the same JSON."""
import copy
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from compare_ref import reference_compare
from conftest import ROOT, load_dsl, load_golden
from game_engine_amd import GameTable, RoomBatch, RoomPoolService, RoomService
from game_engine_amd.room_service import FORECAST_SEED_XOR, advise_candidates
from oracle.oracle import Oracle
from parity_util import views_as_oracle_rooms
from test_gpu_advise import _due

pytestmark = pytest.mark.gpu

R, MT = 128, 300
KEYS = ("compared", "better", "worse", "gain", "loss", "diffSq")


def _dumps(x):
    return json.dumps(x, separators=(",", ":"), ensure_ascii=False)


def _stripped(advice):
    out = copy.deepcopy(advice)
    assert out.pop("compare") is True
    for o in out["options"]:
        assert list(o["versus"]) == list(KEYS)
        del o["versus"]
    return out


def _reference_versus(orc, tb, case, view, turn, seat, seat_view):
    key = (case["room"] << 16) & (2 ** 64 - 1)
    seed = case["seed"] ^ FORECAST_SEED_XOR
    cands = advise_candidates(tb, view)
    acts = [[(seat, c)] for c in cands] + [[]]
    k = len(acts)
    rec = views_as_oracle_rooms(orc, np.asarray(view).reshape(1))[0]
    _, st, cmp = reference_compare(lambda r: (orc, rec), [0] * k, [key] * k, [turn] * k, [seat if seat_view else 0] * k, acts,
                                   [k - 1] * k, [seat] * k, R, MT, seed)
    return {c: dict(zip(KEYS, (int(x) for x in cmp[j]))) for j, c in enumerate(cands) if st[j] == 0}


@pytest.mark.parametrize("name", ["strings_human_werewolf_n8.json", "strings_human_two_truths_and_a_lie_n4.json"])
def test_compare_adds_versus_and_changes_nothing_else(name):
    g = load_golden(name)
    case = g["cases"][0]
    dsl = load_dsl(g["game"])
    orc, tb = Oracle(dsl, g["n_players"]), GameTable(dsl)
    players = [{"name": nm, "gamePlayerId": i + 1, "isBot": (i + 1) not in case["human_seats"]} for i, nm in enumerate(case["names"])]
    seat = min(case["human_seats"])
    seen = {}
    for pool in (False, True):
        svc = RoomPoolService(seed=case["seed"], chunk_rooms=8) if pool else RoomService(seed=case["seed"])
        svc.create_room("t", g["game"], players, dsl=dsl, room_index=case["room"])
        lines, better, worse = [], 0, 0
        for k, want in enumerate(case["messages"]):
            room = svc._rooms["t"]
            view = room["view"]
            if _due(orc, view, seat, tb):
                turn = room["turn"] if pool else room["batch"].turn
                for v in ("full", "seat"):
                    got = svc.advise("t", n_rollouts=R, max_turns=MT, view=v, compare=True)
                    plain = svc.advise("t", n_rollouts=R, max_turns=MT, view=v)
                    assert _dumps(_stripped(got)) == _dumps(plain), (name, k, v)
                    ref = _reference_versus(orc, tb, case, view, turn, seat, v == "seat")
                    assert {o["choice"]: o["versus"] for o in got["options"]} == ref, (name, k, v)
                    better += sum(x["better"] for x in ref.values())
                    worse += sum(x["worse"] for x in ref.values())
                    lines.append(_dumps(got))
            svc.handle_message("t", want["message"])
        svc.close()
        assert lines and better > 0 and worse > 0                          # on the reference's numbers: the ground is not empty
        seen[pool] = lines
    assert seen[False] == seen[True]


def test_pool_makes_one_compare_call_per_chunk(monkeypatch):
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
    calls = []
    for method in ("rollout_compare", "rollout_seats", "rollout_actions", "rollout_rooms"):
        orig = getattr(RoomBatch, method)
        monkeypatch.setattr(RoomBatch, method, (lambda o, m: lambda self, *a, **kw: (calls.append((m, id(self), len(a[0]))), o(self, *a, **kw))[1])(orig, method))
    for view in ("full", "seat"):
        calls.clear()
        got = pool.advises(tids[::-1], n_rollouts=300, max_turns=500, view=view, compare=True)
        chunks = {id(pool._rooms[t]["chunk"]) for t in tids}
        assert [m for m, _, _ in calls] == ["rollout_compare"] * len(chunks) == ["rollout_compare"] * 3
        assert {c for _, c, _ in calls} == chunks and sum(n for _, _, n in calls) == 9 * len(tids)
        calls.clear()
        want = [ref.advise(t, n_rollouts=300, max_turns=500, view=view, compare=True) for t in tids[::-1]]
        assert [m for m, _, _ in calls] == ["rollout_compare"] * len(tids)
        assert got == want and any(o["options"] for o in got)
        calls.clear()                                                      # without compare: the calls made today
        pool.advises(tids, n_rollouts=64, max_turns=50, view=view)
        assert [m for m, _, _ in calls] == ["rollout_seats" if view == "seat" else "rollout_actions"] * 3
    pool.close()
    ref.close()


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not available")
@pytest.mark.parametrize("name", ["strings_human_werewolf_n8.json", "strings_human_two_truths_and_a_lie_n4.json"])
def test_node_compare_prints_the_same_json(tmp_path, name):
    g = load_golden(name)
    case = g["cases"][0]
    script = {"game": g["game"], "dsl": os.path.join(ROOT, "tests", "golden", "dsl", f"{g['game']}.json"), "seed": case["seed"],
              "room": case["room"], "names": case["names"], "humans": case["human_seats"],
              "messages": [m["message"] for m in case["messages"][:14]], "rollouts": R, "maxTurns": MT}
    sp = tmp_path / "script.json"
    sp.write_text(json.dumps(script))
    p = subprocess.run(["node", os.path.join(ROOT, "game_engine_amd", "node", "selftest_compare.js"), str(sp)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    node_lines = p.stdout.strip().splitlines()
    py_lines = []
    for svc in (RoomService(seed=case["seed"]), RoomPoolService(seed=case["seed"], chunk_rooms=8)):
        players = [{"name": nm, "gamePlayerId": i + 1, "isBot": (i + 1) not in case["human_seats"]} for i, nm in enumerate(case["names"])]
        svc.create_room("t", g["game"], players, dsl=load_dsl(g["game"]), room_index=case["room"])
        for text in script["messages"]:
            for view in ("full", "seat"):
                py_lines.append(_dumps(svc.advise("t", n_rollouts=R, max_turns=MT, view=view, compare=True)))
            svc.handle_message("t", text)
        svc.close()
    assert node_lines == py_lines and any('"versus":{"compared":128' in x for x in py_lines)

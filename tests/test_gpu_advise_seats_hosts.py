"""ge_batch_advise_seats through the hosts (-m gpu): the Python and the Node binding give the same words for the same calls
(node/selftest_advise_seats.js), and RoomService.hint / RoomPoolService.hints give, in both hosts, the advised seat's own numbers
inside advise's option forecasts for the same thread - from the seat's view and from the full view."""
import json
import os
import shutil
import subprocess

import pytest

from conftest import load_dsl
from game_engine_amd import GameTable, RoomBatch, RoomPoolService, RoomService
from test_advise_host import _assert_hint_is_advise, _players

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE_DIR = os.path.join(ROOT, "game_engine_amd", "node")
STEPS = 9
R, M = 70, 48
SERVICE = {"seed": 0x5EED, "rollouts": 100, "maxTurns": 200,
           "threads": [{"id": "w", "game": "werewolf-(mafia)", "dsl": "ww", "n": 8, "humans": [2], "other": 6},
                       {"id": "t", "game": "two-truths-and-a-lie", "dsl": "tt", "n": 4, "humans": [1], "other": 3}]}
POOL = {"seed": 0xBEE, "chunkRooms": 2, "rollouts": 70, "maxTurns": 100,
        "threads": [{"id": "a", "game": "werewolf-(mafia)", "dsl": "ww", "n": 8, "humans": [2, 5]},
                    {"id": "b", "game": "werewolf-(mafia)", "dsl": "ww", "n": 8, "humans": [2, 5]},
                    {"id": "c", "game": "werewolf-(mafia)", "dsl": "ww", "n": 8, "humans": [2, 5]},
                    {"id": "x", "game": "two-truths-and-a-lie", "dsl": "tt", "n": 4, "humans": [1]},
                    {"id": "y", "game": "two-truths-and-a-lie", "dsl": "tt", "n": 4, "humans": [1]}]}


def _calls():
    rooms = [r for r in range(64) for _ in range(8 if r < 40 else 4)]
    seats = [s for r in range(64) for s in range(1, (8 if r < 40 else 4) + 1)]
    keys = [(k * 0x9E3779B97F4A7C15 + (k % 2 << 63)) % (1 << 64) for k in range(len(rooms))]
    turns = [STEPS + k % 5 for k in range(len(rooms))]
    base = {"rooms": rooms, "keys": [str(k) for k in keys], "turns": turns, "seats": seats}
    return [dict(base, nRollouts=R, maxTurns=M, seed="12345678901234567890", fullView=False),
            dict(base, nRollouts=1, maxTurns=8, seed=None, fullView=True)]


def _as_node(adv):
    """An ADVICE_DTYPE array as index.js decodes it."""
    out = []
    for a in adv:
        cs = [c for c in range(1, 13) if (int(a["legal"]) >> (c - 1)) & 1]
        opt = lambda o: {"finished": int(o["finished"]), "wins": int(o["wins"]), "score": int(o["score"])}
        out.append({"status": int(a["status"]), "legal": cs, "best": int(a["best"]), "phaseId": int(a["phase_id"]), "policy": opt(a["policy"]),
                    "options": [dict(choice=c, **opt(a["option"][c - 1])) for c in cs]})
    return out


def _python_calls(ww, tt):
    with RoomBatch([(GameTable(ww), 8, 40, 0b1), (GameTable(tt), 4, 24, 0b10)], seed=11, first_room=5) as b:
        b.step(STEPS)
        return [_as_node(b.advise_seats(c["rooms"], [int(k) for k in c["keys"]], c["turns"], c["seats"], c["nRollouts"], c["maxTurns"],
                                        seed=None if c["seed"] is None else int(c["seed"]), full_view=c["fullView"])) for c in _calls()]


def _python_service(dsl):
    s = SERVICE
    svc = RoomService(seed=s["seed"])
    res = []
    for t in s["threads"]:
        svc.create_room(t["id"], t["game"], _players(t["n"], humans=t["humans"]), dsl=dsl[t["dsl"]])
        svc.run_room(t["id"], 64, ("person", "end"))
        res.append({"seat": svc.hint(t["id"], None, s["rollouts"], s["maxTurns"]),
                    "full": svc.hint(t["id"], t["humans"][0], s["rollouts"], s["maxTurns"], "full"),
                    "other": svc.hint(t["id"], t["other"], s["rollouts"], s["maxTurns"]),
                    "adviseSeat": svc.advise(t["id"], None, s["rollouts"], s["maxTurns"], "seat"),
                    "adviseFull": svc.advise(t["id"], None, s["rollouts"], s["maxTurns"])})
        svc.close(t["id"])
    return res


def _python_pool(dsl):
    p = POOL
    pool = RoomPoolService(seed=p["seed"], chunk_rooms=p["chunkRooms"])
    ids = [t["id"] for t in p["threads"]]
    for t in p["threads"]:
        pool.create_room(t["id"], t["game"], _players(t["n"], humans=t["humans"]), dsl=dsl[t["dsl"]])
    pool.run_rooms(ids, 64, ("person", "end"))
    out = {"waiting": pool.waiting(), "all": pool.hints(None, None, p["rollouts"], p["maxTurns"]),
           "listed": pool.hints(ids, None, p["rollouts"], p["maxTurns"], "full"), "one": pool.hints([ids[0]], [5], p["rollouts"], p["maxTurns"])[0],
           "advises": pool.advises(ids, None, p["rollouts"], p["maxTurns"], "seat")}
    full = pool.advises(ids, None, p["rollouts"], p["maxTurns"])
    pool.close()
    return out, full


def test_hint_numbers_are_those_inside_advise_in_both_views():
    dsl = {"ww": load_dsl("werewolf-(mafia)"), "tt": load_dsl("two-truths-and-a-lie")}
    seen = 0
    for t, r in zip(SERVICE["threads"], _python_service(dsl)):
        ww = t["dsl"] == "ww"
        assert r["seat"]["view"] == "seat" and "view" not in r["full"], t["id"]
        seen += len(r["seat"]["options"])
        _assert_hint_is_advise(r["seat"], r["adviseSeat"], ww)
        _assert_hint_is_advise(r["full"], r["adviseFull"], ww)
        assert r["other"]["playerId"] == t["other"]
    out, full = _python_pool(dsl)
    ids = [t["id"] for t in POOL["threads"]]
    assert seen >= 3 and len(out["waiting"]) >= 3                  # (a thread whose person died in the first night may have run to its end)
    assert [(h["threadId"], h["playerId"]) for h in out["all"]] == [(t, s) for t in ids if t in out["waiting"] for s in out["waiting"][t]]
    lowest = {a["threadId"]: a for a in out["advises"]}
    for h in out["all"]:
        assert h["options"], h
        if h["playerId"] == lowest[h["threadId"]]["playerId"]:
            _assert_hint_is_advise(h, lowest[h["threadId"]], h["threadId"] in "abc")
    for h, a in zip(out["listed"], full):
        _assert_hint_is_advise(h, a, h["threadId"] in "abc")
    assert [h for h in out["all"] if (h["threadId"], h["playerId"]) == ("a", out["one"]["playerId"])] in ([], [out["one"]])


@pytest.mark.skipif(shutil.which("node") is None or not os.path.exists(os.path.join(NODE_DIR, "ge_addon.node")),
                    reason="node or the built addon is not available")
def test_node_gives_the_same_words_and_the_same_hints(tmp_path):
    dsl = {"ww": load_dsl("werewolf-(mafia)"), "tt": load_dsl("two-truths-and-a-lie")}
    want_calls = _python_calls(dsl["ww"], dsl["tt"])
    assert any(a["options"] for a in want_calls[0]) and any(a["status"] for a in want_calls[0])
    spec = tmp_path / "spec.json"
    spec.write_text(json.dumps({"ww": dsl["ww"], "tt": dsl["tt"], "steps": STEPS, "calls": _calls(), "service": SERVICE, "pool": POOL}))
    p = subprocess.run(["node", os.path.join(NODE_DIR, "selftest_advise_seats.js"), str(spec)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert got["calls"] == want_calls
    assert got["service"] == json.loads(json.dumps(_python_service(dsl)))
    assert got["pool"] == json.loads(json.dumps(_python_pool(dsl)[0]))

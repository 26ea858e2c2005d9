"""run_room(playout=True) / run_rooms(playout=True) of the Python services on the GPU (-m gpu): threads with playout bots played on
by one run_rooms_playout call per thread or chunk, equal to a twin service's continue_room loop - every turn's output, the final
state and the next message's output - with a human seat's answers in between; without the option the refusal stands; and the
Node twins (node/selftest_run_playout.js) against the Python pool."""
import copy
import json
import os
import shutil
import subprocess

import pytest

from conftest import GOLD, ROOT, load_dsl
from game_engine_amd import RoomPoolService, RoomService
from test_gpu_run_service import GAMES, _answer, _players, _shared
from test_strings_golden import _strip

pytestmark = pytest.mark.gpu

OPTS = dict(playout_rollouts=16, playout_max_turns=24)


@pytest.mark.parametrize("game,n,humans,bots", [("werewolf-(mafia)", 8, (1,), (2, 5)), ("werewolf-(mafia)", 12, (3,), (1, 7, 12)),
                                                ("two-truths-and-a-lie", 4, (2,), (1, 4))])
def test_run_room_with_playout_equals_a_twin_services_continue_loop(game, n, humans, bots):
    dsl = load_dsl(game)
    items = [{"id": "x1", "type": "text"}]
    one, pool, twin = RoomService(seed=5, **OPTS), RoomPoolService(seed=5, chunk_rooms=4, **OPTS), RoomService(seed=5, **OPTS)
    threads = ["a", "b", "c", "d", "e", "f"]                    # the pool spreads them over two chunks; every other thread has bots
    try:
        for s in (one, pool, twin):
            for j, t in enumerate(threads):
                s.create_room(t, game, _players(n, humans), dsl=dsl, playout_seats=bots if j % 2 == 0 else ())
        with pytest.raises(ValueError, match="playout=True"):
            one.run_room("a")
        with pytest.raises(ValueError, match="playout=True"):
            pool.run_rooms(threads)
        decided_late = 0
        for until, max_turns in ((("person", "end"), 64), ((), 3), (("phase",), 9), (("person", "end"), 64)):
            got_pool = pool.run_rooms(threads, max_turns, until, [items] * len(threads), playout=True)
            for j, t in enumerate(threads):
                got = one.run_room(t, max_turns, until, items, playout=True)
                want = [copy.deepcopy(twin.continue_room(t, items)) for _ in range(got["played"])]   # as its caller sees each then
                for o in (got, got_pool[j]):
                    assert o["played"] == len(want) and _strip(o["turns"]) == _strip(want), (game, until, t)
                    assert o["stopped"] == got["stopped"] and set(o["stopped"]) <= set(until)
                assert got["stopped"] or got["played"] == max_turns
                decided_late += got["played"] > 1
                if "person" in got["stopped"]:                  # the person answers: the same seat and choice in all three
                    answers = {_answer(s, t, humans, n) for s in (one, pool, twin)}
                    assert len(answers) == 1 and None not in answers, (game, t, answers)
                nxt = _strip(twin.handle_message(t, "Continue", items))
                assert _strip(one.handle_message(t, "Continue", items)) == nxt and _strip(pool.handle_message(t, "Continue", items)) == nxt
        assert decided_late
    finally:
        for s in (one, pool, twin):
            s.close()


# ---- the Node twins: one script through node/selftest_run_playout.js and through the Python pool
def _script():
    ops = [["create", "w1", GAMES[0], _players(8, (1,)), [3, 6]], ["create", "w2", GAMES[0], _players(8)],
           ["create", "w3", GAMES[0], _players(12, (3, 12)), [1, 7]], ["create", "t1", GAMES[1], _players(4, (2,)), [1, 4]],
           ["create", "t2", GAMES[1], _players(5), [5]], ["create", "w4", GAMES[0], _players(8), [1, 2, 3, 4, 5, 6, 7, 8]]]
    threads = ["w1", "t1", "w2", "w3", "t2", "w4"]
    items = [{"id": "x1", "type": "text"}]
    for until, max_turns in ((["person", "end"], 64), ([], 3), (["phase"], 9), (["person", "end"], 64), (["person", "end", "phase"], 1),
                             (["person", "end"], 40)):
        ops.append(["run", threads, max_turns, until, items])
        ops += [["answer", t] for t in ("w1", "w3", "t1")]
        ops += [["message", t, "Continue"] for t in ("w1", "t2")]
    ops.append(["refused", "w1"])
    return ops


def _run_python(ops, seed, chunk_rooms):
    pool = RoomPoolService(seed=seed, chunk_rooms=chunk_rooms, **OPTS)
    info, outputs = {}, []
    try:
        for op in ops:
            if op[0] == "create":
                players = op[3]
                pool.create_room(op[1], op[2], players, dsl=load_dsl(op[2]), playout_seats=tuple(op[4]) if len(op) > 4 else ())
                info[op[1]] = (len(players), [i + 1 for i, p in enumerate(players) if p["isBot"] is False])
                outputs.append(None)
            elif op[0] == "run":
                outputs.append(_strip(pool.run_rooms(op[1], op[2], tuple(op[3]), [op[4]] * len(op[1]), playout=True)))
            elif op[0] == "answer":
                a = _answer(pool, op[1], info[op[1]][1], info[op[1]][0])
                outputs.append(None if a is None else list(a))
            elif op[0] == "message":
                outputs.append(_strip(pool.handle_message(op[1], op[2])))
            else:
                outputs.append(None)
    finally:
        pool.close()
    return outputs


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not available")
def test_node_run_room_with_playout_gives_the_same_outputs(tmp_path):
    ops = _script()
    script = {"seed": 5, "chunkRooms": 2, "ops": ops, "plain": "w2", "playoutRollouts": OPTS["playout_rollouts"],
              "playoutMaxTurns": OPTS["playout_max_turns"], "dsls": {g: os.path.join(GOLD, "dsl", g + ".json") for g in GAMES}}
    sp, op = tmp_path / "script.json", tmp_path / "out.json"
    sp.write_text(json.dumps(script))
    out = subprocess.run(["node", os.path.join(ROOT, "game_engine_amd", "node", "selftest_run_playout.js"), str(sp), str(op)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["ok"] is True and r["turns"] > 100
    node_out = json.loads(op.read_text())
    py_out = json.loads(json.dumps(_run_python(ops, seed=5, chunk_rooms=2)))
    assert len(node_out) == len(py_out) == len(ops)
    answered = 0
    for k, (a, b) in enumerate(zip(node_out, py_out)):
        for x, y in zip(a if ops[k][0] == "run" else [a], b if ops[k][0] == "run" else [b]):
            assert _shared(x) == _shared(y), f"op {k} ({ops[k][0]}): the Node pool and the Python pool differ"
        answered += ops[k][0] == "answer" and a is not None
    assert answered > 0

"""run_room(forecast=True) of the services on the GPU (-m gpu; POLICY.md §3i): element 0 of "forecasts" is forecast() before the
run and the last element forecast() after it, on a real N = 1 RoomService and on a RoomPoolService with 3 threads in one chunk,
for Werewolf and Two-Truths; without the option the output is a twin's plain run_room; and the Node twins
(node/selftest_timeline.js) give the Python pool's JSON."""
import json
import os
import shutil
import subprocess

import pytest

from conftest import GOLD, ROOT, load_dsl
from game_engine_amd import RoomPoolService, RoomService
from test_strings_golden import _strip

pytestmark = pytest.mark.gpu

GAMES = ("werewolf-(mafia)", "two-truths-and-a-lie")
R, M = 96, 64
RUNS = ((("person", "end"), 40), ((), 3), (("end",), 64))


def _players(n, humans=()):
    return [{"name": f"P{i + 1}", "gamePlayerId": i + 1, "isBot": (i + 1) not in humans} for i in range(n)]


@pytest.mark.parametrize("game,n,humans,seat", [(GAMES[0], 8, (1,), 4), (GAMES[0], 8, (), None), (GAMES[1], 4, (2,), 1), (GAMES[1], 4, (), None)])
def test_run_room_forecasts_on_a_room_service(game, n, humans, seat):
    dsl = load_dsl(game)
    one, twin = RoomService(seed=5), RoomService(seed=5)
    try:
        for s in (one, twin):
            s.create_room("a", game, _players(n, humans), dsl=dsl)
        for until, max_turns in RUNS:
            before = one.forecast("a", R, M, seat)
            out = one.run_room("a", max_turns, until, forecast=True, forecast_rollouts=R, forecast_max_turns=M, forecast_seat=seat)
            plain = twin.run_room("a", max_turns, until)
            f = out["forecasts"]
            assert len(f) == out["played"] + 1 and f[0] == before and f[-1] == one.forecast("a", R, M, seat), (game, until)
            assert [x["turn"] for x in f] == [before["turn"] + p for p in range(len(f))] and all(x["rollouts"] == R for x in f)
            assert "forecasts" not in plain and _strip({k: out[k] for k in plain}) == _strip(plain)
            assert json.loads(json.dumps(f)) == f
    finally:
        one.close()
        twin.close()


@pytest.mark.parametrize("game,n,humans", [(GAMES[0], 8, (1,)), (GAMES[1], 4, (2,))])
def test_run_rooms_forecasts_on_a_pool_of_three_threads_in_one_chunk(game, n, humans):
    dsl = load_dsl(game)
    pool, twin = RoomPoolService(seed=5, chunk_rooms=4), RoomPoolService(seed=5, chunk_rooms=4)
    threads, seats = ["a", "b", "c"], [None, 3, 2 if n > 4 else 4]
    try:
        for s in (pool, twin):
            for t in threads:
                s.create_room(t, game, _players(n, humans), dsl=dsl)
            s.continue_room("b")                                 # the threads stand at different turns
        for until, max_turns in RUNS:
            before = pool.forecasts(threads, R, M, seats)
            outs = pool.run_rooms(threads, max_turns, until, forecast=True, forecast_rollouts=R, forecast_max_turns=M, forecast_seats=seats)
            plain = twin.run_rooms(threads, max_turns, until)
            after = pool.forecasts(threads, R, M, seats)
            for j, o in enumerate(outs):
                assert len(o["forecasts"]) == o["played"] + 1 and o["forecasts"][0] == before[j] and o["forecasts"][-1] == after[j], (game, until, j)
                assert _strip({k: o[k] for k in plain[j]}) == _strip(plain[j]) and "forecasts" not in plain[j]
            one = pool.run_room("a", 2, (), forecast=True, forecast_rollouts=R, forecast_max_turns=M)
            twin.run_room("a", 2, ())
            assert one["forecasts"][0] == after[0] and len(one["forecasts"]) == 3
    finally:
        pool.close()
        twin.close()


# ---- the Node twins: one script through node/selftest_timeline.js and through the Python pool
def _script():
    ops = [["create", "w1", GAMES[0], _players(8, (1,))], ["create", "w2", GAMES[0], _players(8)], ["create", "t1", GAMES[1], _players(4, (2,))],
           ["create", "p1", GAMES[0], _players(8, (1,)), [3]]]
    threads, seats = ["w1", "t1", "w2"], [5, 1, None]
    for until, max_turns in ((["person", "end"], 40), ([], 3), (["end"], 64)):
        ops.append(["run", threads, max_turns, until, R, M, seats])
        ops.append(["plain", threads, 1, []])
    ops.append(["refused", "w2", "p1"])
    return ops


def _run_python(ops, seed, chunk_rooms):
    pool = RoomPoolService(seed=seed, chunk_rooms=chunk_rooms, playout_rollouts=8, playout_max_turns=16)
    outputs = []
    try:
        for op in ops:
            if op[0] == "create":
                pool.create_room(op[1], op[2], op[3], dsl=load_dsl(op[2]), playout_seats=tuple(op[4]) if len(op) > 4 else ())
                outputs.append(None)
            elif op[0] == "run":
                got = pool.run_rooms(op[1], op[2], tuple(op[3]), forecast=True, forecast_rollouts=op[4], forecast_max_turns=op[5], forecast_seats=op[6])
                outputs.append([{"played": o["played"], "stopped": o["stopped"], "forecasts": o["forecasts"]} for o in got])
            elif op[0] == "plain":
                pool.run_rooms(op[1], op[2], tuple(op[3]))
                outputs.append(None)
            else:
                outputs.append(None)
    finally:
        pool.close()
    return outputs


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not available")
def test_node_run_room_forecasts_are_the_python_json(tmp_path):
    ops = _script()
    script = {"seed": 5, "chunkRooms": 4, "ops": ops, "dsls": {g: os.path.join(GOLD, "dsl", g + ".json") for g in GAMES}}
    sp, op = tmp_path / "script.json", tmp_path / "out.json"
    sp.write_text(json.dumps(script))
    out = subprocess.run(["node", os.path.join(ROOT, "game_engine_amd", "node", "selftest_timeline.js"), str(sp), str(op)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["ok"] is True and r["points"] > 12
    node_text = op.read_text()
    py_out = _run_python(ops, seed=5, chunk_rooms=4)
    assert node_text == json.dumps(py_out, separators=(",", ":")), "the Node pool's forecasts are not the Python pool's JSON"

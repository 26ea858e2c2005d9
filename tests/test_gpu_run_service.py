"""run_room / run_rooms of the services on the GPU (-m gpu): equal to a twin service's continue_room loop - every turn's output,
the final state and the next message's output -, a person-message golden replayed with every run of "Continue" messages collapsed
into one run_room, the refusal of threads with playout seats, and the Node twins (node/selftest_run.js) against the Python pool."""
import copy
import json
import os
import shutil
import subprocess

import pytest

from conftest import GOLD, ROOT, load_dsl, load_golden
from game_engine_amd import GeError, RoomPoolService, RoomService
from test_messages import _check_turn
from test_strings_golden import _strip

pytestmark = pytest.mark.gpu

FILES = sorted(f for f in os.listdir(GOLD) if f.startswith("strings_human_"))


def _players(n, humans=()):
    return [{"name": f"P{i + 1}", "gamePlayerId": i + 1, "isBot": (i + 1) not in humans} for i in range(n)]


def _answer(svc, thread_id, seats, n):
    """The first (human seat, choice) the thread accepts, seats and choices ascending; only the services' refusal (GeError,
    GE_ERR_ARG) counts as "not this one"."""
    for seat in seats:
        for c in range(1, max(n, 3) + 1):
            try:
                svc.human_action(thread_id, seat, c)
                return seat, c
            except GeError as e:
                if e.status != -1:
                    raise
    return None


@pytest.mark.parametrize("game,n,humans", [("werewolf-(mafia)", 8, (1,)), ("werewolf-(mafia)", 12, (3, 12)), ("two-truths-and-a-lie", 4, (2,)),
                                           ("draft-werewolf-(mafia)", 8, ())])
def test_run_room_equals_a_twin_services_continue_loop(game, n, humans):
    dsl = load_dsl(game)
    items = [{"id": "x1", "type": "text"}]
    one, pool, twin = RoomService(seed=5), RoomPoolService(seed=5, chunk_rooms=4), RoomService(seed=5)
    threads = ["a", "b", "c", "d", "e", "f"]                    # the pool spreads them over two chunks
    try:
        for s in (one, pool, twin):
            for t in threads:
                s.create_room(t, game, _players(n, humans), dsl=dsl)
        for until, max_turns in ((("person", "end"), 64), ((), 3), (("phase",), 9), (("person", "end"), 64), (("end",), 120)):
            got_pool = pool.run_rooms(threads, max_turns, until, [items] * len(threads))
            for j, t in enumerate(threads):
                got = one.run_room(t, max_turns, until, items)
                want = [copy.deepcopy(twin.continue_room(t, items)) for _ in range(got["played"])]   # as its caller sees each then
                for o in (got, got_pool[j]):
                    assert o["played"] == len(want) and _strip(o["turns"]) == _strip(want), (game, until, t)
                    assert o["stopped"] == got["stopped"] and set(o["stopped"]) <= set(until)
                assert got["stopped"] or got["played"] == max_turns
                if "person" in got["stopped"]:                  # the person answers: the same seat and choice in all three
                    answers = {_answer(s, t, humans, n) for s in (one, pool, twin)}
                    assert len(answers) == 1 and None not in answers, (game, t, answers)
                nxt = _strip(twin.handle_message(t, "Continue", items))
                assert _strip(one.handle_message(t, "Continue", items)) == nxt and _strip(pool.handle_message(t, "Continue", items)) == nxt
        # the last run named END alone: it stopped there exactly if the thread's phase is now terminal (an all-bot thread always
        # gets there; one that waits for a host-driven seat makes no progress on its own and hits the limit)
        terminal = {r["phase_id"] for r in one.table(game).rows() if not r["branches"]}
        for t in threads:
            last = one.run_room(t, 1, ("end",))
            assert (last["stopped"] == ["end"]) == (last["turns"][-1]["state"]["current_phase_id"] in terminal)
        if not humans:
            assert got["stopped"] == ["end"]
    finally:
        for s in (one, pool, twin):
            s.close()


@pytest.mark.parametrize("pooled", [False, True])
@pytest.mark.parametrize("name", FILES)
def test_golden_with_continue_runs_collapsed_gives_the_same_log(name, pooled):
    g = load_golden(name)
    for case in g["cases"]:
        svc = RoomPoolService(seed=case["seed"], chunk_rooms=2) if pooled else RoomService(seed=case["seed"])
        try:
            players = [{"name": nm, "gamePlayerId": i + 1, "isBot": (i + 1) not in case["human_seats"]} for i, nm in enumerate(case["names"])]
            svc.create_room("t", g["game"], players, dsl=load_dsl(g["game"]), room_index=case["room"])
            msgs, sizes, state, k, runs = case["messages"], (0, 0, 0), None, 0, 0
            while k < len(msgs):
                end = k
                while end < len(msgs) and msgs[end]["message"] == "Continue" and msgs[end]["played"]:
                    end += 1
                if end > k:                                     # a run of "Continue": one run_room of that length
                    out = svc.run_room("t", max_turns=end - k, until=())
                    assert out["played"] == end - k and out["stopped"] == []
                    for j, turn in enumerate(out["turns"]):
                        sizes = _check_turn(turn["state"], sizes, msgs[k + j], f"{name} message {k + j} (in a run)")
                    state, k, runs = out["turns"][-1]["state"], end, runs + 1
                    continue
                out = svc.handle_message("t", msgs[k]["message"])
                assert out["played"] == msgs[k]["played"]
                sizes = _check_turn(out["state"], sizes, msgs[k], f"{name} message {k}")
                state, k = out["state"], k + 1
            final = case["final"]
            assert _strip(state["playerActions"]) == final["playerActions"]
            assert state["game_notes"] == final["game_notes"] and _strip(state["phase_history"]) == final["phase_history"]
            assert runs > 0, f"{name}: no run of Continue messages to collapse"
        finally:
            svc.close()


def test_threads_with_playout_seats_are_refused_before_anything_runs():
    dsl = load_dsl("werewolf-(mafia)")
    one, pool = RoomService(seed=2, playout_rollouts=8, playout_max_turns=16), RoomPoolService(seed=2, chunk_rooms=4, playout_rollouts=8, playout_max_turns=16)
    try:
        for s in (one, pool):
            s.create_room("p", "werewolf-(mafia)", _players(8, (1,)), dsl=dsl, playout_seats=(3,))
            s.create_room("q", "werewolf-(mafia)", _players(8, (1,)), dsl=dsl)
        with pytest.raises(ValueError):
            one.run_room("p")
        with pytest.raises(ValueError):
            pool.run_rooms(["q", "p"])
        fresh = RoomService(seed=2)
        fresh.create_room("q", "werewolf-(mafia)", _players(8, (1,)), dsl=dsl)
        want = _strip(fresh.continue_room("q"))
        fresh.close()
        assert _strip(pool.continue_room("q")) == want and _strip(one.continue_room("q")) == want     # q had not moved
    finally:
        one.close()
        pool.close()


# ---- the Node twins: one script through node/selftest_run.js and through the Python pool
GAMES = ("werewolf-(mafia)", "two-truths-and-a-lie")


def _script():
    ops = [["create", "w1", GAMES[0], _players(8, (1,))], ["create", "w2", GAMES[0], _players(8)], ["create", "w3", GAMES[0], _players(12, (3, 12))],
           ["create", "t1", GAMES[1], _players(4, (2,))], ["create", "t2", GAMES[1], _players(5)],
           ["create", "p1", GAMES[0], _players(8, (1,)), [3]]]
    threads = ["w1", "t1", "w2", "w3", "t2"]
    items = [{"id": "x1", "type": "text"}]
    for until, max_turns in ((["person", "end"], 64), ([], 3), (["phase"], 9), (["person", "end"], 64), (["person", "end", "phase"], 1),
                             (["person", "end"], 40), (["end"], 100)):
        ops.append(["run", threads, max_turns, until, items])
        ops += [["answer", t] for t in ("w1", "w3", "t1")]
        ops += [["message", t, "Continue"] for t in ("w1", "t2")]
    ops.append(["refused", "p1"])
    return ops


def _shared(o):
    """what both hosts' outputs carry: the AgentState fields of the reference (the Python state has two more), the calls"""
    if not isinstance(o, dict):
        return o
    if "turns" in o:
        return {"turns": [_shared(t) for t in o["turns"]], "played": o["played"], "stopped": o["stopped"]}
    keep = ("current_phase_id", "current_phase_name", "player_states", "playerActions", "game_notes", "phase_history", "gameName")
    out = {"state": {k: o["state"].get(k) for k in keep}}
    for k in ("toolCalls", "uiCalls", "played", "kind"):
        if k in o:
            out[k] = o[k]
    return out


def _run_python(ops, seed, chunk_rooms):
    pool = RoomPoolService(seed=seed, chunk_rooms=chunk_rooms, playout_rollouts=8, playout_max_turns=16)
    info, outputs = {}, []
    try:
        for op in ops:
            if op[0] == "create":
                players = op[3]
                pool.create_room(op[1], op[2], players, dsl=load_dsl(op[2]), playout_seats=tuple(op[4]) if len(op) > 4 else ())
                info[op[1]] = (len(players), [i + 1 for i, p in enumerate(players) if p["isBot"] is False])
                outputs.append(None)
            elif op[0] == "run":
                outputs.append(_strip(pool.run_rooms(op[1], op[2], tuple(op[3]), [op[4]] * len(op[1]))))
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
def test_node_run_room_and_run_rooms_give_the_same_outputs(tmp_path):
    ops = _script()
    script = {"seed": 5, "chunkRooms": 2, "ops": ops, "plain": "w2", "dsls": {g: os.path.join(GOLD, "dsl", g + ".json") for g in GAMES}}
    sp, op = tmp_path / "script.json", tmp_path / "out.json"
    sp.write_text(json.dumps(script))
    out = subprocess.run(["node", os.path.join(ROOT, "game_engine_amd", "node", "selftest_run.js"), str(sp), str(op)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["ok"] is True and r["turns"] > 300
    node_out = json.loads(op.read_text())
    py_out = json.loads(json.dumps(_run_python(ops, seed=5, chunk_rooms=2)))
    assert len(node_out) == len(py_out) == len(ops)
    answered = 0
    for k, (a, b) in enumerate(zip(node_out, py_out)):
        for x, y in zip(a if ops[k][0] == "run" else [a], b if ops[k][0] == "run" else [b]):
            assert _shared(x) == _shared(y), f"op {k} ({ops[k][0]}): the Node pool and the Python pool differ"
        answered += ops[k][0] == "answer" and a is not None
    assert answered > 0

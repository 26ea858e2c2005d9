"""RoomPoolService on the GPU (-m gpu): many threads in shared batch chunks, each stepped under its own key and turn
(ge_batch_step_rooms), must serve every thread exactly as RoomService's one batch per thread does - the reference runs of
the strings_human_* goldens message by message, 48 threads in random ticks against RoomService, and the Node twin."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLD, ROOT, load_dsl, load_golden
from test_messages import _replay
from test_strings_golden import _strip

pytestmark = pytest.mark.gpu

FILES = sorted(f for f in os.listdir(GOLD) if f.startswith("strings_human_"))
GAMES = {"werewolf-(mafia)": [8, 12], "two-truths-and-a-lie": [4]}


@pytest.mark.parametrize("name", FILES)
def test_person_messages_through_the_pool_equal_reference_run(name):
    from game_engine_amd import RoomPoolService
    g = load_golden(name)
    for case in g["cases"]:
        _replay(RoomPoolService(seed=case["seed"], chunk_rooms=16), g, case, f"{name} seed={case['seed']:#x} room={case['room']} (pool)")


def _script(seed=11, n_threads=48, ticks=40):
    """creates / ticks / closes: 48 threads over Werewolf x 8 and x 12 and Two-Truths x 4 with mixed human and bot seats;
    threads closed mid-run and new ones opened in the freed slots"""
    rng = np.random.default_rng(seed)
    ops, live, opened = [], [], 0

    def create():
        nonlocal opened
        game = ["werewolf-(mafia)", "two-truths-and-a-lie"][int(rng.integers(0, 2))]
        n = int(rng.choice(GAMES[game]))
        humans = [1] if rng.random() < 0.5 else ([1, 3] if rng.random() < 0.3 else [])
        players = [{"name": f"P{i + 1}", "gamePlayerId": i + 1, "isBot": (i + 1) not in humans} for i in range(n)]
        tid = f"thread-{opened}"
        opened += 1
        ops.append(["create", tid, game, players])
        live.append((tid, n))

    for _ in range(n_threads):
        create()
    for tick in range(ticks):
        sub = rng.permutation(len(live))[: int(rng.integers(1, len(live) + 1))]
        msgs = []
        for i in sub:
            tid, n = live[int(i)]
            r = rng.random()
            if r < 0.55:
                text = "Continue"
            elif r < 0.65:
                text = "Player P1 in game chat: hello"
            elif r < 0.85:
                text = f'Player 1 voted "P{int(rng.integers(1, n + 1))}" in voting x'
            elif r < 0.95:
                text = "Input: my three statements"
            else:
                text = "Start game."
            msgs.append([tid, text])
        ops.append(["tick", msgs])
        if tick % 10 == 9:
            for _ in range(3):
                tid, _n = live.pop(int(rng.integers(0, len(live))))
                ops.append(["close", tid])
            for _ in range(3):
                create()
    return ops


def _run_python(ops, seed, chunk_rooms):
    from game_engine_amd import RoomPoolService, RoomService
    dsls = {g: load_dsl(g) for g in GAMES}
    pool, ref = RoomPoolService(seed=seed, chunk_rooms=chunk_rooms), RoomService(seed=seed)
    outputs = []
    for op in ops:
        if op[0] == "create":
            a = pool.create_room(op[1], op[2], op[3], dsl=dsls[op[2]])
            b = ref.create_room(op[1], op[2], op[3], dsl=dsls[op[2]])
            assert _strip(a) == _strip(b), op[1]
            outputs.append(_strip(a))
        elif op[0] == "tick":
            got = pool.handle_messages([(t, text) for t, text in op[1]])
            for (t, text), o in zip(op[1], got):
                assert _strip(o) == _strip(ref.handle_message(t, text)), (t, text)
            outputs.append([_strip(o) for o in got])
        else:
            pool.close(op[1])
            ref.close(op[1])
            outputs.append(None)
    pool.close()
    ref.close()
    return outputs


def test_many_threads_in_ticks_equal_room_service():
    ops = _script()
    outputs = _run_python(ops, seed=5, chunk_rooms=8)             # 8-slot chunks: several per pool, slots reused
    played = sum(o["played"] for tick in outputs if isinstance(tick, list) for o in tick)
    assert played > 500


def test_a_thread_named_twice_is_refused():
    from game_engine_amd import RoomPoolService
    pool = RoomPoolService(seed=1)
    players = [{"name": f"P{i + 1}", "gamePlayerId": i + 1} for i in range(8)]
    pool.create_room("a", "werewolf-(mafia)", players, dsl=load_dsl("werewolf-(mafia)"))
    with pytest.raises(ValueError):
        pool.handle_messages([("a", "Continue"), ("a", "Continue")])
    assert pool.handle_message("a", "Continue")["played"]
    pool.close()


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not available")
def test_node_pool_gives_the_same_outputs(tmp_path):
    ops = _script()
    script = {"seed": 5, "chunkRooms": 8, "ops": ops, "dsls": {g: os.path.join(GOLD, "dsl", g + ".json") for g in GAMES}}
    sp, op = tmp_path / "script.json", tmp_path / "out.json"
    sp.write_text(json.dumps(script))
    out = subprocess.run(["node", os.path.join(ROOT, "game_engine_amd", "node", "selftest_pool.js"), str(sp), str(op)],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["ok"] is True and r["compared"] > 500
    node_out = json.loads(op.read_text())
    py_out = json.loads(json.dumps(_run_python(ops, seed=5, chunk_rooms=8)))
    assert len(node_out) == len(py_out)
    for k, (a, b) in enumerate(zip(node_out, py_out)):
        for x, y in zip(a if isinstance(a, list) else [a], b if isinstance(b, list) else [b]):
            assert _shared(x) == _shared(y), f"op {k} ({ops[k][0]}): the Node pool and the Python pool differ"


def _shared(o):
    """what both hosts' outputs carry: the AgentState fields of the reference (the Python state has two more), the calls"""
    if o is None:
        return None
    state = o.get("state", o)
    keep = ("current_phase_id", "current_phase_name", "player_states", "playerActions", "game_notes", "phase_history", "gameName")
    out = {"state": {k: state.get(k) for k in keep}}
    for k in ("toolCalls", "uiCalls", "played", "kind"):
        if k in o:
            out[k] = o[k]
    return out

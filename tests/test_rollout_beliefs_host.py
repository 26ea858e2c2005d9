"""ge_batch_rollout_beliefs on the CPU side: the C99 prototype and the ctypes symbol; the reference re-deal of POLICY.md §3j
(tests/rollout_beliefs_ref.py) on its own - equal weights are rollout_seats_ref's re-deal record for record, the pick's identity,
a seat of weight 255 among ones is the wolf in the share the prior odds give, a seat of weight 0 never is while the others
suffice, what the seat knows is never overridden; and the services with their chunks stood in for by an oracle-backed batch -
argument checks before any library call, defaults, beliefs=None identical output, the call made, and the same 16 bytes from
the Python and the JS host."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import load_dsl
from oracle.oracle import Oracle
from oracle.rng import pick
from rollout_beliefs_ref import redeal, reference_beliefs, weighted_index
from rollout_seats_ref import known_sets
from rollout_seats_ref import redeal as redeal_uniform
from test_rollout_actions_host import _players
from test_rollout_seats_host import _SeatChunk, _states

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE_DIR = os.path.join(ROOT, "game_engine_amd", "node")
needs_node = pytest.mark.skipif(shutil.which("node") is None or not os.path.exists(os.path.join(NODE_DIR, "ge_addon.node")),
                                reason="node or the built addon is not available")
W_ROLE, W_TEAM, W_REVEALED = 0, 1, 3


def test_header_declares_rollout_beliefs(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text("""
#include "ge_step.h"
int (*p)(ge_batch *, uint64_t, const uint64_t *, const uint64_t *, const uint32_t *, const uint32_t *, const uint32_t *,
         const uint32_t *, const uint32_t *, int32_t *, const uint8_t *, uint32_t, uint32_t, uint64_t, ge_rollout_stats *,
         const uint32_t *, const uint32_t *, ge_compare_stats *) = ge_batch_rollout_beliefs;
typedef char sixteen_slots[GE_BELIEF_SLOTS == 16 ? 1 : -1];
int main(void) { return p == 0; }
""")
    subprocess.check_call([cc, "-std=c99", "-pedantic", "-Werror", "-Wall", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "t.o")])


def test_symbol_listed_and_version_unchanged():
    from game_engine_amd import _lib
    assert "ge_batch_rollout_beliefs" in _lib.SYMBOLS and _lib.BELIEF_SLOTS == 16 and _lib.GE_ABI_VERSION == 5


def test_equal_weights_pick_is_the_uniform_pick():
    rng = np.random.default_rng(3)
    for d, m, v in zip(rng.integers(0, 2 ** 32, 20000), rng.integers(1, 12, 20000), rng.integers(1, 256, 20000)):
        assert weighted_index([int(v)] * int(m), int(d)) == pick(int(d), int(m))
    assert weighted_index([0, 0, 0], 2 ** 32 - 1) == 2 and weighted_index([0, 7, 0], 0) == 1 and weighted_index([0, 7, 0], 2 ** 32 - 1) == 1


def _row(n, values):
    row = np.zeros(16, dtype=np.uint8)
    row[:n] = values
    return row


@pytest.mark.parametrize("game,n", [("werewolf-(mafia)", 5), ("werewolf-(mafia)", 8), ("werewolf-(mafia)", 12), ("two-truths-and-a-lie", 4)])
def test_equal_rows_reproduce_the_unweighted_redeal(game, n):
    orc, states = _states(game, n, turns=(0, 3, 6, 9, 14, 20))
    slots = n if orc.table.pack == 1 else 3
    for rec in states:
        for seat in range(0, n + 1):
            for g in (0, 5, 2 ** 64 - 1):
                want = redeal_uniform(orc, rec, seat, 7, g, 11).tobytes()
                for v in (1, 16, 255):
                    assert redeal(orc, rec, seat, 7, g, 11, _row(slots, v)).tobytes() == want, (seat, g, v)


def _one_wolf_left():
    """A Werewolf x 8 night after the deal with one of the two wolves revealed: from a Villager's seat need = 1."""
    orc, states = _states(turns=(6,))
    rec = states[0].copy()
    wolves = [c for c in range(8) if rec["p"][c][W_TEAM] == 2]
    rec["p"][wolves[0]][W_REVEALED] = 1
    seat = next(s for s in range(1, 9) if rec["p"][s - 1][W_ROLE] == 1)
    U, Uw, Uv, need = known_sets(orc, rec, seat)
    assert need == 1 and not Uw and not Uv
    return orc, rec, seat, U


def test_a_suspected_seat_is_the_wolf_by_its_prior_odds():
    orc, rec, seat, U = _one_wolf_left()
    m, N = len(U), 20000
    hot = U[2]
    w = np.ones(8, dtype=np.int64)
    w[hot] = 255
    w[seat - 1] = 77                                                       # the seat's own weight and a revealed seat's are never read
    hits = sum(int(redeal(orc, rec, seat, 0xB0B, g, 6, _row(8, w))["p"][hot][W_TEAM] == 2) for g in range(N))
    p = 255 / (254 + m)
    sigma = (p * (1 - p) / N) ** 0.5
    assert abs(hits / N - p) <= 4 * sigma, (hits / N, p, sigma)


def test_a_cleared_seat_is_never_the_wolf_while_the_others_suffice():
    orc, states = _states(turns=(6,))
    rec = states[0]
    seat = next(s for s in range(1, 9) if rec["p"][s - 1][W_ROLE] == 1)
    U, _, _, need = known_sets(orc, rec, seat)
    assert need == 2 and len(U) == 7
    cleared = U[:4]                                                        # three seats keep a weight: enough for two wolves
    w = np.full(8, 9)
    w[cleared] = 0
    spread = set()
    for g in range(3000):
        out = redeal(orc, rec, seat, 0xB0B, g, 6, _row(8, w))
        assert all(out["p"][c][W_TEAM] != 2 for c in cleared), g
        spread.add(tuple(c for c in U if out["p"][c][W_TEAM] == 2))
    assert len(spread) == 3                                                # every pair of the three
    w[U[5:]] = 0                                                           # one seat keeps a weight: it is a wolf, the other pick is uniform
    second = set()
    for g in range(3000):
        out = redeal(orc, rec, seat, 0xB0B, g, 6, _row(8, w))
        wolves = [c for c in U if out["p"][c][W_TEAM] == 2]
        assert U[4] in wolves and len(wolves) == 2
        second.add(next(c for c in wolves if c != U[4]))
    assert second == set(U) - {U[4]}


def test_what_the_seat_knows_wins_over_the_beliefs():
    orc, states = _states()
    rec = states[-1].copy()
    n = 8
    wolf_seat = next(c for c in range(n) if rec["p"][c][W_TEAM] == 2 and rec["p"][c][W_REVEALED] == 0) + 1
    det = next(c for c in range(n) if rec["p"][c][W_ROLE] == 4)
    U = [c for c in range(n) if c != det and rec["p"][c][W_REVEALED] == 0]
    found = next(c for c in U if rec["p"][c][W_TEAM] == 2)
    rec["det"][:] = 0
    rec["det"][found] = 2
    w = np.full(8, 255)
    w[found] = 0                                                           # "surely not a wolf": the Detective knows better
    for g in range(200):
        assert redeal(orc, rec, det + 1, 5, g, 3, _row(8, w))["p"][found][W_TEAM] == 2
        out = redeal(orc, rec, wolf_seat, 5, g, 3, _row(8, np.arange(8) * 30))  # a wolf knows every team
        assert (out["p"][:n, W_TEAM] == rec["p"][:n, W_TEAM]).all()
    tt, tstates = _states("two-truths-and-a-lie", 4, turns=range(0, 24))
    seen = 0
    for trec in tstates:
        p = trec["p"]
        sp = next((c for c in range(4) if p[c][0]), None)
        if sp is None or p[sp][3] or p[sp][2] == 0:
            continue
        voter = next(s for s in range(1, 5) if s != sp + 1)
        lies = {int(redeal(tt, trec, voter, 9, g, 4, _row(3, [0, 200, 0]))["p"][sp][2]) for g in range(60)}
        assert lies == {2}
        assert {int(redeal(tt, trec, sp + 1, 9, g, 4, _row(3, [0, 200, 0]))["p"][sp][2]) for g in range(20)} == {int(p[sp][2])}
        assert {int(redeal(tt, trec, voter, 9, g, 4, _row(3, 0))["p"][sp][2]) for g in range(80)} == {1, 2, 3}
        seen += 1
    assert seen


class _BeliefChunk(_SeatChunk):
    """_SeatChunk plus rollout_beliefs, run by the oracle (CPU tests only)."""

    def __init__(self, *a):
        super().__init__(*a)
        self.belief_calls = []

    def rollout_beliefs(self, rooms, keys, turns, seats, actions, beliefs, n_rollouts=4096, max_turns=1024, seed=None, baseline=None,
                        subjects=None):
        seed = self.seed if seed is None else seed
        actions = [[] for _ in rooms] if actions is None else [[(int(p), int(c)) for p, c in a] for a in actions]
        self.belief_calls.append(([int(r) for r in rooms], [int(s) for s in seats], actions, [list(map(int, b)) for b in beliefs],
                                  baseline, subjects))
        w, s, c = reference_beliefs(lambda r: (self.orc, self.rooms[r]), rooms, keys, turns, seats, actions, beliefs, n_rollouts, max_turns,
                                    seed, baseline, subjects)
        return (w, s) if baseline is None else (w, s, c)


def _service(seed=0x5EED):
    from game_engine_amd import RoomPoolService
    chunks = []

    class Svc(RoomPoolService):
        def _new_chunk(self, tb, n_players, human_mask, n_rooms):
            c = _BeliefChunk(Oracle(tb.dsl, n_players), self.seed, n_rooms, human_mask)
            chunks.append(c)
            return c

    return Svc(seed=seed, chunk_rooms=4), chunks


def test_service_argument_checks_defaults_and_the_call():
    svc, chunks = _service()
    svc.create_room("a", "werewolf-(mafia)", _players(8, humans=(2,)), dsl=load_dsl("werewolf-(mafia)"))
    svc.create_room("b", "two-truths-and-a-lie", _players(4, humans=(2,)), dsl=load_dsl("two-truths-and-a-lie"))
    for _ in range(7):
        svc.handle_messages([("a", "Continue"), ("b", "Continue")])
    ww, tt = chunks
    for bad in ({9: 1}, {0: 1}, {"x": 1}, {1: 256}, {1: -1}, {1: 1.5}, {1: True}, [1, 2]):
        with pytest.raises(ValueError):
            svc.forecast("a", n_rollouts=4, max_turns=5, seat=3, beliefs=bad)
        with pytest.raises(ValueError):
            svc.advise("a", n_rollouts=4, max_turns=5, view="seat", beliefs=bad)
    with pytest.raises(ValueError):
        svc.forecast("b", n_rollouts=4, max_turns=5, seat=3, beliefs={4: 1})       # Two-Truths: statements 1-3, not seats
    with pytest.raises(ValueError):
        svc.forecast("a", n_rollouts=4, max_turns=5, beliefs={1: 1})               # beliefs without a seat view
    with pytest.raises(ValueError):
        svc.advise("a", n_rollouts=4, max_turns=5, beliefs={1: 1})
    with pytest.raises(ValueError):
        svc.advise("a", n_rollouts=4, max_turns=5, view="full", compare=True, beliefs={1: 1})
    assert not ww.belief_calls and not tt.belief_calls and not ww.seat_calls and not ww.action_calls    # refused before any call
    # beliefs=None: today's path and today's output
    plain = svc.forecast("a", n_rollouts=6, max_turns=25, seat=3)
    assert svc.forecast("a", n_rollouts=6, max_turns=25, seat=3, beliefs=None) == plain and "beliefs" not in plain
    a_plain = svc.advise("a", n_rollouts=5, max_turns=20, view="seat")
    assert svc.advise("a", n_rollouts=5, max_turns=20, view="seat", beliefs=None) == a_plain and not ww.belief_calls
    # defaults: unnamed slots 16, slots past the seats 0; keys as JSON makes them
    f = svc.forecast("a", n_rollouts=6, max_turns=25, seat=3, beliefs={"2": 255, 5: 0})
    want = [16, 255, 16, 16, 0, 16, 16, 16] + [0] * 8
    rooms, seats, actions, bel, base, subj = ww.belief_calls[-1]
    assert seats == [3] and actions == [[]] and bel == [want] and base is None and subj is None
    assert f["beliefs"] == want and list(f)[-1] == "beliefs" and {k: v for k, v in f.items() if k != "beliefs"}.keys() == plain.keys()
    assert json.loads(json.dumps(f)) == f
    assert svc.forecast("a", n_rollouts=6, max_turns=25, seat=3, beliefs={}) == {**plain, "beliefs": [16] * 8 + [0] * 8}   # equal weights
    t = svc.forecast("b", n_rollouts=6, max_turns=25, seat=1, beliefs={3: 9})
    assert t["beliefs"] == [16, 16, 9] + [0] * 13 and tt.belief_calls[-1][3] == [[16, 16, 9] + [0] * 13]
    adv = svc.advise("a", n_rollouts=5, max_turns=20, view="seat", beliefs={2: 255, 5: 0})
    rooms, seats, actions, bel, base, subj = ww.belief_calls[-1]
    assert seats == [2] * 9 and actions == [[(2, c)] for c in range(1, 9)] + [[]] and bel == [want] * 9 and base is None
    assert adv["beliefs"] == want and list(adv)[-1] == "beliefs" and set(adv) == set(a_plain) | {"beliefs"}
    advc = svc.advise("a", n_rollouts=5, max_turns=20, view="seat", compare=True, beliefs={2: 255, 5: 0})
    assert ww.belief_calls[-1][4] == [8] * 9 and ww.belief_calls[-1][5] == [2] * 9 and advc["compare"] is True
    assert all("versus" in o for o in advc["options"]) and advc["policy"] == adv["policy"]
    # plural forms: one call per chunk, a thread without beliefs under equal weights and without the key
    svc.create_room("c", "werewolf-(mafia)", _players(8, humans=(2,)), dsl=load_dsl("werewolf-(mafia)"))
    n_calls = len(ww.belief_calls)
    both = svc.forecasts(["c", "a"], n_rollouts=6, max_turns=25, seats=[4, 3], beliefs=[None, {"2": 255, 5: 0}])
    assert len(ww.belief_calls) == n_calls + 1 and ww.belief_calls[-1][3] == [[16] * 8 + [0] * 8, want]
    assert both[1] == f and both[0] == svc.forecast("c", n_rollouts=6, max_turns=25, seat=4) and "beliefs" not in both[0]
    with pytest.raises(ValueError):
        svc.forecasts(["c", "a"], n_rollouts=6, max_turns=25, seats=[None, 3], beliefs=[{1: 1}, None])
    with pytest.raises(ValueError):
        svc.forecasts(["c", "a"], n_rollouts=6, max_turns=25, seats=[4, 3], beliefs=[None])


@needs_node
def test_python_and_js_make_the_same_bytes():
    from game_engine_amd import GameTable
    from game_engine_amd.room_service import belief_bytes, neutral_beliefs
    cases = [(1, 8, {"2": 255, "5": 0}), (1, 12, {"12": 1, "1": 0}), (1, 4, {}), (2, 4, {"3": 9}), (2, 12, {"1": 0, "2": 0, "3": 0})]
    script = ("const s = require(process.argv[1]); const c = JSON.parse(process.argv[2]);"
              "const bad = [[1, 8, { 9: 1 }, true], [2, 4, { 4: 1 }, true], [1, 8, { 1: 256 }, true], [1, 8, { 1: 1.5 }, true], [1, 8, { x: 1 }, true],"
              " [1, 8, { 1: 1 }, false], [1, 8, [1], true]];"
              "const refused = bad.map(([p, n, b, v]) => { try { s.beliefBytes('t', p, n, b, v); return false; } catch (e) { return e instanceof RangeError; } });"
              "console.log(JSON.stringify({ bytes: c.map(([p, n, b]) => s.beliefBytes('t', p, n, b, true)), neutral: c.map(([p, n]) => s.neutralBeliefs(p, n)),"
              " none: s.beliefBytes('t', 1, 8, null, false), refused }));")
    p = subprocess.run(["node", "-e", script, os.path.join(NODE_DIR, "room_service.js"), json.dumps(cases)], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    tables = {1: GameTable(load_dsl("werewolf-(mafia)")), 2: GameTable(load_dsl("two-truths-and-a-lie"))}
    assert got["bytes"] == [list(belief_bytes("t", tables[pk], n, b, True)) for pk, n, b in cases]
    assert got["neutral"] == [list(neutral_beliefs(tables[pk], n)) for pk, n, _ in cases]
    assert got["none"] is None and belief_bytes("t", tables[1], 8, None, False) is None
    assert got["refused"] == [True] * 7

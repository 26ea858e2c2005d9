"""ge_batch_rollout_seats on the CPU side: the C99 prototype, the ctypes symbol, properties of the reference re-deal of
POLICY.md §3c (tests/rollout_seats_ref.py) - identity for seat 0, what never moves, the role multiset, a wolf's and a
Detective's knowledge, the Detective's memory, the Two-Truths lie - its uniformity over the consistent deals, and the pool
service's seat view with its chunks stood in for by an oracle-backed batch (keys, seed, one call per chunk, output shape, and
the default outputs unchanged)."""
import itertools
import json
import os
import shutil
import subprocess
from collections import Counter

import numpy as np
import pytest

from conftest import load_dsl
from oracle.oracle import Oracle
from rollout_seats_ref import known_sets, redeal, reference_rollout_seats, tuple_fields
from test_rollout_actions_host import MASK64, _ActChunk, _players

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W_ROLE, W_TEAM = 0, 1


def test_header_declares_rollout_seats(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text("""
#include "ge_step.h"
int (*p)(ge_batch *, uint64_t, const uint64_t *, const uint64_t *, const uint32_t *, const uint32_t *, const uint32_t *,
         const uint32_t *, const uint32_t *, int32_t *, uint32_t, uint32_t, uint64_t, ge_rollout_stats *) = ge_batch_rollout_seats;
int main(void) { return p == 0; }
""")
    subprocess.check_call([cc, "-std=c99", "-pedantic", "-Werror", "-Wall", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "t.o")])


def test_symbol_listed():
    from game_engine_amd import _lib
    assert "ge_batch_rollout_seats" in _lib.SYMBOLS


def _states(game="werewolf-(mafia)", n=8, turns=(0, 1, 3, 6, 9, 14, 20, 30), seed=0x51):
    """Records of one oracle room at several turns of its game (pre-deal, night, day, after deaths)."""
    orc = Oracle(load_dsl(game), n)
    out = []
    for t in turns:
        rooms = orc.init_rooms(1)
        if t:
            orc.run(rooms, seed, 3, 0, t)
        out.append(rooms[0].copy())
    return orc, out


def _hidden(orc, rec, c):
    return tuple(int(rec["p"][c][f]) for f in tuple_fields(orc, rec))


@pytest.mark.parametrize("n", [5, 8, 12])
def test_redeal_keeps_what_the_seat_can_see(n):
    orc, states = _states(n=n)
    for rec in states:
        for seat in range(0, n + 1):
            for g in (0, 1, 2 ** 64 - 1):
                out = redeal(orc, rec, seat, 7, g, 11)
                if seat == 0:
                    assert out.tobytes() == rec.tobytes()
                    continue
                fields = tuple_fields(orc, rec)
                rest = [f for f in range(12) if f not in fields]
                assert (out["p"][:, rest] == rec["p"][:, rest]).all()                  # no field outside the tuple moves
                for k in ("phase", "prev", "phase0_done", "end_turn", "games"):
                    assert out[k] == rec[k]
                U, Uw, Uv, _ = known_sets(orc, rec, seat)
                for c in range(16):
                    if c not in U:                                                    # the seat itself, revealed seats
                        assert (out["p"][c] == rec["p"][c]).all() and out["det"][c] == rec["det"][c]
                assert sorted(_hidden(orc, out, c) for c in U) == sorted(_hidden(orc, rec, c) for c in U)   # the multiset
                assert Counter(out["p"][:n, W_ROLE].tolist()) == Counter(rec["p"][:n, W_ROLE].tolist())
                for c in Uw:
                    assert out["p"][c][W_TEAM] == 2
                for c in Uv:
                    assert out["p"][c][W_TEAM] != 2
                me = rec["p"][seat - 1]
                if me[W_TEAM] == 2:                                                   # a wolf knows every team
                    assert (out["p"][:n, W_TEAM] == rec["p"][:n, W_TEAM]).all()
                if me[W_ROLE] == 4:                                                   # the Detective keeps its memory
                    assert (out["det"] == rec["det"]).all()
                else:                                                                 # anyone else's copy follows the deal
                    for c in U:
                        if rec["det"][c]:
                            assert out["det"][c] == (2 if out["p"][c][W_TEAM] == 2 else 1)


def test_redeal_moves_something():
    orc, states = _states()
    rec = states[-1]
    seat = next(s for s in range(1, 9) if rec["p"][s - 1][W_TEAM] == 1 and rec["p"][s - 1][W_ROLE] == 1)
    outs = {redeal(orc, rec, seat, 7, g, 11)["p"].tobytes() for g in range(64)}
    assert len(outs) > 10


def test_redeal_detective_knowledge_and_inconsistent_memory():
    orc, states = _states()
    rec = states[-1].copy()
    det = next(c for c in range(8) if rec["p"][c][W_ROLE] == 4)
    U = [c for c in range(8) if c != det and rec["p"][c][3] == 0]
    wolf = next(c for c in U if rec["p"][c][W_TEAM] == 2)
    rec["det"][:] = 0
    rec["det"][wolf] = 2
    for g in range(200):
        assert redeal(orc, rec, det + 1, 5, g, 3)["p"][wolf][W_TEAM] == 2                # a found wolf stays a wolf
    bad = rec.copy()
    bad["det"][[c for c in U if c != wolf]] = 2                                         # more "wolves" than there are
    _, Uw, Uv, need = known_sets(orc, bad, det + 1)
    assert Uw == [] and Uv == [] and need == sum(1 for c in U if rec["p"][c][W_TEAM] == 2)


def test_two_truths_lie_redrawn_only_for_others_before_the_reveal():
    orc, states = _states("two-truths-and-a-lie", 4, turns=range(0, 24))
    seen = 0
    for rec in states:
        p = rec["p"]
        sp = next((c for c in range(4) if p[c][0]), None)
        for seat in range(0, 5):
            outs = [redeal(orc, rec, seat, 9, g, 4) for g in range(40)]
            for out in outs:
                mask = np.ones_like(rec["p"], dtype=bool)
                if sp is not None:
                    mask[sp][2] = False
                assert (out["p"][mask] == rec["p"][mask]).all()
            lies = {int(o["p"][sp][2]) for o in outs} if sp is not None else set()
            if sp is not None and seat not in (0, sp + 1) and p[sp][3] == 0 and p[sp][2] != 0:
                assert lies == {1, 2, 3}
                seen += 1
            elif sp is not None:
                assert lies == {int(p[sp][2])}
    assert seen


def test_redeal_is_uniform_over_the_consistent_deals():
    """A Villager's view of a Werewolf x 8 night after the deal: every arrangement of the 7 other seats' hidden tuples is
    consistent with what it knows, so 2^16 replicas must spread evenly over all of them (chi-square at mean + 6 sd)."""
    orc, states = _states(turns=(6,))
    rec = states[0]
    seat = next(s for s in range(1, 9) if rec["p"][s - 1][W_ROLE] == 1)
    U, _, _, _ = known_sets(orc, rec, seat)
    tuples = [_hidden(orc, rec, c) for c in U]
    cells = sorted(set(itertools.permutations(tuples)))
    assert len(cells) == 840                                         # 7! / 3!: two wolves (their targets differ), three Villagers
    idx = {c: i for i, c in enumerate(cells)}
    counts = np.zeros(len(cells))
    N = 1 << 16
    for g in range(N):
        out = redeal(orc, rec, seat, 0xD1CE, g, 6)
        counts[idx[tuple(_hidden(orc, out, c) for c in U)]] += 1
    exp = N / len(cells)
    chi2 = float(((counts - exp) ** 2 / exp).sum())
    dof = len(cells) - 1
    assert chi2 < dof + 6 * (2 * dof) ** 0.5, chi2                    # mean 839, sd 41


class _SeatChunk(_ActChunk):
    """_ActChunk plus rollout_seats, run by the oracle (CPU tests only)."""

    def __init__(self, *a):
        super().__init__(*a)
        self.seat_calls = []

    def rollout_seats(self, rooms, keys, turns, seats, actions=None, n_rollouts=4096, max_turns=1024, seed=None):
        seed = self.seed if seed is None else seed
        actions = [[] for _ in rooms] if actions is None else [[(int(p), int(c)) for p, c in a] for a in actions]
        self.seat_calls.append(([int(r) for r in rooms], [int(k) for k in keys], [int(t) for t in turns], [int(s) for s in seats],
                                actions, n_rollouts, max_turns, seed))
        res = [reference_rollout_seats(self.orc, self.rooms[int(r)].copy(), seed, int(k), int(t), int(s), a, n_rollouts, max_turns)
               for r, k, t, s, a in zip(rooms, keys, turns, seats, actions)]
        return np.stack([w for w, _ in res]), np.array([s for _, s in res], dtype=np.int32)


def _service(chunk_rooms=2, seed=0x5EED):
    from game_engine_amd import RoomPoolService
    chunks = []

    class Svc(RoomPoolService):
        def _new_chunk(self, tb, n_players, human_mask, n_rooms):
            c = _SeatChunk(Oracle(tb.dsl, n_players), self.seed, n_rooms, human_mask)
            chunks.append(c)
            return c

    return Svc(seed=seed, chunk_rooms=chunk_rooms), chunks


def test_pool_seat_view_keys_seed_and_shape():
    from game_engine_amd import room_index_of
    from game_engine_amd.room_service import FORECAST_SEED_XOR
    seed = 0x5EED
    svc, chunks = _service(chunk_rooms=4, seed=seed)
    svc.create_room("a", "werewolf-(mafia)", _players(8, humans=(2,)), dsl=load_dsl("werewolf-(mafia)"))
    svc.create_room("b", "werewolf-(mafia)", _players(8, humans=(2,)), dsl=load_dsl("werewolf-(mafia)"))
    for _ in range(7):
        svc.handle_messages([("a", "Continue"), ("b", "Continue")])
    full = svc.forecast("a", n_rollouts=6, max_turns=25)
    assert "seat" not in full and not chunks[0].seat_calls                       # the default is the full view, unchanged
    f = svc.forecast("a", n_rollouts=6, max_turns=25, seat=3)
    rooms, keys, turns, seats, actions, R, M, s = chunks[0].seat_calls[-1]
    assert rooms == [0] and seats == [3] and actions == [[]] and R == 6 and M == 25 and s == seed ^ FORECAST_SEED_XOR
    assert keys == [(room_index_of("a") << 16) & MASK64] and turns == [7]
    assert f["seat"] == 3 and {k: v for k, v in f.items() if k != "seat"}.keys() == full.keys()
    assert list(f)[-1] == "seat" and json.loads(json.dumps(f)) == f
    both = svc.forecasts(["b", "a"], n_rollouts=6, max_turns=25, seats=[None, 3])
    assert len(chunks[0].seat_calls) == 2 and chunks[0].seat_calls[-1][3] == [0, 3]         # one call for the chunk
    assert both[1] == f and both[0] == svc.forecast("b", n_rollouts=6, max_turns=25)
    with pytest.raises(ValueError):
        svc.forecast("a", seat=9)
    a_full = svc.advise("a", n_rollouts=5, max_turns=20)
    assert "view" not in a_full
    a_seat = svc.advise("a", n_rollouts=5, max_turns=20, view="seat")
    rooms, keys, turns, seats, actions, R, M, s = chunks[0].seat_calls[-1]
    assert seats == [2] * 9 and actions == [[(2, c)] for c in range(1, 9)] + [[]] and s == seed ^ FORECAST_SEED_XOR
    assert a_seat["view"] == "seat" and set(a_seat) == set(a_full) | {"view"}
    assert a_seat["policy"] == {k: v for k, v in svc.forecast("a", n_rollouts=5, max_turns=20, seat=2).items() if k != "seat"}
    assert svc.advises(["a"], n_rollouts=5, max_turns=20, view="seat") == [a_seat]
    with pytest.raises(ValueError):
        svc.advise("a", view="spectator")

"""ge_batch_step_rooms_playout on the CPU side: the C99 prototype and the ctypes symbol; the candidate restatement of
tests/playout_ref.py (POLICY.md §3d steps 1-2) pinned against ge_oracle.c - on every golden trajectory's states, the
reference's "policy choice" of every due seat (what a playout seat takes when every candidate ties) is the oracle's own logged
choice, and the due seats are exactly the seats the oracle has act; the all-tied reference turn equals the oracle's turn; the
structural refusals that need no device."""
import os
import shutil
import subprocess

import pytest

import game_engine_amd
from conftest import golden_dsl, golden_files, load_dsl, load_golden
from oracle.oracle import Oracle
from game_engine_amd.room_service import playout_mask
from playout_ref import candidates, due_seats, policy_choice, reference_step_playout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GE_ERR_ARG = -1


def test_header_declares_step_rooms_playout(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text("""
#include "ge_step.h"
int (*p)(ge_batch *, uint64_t, const uint64_t *, const uint64_t *, const uint32_t *, const uint32_t *, const uint64_t *,
         uint32_t, uint32_t, uint64_t, uint32_t, ge_turn_event *, uint32_t *) = ge_batch_step_rooms_playout;
int main(void) { return p == 0 || GE_PLAYOUT_FULL_VIEW != 1u; }
""")
    subprocess.check_call([cc, "-std=c99", "-pedantic", "-Werror", "-Wall", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "t.o")])


def test_symbol_listed_and_null_batch_refused():
    from game_engine_amd import _lib
    assert "ge_batch_step_rooms_playout" in _lib.SYMBOLS
    lib = _lib.load()
    assert lib.ge_batch_step_rooms_playout(None, 0, None, None, None, None, None, 1, 1, 0, 0, None, None) == GE_ERR_ARG
    assert lib.ge_batch_step_rooms_playout(None, 1, None, None, None, None, None, 1, 1, 0, 0, None, None) == GE_ERR_ARG


@pytest.mark.parametrize("name", golden_files())
def test_policy_choice_restatement_matches_the_oracle_on_golden_states(name):
    g = load_golden(name)
    orc = Oracle(golden_dsl(g), g["n_players"], g.get("rounds", 1))
    checked = 0
    for case in g["cases"]:
        seed, key = case["seed"], case["room"]
        rooms = orc.init_rooms(1)
        for t, want in enumerate(case["turns"]):
            before = rooms[0].copy()
            due = due_seats(orc, before, seed, key, t, False, 0)
            guard = int(before["phase"]) == 0 and not before["phase0_done"]
            orc.run(rooms, seed, key, t, 1)
            assert orc.project(rooms[0], declared_only=True) == want, (name, t)       # these are the golden states
            if guard:
                continue
            newly = int(rooms[0]["ev_newly"])
            assert sorted(due) == [s for s in range(1, orc.n + 1) if (newly >> (s - 1)) & 1], (name, case["room"], t)
            for s in due:
                assert policy_choice(orc, before, seed, key, t, s) == int(rooms[0]["ev_choice"][s - 1]), (name, t, s)
                assert policy_choice(orc, before, seed, key, t, s) in candidates(orc, before, s)
                checked += 1
    assert checked > 0


@pytest.mark.parametrize("game,n", [("werewolf-(mafia)", 8), ("werewolf-(mafia)", 12), ("two-truths-and-a-lie", 4)])
def test_all_tied_reference_turn_is_the_oracle_turn(game, n):
    """max_turns = 0: no playout finishes, every candidate ties, so the reference turn is the oracle's turn word for word (the
    injected-then-played record equals the record of the bot acting inside the turn), with decisions made."""
    orc = Oracle(load_dsl(game), n)
    rooms = orc.init_rooms(1)
    decided = 0
    for t in range(40):
        want = rooms.copy()
        orc.run(want, 0xD1CE, 5, t, 1)
        got = rooms.copy()
        decided |= reference_step_playout(orc, got, 0, 0xD1CE, 5, t, (1 << n) - 1, 99, 7, 4, 0)
        assert got.tobytes() == want.tobytes(), t
        rooms = want
    assert decided != 0


@pytest.mark.parametrize("cls", ["RoomService", "RoomPoolService"])
def test_service_playout_options_are_checked_before_anything_is_created(cls):
    svc_cls = getattr(game_engine_amd, cls)
    for bad in ({"playout_rollouts": 0}, {"playout_rollouts": (1 << 16) + 1}, {"playout_max_turns": 4097}, {"playout_view": "mine"}):
        with pytest.raises(ValueError):
            svc_cls(**bad)
    svc = svc_cls(seed=1)
    assert (svc.playout_rollouts, svc.playout_max_turns, svc.playout_full) == (256, 256, False)
    assert svc_cls(playout_view="full").playout_full
    dsl = load_dsl("werewolf-(mafia)")
    players = [{"name": f"P{i + 1}", "isBot": i != 0} for i in range(8)]
    for seats in ((1,), (0,), (9,), (2, 9)):                  # a human seat, ids outside 1..8
        with pytest.raises(ValueError):
            svc.create_room("t", "werewolf-(mafia)", players, dsl=dsl, playout_seats=seats)
    assert not svc._rooms


def test_playout_mask():
    assert playout_mask(8, 0b1, (2, 3, 8)) == 0b10000110
    assert playout_mask(8, 0, ()) == 0
    with pytest.raises(ValueError):
        playout_mask(8, 0b1, (1,))
    with pytest.raises(ValueError):
        playout_mask(4, 0, (5,))

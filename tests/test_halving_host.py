"""GE_PLAYOUT_HALVING on the CPU side: tests/halving_ref.py (POLICY.md §3h on the oracle) checked alone - the offsets, the playout
counts, a full tie, the cases that are §3d exactly, a finalist's value - and the input conditions of tests/test_gpu_halving.py
proved on the very room sets it uses; the header's define and the hosts' option checks."""
import os
import shutil
import subprocess

import pytest

import game_engine_amd
import halving_ref as H
import playout_ref
from conftest import load_dsl
from oracle.oracle import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("c", range(2, 13))
def test_offsets_and_playout_counts(c):
    for n in (1, 2, 5, 24, 200, 1 << 20):
        R, o = H.rounds(c), H.offsets(n, c)
        assert R == {2: 1, 3: 2, 4: 2}.get(c, 3 if c <= 8 else 4)
        assert len(o) == R + 1 and o[0] == 0 and o[R] == n and all(a <= b for a, b in zip(o, o[1:]))
        assert n * ((1 << R) - 1) < 1 << 32                                     # the product fits 32 bits
        # distinct values: no tie at any cut, so the closed form; all equal: nobody is cut, c * n
        _, last, played, tie_kept = H.halve(list(range(1, c + 1)), n, lambda x, lo, hi: x * (hi - lo))
        assert played <= c * n and H.nominal_playouts(n, c) <= c * n
        if o[1] > 0:                                                            # (an empty round 0 is a full tie at its cut)
            assert not tie_kept and played == H.nominal_playouts(n, c)
            assert len(last) == -(-c // (1 << (R - 1))) and c in last
        _, last, played, _ = H.halve(list(range(1, c + 1)), n, lambda x, lo, hi: 0)
        assert played == c * n and last == list(range(1, c + 1))


def test_the_issue_table():
    """candidates -> playouts in units of n, for an n the offsets divide (no rounding)."""
    for c, n, want in ((3, 3, 7), (7, 7, 23), (11, 15, 51)):                    # 2.33 n, 3.29 n, 3.4 n
        assert H.nominal_playouts(n, c) == want


@pytest.mark.parametrize("game,n", [("werewolf-(mafia)", 8), ("werewolf-(mafia)", 12), ("two-truths-and-a-lie", 4)])
def test_full_tie_is_the_policy_and_small_cases_are_the_uniform_rule(game, n):
    orc = Oracle(load_dsl(game), n)
    rooms = orc.init_rooms(1)
    decided = compared = 0
    for t in range(36):
        room, mask = rooms[0].copy(), (1 << n) - 1
        # M = 0: every candidate has 0 wins - the policy's own choice for every seat
        got = H.decide_halving(orc, room, 0xD1CE, 5, t, mask, 99, 7, 24, 0, False)
        assert got == [(s, playout_ref.policy_choice(orc, room, 0xD1CE, 5, t, s)) for s, _ in got]
        want = rooms.copy()
        orc.run(want, 0xD1CE, 5, t, 1)
        one = rooms.copy()
        decided |= H.reference_step_playout_halving(orc, one, 0, 0xD1CE, 5, t, mask, 99, 7, 24, 0)
        assert one.tobytes() == want.tobytes(), t
        if t % 4 == 0:
            # n = 1 (o_{R-1} = 0: nothing is played before the last round) is §3d exactly
            assert H.decide_halving(orc, room, 0xD1CE, 5, t, mask, 99, 7, 1, 24, False) == \
                playout_ref.decide(orc, room, 0xD1CE, 5, t, mask, 99, 7, 1, 24, False)
            compared += 1
        rooms = want
    assert decided and compared


def test_two_candidates_are_the_uniform_rule():
    """c = 2 is one round over replicas 0 .. n - 1: Werewolf x 8 late games, where seats with 2 candidates decide."""
    orc = Oracle(load_dsl("werewolf-(mafia)"), 8)
    import numpy as np
    rng, seen = np.random.default_rng(8), 0
    for room in H.played_rooms(orc, 40, rng, 12, 40):
        if any(len(playout_ref.candidates(orc, room, s)) == 2 for s in playout_ref.due_seats(orc, room, 3, 4, 50, False, 0)):
            mask = sum(1 << (s - 1) for s in range(1, 9) if len(playout_ref.candidates(orc, room, s)) == 2)
            got = H.decide_halving(orc, room, 3, 4, 50, mask, 77, 9, 12, 32, False)
            assert got == playout_ref.decide(orc, room, 3, 4, 50, mask, 77, 9, 12, 32, False)
            seen += len(got)
    assert seen > 0


@pytest.fixture(scope="module")
def logs():
    return {name: H.shared_reference(name, False)[3] for name in H.CASES}


def test_input_conditions_of_the_gpu_tests(logs):
    """On the room sets tests/test_gpu_halving.py steps: decisions of 2, 3 and 4 rounds, a halving choice that is not the
    uniform choice, a cut that kept more than k through a tie, a seat in a room with two deciding seats."""
    every = [d for log in logs.values() for d in log]
    for name, log in logs.items():
        assert len(log) > 10, name
        for d in log:
            n = H.N_REF
            assert d["played"] <= d["c"] * n
            assert d["tie_kept"] or d["played"] == H.nominal_playouts(n, d["c"])
            assert all(d["V"][x] == d["U"][x] for x in d["last"])              # a finalist's V is the uniform value
            assert all(d["V"][x] <= d["U"][x] for x in d["V"])
    assert {2, 3} <= {d["R"] for d in logs["ww8"]}
    assert 4 in {d["R"] for d in logs["ww12"]}
    assert {d["R"] for d in logs["tt4"]} == {2}
    assert any(d["choice"] != d["uniform"] for d in every), "an implementation that never cuts would pass"
    assert any(d["choice"] != d["uniform"] for d in logs["ww8"])
    assert any(d["tie_kept"] for d in every)
    assert any(d["deciders"] >= 2 for d in every)
    assert any(d["deciders"] >= 2 for d in logs["ww_generic"])


def test_header_defines_the_flag_as_four(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text('#include "ge_step.h"\nint main(void) { return !(GE_PLAYOUT_HALVING == 4u && GE_PLAYOUT_FULL_VIEW == 1u && GE_ABI_VERSION == 5); }\n')
    subprocess.check_call([cc, "-std=c99", "-pedantic", "-Werror", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "t")])
    subprocess.check_call([str(tmp_path / "t")])


@pytest.mark.parametrize("cls", ["RoomService", "RoomPoolService"])
def test_service_option_is_checked_and_off_by_default(cls):
    svc_cls = getattr(game_engine_amd, cls)
    assert svc_cls(seed=1).playout_halving is False
    assert svc_cls(seed=1, playout_halving=True).playout_halving is True
    for bad in (1, "yes", None):
        with pytest.raises(ValueError):
            svc_cls(playout_halving=bad)

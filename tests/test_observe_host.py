"""What a seat is shown (POLICY.md §3n), on the CPU: the rule itself - a field is hidden from seat s exactly when §3c's re-deal from
seat s may change it - as a property of tests/observe_ref.py over the oracle's re-deal, the layout of ge_seat_obs from a C99
program against the header, the two symbols, and the refusals that need no device."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from game_engine_amd import _lib
from game_engine_amd.stepper import SEAT_OBS_DTYPE
from observe_ref import redact
from rollout_seats_ref import ROLE_DETECTIVE, TEAM_WEREWOLVES, W_ROLE, W_TEAM, known_sets, redeal
from run_ref import case_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GE_ERR_ARG = -1
CASES = ["ww8", "ww12_h2", "tt4_h1", "draft8_h1", "ww8_generic_h1"]
KEYS = [(0x52554E, 5, 0), (7, (1 << 35) + 11, 213), (0xFEEDFACE, 123456789, 0xFFFFFF00)]      # (seed, key, turn) of the re-deal
PER = 24


def _without_won(rec):
    raw = np.frombuffer(rec.tobytes(), dtype=np.uint8).copy()
    raw[SEAT_OBS_DTYPE.fields["won"][1]] = 0
    return raw.tobytes()


def _check_invariance(orc, rooms):
    """redact(redeal(room, s, ..), s) == redact(room, s) in every byte but `won`; returns (pairs compared, pairs the re-deal changed)"""
    seen = moved = 0
    for i in range(len(rooms)):
        for seat in range(1, orc.n + 1):
            want = redact(orc, rooms[i], seat)
            for seed, key, turn in KEYS:
                dealt = redeal(orc, rooms[i], seat, seed, key, turn)
                got = redact(orc, dealt, seat)
                if _without_won(got) != _without_won(want):
                    bad = [f for f in SEAT_OBS_DTYPE.names if f != "won" and not np.array_equal(got[f], want[f])]
                    raise AssertionError(f"room {i} seat {seat} key {(seed, key, turn)}: fields {bad} differ after the re-deal")
                seen += 1
                moved += dealt.tobytes() != np.asarray(rooms[i]).tobytes()
    return seen, moved


@pytest.mark.parametrize("name", CASES)
def test_what_the_redeal_may_change_is_hidden(name):
    """The rule.  `legal` is part of the property: it proved invariant on every case here."""
    segs = case_inputs(name, PER, True)[0]
    for orc, _, _, _, rooms in segs:
        seen, moved = _check_invariance(orc, rooms)
        # (the re-deal is no identity on these rooms; in Two-Truths it moves a lie only between the statements and the reveal)
        assert seen == PER * orc.n * len(KEYS) and moved > (seen // 4 if orc.table.pack == 1 else 0), (seen, moved)


def _with_detective_memory(orc, rooms, rng):
    """Copies of Werewolf rooms with Detective memory written in.  Per room one of three kinds: 0 a random subset of the truth (what
    a game reaches); 1 more seats marked as werewolves than the room has werewolves left outside the Detective's own seat; 2 so
    many marked as villagers that the werewolves no longer fit among the rest.  Kinds 1 and 2 contradict the record's counts
    for every Detective seat, which is what §3c's inconsistent-knowledge rule (Uw = Uv = empty) tests.  A memory that is wrong
    and still fits the counts is not in the set: neither the re-deal nor the observation can tell it from a right one, and the
    re-deal then places a werewolf on a seat the memory calls one - the team shown for that seat is the stored one by §3n's
    text, so the property does not hold for such records, and no game produces them."""
    out = rooms.copy()
    kinds = []
    for i in range(len(out)):
        n = orc.n
        team = out[i]["p"][:n, W_TEAM]
        truth = np.where(team == TEAM_WEREWOLVES, 2, 1).astype(np.uint8)
        kind = int(rng.integers(0, 3))
        det = np.zeros(16, dtype=np.uint8)
        if kind == 0:
            det[:n] = np.where(rng.random(n) < 0.5, truth, 0)
        elif kind == 1:
            det[:n] = 2
        else:
            det[:n] = 1
        out[i]["det"] = det
        kinds.append(kind)
    return out, kinds


@pytest.mark.parametrize("name", ["ww8", "ww12_h2", "draft8_h1", "ww8_generic_h1"])
def test_the_rule_with_detective_memory_written_in(name):
    rng = np.random.default_rng(len(name))
    segs = case_inputs(name, PER, True)[0]
    dropped = kept = 0
    for orc, _, _, _, rooms in segs:
        fuzzed, kinds = _with_detective_memory(orc, rooms, rng)
        _check_invariance(orc, fuzzed)
        for i in range(len(fuzzed)):
            for seat in range(1, orc.n + 1):
                p = fuzzed[i]["p"]
                if p[seat - 1][W_ROLE] != ROLE_DETECTIVE or p[seat - 1][W_TEAM] == TEAM_WEREWOLVES:
                    continue
                U, Uw, Uv, _ = known_sets(orc, fuzzed[i], seat)
                marked = [c for c in U if fuzzed[i]["det"][c]]
                if marked and not Uw and not Uv:
                    dropped += 1
                    assert kinds[i] != 0, "a truthful memory was dropped as inconsistent"
                    assert not redact(orc, fuzzed[i], seat)["players"][U, 1].any(), "a dropped memory still shows a team"
                kept += bool(Uw or Uv)
    assert dropped > 0 and kept > 0, (dropped, kept)


LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "ge_step.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d\n", sizeof(ge_seat_obs),
           offsetof(ge_seat_obs, seat), offsetof(ge_seat_obs, n_players), offsetof(ge_seat_obs, pack), offsetof(ge_seat_obs, act),
           offsetof(ge_seat_obs, phase_row), offsetof(ge_seat_obs, done), offsetof(ge_seat_obs, won), offsetof(ge_seat_obs, legal),
           offsetof(ge_seat_obs, unknown), offsetof(ge_seat_obs, phase_id), offsetof(ge_seat_obs, prev_phase_id),
           offsetof(ge_seat_obs, end_turn), offsetof(ge_seat_obs, games), offsetof(ge_seat_obs, pad1), offsetof(ge_seat_obs, players),
           offsetof(ge_seat_obs, det), offsetof(ge_seat_obs, pad2), GE_ABI_VERSION);
    return 0;
}
"""


def test_the_record_layout_from_a_c99_program(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    names = ["seat", "n_players", "pack", "act", "phase_row", "done", "won", "legal", "unknown", "phase_id", "prev_phase_id", "end_turn",
             "games", "pad1", "players", "det", "pad2"]
    assert got[0] == 192 == SEAT_OBS_DTYPE.itemsize == C.sizeof(_lib.SeatObs)
    assert got[1:-1] == [0, 1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20, 24, 28, 32, 176, 188]
    assert got[1:-1] == [SEAT_OBS_DTYPE.fields[f][1] for f in names] == [getattr(_lib.SeatObs, f).offset for f in names]
    assert got[-1] == 5 == _lib.GE_ABI_VERSION


def test_both_symbols_are_declared_and_exported():
    assert "ge_batch_observe_seats" in _lib.SYMBOLS and "ge_batch_act_seats" in _lib.SYMBOLS
    lib = _lib.load()
    assert hasattr(lib, "ge_batch_observe_seats") and hasattr(lib, "ge_batch_act_seats")


def test_refusals_that_need_no_device():
    """Without a device there is no batch: every form of the call is refused at its first check, a NULL batch, whatever else it
    carries - NULL arrays, more than twelve seats, a repeated seat - and never gets as far as a launch."""
    lib = _lib.load()
    seats = (C.c_uint32 * 13)(*range(1, 14))
    twice = (C.c_uint32 * 2)(3, 3)
    buf = (C.c_uint8 * 192)()
    ptr = C.cast(buf, C.c_void_p)
    for n_seats, s in ((1, None), (13, seats), (2, twice), (1, seats), (0, None)):
        assert lib.ge_batch_observe_seats(None, 0, 1, n_seats, s, None, 0, None) == GE_ERR_ARG
        assert lib.ge_batch_observe_seats(None, 0, 1, n_seats, s, ptr, 192, None) == GE_ERR_ARG
        assert lib.ge_batch_act_seats(None, 0, 1, n_seats, s, None, None, None) == GE_ERR_ARG
        assert lib.ge_batch_act_seats(None, 0, 0, n_seats, s, ptr, ptr, None) == GE_ERR_ARG
    assert bytes(buf) == bytes(192)

"""ge_batch_find_rooms without a GPU: the exported symbol, the header's record and constants through a C compiler, the names of
the Python host, and proof on the oracle-side reference alone (tests/find_ref.py) that the inputs the GPU tests share hold every
situation - so a later change of the inputs cannot empty a category silently."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from find_ref import FIND_CASES, case_facts, expected_hits, find_ref, room_facts
from game_engine_amd import _lib
from run_ref import CASES, END, PERSON, PHASE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

def test_library_exports_the_symbol_and_the_names_map_to_its_bits():
    from game_engine_amd.stepper import ROOM_HIT_DTYPE, find_want_bits, find_want_names, pending_seats
    lib = _lib.load()
    assert "ge_batch_find_rooms" in _lib.SYMBOLS and lib.ge_batch_find_rooms is not None
    assert lib.ge_batch_find_rooms(None, 0, 0, 3, None, None, 0, None, None) == -1
    assert C.sizeof(_lib.RoomHit) == 16 and ROOM_HIT_DTYPE.itemsize == 16
    for f in ("room", "why", "pending", "phase_id", "segment"):
        assert ROOM_HIT_DTYPE.fields[f][1] == getattr(_lib.RoomHit, f).offset
    assert find_want_bits(("person", "end")) == 3 and find_want_bits("phase") == 4 and find_want_bits(5) == 5
    assert find_want_names(6) == ["end", "phase"] and pending_seats(0b100000000101) == [1, 3, 12]
    with pytest.raises(ValueError):
        find_want_bits(("person", "nobody"))


def test_header_pins_the_hit_record_and_the_constants(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text("""
#include <stddef.h>
#include "ge_step.h"
typedef char hit_is_16_bytes[sizeof(ge_room_hit) == 16 ? 1 : -1];
typedef char hit_fields[offsetof(ge_room_hit, why) == 8 && offsetof(ge_room_hit, pending) == 12 && offsetof(ge_room_hit, phase_id) == 14 &&
                        offsetof(ge_room_hit, segment) == 15 ? 1 : -1];
typedef char person_is_run_until_person[GE_FIND_PERSON == GE_RUN_UNTIL_PERSON ? 1 : -1];
typedef char end_is_run_until_end[GE_FIND_END == GE_RUN_UNTIL_END ? 1 : -1];
typedef char phase_is_4[GE_FIND_PHASE == 4u ? 1 : -1];
typedef char abi_stays_5[GE_ABI_VERSION == 5 ? 1 : -1];
int (*p)(ge_batch *, uint64_t, uint64_t, uint32_t, const uint32_t *, ge_room_hit *, uint64_t, uint64_t *, uint64_t *) = ge_batch_find_rooms;
int main(void) { return p == 0; }
""")
    subprocess.check_call([cc, "-std=c99", "-pedantic", "-Werror", "-Wall", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "t.o")])


def test_reference_is_the_definition_on_a_known_room(dsl_ww):
    """A fresh Werewolf room stands in phase 0, nobody pending, not terminal; PHASE follows the mask alone."""
    from oracle.oracle import Oracle
    orc = Oracle(dsl_ww, 8)
    facts = room_facts(orc, orc.init_rooms(3), 0b11)
    assert facts == [(0, False, 0)] * 3
    assert find_ref(facts, PERSON | END | PHASE, 0b1) == [(PHASE, 0, 0)] * 3 and find_ref(facts, PERSON | END | PHASE, 0b10) == [(0, 0, 0)] * 3
    assert expected_hits([facts, facts], PHASE, [1, 0]) == [(0, PHASE, 0, 0, 0), (1, PHASE, 0, 0, 0), (2, PHASE, 0, 0, 0)]
    assert expected_hits([facts, facts], PHASE, [1, 1], first=2, count=2) == [(2, PHASE, 0, 0, 0), (3, PHASE, 0, 0, 1)]


@pytest.mark.parametrize("name", [n for n in FIND_CASES if n != "mixed"])
def test_the_shared_inputs_hold_every_situation(name):
    """At 130 rooms per segment: PERSON matches where there is a human mask (between 4 and 55), END matches without restart for
    every Werewolf case and Two-Truths x 4 (tt12_h2 has none: nothing is claimed for it), rooms with two pending seats in the
    two-seat cases under restart (also at 65 rooms, ww12_generic_h2 aside), never pending and terminal at once, and under
    restart most rooms match nothing."""
    game, n, mask = CASES[name][0]
    for restart in (False, True):
        _, (facts,) = case_facts(name, 130, restart)
        ref = find_ref(facts, PERSON | END)
        person = sum(1 for why, _, _ in ref if why & PERSON)
        end = sum(1 for why, _, _ in ref if why & END)
        two = sum(1 for _, pending, _ in ref if bin(pending).count("1") >= 2)
        assert not any(why == PERSON | END for why, _, _ in ref), (name, restart)
        if restart:                                              # (without restart about half the rooms have ended)
            assert sum(1 for why, _, _ in ref if why == 0) > 65, (name, restart)
        if mask:
            assert 4 <= person <= 55, (name, restart, person)
        else:
            assert person == 0
        if not restart and (game in ("ww", "draft", "ww_generic") or n <= 4):
            assert end > 0, (name, end)
        if name == "tt12_h2":
            assert end == 0 or restart, (name, restart, end)
        if restart and name in ("ww8_h2", "ww12_h2", "tt4_h2", "tt12_h2"):
            assert 3 <= two <= 10, (name, two)
            _, (facts65,) = case_facts(name, 65, restart)
            assert sum(1 for p, _, _ in facts65 if bin(p).count("1") >= 2) >= 2, name
        if restart and name == "ww12_generic_h2":
            assert two == 1, two
            _, (facts65,) = case_facts(name, 65, restart)
            assert not any(bin(p).count("1") >= 2 for p, _, _ in facts65)


def test_the_mixed_inputs_have_hits_in_every_segment_with_people():
    for restart in (False, True):
        segs, per_segment = case_facts("mixed", 130, restart)
        hits = expected_hits(per_segment, PERSON | END)
        by_seg = {g: [h for h in hits if h[4] == g] for g in range(4)}
        assert all(any(h[1] & PERSON for h in by_seg[g]) for g in (0, 1, 3)) and not any(h[1] & PERSON for h in by_seg[2])
        assert len(hits) < 260
        assert [h[0] for h in hits] == sorted(h[0] for h in hits)
        assert np.all(np.array([h[1] for h in hits]) != 0)

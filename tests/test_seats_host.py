"""Per-room host-driven seats without a GPU (POLICY.md §3l): the header's declarations through a C compiler, the exported symbols
and the Python names, the refusals that need no device, and proof on the oracle alone that the inputs the GPU tests share
(tests/seats_ref.py) make the masks matter - so no GPU comparison there can pass vacuously."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from game_engine_amd import _lib
from seats_ref import SEAT_CASES, masks_matter, seat_case, seat_masks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GE_ERR_ARG = -1


def test_header_declares_the_three_calls_as_c99(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text("""
#include "ge_step.h"
typedef char abi_stays_5[GE_ABI_VERSION == 5 ? 1 : -1];
int (*set_seats)(ge_batch *, uint64_t, const uint64_t *, const uint32_t *) = ge_batch_set_seats;
int (*get_seats)(ge_batch *, uint64_t, uint64_t, uint32_t *) = ge_batch_get_seats;
int (*clear_seats)(ge_batch *) = ge_batch_clear_seats;
int main(void) { return set_seats == 0 || get_seats == 0 || clear_seats == 0; }
""")
    subprocess.check_call([cc, "-std=c99", "-pedantic", "-Werror", "-Wall", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "t.o")])


def test_library_exports_the_symbols_and_refuses_a_null_batch():
    from game_engine_amd import RoomBatch
    lib = _lib.load()
    assert _lib.GE_ABI_VERSION == 5 and lib.ge_abi_version() == 5
    for name in ("ge_batch_set_seats", "ge_batch_get_seats", "ge_batch_clear_seats"):
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
    one64, one32 = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint32)
    assert lib.ge_batch_set_seats(None, 1, one64.ctypes.data, one32.ctypes.data) == GE_ERR_ARG
    assert lib.ge_batch_set_seats(None, 0, None, None) == GE_ERR_ARG
    assert lib.ge_batch_get_seats(None, 0, 1, one32.ctypes.data) == GE_ERR_ARG
    assert lib.ge_batch_clear_seats(None) == GE_ERR_ARG
    assert all(callable(getattr(RoomBatch, m)) for m in ("set_seats", "seats", "clear_seats"))


def test_masks_cycle_through_the_six_forms_inside_a_wavefront():
    for n in (4, 7, 8, 12):
        m = seat_masks(n, 64, np.random.default_rng(n))
        every, top = (1 << n) - 1, 1 << (n - 1)
        assert m[0] == 0 and m[1] == 1 and m[2] == top and m[3] == 0b11 and m[4] == every and not (m >> n).any()
        assert bin(int(m[9])).count("1") == 2 and m[9] & top
        assert len(set(m[5::6].tolist())) > 3, "the random masks repeat"
    _, _, _, _, masks = seat_case("mixed", 65, False)
    assert [len(x) for x in masks] == [65] * 4 and all(len(set(x[:64].tolist())) >= 6 for x in masks)


@pytest.mark.parametrize("name", SEAT_CASES)
def test_the_shared_inputs_make_the_masks_matter(name):
    """At 130 rooms per segment, keys 1000 + i and turn 5: the rooms whose record after one turn differs from the mask-0 result, and
    the rooms that stop on PERSON within 12 turns."""
    differ, stops = masks_matter(name)
    print(f"{name}: {differ} rooms differ after one turn, {stops} stop on PERSON")
    assert differ >= 5 and stops >= 25, (name, differ, stops)


def test_set_human_seats_refuses_before_anything_changes():
    """What runs without a device: an unknown thread in both services, and the seats a room's player count does not have."""
    from game_engine_amd import RoomPoolService, RoomService
    from game_engine_amd.room_service import seats_mask
    for service in (RoomService, RoomPoolService):
        with pytest.raises(ValueError):
            service().set_human_seats("nobody", [1])
    assert seats_mask("t", 8, [1, 8]) == 0b10000001 and seats_mask("t", 12, ()) == 0 and seats_mask("t", 4, [2, 2]) == 0b10
    for n, bad in ((8, [0]), (8, [9]), (4, [5]), (12, [-1]), (8, [1.5]), (8, [True])):
        with pytest.raises(ValueError):
            seats_mask("t", n, bad)

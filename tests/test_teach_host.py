"""ge_batch_teach_seats (POLICY.md §3o), on the CPU: the declaration in the header as a C99 program sees it, the size of the record
it stores, the ABI version, the symbol, the Python surface, the key rule, and the refusals that need no device."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

from game_engine_amd import RoomBatch, SeatEnv, _lib
from game_engine_amd.stepper import ADVICE_DTYPE
from teach_ref import MASK64, key_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GE_ERR_ARG = -1

# the assignment to a pointer of the issue's signature fails to compile (-Werror) where the header declares anything else
DECL_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "ge_step.h"
typedef int (*teach_fn)(ge_batch *, uint64_t, uint64_t, uint32_t, const uint32_t *, const uint64_t *, uint64_t, uint32_t, uint32_t, uint32_t,
                        uint64_t, uint32_t, ge_advice *, size_t, void *);
int main(void) {
    size_t ptr = sizeof(((teach_fn *)0)[0] = ge_batch_teach_seats);   /* type-checked, not evaluated: nothing to link */
    printf("%zu %d %d\n", sizeof(ge_advice), GE_ABI_VERSION, ptr == sizeof(teach_fn));
    return 0;
}
"""


def test_the_declaration_from_a_c99_program(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    src = tmp_path / "decl.c"
    src.write_text(DECL_C)
    exe = tmp_path / "decl"
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [224, 5, 1]
    assert ADVICE_DTYPE.itemsize == 224 and _lib.GE_ABI_VERSION == 5


def test_the_symbol_is_declared_and_exported():
    assert "ge_batch_teach_seats" in _lib.SYMBOLS
    lib = _lib.load()
    assert hasattr(lib, "ge_batch_teach_seats") and lib.ge_abi_version() == 5
    assert len(lib.ge_batch_teach_seats.argtypes) == 15


def test_the_python_surface():
    sig = inspect.signature(RoomBatch.teach_seats)
    assert list(sig.parameters)[:5] == ["self", "seats", "out", "n_rollouts", "max_turns"] and sig.parameters["max_turns"].default == 1024
    for name, default in (("first", 0), ("count", None), ("keys", None), ("key0", 0), ("turn", None), ("seed", None), ("full_view", False),
                          ("stream", 0)):
        p = sig.parameters[name]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == default, name
    sig = inspect.signature(SeatEnv.teach)
    assert list(sig.parameters) == ["self", "n_rollouts", "max_turns", "key0", "full_view"]
    assert (sig.parameters["max_turns"].default, sig.parameters["key0"].default, sig.parameters["full_view"].default) == (1024, 0, False)
    assert callable(SeatEnv.advice_fields)


def test_the_key_rule_wraps():
    assert key_of(0, 5) == 5 and key_of(3, 5) == 5 + (3 << 20)
    assert key_of(1, MASK64) == (1 << 20) - 1                    # 2^64 - 1 + 2^20 wraps
    assert key_of(1 << 44, 7) == 7                               # r << 20 itself wraps
    assert key_of(2, (1 << 40) + 5) == (1 << 40) + 5 + (2 << 20) > 1 << 32 > key_of(2, 5)
    assert all(key_of(r + 1, 9) - key_of(r, 9) == 1 << 20 for r in range(4))   # room for n_rollouts <= 2^20 replica keys each


def test_refusals_that_need_no_device():
    """Without a device there is no batch: every form of the call is refused at its first check, a NULL batch."""
    lib = _lib.load()
    seats = (C.c_uint32 * 2)(1, 2)
    buf = (C.c_uint8 * 448)(*([0xA5] * 448))
    ptr = C.cast(buf, C.c_void_p)
    for n_rollouts, flags in ((4, 0), (0, 0), (4, 2)):
        assert lib.ge_batch_teach_seats(None, 0, 1, 2, seats, None, 0, 0, n_rollouts, 8, 7, flags, ptr, 448, None) == GE_ERR_ARG
    assert bytes(buf) == bytes([0xA5] * 448)

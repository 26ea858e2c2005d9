"""Decision lists (POLICY.md §3q), on the CPU: the two prototypes and constants from a C99 program against the header, the
symbols, the refusal that needs no device, and - so that the GPU comparison of tests/test_gpu_gather_seats.py cannot pass
vacuously - what the filter of tests/gather_ref.py does to the reference records of every case it runs.
Two of those properties are asserted in a narrower form than the feature's issue worded them, because the cases, which
are used as they are, and the rule itself rule the wider form out: "the filter keeps some entries" cannot hold for tt12_h2 under
END, a case without a finished room under either restart setting - the empty list is asserted there -, and "some room has a
proper, non-empty subset of its listed seats due" cannot hold under END alone, since a finished room lists every seat - it is
asserted under SEAT and SEAT | END, and all-or-none under END."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from game_engine_amd import _lib
from gather_ref import END, SEAT, WANTS, dense_choices, due, gather
from observe_ref import OBSERVE_CASES, case_all_seats, case_records, seat_lists

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GE_ERR_ARG = -1

HEADER_C = r"""
#include <stdio.h>
#include "ge_step.h"
typedef int (*gather_fn)(ge_batch *, uint64_t, uint64_t, uint32_t, const uint32_t *, uint32_t, ge_seat_obs *, uint32_t *, uint64_t,
                         uint32_t *, void *);
typedef int (*listed_fn)(ge_batch *, uint64_t, uint64_t, uint32_t, const uint32_t *, const uint32_t *, uint64_t, const uint32_t *,
                         const int32_t *, int32_t *, void *);
#ifdef PROTOTYPES                                    /* compiled, not linked: a prototype that differs from these does not compile */
gather_fn the_gather = ge_batch_gather_seats;
listed_fn the_listed = ge_batch_act_listed;
#else
int main(void) {
    printf("%u %u %d\n", GE_GATHER_SEAT, GE_GATHER_END, GE_ABI_VERSION);
    return 0;
}
#endif
"""


def test_the_header_compiles_as_c_with_both_prototypes(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    src = tmp_path / "decide.c"
    src.write_text(HEADER_C)
    exe = tmp_path / "decide"
    flags = [cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)]
    subprocess.run(flags + ["-DPROTOTYPES", "-c", "-o", str(tmp_path / "decide.o")], check=True)
    subprocess.run(flags + ["-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [SEAT, END, 5]
    assert _lib.GATHER_WANT == {"seat": SEAT, "end": END} and _lib.GE_ABI_VERSION == 5


def test_both_symbols_are_declared_and_exported():
    assert "ge_batch_gather_seats" in _lib.SYMBOLS and "ge_batch_act_listed" in _lib.SYMBOLS
    lib = _lib.load()
    assert hasattr(lib, "ge_batch_gather_seats") and hasattr(lib, "ge_batch_act_listed")
    assert lib.ge_abi_version() == 5


def test_a_null_batch_is_refused_whatever_else_the_call_carries():
    lib = _lib.load()
    seats = (C.c_uint32 * 2)(1, 2)
    buf = (C.c_uint8 * 256)()
    ptr = C.cast(buf, C.c_void_p)
    for want in (0, 1, 2, 3, 4):
        assert lib.ge_batch_gather_seats(None, 0, 1, 2, seats, want, ptr, ptr, 1, ptr, None) == GE_ERR_ARG
        assert lib.ge_batch_gather_seats(None, 0, 0, 0, None, want, None, None, 0, None, None) == GE_ERR_ARG
    assert lib.ge_batch_act_listed(None, 0, 1, 2, seats, ptr, 1, ptr, ptr, ptr, None) == GE_ERR_ARG
    assert lib.ge_batch_act_listed(None, 0, 0, 0, None, None, 0, None, None, None, None) == GE_ERR_ARG
    assert bytes(buf) == bytes(256)


@pytest.mark.parametrize("restart", [False, True])
@pytest.mark.parametrize("name", OBSERVE_CASES)
def test_the_filter_keeps_some_entries_and_drops_some(name, restart):
    """For the list of every seat and each `want`: the list is neither empty nor everything.  Under SEAT (alone or with END) some
    room has a proper, non-empty subset of its listed seats due - what the rank of a seat among its room's due seats is for.
    Under END alone no room can: a finished room emits every listed seat (the rule), which is asserted instead.  One case has no
    finished room at all, tt12_h2 (twelve players' rounds outlast the turns run_ref steps it): its END list is empty, which is
    asserted as such - the GPU test then checks the empty list, M = 0 - and every other case has finished rooms."""
    segs, _ = case_all_seats(name, restart)
    rec = case_records(name, restart, seat_lists(segs)[2])
    for want in WANTS:
        d = due(rec, want)
        per_room = d.sum(axis=1)
        if name == "tt12_h2" and want == END:
            assert d.sum() == 0
            continue
        assert 0 < d.sum() < d.size, (name, restart, want)
        partial = int(((per_room > 0) & (per_room < d.shape[1])).sum())
        if want & SEAT:
            assert partial > 0, (name, restart, want)
        else:
            assert partial == 0 and (per_room == d.shape[1]).any()
        got, entries, n = gather(rec, want)
        assert n[0] == n[1] == d.sum() == len(entries) and np.all(np.diff(entries.astype(np.int64)) > 0)
        assert got.tobytes() == rec.reshape(-1)[entries].tobytes()
        kept, e2, n2 = gather(rec, want, cap=3)
        assert list(n2) == [3, d.sum()] and np.array_equal(e2, entries[:3]) and kept.tobytes() == got[:3].tobytes()


@pytest.mark.parametrize("name", ["ww8_h1", "tt4_h1"])
def test_a_finished_room_is_emitted_under_end_with_winners_and_losers(name):
    segs, _ = case_all_seats(name, False)
    rec = case_records(name, False, seat_lists(segs)[2])
    got, entries, _ = gather(rec, END)
    assert len(got) and (got["done"] == 1).all() and got["won"].any() and (got["won"] == 0).any()
    rooms = entries // rec.shape[1]
    assert np.all(np.bincount(rooms)[np.unique(rooms)] == rec.shape[1])      # every listed seat of a finished room, each with its own `won`
    assert (got["legal"] == 0).any()                                         # ... that SEAT alone would not list


def test_the_dense_array_of_a_list():
    d = dense_choices(6, 3, 8, np.array([4, 9, 0, 5], dtype=np.uint32), np.array([7, 2, -1, 3], dtype=np.int32))
    assert list(d) == [-1, 0, 0, 0, 7, 0]                                    # entry 9 is beyond the grid, list position 3 beyond n
    assert list(dense_choices(6, 9, 2, np.array([4, 5, 0], dtype=np.uint32), np.array([1, 2, 3], dtype=np.int32))) == [0, 0, 0, 0, 1, 2]

"""Reference of ge_batch_teach_seats (POLICY.md §3o), which is its composition rule stated as code: entry (r - first) * n_seats + j
is what the batch's own advise_seats returns for (room r, key_of(r), turn, seats[j]).  No playout logic here; advise_seats itself
is held to the oracle by tests/test_gpu_advise_seats_device.py, and tests/test_gpu_teach_seats.py holds two cases of this call to
the oracle directly.  Also what the GPU tests of the call share: the cases' batches, stepped, and the windows."""
import numpy as np

from game_engine_amd.stepper import ADVICE_DTYPE
from observe_ref import DeviceBuffer, make_batch
from run_ref import SEED, case_inputs

MASK64 = (1 << 64) - 1
PER = 67                               # rooms per segment: a full wavefront and a tail of 3
STEPS = 10                             # turns the batch is stepped before it is advised
FIRST_ROOM = 777                       # observe_ref.make_batch
R, M = 70, 48                          # two wavefronts per entry, the second partly filled
TEACH_CASES = ["ww8_h1", "ww12_h2", "tt4_h1", "tt8_h1", "draft8_h1", "mixed"]


def key_of(r: int, key0: int) -> int:
    """the key room r (batch index) is played under where no keys are given: key0 + (r << 20) mod 2^64"""
    return (int(key0) + (int(r) << 20)) & MASK64


def windows(n_seg):
    """(first, count): observe_ref.windows at PER rooms per segment - everything, the tail of segment 0 from inside its first
    wavefront, nothing, and a window that starts in segment 0 and ends inside segment 2"""
    w = [(0, PER * n_seg), (30, PER - 30), (17, 0)]
    if n_seg > 1:
        w.append((PER - 5, PER + 40))
    return w


def pairs(first, count, seats):
    """(rooms, seats) of the call's entries in their order"""
    return np.repeat(np.arange(first, first + count, dtype=np.uint64), len(seats)), np.tile(np.asarray(seats, dtype=np.uint32), count)


def expected(batch, first, count, seats, n_rollouts, max_turns, keys=None, key0=0, turn=None, seed=None, full_view=False):
    """[count * len(seats)] ADVICE_DTYPE records: the batch's own advise_seats over the same pairs"""
    rooms, s = pairs(first, count, seats)
    if keys is None:
        k = np.array([key_of(r, key0) for r in rooms], dtype=np.uint64)
    else:
        k = np.repeat(np.asarray(keys, dtype=np.uint64), len(seats))
    turns = np.full(len(rooms), batch.turn if turn is None else turn, dtype=np.uint32)
    return batch.advise_seats(rooms, k, turns, s, n_rollouts, max_turns, seed=seed, full_view=full_view)


def teach(batch, first, count, seats, n_rollouts, max_turns, pad=3 * ADVICE_DTYPE.itemsize + 5, **kw):
    """(records, the bytes behind them): teach_seats into a 0xA5-filled buffer of `pad` bytes more than the call needs"""
    need = count * len(seats) * ADVICE_DTYPE.itemsize
    buf = DeviceBuffer(need + pad, fill=0xA5)
    batch.teach_seats(seats, buf, n_rollouts, max_turns, first=first, count=count, **kw)
    raw = buf.host()
    return raw[:need].view(ADVICE_DTYPE), raw[need:]


def stepped_batch(name, **kw):
    """(segments of case_inputs(name, PER, True), the batch with their rooms written, stepped STEPS turns with restart on)"""
    segs = case_inputs(name, PER, True)[0]
    b = make_batch(segs, True, **kw)
    b.step(STEPS)
    return segs, b


def oracle_rooms_after(segs, n_turns=STEPS):
    """per segment (oracle, its rooms advanced by orc.run as the batch's step advances them)"""
    out, base = [], 0
    for orc, _, _, mask, rooms in segs:
        rooms = rooms.copy()
        orc.run(rooms, SEED, FIRST_ROOM + base, 0, n_turns, threads=1, restart=True, human_mask=mask)
        out.append((orc, rooms))
        base += len(rooms)
    return out


def differing(got, want):
    """indices of the records in which two ADVICE_DTYPE arrays differ (for assertion messages)"""
    g = np.ascontiguousarray(got).view(np.uint8).reshape(len(got), -1)
    w = np.ascontiguousarray(want).view(np.uint8).reshape(len(want), -1)
    return np.flatnonzero((g != w).any(axis=1))[:8].tolist()

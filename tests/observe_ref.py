"""Reference of ge_batch_observe_seats (POLICY.md §3n) on oracle ROOM_DTYPE records (tests only): what a seat is shown, built on
rollout_seats_ref's known_sets / tuple_fields - the sets and the tuple the re-deal itself uses -, `legal` by Oracle.inject on
copies (as find_ref.room_facts decides `pending`), `won` by the rollout reference's seat rule, packed into the 192-byte record."""
import ctypes as C

import numpy as np

from game_engine_amd.stepper import SEAT_OBS_DTYPE
from rollout_ref import seat_words
from rollout_seats_ref import ROLE_DETECTIVE, T_LIE, T_REVEALED, T_SPEAKER, W_ROLE, W_TEAM, known_sets, tuple_fields
from parity_util import oracle_rooms_as_views
from run_ref import SEED, case_inputs

assert SEAT_OBS_DTYPE.itemsize == 192


def legal_mask(orc, room, seat):
    """bit c-1: Oracle.inject accepts (seat, c) on a copy of the room"""
    one = np.asarray(room).reshape(1)
    return sum(1 << (c - 1) for c in range(1, 13) if orc.inject(one.copy(), 0, seat, c))


def redact(orc, room, seat):
    """The ge_seat_obs of oracle record `room` for seat `seat` (1-based), as a SEAT_OBS_DTYPE record."""
    room = np.asarray(room).reshape(1)[0]
    n, s = orc.n, seat - 1
    p = room["p"].copy()
    det = room["det"].copy()
    phase = int(room["phase"])
    ph = orc.table.phases[phase]
    unknown = 0
    if orc.table.pack == 1:
        U, Uw, Uv, _ = known_sets(orc, room, seat)
        fields = tuple_fields(orc, room)
        for c in U:
            for f in fields:
                if not (f == W_TEAM and (c in Uw or c in Uv)):
                    p[c][f] = 0
            unknown |= 1 << c
        if room["p"][s][W_ROLE] != ROLE_DETECTIVE:
            det[:] = 0
    else:
        det[:] = 0
        speakers = [c for c in range(n) if p[c][T_SPEAKER]]
        if speakers and speakers[0] != s and p[speakers[0]][T_REVEALED] == 0:
            p[speakers[0]][T_LIE] = 0
            unknown = 1 << speakers[0]
    done = not ph.branches
    o = np.zeros(1, dtype=SEAT_OBS_DTYPE)[0]
    o["seat"], o["n_players"], o["pack"], o["act"] = seat, n, orc.table.pack, ph.act
    o["phase_row"], o["done"] = phase, int(done)
    o["won"] = int(seat_words(orc, room.reshape(1))[12 + s]) if done else 0
    o["legal"], o["unknown"] = legal_mask(orc, room, seat), unknown
    o["phase_id"], o["prev_phase_id"] = orc.ids[phase], orc.ids[int(room["prev"])]
    o["end_turn"], o["games"] = room["end_turn"], room["games"]
    o["players"][:n, :11] = p[:n, :11]
    o["det"][:n] = det[:n]
    return o


def observe_rooms(orc, rooms, seats):
    """[len(rooms), len(seats)] records: room r as seat seats[j] is shown it"""
    out = np.zeros((len(rooms), len(seats)), dtype=SEAT_OBS_DTYPE)
    for r in range(len(rooms)):
        for j, seat in enumerate(seats):
            out[r, j] = redact(orc, rooms[r], seat)
    return out


def observe_batch(segs, seats):
    """The records of a whole batch (segments of run_ref.case_inputs, or (orc, rooms) pairs) for one seat list, [rooms, seats]"""
    return np.concatenate([observe_rooms(seg[0], seg[-1], seats) for seg in segs])


# the cases tests/test_gpu_observe_seats.py and tests/test_gpu_act_seats.py run (run_ref.CASES), 135 rooms per segment: two
# full wavefronts and a tail of 7
OBSERVE_CASES = ["ww8_h1", "ww12_h2", "tt4_h1", "tt12_h2", "draft8_h1", "ww12_generic_h2", "mixed"]
PER = 135
_ALL = {}


def case_all_seats(name, restart):
    """(segments of case_inputs, per segment the records of every seat 1 .. n: [PER, n]), computed once per (case, restart)"""
    key = (name, restart)
    if key not in _ALL:
        segs = case_inputs(name, PER, restart)[0]
        _ALL[key] = (segs, [observe_rooms(orc, rooms, list(range(1, n + 1))) for orc, _, n, _, rooms in segs])
    return _ALL[key]


def case_records(name, restart, seats):
    """the whole batch's records for `seats` (every seat at most the smallest segment's player count), from case_all_seats"""
    segs, per_seg = case_all_seats(name, restart)
    return np.concatenate([rec[:, [s - 1 for s in seats]] for rec in per_seg])


# ---- what the GPU tests of the two calls share
_TABLES = {}


def _table(dsl):
    key = id(dsl)
    if key not in _TABLES:
        from game_engine_amd import GameTable
        _TABLES[key] = (GameTable(dsl), dsl)                     # (the dsl is kept alive: its id is the key)
    return _TABLES[key][0]


def make_batch(segs, restart, max_fuse=1, trace=False, views=None):
    """The segments' start rooms (or `views`, one array per segment) written as views."""
    from game_engine_amd import RoomBatch
    b = RoomBatch([(_table(dsl), n, len(rooms), mask) for _, dsl, n, mask, rooms in segs], seed=SEED, first_room=777,
                  max_fuse=max_fuse, restart=restart, trace=trace)
    base = 0
    for g, (orc, _, _, _, rooms) in enumerate(segs):
        b.write_rooms(base, oracle_rooms_as_views(orc, rooms) if views is None else views[g])
        base += len(rooms)
    return b


def seat_lists(segs):
    n = min(s[2] for s in segs)
    return [[1], [n, 2, 1], list(range(1, n + 1))]


def windows(n_seg):
    total = PER * n_seg
    w = [(0, total), (63, 67), (17, 0)]
    if n_seg > 1:
        w.append((PER - 5, PER + 70))                            # starts in segment 0, ends inside segment 2
    return w


class DeviceBuffer:
    """Device memory of the test's own (hipMalloc), as the calls take it: an object with data_ptr() and nbytes.  The tests of the
    two C calls use it instead of a torch tensor: torch brings a HIP runtime of its own, which has to be loaded before the
    library's (tests/test_gpu_seat_env.py runs the torch loop in a process that does so)."""

    def __init__(self, nbytes, fill=0):
        self.hip = C.CDLL("libamdhip64.so")
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), C.c_size_t(max(self.nbytes, 16))) == 0
        self.ptr = p.value
        assert self.hip.hipMemset(C.c_void_p(self.ptr), C.c_int(fill), C.c_size_t(max(self.nbytes, 16))) == 0

    @classmethod
    def of(cls, array):
        array = np.ascontiguousarray(array)
        buf = cls(array.nbytes)
        if array.nbytes:
            assert buf.hip.hipMemcpy(C.c_void_p(buf.ptr), C.c_void_p(array.ctypes.data), C.c_size_t(array.nbytes), 1) == 0
        return buf

    def data_ptr(self):
        return self.ptr

    def host(self, dtype=np.uint8):
        """a copy on the host (the device is synchronised by the copy)"""
        raw = np.empty(self.nbytes, dtype=np.uint8)
        if self.nbytes:
            assert self.hip.hipMemcpy(C.c_void_p(raw.ctypes.data), C.c_void_p(self.ptr), C.c_size_t(self.nbytes), 2) == 0
        return raw.view(dtype)

    def __del__(self):
        if getattr(self, "ptr", None):
            self.hip.hipFree(C.c_void_p(self.ptr))
            self.ptr = None


def differing_fields(got, want):
    """names of the SEAT_OBS_DTYPE fields in which two record arrays differ (for assertion messages)"""
    return [f for f in SEAT_OBS_DTYPE.names if not np.array_equal(got[f], want[f])]

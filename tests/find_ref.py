"""Reference of ge_batch_find_rooms (POLICY.md §3k) on the oracle: per room (why, pending, phase_id).  `pending` is decided by the
definition itself - bit i is set when seat i+1 is host-driven and Oracle.inject accepts some choice of it on a copy of the room, as
run_ref.person_pending asks for any seat -, END by run_ref.is_terminal, PHASE by the mask: no condition evaluator of its own.
tests/test_find_host.py and the GPU tests share it."""
import numpy as np

from run_ref import END, PERSON, PHASE, case_inputs, is_terminal

HIT_FIELDS = ("room", "why", "pending", "phase_id", "segment")


def room_facts(orc, rooms, mask):
    """Per room what every `want` is answered from: (pending seats of the human mask, terminal, phase id)."""
    out = []
    for i in range(len(rooms)):
        one = rooms[i:i + 1]
        pending = 0
        for seat in range(orc.n):
            if (mask >> seat) & 1 and any(orc.inject(one.copy(), 0, seat + 1, c) for c in range(1, max(orc.n, 3) + 1)):
                pending |= 1 << seat
        out.append((pending, bool(is_terminal(orc, one)), int(orc.ids[int(one["phase"][0])])))
    return out


# the cases tests/test_gpu_find_rooms.py runs (run_ref.CASES)
FIND_CASES = ["ww8_h1", "ww8_h2", "ww12_h1", "ww12_h2", "tt4_h1", "tt4_h2", "tt8_h1", "tt12_h2", "draft8_h1", "ww8_generic_h1",
              "ww12_generic_h2", "tt4_generic_h1", "ww8", "mixed"]
_FACTS = {}


def case_facts(name, per, restart):
    """(segments of case_inputs, room_facts per segment), computed once per (case, rooms per segment, restart)."""
    key = (name, per, restart)
    if key not in _FACTS:
        segs = case_inputs(name, per, restart)[0]
        _FACTS[key] = (segs, [room_facts(orc, rooms, mask) for orc, _, _, mask, rooms in segs])
    return _FACTS[key]


def find_ref(facts, want, phase_mask=0):
    """room_facts -> per room (why, pending, phase_id) under `want`; pending is 0 unless PERSON is asked for."""
    out = []
    for pending, terminal, pid in facts:
        p = pending if want & PERSON else 0
        why = (PERSON if p else 0) | (END if want & END and terminal else 0) | (PHASE if want & PHASE and (phase_mask >> pid) & 1 else 0)
        out.append((why, p, pid))
    return out


def expected_hits(per_segment, want, phase_masks=None, first=0, count=None):
    """per_segment: one room_facts list per segment of a batch.  The hits of the range as (room, why, pending, phase_id, segment)
    tuples in ascending room order."""
    hits, base = [], 0
    total = sum(len(f) for f in per_segment)
    last = total if count is None else first + count
    for g, facts in enumerate(per_segment):
        for i, (why, pending, pid) in enumerate(find_ref(facts, want, phase_masks[g] if phase_masks is not None else 0)):
            if why and first <= base + i < last:
                hits.append((base + i, why, pending, pid, g))
        base += len(facts)
    return hits


def hits_as_tuples(hits: np.ndarray):
    return [tuple(int(h[f]) for f in HIT_FIELDS) for h in hits]

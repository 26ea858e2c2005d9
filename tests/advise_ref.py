"""Reference of ge_batch_advise_seats (POLICY.md §3m), by composition only: `legal` is what Oracle.inject accepts on a copy of the
room (as find_ref.room_facts decides `pending`), and every word of an option is taken from rollout_seats_ref.reference_rollout_seats
of the entry the definition names.  No playout logic of its own.  tests/test_advise_host.py and the GPU tests share it."""
import numpy as np

from rollout_seats_ref import reference_rollout_seats
from run_ref import SEED, case_inputs

GE_ERR_ARG = -1
OPTIONS = 12
W_FINISHED, W_SEAT_WINS, W_SEAT_SCORE = 1, 41 + 12, 41 + 24      # words of ge_rollout_stats: summary.finished, seat_wins, seat_score
ADVICE_REF_DTYPE = np.dtype([("status", "<i4"), ("legal", "<u4"), ("best", "<u4"), ("phase_id", "<u4"),
                             ("policy", [("finished", "<u4"), ("wins", "<u4"), ("score", "<u8")]),
                             ("option", [("finished", "<u4"), ("wins", "<u4"), ("score", "<u8")], (OPTIONS,))])


def n_choices(orc) -> int:
    """C of §3m: the segment's players in Werewolf, the three statements in Two-Truths."""
    return orc.n if orc.table.pack == 1 else 3


def legal_mask(orc, room, seat: int) -> int:
    """bit c-1: Oracle.inject accepts (seat, c) on a copy of `room` (one oracle record)."""
    one = np.asarray(room).reshape(1)
    return sum(1 << (c - 1) for c in range(1, n_choices(orc) + 1) if orc.inject(one.copy(), 0, seat, c))


def reference_advice(orc, room, seed: int, key: int, turn: int, seat: int, n_rollouts: int, max_turns: int, full_view: bool = False):
    """One ADVICE_REF_DTYPE record: entry (room, key, turn, seat) under (n_rollouts, max_turns, seed)."""
    out = np.zeros((), dtype=ADVICE_REF_DTYPE)
    legal = legal_mask(orc, room, seat)
    if not legal:
        out["status"] = GE_ERR_ARG
        return out
    view = 0 if full_view else seat

    def words(actions):
        w, st = reference_rollout_seats(orc, np.asarray(room).copy(), seed, key, turn, view, actions, n_rollouts, max_turns)
        assert st == 0
        return int(w[W_FINISHED]), int(w[W_SEAT_WINS + seat - 1]), int(w[W_SEAT_SCORE + seat - 1])

    out["legal"] = legal
    out["phase_id"] = int(orc.ids[int(np.asarray(room)["phase"])])
    best, top = 0, -1
    for c in range(1, n_choices(orc) + 1):
        if not (legal >> (c - 1)) & 1:
            continue
        fin, wins, score = words([(seat, c)])
        out["option"][c - 1] = (fin, wins, score)
        value = wins if orc.table.pack == 1 else score
        if value > top:                                          # the lowest choice on a tie
            best, top = c, value
    out["best"] = best
    out["policy"] = words([])
    return out


# ---- the shared inputs of the GPU tests: run_ref.case_inputs(case, 16, restart=False), every (room, seat) of every room
ADVISE_CASES = ["ww8_h1", "ww12_h2", "tt4_h1", "tt8_h1", "ww8_generic_h1", "tt4_generic_h1", "draft8_h1", "mixed"]
PER = 16
_ENTRIES, _REF = {}, {}


def case_entries(name):
    """(segments of case_inputs, rooms, keys, turns, seats): keys on both sides of 2^32, distinct; turns below 300."""
    if name not in _ENTRIES:
        segs = case_inputs(name, PER, False)[0]
        rng = np.random.default_rng(sum(map(ord, name)) + 77)
        rooms, seats = [], []
        for g, (orc, _, n, _, _) in enumerate(segs):
            for i in range(PER):
                for s in range(1, n + 1):
                    rooms.append(g * PER + i); seats.append(s)
        keys = rng.choice(1 << 31, size=len(rooms), replace=False).astype(np.uint64)
        keys[1::2] += np.uint64(1 << 33)
        turns = rng.integers(0, 300, len(rooms)).astype(np.uint32)
        _ENTRIES[name] = (segs, np.array(rooms, dtype=np.uint64), keys, turns, np.array(seats, dtype=np.uint32))
    return _ENTRIES[name]


def entry_reference(segs, room, key, turn, seat, n_rollouts, max_turns, full_view=False, seed=SEED):
    orc, _, _, _, recs = segs[int(room) // PER]
    return reference_advice(orc, recs[int(room) % PER], seed, int(key), int(turn), int(seat), n_rollouts, max_turns, full_view)


def case_reference(name, n_rollouts, max_turns, full_view=False):
    """The reference records of case_entries(name), computed once per (case, n_rollouts, max_turns, view) and left unchanged."""
    k = (name, n_rollouts, max_turns, full_view)
    if k not in _REF:
        segs, rooms, keys, turns, seats = case_entries(name)
        ref = np.array([entry_reference(segs, r, q, t, s, n_rollouts, max_turns, full_view) for r, q, t, s in zip(rooms, keys, turns, seats)],
                       dtype=ADVICE_REF_DTYPE)
        ref.setflags(write=False)
        _REF[k] = ref
    return _REF[k]

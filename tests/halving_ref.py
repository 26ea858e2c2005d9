"""Oracle-side reference of GE_PLAYOUT_HALVING (tests only): POLICY.md §3h restated on oracle ROOM_DTYPE records.  Who decides
and from which candidates is playout_ref's (§3d steps 1-2); a candidate's value in round j is rollout_seats_ref's entry under
key pkey + o_j with o_{j+1} - o_j playouts; the cut keeps every candidate tied with the k-th largest value; the choice is the
argmax among the last round's candidates with the pick(d, m) tie-break.  Also the room sets tests/test_halving_host.py and
tests/test_gpu_halving.py share: the host test proves on the oracle alone that they hold the decisions the GPU tests need."""
import numpy as np

from conftest import load_dsl
from oracle import dsl_variants
from oracle.oracle import Oracle
from oracle.rng import pick
from parity_util import oracle_events
from playout_ref import SEAT_WINS, candidates, due_seats, seat_draw
from rollout_seats_ref import reference_rollout_seats

M64 = (1 << 64) - 1


def rounds(c: int) -> int:
    """R = ceil(log2 c) for c >= 2 candidates."""
    return (c - 1).bit_length()


def offsets(n: int, c: int):
    """[o_0 .. o_R] for n playouts and c candidates."""
    R = rounds(c)
    return [n * ((1 << j) - 1) // ((1 << R) - 1) for j in range(R + 1)]


def nominal_playouts(n: int, c: int) -> int:
    """The playouts of one decision when no cut meets a tie: sum_j ceil(c / 2^j) (o_{j+1} - o_j)."""
    o = offsets(n, c)
    return sum(-(-c // (1 << j)) * (o[j + 1] - o[j]) for j in range(rounds(c)))


def halve(cand, n: int, value):
    """§3h for one seat: value(x, lo, hi) = the seat's wins of candidate x over replicas lo .. hi - 1.  Returns (V of every
    candidate that was ever valued, the last round's candidates, playouts played, a cut kept more than k)."""
    c, R, o = len(cand), rounds(len(cand)), offsets(n, len(cand))
    V = {x: 0 for x in cand}
    live, played, tie_kept = list(cand), 0, False
    for j in range(R):
        if o[j + 1] > o[j]:
            for x in live:
                V[x] += value(x, o[j], o[j + 1])
            played += len(live) * (o[j + 1] - o[j])
        if j < R - 1:
            k = -(-c // (1 << (j + 1)))
            theta = sorted((V[x] for x in live), reverse=True)[k - 1]
            live = [x for x in live if V[x] >= theta]
            tie_kept |= len(live) > k
    return V, live, played, tie_kept


def decide_halving(orc, room, seed: int, key: int, turn: int, mask: int, pkey: int, pseed: int, n: int, M: int, full_view: bool,
                   restart: bool = False, human_mask: int = 0, log=None):
    """[(seat, choice)] of the playout seats that decide in this turn under the flag (ascending seat).  log (a list): one dict
    per decision with what the input conditions ask about, the uniform (§3d) choice among it - valued from the same entries,
    every candidate over every round's range."""
    out = []
    deciders = [s for s in due_seats(orc, room, seed, key, turn, restart, human_mask)
                if (mask >> (s - 1)) & 1 and len(candidates(orc, room, s)) >= 2]
    for s in deciders:
        cand = candidates(orc, room, s)
        memo = {}

        def value(x, lo, hi):
            if (x, lo) not in memo:
                words = reference_rollout_seats(orc, room, pseed, (pkey + lo) & M64, turn, 0 if full_view else s, [(s, x)], hi - lo, M)[0]
                memo[(x, lo)] = int(words[SEAT_WINS + s - 1])
            return memo[(x, lo)]

        V, last, played, tie_kept = halve(cand, n, value)
        d = seat_draw(seed, key, turn, s)
        top = max(V[x] for x in last)
        tied = [x for x in last if V[x] == top]
        choice = tied[pick(d, len(tied))]
        out.append((s, choice))
        if log is not None:
            o = offsets(n, len(cand))
            U = {x: sum(value(x, o[j], o[j + 1]) for j in range(rounds(len(cand))) if o[j + 1] > o[j]) for x in cand}
            u_tied = [x for x in cand if U[x] == max(U.values())]
            log.append({"c": len(cand), "R": rounds(len(cand)), "played": played, "tie_kept": tie_kept, "deciders": len(deciders),
                        "choice": choice, "uniform": u_tied[pick(d, len(u_tied))], "V": V, "U": U, "last": last})
    return out


def reference_step_playout_halving(orc, rooms, i, seed: int, key: int, turn: int, mask: int, pkey: int, pseed: int, n: int, M: int,
                                   full_view: bool = False, restart: bool = False, human_mask: int = 0, log=None):
    """playout_ref.reference_step_playout with §3h's decision: room i of `rooms` one turn, changed in place; the decided mask."""
    chosen = decide_halving(orc, rooms[i], seed, key, turn, mask, pkey, pseed, n, M, full_view, restart, human_mask, log)
    one = rooms[i:i + 1].copy()
    for s, c in chosen:
        assert orc.inject(one, 0, s, c), (s, c)
    orc.run(one, seed, key, turn, 1, threads=1, restart=restart, human_mask=human_mask)
    dmask = 0
    for s, c in chosen:
        one[0]["ev_newly"] |= 1 << (s - 1)
        one[0]["ev_choice"][s - 1] = c
        dmask |= 1 << (s - 1)
    rooms[i] = one[0]
    return dmask


# ---- the shared room sets: ~70 listed rooms per segment (two plan wavefronts, one partly filled), each advanced 0 .. 39 turns
# under its own key, every seat a playout seat
SEED, PSEED, N_REF, M_REF, ROOMS = 0x5EED, 0xF00D, 24, 48, 70
CASES = {"ww8": ("ww", 8, 101), "ww12": ("ww", 12, 102), "tt4": ("tt", 4, 103), "ww_generic": ("ww_generic", 8, 104)}


def case_dsl(game):
    if game == "ww":
        return load_dsl("werewolf-(mafia)")
    if game == "tt":
        return load_dsl("two-truths-and-a-lie")
    return dsl_variants.build("ww_generic", load_dsl("werewolf-(mafia)"))


def played_rooms(orc, R, rng, lo=0, hi=40):
    rooms = orc.init_rooms(R)
    for i in range(R):
        orc.run(rooms[i:i + 1], int(rng.integers(0, 1 << 30)), int(rng.integers(0, 1 << 20)), 0, int(rng.integers(lo, hi)))
    return rooms


_INPUTS, _REFS = {}, {}


def case_inputs(name):
    """(dsl, orc, rooms, listed, keys, turns, masks, pkeys) of a named case, built once per process."""
    if name not in _INPUTS:
        game, n, rs = CASES[name]
        rng = np.random.default_rng(rs)
        dsl = case_dsl(game)
        orc = Oracle(dsl, n)
        rooms = played_rooms(orc, ROOMS, rng)
        listed = rng.permutation(ROOMS).astype(np.uint64)
        keys = rng.integers(0, 1 << 40, ROOMS).astype(np.uint64)
        turns = rng.integers(0, 50000, ROOMS).astype(np.uint32)
        masks = np.full(ROOMS, (1 << n) - 1, dtype=np.uint32)
        pkeys = rng.integers(0, 1 << 63, ROOMS).astype(np.uint64)
        _INPUTS[name] = (dsl, orc, rooms, listed, keys, turns, masks, pkeys)
    return _INPUTS[name]


def reference_call(orc, rooms, listed, keys, turns, masks, pkeys, n, M, full_view, pseed=PSEED, log=None):
    """(rooms after, events, decided) of one flagged step over the listed rooms of one segment."""
    after = rooms.copy()
    events, decided = [], []
    for room, key, turn, mask, pkey in zip(listed, keys, turns, masks, pkeys):
        i = int(room)
        decided.append(reference_step_playout_halving(orc, after, i, SEED, int(key), int(turn), int(mask), int(pkey), pseed, n, M,
                                                      full_view, log=log))
        events.append(oracle_events(orc, after[i:i + 1], int(turn))[0])
    return after, events, np.array(decided, dtype=np.uint32)


def shared_reference(name, full_view):
    """The reference of a case's flagged step (n = 24, M = 48) with its decision log, computed once per process."""
    if (name, full_view) not in _REFS:
        _, orc, rooms, listed, keys, turns, masks, pkeys = case_inputs(name)
        log = []
        _REFS[(name, full_view)] = reference_call(orc, rooms, listed, keys, turns, masks, pkeys, N_REF, M_REF, full_view, log=log) + (log,)
    return _REFS[(name, full_view)]

"""Reference of ge_batch_run_rooms (POLICY.md §3f), restated on the oracle by composition: room k takes the oracle's single turns
(seed, key, turn + t) with step_rooms's restart rule until the record a turn left meets a named condition or max_turns turns are
played.  PERSON is decided by the definition itself - would Oracle.inject accept any (human seat, choice) on a copy of the room? -
so the reference has no condition evaluator of its own.  Also the inputs tests/test_run_host.py and tests/test_gpu_run_rooms.py
share: the host test proves on the oracle alone that every stop reason occurs in them."""
import numpy as np

from conftest import load_dsl
from oracle import dsl_variants
from oracle.oracle import Oracle
from parity_util import oracle_events, oracle_rooms_as_views

PERSON, END, PHASE = 1, 2, 4


def dsl_of(game):
    if game == "ww":
        return load_dsl("werewolf-(mafia)")
    if game == "tt":
        return load_dsl("two-truths-and-a-lie")
    if game == "draft":
        return load_dsl("draft-werewolf-(mafia)")
    if game == "ww_generic":
        return dsl_variants.build("ww_generic", load_dsl("werewolf-(mafia)"))
    return dsl_variants.build("tt_generic", load_dsl("two-truths-and-a-lie"))


def person_pending(orc, room, mask):
    """`room`: a length-1 oracle array.  True if an injected action of some host-driven seat would be accepted."""
    for seat in range(orc.n):
        if not (mask >> seat) & 1:
            continue
        for choice in range(1, max(orc.n, 3) + 1):
            if orc.inject(room.copy(), 0, seat + 1, choice):
                return True
    return False


def is_terminal(orc, room):
    return not orc.table.phases[int(room["phase"][0])].branches


def run_ref(orc, rooms, i, seed, key, turn, max_turns, until, restart, mask):
    """Plays rooms[i] on in place.  Returns (played, stopped, events, views): one event and one view per played turn."""
    one = rooms[i:i + 1]
    events, views, stopped = [], [], 0
    for t in range(max_turns):
        orc.run(one, seed, key, turn + t, 1, threads=1, restart=restart, human_mask=mask)
        ev = oracle_events(orc, one, turn + t)[0]
        events.append(ev)
        views.append(oracle_rooms_as_views(orc, one)[0])
        stopped = 0
        if until & PERSON and person_pending(orc, one, mask):
            stopped |= PERSON
        if until & END and is_terminal(orc, one):
            stopped |= END
        if until & PHASE and ev["to_phase_id"] != ev["from_phase_id"]:
            stopped |= PHASE
        if stopped:
            break
    return len(events), stopped, events, views


# ---- shared inputs: (game, n_players, human mask) per segment; every layout, shipped and GENERIC tables, the draft Werewolf,
# human masks of 0 / one / two seats, and a mixed four-segment batch
CASES = {
    "ww8": [("ww", 8, 0)], "ww12": [("ww", 12, 0)], "tt4": [("tt", 4, 0)], "tt8": [("tt", 7, 0)], "tt12": [("tt", 12, 0)],
    "ww8_h1": [("ww", 8, 0b1)], "ww8_h2": [("ww", 8, 0b10000100)], "ww12_h1": [("ww", 11, 0b100)], "ww12_h2": [("ww", 12, 0b100000000001)],
    "tt4_h1": [("tt", 4, 0b10)], "tt4_h2": [("tt", 3, 0b101)], "tt8_h1": [("tt", 8, 0b1)], "tt12_h2": [("tt", 12, 0b100000001000)],
    "draft8_h1": [("draft", 8, 0b1)], "ww8_generic_h1": [("ww_generic", 8, 0b10)], "ww12_generic_h2": [("ww_generic", 12, 0b11)],
    "tt4_generic_h1": [("tt_generic", 4, 0b1)], "tt8_generic_h1": [("tt_generic", 5, 0b10000)], "tt12_generic": [("tt_generic", 9, 0)],
    "mixed": [("ww", 6, 0b1), ("tt", 4, 0b10), ("ww", 10, 0), ("tt", 7, 0b1000000)],
}
SEED = 0x52554E


def case_inputs(name, rooms_per_segment, restart, rng_seed=0):
    """Deterministic inputs of a case: per segment (oracle, dsl, n, mask, start rooms) - every room played by the oracle from the
    initial state for its own number of turns under its own key, so the starts are reachable states all over the game - and for
    the whole batch the listed rooms (a shuffled two thirds, segments interleaved), their keys (distinct, below and above 2^32)
    and first turns."""
    rng = np.random.default_rng(sum(map(ord, name)) * 2 + int(restart) + 1000 * rng_seed)
    segs = []
    for game, n, mask in CASES[name]:
        dsl = dsl_of(game)
        orc = Oracle(dsl, n)
        rooms = orc.init_rooms(rooms_per_segment)
        for i in range(rooms_per_segment):
            orc.run(rooms[i:i + 1], SEED, int(rng.integers(0, 1 << 40)), 0, int(rng.integers(0, 70)), threads=1, restart=restart, human_mask=0)
        segs.append((orc, dsl, n, mask, rooms))
    total = rooms_per_segment * len(segs)
    listed = rng.permutation(total)[: max(1, (2 * total) // 3)]
    keys = rng.choice(1 << 40, size=len(listed), replace=False).astype(np.uint64)
    keys[::2] = rng.choice(1 << 20, size=len(keys[::2]), replace=False)
    turns = rng.integers(0, 300, len(listed)).astype(np.uint32)
    turns[0] = 0xFFFFFFFF - 64                                  # the last turns a room can take: first + max_turns <= 2^32 - 1
    return segs, listed, keys, turns


def reference_call(segs, listed, keys, turns, max_turns, until, restart):
    """run_ref over a call's entries, on copies of the segments' rooms.  Returns (played, stopped, events, views, rooms after)."""
    after = [rooms.copy() for _, _, _, _, rooms in segs]
    per = len(after[0])
    played, stopped, events, views = [], [], [], []
    for k, r in enumerate(listed):
        s, i = divmod(int(r), per)
        orc, _, _, mask, _ = segs[s]
        p, why, ev, vw = run_ref(orc, after[s], i, SEED, int(keys[k]), int(turns[k]), max_turns, until, restart, mask)
        played.append(p); stopped.append(why); events.append(ev); views.append(vw)
    return np.array(played, dtype=np.uint32), np.array(stopped, dtype=np.uint32), events, views, after

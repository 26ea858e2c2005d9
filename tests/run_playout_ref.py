"""Reference of ge_batch_run_rooms_playout (POLICY.md §3g), restated on the oracle by composition: run_ref's loop and stop tests
(person_pending / is_terminal, PHASE on the turn's event) around playout_ref.reference_step_playout instead of the oracle's plain
turn.  Also the inputs tests/test_run_playout_host.py and tests/test_gpu_run_playout.py share - run_ref's cases with playout masks
added: the host test proves on the oracle alone that they reach every stop reason, the limit, a decision behind the first turn and
a room that decides after another of its list has stopped."""
import numpy as np

from parity_util import oracle_events, oracle_rooms_as_views
from playout_ref import reference_step_playout
from run_ref import END, PERSON, PHASE, SEED, case_inputs, is_terminal, person_pending

R_SMALL, M_SMALL, PSEED = 8, 16, 0xF00D5
# the cases of the GPU test against this reference: run_ref.CASES names; per case the (until, max_turns) calls, restart off and on
REF_CASES = ["ww8_h1", "ww12_h2", "tt4_h2", "mixed"]
REF_CALLS = [(PERSON | END, 40), (PERSON, 24), (END | PHASE, 12), (0, 13)]


def run_playout_ref(orc, rooms, i, seed, key, turn, mask, pkey, pseed, R, M, full_view, max_turns, until, restart, human_mask):
    """Plays rooms[i] on in place.  Returns (played, stopped, events, views, decided): one of each per played turn."""
    one = rooms[i:i + 1]
    events, views, decided, stopped = [], [], [], 0
    for t in range(max_turns):
        decided.append(reference_step_playout(orc, rooms, i, seed, key, turn + t, mask, pkey, pseed, R, M, full_view, restart, human_mask))
        ev = oracle_events(orc, one, turn + t)[0]
        events.append(ev)
        views.append(oracle_rooms_as_views(orc, one)[0])
        stopped = 0
        if until & PERSON and person_pending(orc, one, human_mask):
            stopped |= PERSON
        if until & END and is_terminal(orc, one):
            stopped |= END
        if until & PHASE and ev["to_phase_id"] != ev["from_phase_id"]:
            stopped |= PHASE
        if stopped:
            break
    return len(events), stopped, events, views, decided


def playout_inputs(name, rooms_per_segment, restart, rng_seed=0):
    """run_ref.case_inputs plus, per listed room, a playout mask of 1 - 3 bot seats of its segment (every fifth room: none) and a
    playout key."""
    segs, listed, keys, turns = case_inputs(name, rooms_per_segment, restart, rng_seed)
    rng = np.random.default_rng(sum(map(ord, name)) + 7 * int(restart) + 1000 * rng_seed)
    per = rooms_per_segment
    masks = np.zeros(len(listed), dtype=np.uint32)
    for k, r in enumerate(listed):
        _, _, n, hmask, _ = segs[int(r) // per]
        bots = [s for s in range(n) if not (hmask >> s) & 1]
        if k % 5 != 4:
            for s in rng.choice(bots, size=min(len(bots), int(rng.integers(1, 4))), replace=False):
                masks[k] |= np.uint32(1 << int(s))
    pkeys = rng.integers(0, 1 << 63, len(listed)).astype(np.uint64)
    return segs, listed, keys, turns, masks, pkeys


def reference_call(segs, listed, keys, turns, masks, pkeys, max_turns, until, restart, R=R_SMALL, M=M_SMALL, pseed=PSEED, full_view=False):
    """run_playout_ref over a call's entries, on copies of the segments' rooms.  Returns (played, stopped, events, views, decided,
    rooms after)."""
    after = [rooms.copy() for _, _, _, _, rooms in segs]
    per = len(after[0])
    played, stopped, events, views, decided = [], [], [], [], []
    for k, r in enumerate(listed):
        s, i = divmod(int(r), per)
        orc, _, _, hmask, _ = segs[s]
        p, why, ev, vw, dec = run_playout_ref(orc, after[s], i, SEED, int(keys[k]), int(turns[k]), int(masks[k]), int(pkeys[k]), pseed, R, M,
                                              full_view, max_turns, until, restart, hmask)
        played.append(p); stopped.append(why); events.append(ev); views.append(vw); decided.append(dec)
    return np.array(played, dtype=np.uint32), np.array(stopped, dtype=np.uint32), events, views, decided, after


_CACHE = {}


def shared_reference(name, restart, until, max_turns):
    """The reference of one shared call (24 listed rooms), computed once per process."""
    key = (name, restart, until, max_turns)
    if key not in _CACHE:
        inputs = playout_inputs(name, 9 if name == "mixed" else 36, restart)
        _CACHE[key] = (inputs, reference_call(*inputs, max_turns, until, restart))
    return _CACHE[key]

"""Oracle-side reference of ge_batch_rollout_beliefs (tests only): POLICY.md §3j restated on oracle ROOM_DTYPE records - the
re-deal of rollout_seats_ref with its two belief-dependent draws replaced (which seats of Uq are wolves, which statement is the
lie), then the copies played and reduced as rollout_seats_ref / compare_ref do."""
import numpy as np

from compare_ref import COMPARE_WORDS, compare_sums, entry_words, outcomes
from oracle.rng import draw, pick
from rollout_actions_ref import inject_all
from rollout_ref import ROLLOUT_WORDS
from rollout_seats_ref import (ROLE_DETECTIVE, T_LIE, T_REVEALED, T_SPEAKER, TEAM_WEREWOLVES, W_TEAM, W_ROLE, known_sets, tuple_fields,
                               view_key)

SLOTS = 16


def weighted_index(weights, d: int) -> int:
    """The index §3j takes from `weights` (the weights of the slots still free, in ascending slot order) under draw d: the first
    whose running sum exceeds pick(d, W); W == 0: every weight 1."""
    ws = [int(w) for w in weights]
    if sum(ws) == 0:
        ws = [1] * len(ws)
    x = pick(d, sum(ws))
    acc = 0
    for i, w in enumerate(ws):
        acc += w
        if acc > x:
            return i
    raise AssertionError("pick(d, W) < W")


def redeal(orc, room, seat: int, seed: int, g: int, turn0: int, beliefs):
    """rollout_seats_ref.redeal under `beliefs` (16 bytes): a copy of oracle record `room` as replica g sees it from `seat`."""
    rec = np.asarray(room).reshape(1).copy()[0]
    if seat == 0:
        return rec
    w = [int(x) for x in beliefs]
    assert len(w) == SLOTS
    vk = view_key(seed, g, turn0)
    n, p = orc.n, rec["p"]
    if orc.table.pack != 1:
        speakers = [c for c in range(n) if p[c][T_SPEAKER]]
        if speakers:
            sp = speakers[0]
            if sp != seat - 1 and p[sp][T_REVEALED] == 0 and p[sp][T_LIE] != 0:
                p[sp][T_LIE] = 1 + weighted_index(w[:3], draw(vk, 80))
        return rec
    fields = tuple_fields(orc, rec)
    U, Uw, Uv, need = known_sets(orc, rec, seat)
    Uq = [c for c in U if c not in Uw and c not in Uv]
    A = sorted(tuple(int(p[c][f]) for f in fields) for c in U if p[c][W_TEAM] == TEAM_WEREWOLVES)
    B = sorted(tuple(int(p[c][f]) for f in fields) for c in U if p[c][W_TEAM] != TEAM_WEREWOLVES)
    SW, rem = list(Uw), list(Uq)
    for j in range(need):                                    # step (1): the only Werewolf draw the beliefs touch
        SW.append(rem.pop(weighted_index([w[c] for c in rem], draw(vk, 32 + j))))
    SW = sorted(SW)
    SV = [c for c in U if c not in SW]
    for tuples, seats, base in ((A, SW, 48), (B, SV, 64)):
        left = list(seats)
        for i, t in enumerate(tuples):
            c = left.pop(pick(draw(vk, base + i), len(left)))
            for f, v in zip(fields, t):
                p[c][f] = v
    if p[seat - 1][W_ROLE] != ROLE_DETECTIVE:
        for c in U:
            if rec["det"][c] != 0:
                rec["det"][c] = 2 if p[c][W_TEAM] == TEAM_WEREWOLVES else 1
    return rec


def play_entry(orc, room, seed: int, key: int, turn: int, seat: int, actions, beliefs, n_rollouts: int, max_turns: int, threads: int = 1):
    """(the n_rollouts played copies, 0) of one entry, or (None, the refused action's status)."""
    rec, st = inject_all(orc, room, actions)
    if st != 0:
        return None, st
    copies = np.stack([redeal(orc, rec, seat, seed, key + r, turn, beliefs) for r in range(n_rollouts)])
    if max_turns:
        orc.run(copies, seed, key, turn, max_turns, threads=threads, restart=False, human_mask=0)
    return copies, 0


def reference_beliefs(orc_of, rooms, keys, turns, seats, actions, beliefs, n_rollouts: int, max_turns: int, seed: int,
                      baseline=None, subjects=None, threads: int = 1):
    """(words (n, 77), status (n,), cmp (n, 6) or None) of one call.  orc_of(room) -> (oracle, that room's oracle record).  A
    refused entry has zero words; cmp[k] is zero when entry k or its baseline was refused."""
    n = len(rooms)
    words = np.zeros((n, ROLLOUT_WORDS), dtype=np.uint64)
    status = np.zeros(n, dtype=np.int32)
    played = []
    for k in range(n):
        orc, rec = orc_of(int(rooms[k]))
        copies, st = play_entry(orc, rec.copy(), seed, int(keys[k]), int(turns[k]), int(seats[k]), actions[k] if actions is not None else [],
                                beliefs[k], n_rollouts, max_turns, threads)
        status[k] = st
        played.append(copies)
        if st == 0:
            words[k] = entry_words(orc, copies, int(keys[k]), int(turns[k]), max_turns)
    if baseline is None:
        return words, status, None
    cmp = np.zeros((n, COMPARE_WORDS), dtype=np.uint64)
    for k in range(n):
        b = int(baseline[k])
        if played[k] is None or played[b] is None:
            continue
        orc, _ = orc_of(int(rooms[k]))
        cmp[k] = compare_sums(outcomes(orc, played[k], int(subjects[k])), outcomes(orc, played[b], int(subjects[k])))
    return words, status, cmp

"""Oracle-side reference of ge_batch_rollout_seats (tests only): POLICY.md §3c restated on oracle ROOM_DTYPE records with
oracle.rng - the entry's actions logged by Oracle.inject, then every replica's copy re-dealt from seat `seat`'s view, then the
copies played by the oracle as rollout_ref does."""
import numpy as np

from oracle.rng import GOLDEN, M32, draw, mix32, pick, room_key
from oracle.summary import reference_summary_words
from rollout_actions_ref import inject_all
from rollout_ref import ROLLOUT_WORDS, seat_words

VIEW_SALT = 0x56494557
ROLE_DETECTIVE, TEAM_WEREWOLVES = 4, 2
ACT_PRIVATE = (1, 2, 3)            # WOLF_TARGET, DOCTOR_PROTECT, DETECTIVE: the action log is private
W_ROLE, W_TEAM, W_REVEALED, W_SECRET, W_ELIG, W_SUB, W_TARGET, W_ACTED, W_CHOICE = 0, 1, 3, 5, 6, 7, 8, 9, 10
T_SPEAKER, T_LIE, T_REVEALED = 0, 2, 3


def view_key(seed: int, g: int, turn0: int) -> int:
    return mix32(room_key(seed, g & 0xFFFFFFFFFFFFFFFF) ^ VIEW_SALT ^ ((turn0 * GOLDEN) & M32))


def tuple_fields(orc, room):
    """The fields of a seat's hidden tuple in view order (role, team, has_secret_role, night_action_eligible,
    night_action_submitted, selected_target_id[, acted, choice])."""
    act = orc.table.phases[int(room["phase"])].act
    base = [W_ROLE, W_TEAM, W_SECRET, W_ELIG, W_SUB, W_TARGET]
    return base + [W_ACTED, W_CHOICE] if act in ACT_PRIVATE else base


def known_sets(orc, room, seat):
    """(U, Uw, Uv, need) of §3c as sorted seat-index lists (0-based)."""
    n, p = orc.n, room["p"]
    s = seat - 1
    U = [c for c in range(n) if c != s and p[c][W_REVEALED] == 0]
    if p[s][W_TEAM] == TEAM_WEREWOLVES:
        Uw = [c for c in U if p[c][W_TEAM] == TEAM_WEREWOLVES]
        Uv = [c for c in U if p[c][W_TEAM] != TEAM_WEREWOLVES]
    elif p[s][W_ROLE] == ROLE_DETECTIVE:
        Uw = [c for c in U if room["det"][c] == 2]
        Uv = [c for c in U if room["det"][c] == 1]
    else:
        Uw, Uv = [], []
    n_a = sum(1 for c in U if p[c][W_TEAM] == TEAM_WEREWOLVES)
    uq = [c for c in U if c not in Uw and c not in Uv]
    if not 0 <= n_a - len(Uw) <= len(uq):
        Uw, Uv = [], []
    return U, Uw, Uv, n_a - len(Uw)


def redeal(orc, room, seat: int, seed: int, g: int, turn0: int):
    """A copy of oracle record `room` as replica g (global room key) sees it from seat `seat` (1-based; 0 = unchanged)."""
    rec = np.asarray(room).reshape(1).copy()[0]
    if seat == 0:
        return rec
    vk = view_key(seed, g, turn0)
    n, p = orc.n, rec["p"]
    if orc.table.pack != 1:
        speakers = [c for c in range(n) if p[c][T_SPEAKER]]
        if speakers:
            sp = speakers[0]
            if sp != seat - 1 and p[sp][T_REVEALED] == 0 and p[sp][T_LIE] != 0:
                p[sp][T_LIE] = 1 + pick(draw(vk, 80), 3)
        return rec
    fields = tuple_fields(orc, rec)
    U, Uw, Uv, need = known_sets(orc, rec, seat)
    Uq = [c for c in U if c not in Uw and c not in Uv]
    A = sorted(tuple(int(p[c][f]) for f in fields) for c in U if p[c][W_TEAM] == TEAM_WEREWOLVES)
    B = sorted(tuple(int(p[c][f]) for f in fields) for c in U if p[c][W_TEAM] != TEAM_WEREWOLVES)
    SW, rem = list(Uw), list(Uq)
    for j in range(need):
        SW.append(rem.pop(pick(draw(vk, 32 + j), len(rem))))
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


def reference_rollout_seats(orc, room, seed: int, key: int, turn: int, seat: int, actions, n_rollouts: int, max_turns: int,
                            threads: int = 1):
    """(77 words, status) of entry (room, key, turn, seat, actions): refused -> 77 zero words and the refused action's status."""
    rec, st = inject_all(orc, room, actions)
    words = np.zeros(ROLLOUT_WORDS, dtype=np.uint64)
    if st != 0:
        return words, st
    copies = np.stack([redeal(orc, rec, seat, seed, key + r, turn) for r in range(n_rollouts)])
    if max_turns:
        orc.run(copies, seed, key, turn, max_turns, threads=threads, restart=False, human_mask=0)
    words[:41] = reference_summary_words([(orc.table, orc.n, copies)], key, turn + max_turns)
    words[41:] = seat_words(orc, copies)
    return words, st

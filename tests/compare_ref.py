"""Oracle-side reference of ge_batch_rollout_compare (tests only): POLICY.md §3e restated on oracle ROOM_DTYPE records - per entry
the copies after inject_all and rollout_seats_ref.redeal, played by the oracle as rollout_ref does, then the outcome X of every
replica for the entry's subject seat from the fields rollout_ref.seat_words reads, and the six sums of ge_compare_stats against
the baseline entry's copies."""
import numpy as np

from oracle.summary import reference_summary_words
from rollout_actions_ref import inject_all
from rollout_ref import ROLLOUT_WORDS, T_SCORE, TEAM_VILLAGERS, TEAM_WEREWOLVES, W_ALIVE, W_TEAM, seat_words
from rollout_seats_ref import redeal

COMPARE_WORDS = 6


def play_entry(orc, room, seed: int, key: int, turn: int, seat: int, actions, n_rollouts: int, max_turns: int, threads: int = 1):
    """(the n_rollouts played copies, 0) of entry (room, key, turn, seat, actions), or (None, the refused action's status)."""
    rec, st = inject_all(orc, room, actions)
    if st != 0:
        return None, st
    copies = np.stack([redeal(orc, rec, seat, seed, key + r, turn) for r in range(n_rollouts)])
    if max_turns:
        orc.run(copies, seed, key, turn, max_turns, threads=threads, restart=False, human_mask=0)
    return copies, 0


def entry_words(orc, copies, key: int, turn: int, max_turns: int) -> np.ndarray:
    words = np.zeros(ROLLOUT_WORDS, dtype=np.uint64)
    words[:41] = reference_summary_words([(orc.table, orc.n, copies)], key, turn + max_turns)
    words[41:] = seat_words(orc, copies)
    return words


def outcomes(orc, copies, subject: int) -> np.ndarray:
    """X(r) of every played copy for seat `subject` (1-based): Werewolf 1 if finished and the seat's team has won, else 0;
    Two-Truths the seat's total_score, finished or not."""
    s = subject - 1
    if orc.table.pack != 1:
        return copies["p"][:, s, T_SCORE].astype(np.int64)
    terminal = np.array([len(ph.branches) == 0 for ph in orc.table.phases])
    fin = terminal[copies["phase"]]
    n = orc.n
    alive = copies["p"][:, :n, W_ALIVE] != 0
    team = copies["p"][:, :n, W_TEAM]
    wolves = (alive & (team == TEAM_WEREWOLVES)).sum(axis=1)
    won = (fin & (wolves == 0) & (team[:, s] == TEAM_VILLAGERS)) | (fin & (wolves > 0) & (team[:, s] == TEAM_WEREWOLVES))
    return won.astype(np.int64)


def compare_sums(xk: np.ndarray, xb: np.ndarray) -> np.ndarray:
    d = xk - xb
    return np.array([len(d), (d > 0).sum(), (d < 0).sum(), d[d > 0].sum(), -d[d < 0].sum(), (d * d).sum()], dtype=np.uint64)


def reference_compare(orc_of, rooms, keys, turns, seats, actions, baseline, subjects, n_rollouts: int, max_turns: int, seed: int,
                      threads: int = 1):
    """(words (n, 77), status (n,), cmp (n, 6)) of one call.  orc_of(room) -> (oracle, that room's oracle record).  A refused
    entry has zero words; cmp[k] is zero when entry k or its baseline was refused."""
    n = len(rooms)
    words = np.zeros((n, ROLLOUT_WORDS), dtype=np.uint64)
    status = np.zeros(n, dtype=np.int32)
    played = []
    for k in range(n):
        orc, rec = orc_of(int(rooms[k]))
        copies, st = play_entry(orc, rec.copy(), seed, int(keys[k]), int(turns[k]), int(seats[k]), actions[k] if actions is not None else [],
                                n_rollouts, max_turns, threads)
        status[k] = st
        played.append(copies)
        if st == 0:
            words[k] = entry_words(orc, copies, int(keys[k]), int(turns[k]), max_turns)
    cmp = np.zeros((n, COMPARE_WORDS), dtype=np.uint64)
    for k in range(n):
        b = int(baseline[k])
        if played[k] is None or played[b] is None:
            continue
        orc, _ = orc_of(int(rooms[k]))
        cmp[k] = compare_sums(outcomes(orc, played[k], int(subjects[k])), outcomes(orc, played[b], int(subjects[k])))
    return words, status, cmp

"""Oracle-side reference of ge_batch_rollout_rooms (tests only): R copies of one oracle room played by the oracle under global
rooms key .. key + R - 1 (human mask 0, no restart), reduced to the 77 words of ge_rollout_stats."""
import numpy as np

from oracle.summary import reference_summary_words

ROLLOUT_WORDS = 77
TEAM_VILLAGERS, TEAM_WEREWOLVES = 1, 2
W_TEAM, W_ALIVE, T_SCORE = 1, 2, 7


def seat_words(orc, rooms: np.ndarray) -> np.ndarray:
    """seat_alive[12], seat_wins[12], seat_score[12] of finished-or-not oracle rooms (ge_step.h ge_rollout_stats)."""
    n = orc.n
    out = np.zeros(36, dtype=np.uint64)
    terminal = np.array([len(ph.branches) == 0 for ph in orc.table.phases])
    fin = terminal[rooms["phase"]]
    if orc.table.pack == 1:
        alive = rooms["p"][:, :n, W_ALIVE] != 0
        team = rooms["p"][:, :n, W_TEAM]
        wolves = (alive & (team == TEAM_WEREWOLVES)).sum(axis=1)
        village_won = fin & (wolves == 0)
        wolves_won = fin & (wolves > 0)
        out[0:n] = alive.sum(axis=0)
        out[12:12 + n] = ((village_won[:, None] & (team == TEAM_VILLAGERS)) | (wolves_won[:, None] & (team == TEAM_WEREWOLVES))).sum(axis=0)
    else:
        score = rooms["p"][:, :n, T_SCORE].astype(np.int64)
        top = score.max(axis=1)
        out[12:12 + n] = (fin[:, None] & (score == top[:, None])).sum(axis=0)
        out[24:24 + n] = score.sum(axis=0)
    return out


def reference_rollout(orc, room, seed: int, key: int, turn: int, n_rollouts: int, max_turns: int, threads: int = 1) -> np.ndarray:
    """The 77 words of entry (room, key, turn): `room` is one oracle ROOM_DTYPE record (left as it is)."""
    copies = np.repeat(np.asarray(room).reshape(1), n_rollouts)
    if max_turns:
        orc.run(copies, seed, key, turn, max_turns, threads=threads, restart=False, human_mask=0)
    words = np.zeros(ROLLOUT_WORDS, dtype=np.uint64)
    words[:41] = reference_summary_words([(orc.table, orc.n, copies)], key, turn + max_turns)
    words[41:] = seat_words(orc, copies)
    return words

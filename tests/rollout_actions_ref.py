"""Oracle-side reference of ge_batch_rollout_actions (tests only): the entry's actions logged by Oracle.inject in a copy of the
oracle room (every replica starts from that record), then R copies played by the oracle as rollout_ref does."""
import numpy as np

from oracle.summary import reference_summary_words
from rollout_ref import ROLLOUT_WORDS, seat_words

GE_ERR_ARG = -1


def inject_all(orc, room, actions):
    """(record after the actions, GE_OK) or (None, the refused action's status): actions apply in order, as the device does."""
    one = np.asarray(room).reshape(1).copy()
    for player, choice in actions:
        if not orc.inject(one, 0, int(player), int(choice)):
            return None, GE_ERR_ARG
    return one[0], 0


def reference_rollout_actions(orc, room, seed: int, key: int, turn: int, actions, n_rollouts: int, max_turns: int, threads: int = 1):
    """(77 words, status) of entry (room, key, turn, actions): refused -> 77 zero words and the refused action's status."""
    rec, st = inject_all(orc, room, actions)
    words = np.zeros(ROLLOUT_WORDS, dtype=np.uint64)
    if st != 0:
        return words, st
    copies = np.repeat(rec.reshape(1), n_rollouts)
    if max_turns:
        orc.run(copies, seed, key, turn, max_turns, threads=threads, restart=False, human_mask=0)
    words[:41] = reference_summary_words([(orc.table, orc.n, copies)], key, turn + max_turns)
    words[41:] = seat_words(orc, copies)
    return words, st

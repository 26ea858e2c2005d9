"""Reference of ge_batch_gather_seats and ge_batch_act_listed (POLICY.md §3q; tests only): the two composition rules as code.  The
list is a numpy filter over the dense records ge_batch_observe_seats stores (observe_ref restates those on the oracle); the act
rule builds the dense choice array D of ge_batch_act_seats from a list."""
import numpy as np

SEAT, END = 1, 2                                 # GE_GATHER_SEAT, GE_GATHER_END
WANTS = [SEAT, END, SEAT | END]
GE_ERR_ARG = -1


def due(records, want):
    """bool, the shape of `records` (SEAT_OBS_DTYPE): the entry is due under `want`"""
    d = np.zeros(records.shape, dtype=bool)
    if want & SEAT:
        d |= records["legal"] != 0
    if want & END:
        d |= records["done"] != 0
    return d


def gather(records, want, cap=None):
    """records [count, n_seats] -> (the list's records, their entry indices as uint32, n = [min(M, cap), M] as uint32)"""
    flat = records.reshape(-1)
    e = np.flatnonzero(due(flat, want)).astype(np.uint32)
    m = len(e)
    kept = m if cap is None else min(m, cap)
    return flat[e[:kept]], e[:kept], np.array([kept, m], dtype=np.uint32)


def dense_choices(total, n_word, cap, entries, choices):
    """The D of ge_batch_act_listed: `total` zeros except D[entries[i]] = choices[i] for i < min(n_word, cap) with entries[i] <
    total (an entry named twice: the reference takes the last copy - the call promises only one of them, so tests that compare
    against D name no entry twice with different choices)."""
    d = np.zeros(total, dtype=np.int32)
    n = min(int(n_word), int(cap))
    for i in range(n):
        if entries[i] < total:
            d[entries[i]] = choices[i]
    return d


def listed_status(dense_status, total, n_word, cap, entries, fill):
    """status_dev as the call leaves it: the dense call's status at each listed entry, GE_ERR_ARG for an entry at or above total,
    `fill` (what the buffer held) behind the list"""
    out = np.array(fill, dtype=np.int32).copy()
    n = min(int(n_word), int(cap))
    flat = np.asarray(dense_status).reshape(-1)
    for i in range(n):
        out[i] = flat[entries[i]] if entries[i] < total else GE_ERR_ARG
    return out

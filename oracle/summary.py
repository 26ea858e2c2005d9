"""SUMMARY REFERENCE (test infrastructure) — ge_summary (include/ge_step.h) computed on the host from oracle rooms.

`reference_summary_words(segments, first_global, turn)` returns the 41 words ge_batch_summary returns for a batch whose
segments are given as (oracle `Table`, n_players, oracle rooms ROOM_DTYPE), segment-major, the first room of the first
segment having global index `first_global`.  Every word follows the definitions in include/ge_step.h:
  rooms            rooms of the batch
  finished         rooms in a terminal phase: the oracle compiler's phase has no branch (not `end_turn >= 0`)
  village / wolf   Werewolf rooms only: finished with no / some wolf (team_w) alive
  alive_players    Werewolf: alive seats; Two-Truths: n_players per room (the kernel counts every seat: nobody dies there)
  sum_end_turn     over finished rooms whose end_turn is set; a terminal room without one (a written state) adds nothing,
  end_turn_hist      and is in no bucket of the end_turn histogram.  Bucket end_turn // 8, the last one open
  score_hist       Two-Truths: players by total_score, bucket min(score, 15)
  checksum         sum over rooms of the hash of (global room index, canonical packed record)
  turn             `turn`
  games_recycled   sum of `games`
Sums wrap mod 2^64, as on the device.

The packed records are restated here from the layout comments of game_engine_amd/csrc/ge_layout.h, independently of the
product's pack functions (tests/test_summary_reference.py checks them against the product's view_to_words): flags carry
phase0_done and the effect of the previous phase's row, bits of absent seats are 0, and the Werewolf x 8 prepared-deal
cache (word 7, upper half) is the only field left out - it is a cache, not state.

Only tests import this module; the product and bench.py do not.
"""
from __future__ import annotations

from typing import Iterable, Tuple

import numpy as np

from . import dsl_table as T

SUMMARY_WORDS = 41
W_ROOMS, W_FINISHED, W_VILLAGE, W_WOLF, W_ALIVE, W_SUM_END = 0, 1, 2, 3, 4, 5
W_END_HIST, W_SCORE_HIST, W_CHECKSUM, W_TURN, W_GAMES = 6, 22, 38, 39, 40

K_WW8, K_WW12, K_TT4, K_TT8, K_TT12 = range(5)
WORDS = {K_WW8: 8, K_WW12: 10, K_TT4: 6, K_TT8: 8, K_TT12: 12}
END_NONE = 0xFFFF
CHUNK = 1 << 17                      # rooms per part of host work (one thread each)

_U32 = np.uint32


def kind_of(pack: int, n: int) -> int:
    """The record layout of a segment (ge_step.hip create: Werewolf N <= 8 / <= 12, Two-Truths N <= 4 / <= 8 / <= 12)."""
    if pack == T.PACK_WEREWOLF:
        return K_WW8 if n <= 8 else K_WW12
    return K_TT4 if n <= 4 else (K_TT8 if n <= 8 else K_TT12)


def mix32(x) -> np.ndarray:
    """The 32-bit finaliser of ge_device.h, elementwise (uint32 arithmetic wraps)."""
    x = np.array(x, dtype=_U32, copy=True, ndmin=1)
    x ^= x >> _U32(16)
    x *= _U32(0x7FEB352D)
    x ^= x >> _U32(15)
    x *= _U32(0x846CA68B)
    x ^= x >> _U32(16)
    return x


def _mask(cond: np.ndarray, present: np.ndarray) -> np.ndarray:
    """[R, 12] booleans -> one bit per seat (seat i = bit i), absent seats 0."""
    on = (cond & present).astype(_U32)
    return (on << np.arange(12, dtype=_U32)).sum(axis=1, dtype=_U32)


def _fields(vals: np.ndarray, present: np.ndarray, bits: int, seats: range) -> np.ndarray:
    """[R, 12] small integers -> `bits` bits per seat of `seats`, seat seats[0] lowest (uint64)."""
    out = np.zeros(len(vals), dtype=np.uint64)
    m = (1 << bits) - 1
    for k, i in enumerate(seats):
        v = (vals[:, i].astype(np.uint64) & np.uint64(m)) * present[:, i]
        out |= v << np.uint64(bits * k)
    return out


def pack_records(kind: int, rooms: np.ndarray, table: T.Table) -> np.ndarray:
    """Oracle rooms -> the canonical packed records [R, WORDS[kind]] uint32 of ge_layout.h (deal cache 0)."""
    R = len(rooms)
    p = rooms["p"][:, :12, :]
    present = np.arange(12)[None, :] < rooms["n"].astype(np.int64)[:, None]
    effect = np.array([ph.effect for ph in table.phases], dtype=_U32)
    phase, prev = rooms["phase"].astype(_U32), rooms["prev"].astype(_U32)
    flags = (rooms["phase0_done"] != 0).astype(_U32) | (effect[prev] << _U32(1))
    et = rooms["end_turn"]
    end = np.where(et < 0, END_NONE, et & 0xFFFF).astype(_U32)
    games = (rooms["games"] & 0xFFFF).astype(_U32)
    w = np.zeros((R, WORDS[kind]), dtype=_U32)

    def u(x):
        return np.asarray(x, dtype=np.uint64).astype(_U32)

    if kind in (K_WW8, K_WW12):
        role, team, det = p[:, :, 0], p[:, :, 1], rooms["det"][:, :12]
        alive, revealed, can_vote, secret = (_mask(p[:, :, k] != 0, present) for k in (2, 3, 4, 5))
        elig, sub, acted = (_mask(p[:, :, k] != 0, present) for k in (6, 7, 9))
        team_v, team_w = _mask(team == 1, present), _mask(team == 2, present)
        det_v, det_w = _mask(det == 1, present), _mask(det == 2, present)
        if kind == K_WW8:
            vil, wolf, doc, dete = (_mask(role == c, present) for c in (1, 2, 3, 4))     # role classes one-hot
            sel = u(_fields(p[:, :, 8], present, 4, range(8)))
            choice = u(_fields(p[:, :, 10], present, 4, range(8)))
            w[:, 0] = alive | can_vote << 8 | revealed << 16 | secret << 24
            w[:, 1] = elig | sub << 8 | team_v << 16 | team_w << 24
            w[:, 2] = vil | wolf << 8 | doc << 16 | dete << 24
            w[:, 3] = det_v | det_w << 8 | phase << 16 | prev << 24
            w[:, 4], w[:, 5] = sel, choice
            w[:, 6] = end | flags << 16 | acted << 24
            w[:, 7] = games
        else:
            rb0, rb1, rb2 = (_mask((role & b) != 0, present) for b in (1, 2, 4))         # role class as bit-planes
            sel = _fields(p[:, :, 8], present, 4, range(12))
            choice = _fields(p[:, :, 10], present, 4, range(12))
            w[:, 0] = alive | can_vote << 12 | phase << 24
            w[:, 1] = revealed | secret << 12 | prev << 24
            w[:, 2] = elig | sub << 12 | flags << 24
            w[:, 3] = team_v | team_w << 12 | (end & 0xFF) << 24
            w[:, 4] = acted | rb0 << 12 | (end >> 8) << 24
            w[:, 5] = rb1 | rb2 << 12 | (games & 0xFF) << 24
            w[:, 6] = det_v | det_w << 12 | (games >> 8) << 24
            w[:, 7] = u(sel & np.uint64(0xFFFFFFFF))
            w[:, 8] = u(choice & np.uint64(0xFFFFFFFF))
            w[:, 9] = u(sel >> np.uint64(32)) | u(choice >> np.uint64(32)) << 16
        return w

    speaker, submitted, revealed, can_vote, has_voted, acted = (_mask(p[:, :, k] != 0, present) for k in (0, 1, 3, 4, 6, 9))
    lie = u(_fields(p[:, :, 2], present, 2, range(12)))
    vote = u(_fields(p[:, :, 5], present, 2, range(12)))
    choice = u(_fields(p[:, :, 10], present, 2, range(12)))
    rounds = _fields(p[:, :, 8], present, 4, range(12))
    score = [u(_fields(p[:, :, 7], present, 8, range(4 * j, 4 * j + 4))) for j in range(3)]
    if kind == K_TT4:
        w[:, 0] = speaker | submitted << 4 | revealed << 8 | can_vote << 12 | has_voted << 16 | acted << 20 | phase << 24
        w[:, 1] = lie | vote << 8 | choice << 16 | prev << 24
        w[:, 2] = score[0]
        w[:, 3] = u(rounds) | end << 16
        w[:, 4] = flags | games << 16
    elif kind == K_TT8:
        w[:, 0] = speaker | submitted << 8 | revealed << 16 | can_vote << 24
        w[:, 1] = has_voted | acted << 8 | phase << 16 | prev << 24
        w[:, 2] = lie | vote << 16
        w[:, 3] = choice | end << 16
        w[:, 4], w[:, 5] = score[0], score[1]
        w[:, 6] = u(rounds)
        w[:, 7] = flags | games << 16
    else:
        w[:, 0] = speaker | submitted << 12 | phase << 24
        w[:, 1] = revealed | can_vote << 12 | prev << 24
        w[:, 2] = has_voted | acted << 12 | flags << 24
        w[:, 3] = lie | (end & 0xFF) << 24
        w[:, 4] = vote | (end >> 8) << 24
        w[:, 5] = choice
        w[:, 6], w[:, 7], w[:, 8] = score
        w[:, 9] = u(rounds & np.uint64(0xFFFFFFFF))
        w[:, 10] = u(rounds >> np.uint64(32)) | games << 16
    return w


def room_hashes(records: np.ndarray, first_global: int) -> np.ndarray:
    """Each room's 64-bit checksum term: h0 = mix32(lo32(g) ^ mix32(hi32(g) ^ 0xA5A5A5A5)), h = mix32(h ^ w[j]) over the
    record's words, term = h | mix32(h ^ 0x5BD1E995) << 32 (ge_kernels.inl ge_summary_kernel)."""
    g = np.uint64(first_global) + np.arange(len(records), dtype=np.uint64)
    lo = (g & np.uint64(0xFFFFFFFF)).astype(_U32)
    hi = (g >> np.uint64(32)).astype(_U32)
    h = mix32(lo ^ mix32(hi ^ _U32(0xA5A5A5A5)))
    for j in range(records.shape[1]):
        h = mix32(h ^ records[:, j])
    return h.astype(np.uint64) | (mix32(h ^ _U32(0x5BD1E995)).astype(np.uint64) << np.uint64(32))


def _part_words(table: T.Table, n: int, r: np.ndarray, first_global: int) -> np.ndarray:
    """The summary words (turn 0) of consecutive rooms r with global indices first_global.."""
    words = np.zeros(SUMMARY_WORDS, dtype=np.uint64)
    terminal = np.array([len(ph.branches) == 0 for ph in table.phases])
    rec = pack_records(kind_of(table.pack, n), r, table)
    fin = terminal[r["phase"]]
    end = np.where(r["end_turn"] < 0, END_NONE, r["end_turn"] & 0xFFFF).astype(np.int64)   # the record's 16 bits
    ended = fin & (end != END_NONE)          # a terminal room whose end_turn is unset adds no end turn
    words[W_ROOMS] = len(r)
    words[W_FINISHED] = fin.sum()
    if table.pack == T.PACK_WEREWOLF:
        alive = (r["p"][:, :12, 2] != 0) & (np.arange(12)[None, :] < n)
        wolves = (alive & (r["p"][:, :12, 1] == 2)).sum(axis=1)
        words[W_VILLAGE] = (fin & (wolves == 0)).sum()
        words[W_WOLF] = (fin & (wolves > 0)).sum()
        words[W_ALIVE] = alive.sum()
    else:
        words[W_ALIVE] = n * len(r)
        score = r["p"][:, :n, 7].astype(np.int64).ravel()
        words[W_SCORE_HIST:W_SCORE_HIST + 16] = np.bincount(np.minimum(score, 15), minlength=16)
    words[W_SUM_END] = end[ended].sum()
    words[W_END_HIST:W_END_HIST + 16] = np.bincount(np.minimum(end[ended] >> 3, 15), minlength=16)
    words[W_CHECKSUM] = room_hashes(rec, first_global).sum(dtype=np.uint64)
    words[W_GAMES] = (r["games"] & 0xFFFF).sum()
    return words


def add_rooms(words: np.ndarray, table: T.Table, n: int, rooms: np.ndarray, first_global: int) -> np.ndarray:
    """Adds rooms [0, len) with global indices first_global.. (one segment's, or a consecutive part of one) to `words`.
    Parts of CHUNK rooms on a few threads (numpy releases the GIL inside its loops)."""
    from concurrent.futures import ThreadPoolExecutor
    from .oracle import usable_cores
    starts = range(0, len(rooms), CHUNK)
    with ThreadPoolExecutor(max_workers=max(1, min(8, usable_cores(), len(starts)))) as ex:
        parts = list(ex.map(lambda lo: _part_words(table, n, rooms[lo:lo + CHUNK], first_global + lo), starts))
    with np.errstate(over="ignore"):
        for part in parts:
            words += part
    return words


def reference_summary_words(segments: Iterable[Tuple[T.Table, int, np.ndarray]], first_global: int, turn: int) -> np.ndarray:
    """ge_summary of a batch as 41 uint64 words (the layout of RoomBatch.summary_words)."""
    words = np.zeros(SUMMARY_WORDS, dtype=np.uint64)
    g = first_global
    for table, n, rooms in segments:
        add_rooms(words, table, n, rooms, g)
        g += len(rooms)
    words[W_TURN] = np.uint64(turn)
    return words

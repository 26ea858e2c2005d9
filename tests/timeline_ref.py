"""Reference of ge_batch_run_rooms_forecast (POLICY.md §3i), restated on the oracle by composition: run_ref.reference_call
supplies the run, and for point p = 0 .. played[k] of entry k rollout_seats_ref.reference_rollout_seats is applied to a copy of
the oracle room as it stood there - point 0 the room before the call, point p >= 1 the room of views[k][p - 1] - under
(forecast key, turns[k] + p, seat, no actions; n_rollouts, playout_max_turns, the playouts' seed)."""
import numpy as np

from parity_util import views_as_oracle_rooms
from rollout_seats_ref import reference_rollout_seats
from run_ref import reference_call


def point_rooms(orc, start, views):
    """The oracle rooms of an entry's points: `start` (point 0), then the room of each played turn's view."""
    pts = [np.asarray(start).reshape(1).copy()[0]]
    if len(views):
        pts += list(views_as_oracle_rooms(orc, np.array(views).reshape(-1)))
    return pts


def timeline_of(orc, start, views, fseed, fkey, turn, seat, n_rollouts, playout_max_turns):
    """(played + 1, 77) words: the forecast of every point of one entry."""
    out = []
    for p, room in enumerate(point_rooms(orc, start, views)):
        words, st = reference_rollout_seats(orc, room.copy(), fseed, int(fkey), int(turn) + p, int(seat), [], n_rollouts, playout_max_turns)
        assert st == 0
        out.append(words)
    return np.stack(out)


def reference_timeline(segs, listed, keys, turns, max_turns, until, restart, fkeys, seats, n_rollouts, playout_max_turns, fseed):
    """reference_call's (played, stopped, events, views, rooms after) and stats: per entry a (played + 1, 77) array."""
    played, stopped, events, views, after = reference_call(segs, listed, keys, turns, max_turns, until, restart)
    per = len(segs[0][4])
    stats = []
    for k, r in enumerate(listed):
        s, i = divmod(int(r), per)
        orc, _, _, _, rooms = segs[s]
        stats.append(timeline_of(orc, rooms[i], views[k], fseed, fkeys[k], turns[k], seats[k], n_rollouts, playout_max_turns))
    return played, stopped, events, views, after, stats


# ---- shared inputs of tests/test_timeline_host.py and tests/test_gpu_timeline.py: 6 entries per segment of run_ref.case_inputs at 48
# rooms per segment, the two (max_turns, until) shapes, 70 playouts (one full wavefront and one of 6 lanes) of at most 48 turns
PER_SEGMENT, ROOMS_PER_SEGMENT, N_ROLLOUTS, PLAYOUT_MAX_TURNS, FSEED = 6, 48, 70, 48, 0x54494D45
SHAPES = ((5, 0), (40, 3))                                      # (max_turns, until): no condition; PERSON | END
W_IS_ALIVE = 2


def timeline_inputs(name, restart):
    """(segs, listed, keys, turns, forecast keys, seats): the first 6 listed rooms of every segment of the case; entry 0 keeps the
    last turns a room can take in these calls; seats alternate between 0 and a living seat that no person plays."""
    from run_ref import case_inputs
    segs, listed, keys, turns = case_inputs(name, ROOMS_PER_SEGMENT, restart)
    turns = np.minimum(turns, np.uint32(0xFFFFFFFF - max(m for m, _ in SHAPES) - PLAYOUT_MAX_TURNS))
    take, seen = [], [0] * len(segs)
    for k, r in enumerate(listed):
        s = int(r) // ROOMS_PER_SEGMENT
        if seen[s] < PER_SEGMENT:
            seen[s] += 1
            take.append(k)
    listed, keys, turns = listed[take], keys[take], turns[take]
    rng = np.random.default_rng(len(name) + 7 * int(restart))
    fkeys = (rng.integers(1, 1 << 40, len(listed)).astype(np.uint64) << np.uint64(16))
    seats = np.zeros(len(listed), dtype=np.uint32)
    for k, r in enumerate(listed):
        s, i = divmod(int(r), ROOMS_PER_SEGMENT)
        orc, _, n, mask, rooms = segs[s]
        ok = [c + 1 for c in range(n) if not (mask >> c) & 1 and (orc.table.pack != 1 or rooms[i]["p"][c][W_IS_ALIVE])]
        if k % 2 and ok:
            seats[k] = ok[(k // 2) % len(ok)]
    return segs, listed, keys, turns, fkeys, seats

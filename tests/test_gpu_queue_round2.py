"""GPU parity (-m gpu) of the fused lone-wavefront Werewolf x 8 turn where a wavefront's due actions cross one and two rounds of its
action queue (ge_device.h ww_queue_actions): the turn that needs a second round is a path of its own there, a third and later round
runs the loop over rounds behind it, and the one-round turn no longer looks at the total.  The tests pin results, not a build: they
pass on the loop form as well.

What can go wrong is at the totals 64 | 65 and 128 | 129 of one wavefront's turn, and where a room's run of slots straddles
63 | 64 or 127 | 128 (the pull queue finds a slot's owner by counting head words, and the count crosses the rounds).  Such totals do
not come up on demand from the initial state, so the batches here are assembled: rooms of an oracle timeline, each with a known
number of due seats (seats_ref.pending_of: the oracle's own test), are put together 64 to a wavefront so that the counts of a
wavefront's lanes sum to the wanted total in the wanted order, written with RoomBatch.write_rooms and stepped 2 and 3 fused turns
(a turn of the loop and the peeled last turn).  A second set of wavefronts is assembled from rooms that have nobody due now and a
known number due one turn later (a phase without actions is left the same way under every key), so that the classes also fall on
the turn behind the first - the last turn of a launch of 2, which is a copy of its own in the kernel.  Which wavefront-turn has
which total is then worked out again from the oracle's stepped rooms, and asserted, before anything is compared with the GPU.

A wavefront holds 64 rooms of a single-game batch only from 65 536 rooms on (below, a fused launch spreads the rooms over more
wavefronts), so the single-game cases are 65 536 rooms: the assembled wavefronts in front, timeline rooms behind.  A batch of
several segments always runs 64 lanes per wavefront: the two-segment case is small.
Against the oracle: every room's whole view and the summary words behind every launch and, traced, every turn's events.  Integer
path: bit-exact."""
import functools

import numpy as np
import pytest

from conftest import load_dsl
from game_engine_amd import GameTable, RoomBatch
from parity_util import assert_summary_equal, assert_views_equal, oracle_events, oracle_rooms_as_views
from seats_ref import pending_of

pytestmark = pytest.mark.gpu
WW, N, SEED, FIRST, FUSE = "werewolf-(mafia)", 8, 0x20D2B07, 52000, 256
ALL = (1 << N) - 1
ROOMS = 65536                                              # 1 024 wavefronts of 64 rooms
T0 = 40                                                    # the assembled batches start at this turn (the keys and the head stamps follow it)
HUMANS = 0b00100100                                        # players 3 and 6
POOL_ROOMS, POOL_TURNS = 48, 40

# lanes' due counts per assembled wavefront, in lane order (the rest of the 64 lanes: rooms with nobody due); name -> (counts, total)
WAVES = {
    "below64": [8, 7, 5, 1, 8, 2, 7],                      # 38
    "exactly64": [8] * 8,
    "exactly65": [8] * 8 + [1],
    "straddle64_by8": [8] * 7 + [5, 8, 2],                 # slots 61 .. 68 are one room's: 71
    "straddle64_by7": [8] * 7 + [4, 7, 7],                 # slots 60 .. 66: 74
    "exactly128": [8] * 16,
    "exactly129": [8] * 16 + [1],
    "straddle128_by8": [8] * 15 + [5, 8, 8, 4],            # slots 125 .. 132: 145
    "straddle128_by7": [7] * 9 + [8] * 7 + [5, 7, 8],      # 63 + 56 = 119, + 5 = 124: slots 124 .. 130; and 63 | 64 is a boundary between rooms
    "straddle_both": [8] * 7 + [7, 8] + [8] * 6 + [6, 8],  # slots 63 .. 70 and 125 .. 132
}
ORDER = sorted(WAVES)


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle.oracle import Oracle
    return Oracle(load_dsl(WW), N)


def _due(one, mask=ALL):
    return bin(pending_of(_oracle(), one, mask)).count("1")


@functools.lru_cache(maxsize=None)
def _pool():
    """Rooms of a timeline from the initial state, by their number of due seats: now[d] = rooms with d seats due, and nxt[d] = rooms
    in a phase without actions (nobody due, no draw taken in the turn) that have d seats due one turn later.  Read-only."""
    orc = _oracle()
    cur = orc.init_rooms(POOL_ROOMS)
    now, nxt = {}, {}
    for t in range(POOL_TURNS):
        before = cur.copy()
        d0 = [_due(before[i:i + 1]) for i in range(POOL_ROOMS)]
        orc.run(cur, SEED, FIRST, t, 1, threads=1, restart=True)
        for i in range(POOL_ROOMS):
            if before["phase0_done"][i] == 0 or before["end_turn"][i] >= 0:
                continue                                   # (the guard turn and finished rooms: left out, the timeline rooms behind have them)
            now.setdefault(d0[i], []).append(before[i:i + 1].copy())
            if d0[i] == 0 and cur["end_turn"][i] < 0:
                nxt.setdefault(_due(cur[i:i + 1]), []).append(before[i:i + 1].copy())
    return now, nxt


def _assemble(bucket, counts, salt):
    """64 rooms whose due counts are `counts` in lane order, then rooms of count 0; different rooms of a bucket by `salt`"""
    out = []
    for lane in range(64):
        d = counts[lane] if lane < len(counts) else 0
        have = bucket[d]
        out.append(have[(salt * 7 + lane * 3) % len(have)])
    return np.concatenate(out)


@functools.lru_cache(maxsize=None)
def _start(n_rooms=ROOMS):
    """The assembled batch: wavefront w < len(ORDER) has the totals of ORDER[w] on its first turn, wavefront len(ORDER) + w one turn
    later; timeline rooms behind.  Read-only."""
    now, nxt = _pool()
    waves = [_assemble(now, WAVES[k], w) for w, k in enumerate(ORDER)] + [_assemble(nxt, WAVES[k], w) for w, k in enumerate(ORDER)]
    flat = np.concatenate(waves)
    filler = np.concatenate([r for d in sorted(now) for r in now[d]])
    rooms = np.concatenate([flat, np.resize(filler, n_rooms - len(flat))]) if n_rooms > len(flat) else flat[:n_rooms].copy()
    rooms.setflags(write=False)
    return rooms


@functools.lru_cache(maxsize=3)                            # (a setting's run is 100 MB)
def _timeline(restart, human_mask, n_turns=5, first=FIRST, n_rooms=ROOMS, lo=0):
    """The oracle's run of rooms lo .. of the assembled batch from T0 on: rooms[t] behind t turns, events[t] of turn T0 + t.  Read-only."""
    orc = _oracle()
    cur = _start()[lo:lo + n_rooms].copy()
    rooms, events = [cur.copy()], []
    for t in range(n_turns):
        orc.run(cur, SEED, first + lo, T0 + t, 1, threads=0, restart=restart, human_mask=human_mask)
        events.append(oracle_events(orc, cur, T0 + t))
        rooms.append(cur.copy())
    for a in (*rooms, *events):
        a.setflags(write=False)
    return rooms, events


def _totals(rooms_t, mask=ALL, waves=2 * len(WAVES)):
    """per assembled wavefront: its lanes' due counts before the turn that `rooms_t` stands in front of"""
    return [[_due(rooms_t[64 * w + lane:64 * w + lane + 1], mask) for lane in range(64)] for w in range(waves)]


def _classes(counts):
    """the classes of one wavefront-turn, from its lanes' due counts"""
    total, off, out = sum(counts), 0, set()
    out.add("<=64" if total <= 64 else "65..128" if total <= 128 else ">=129")
    if total in (64, 65, 128, 129):
        out.add(f"={total}")
    for c in counts:
        for edge in (64, 128):
            if off < edge < off + c and total > edge:
                out.add(f"straddle{edge}_by{c}")
        off += c
    return out


WANTED = {"<=64", "=64", "=65", "65..128", ">=129", "=128", "=129", "straddle64_by8", "straddle64_by7", "straddle128_by8", "straddle128_by7"}


@functools.lru_cache(maxsize=None)
def _checked_inputs():
    """From the oracle alone: the first turn (a turn of the loop in a launch of 2 or 3) and the second (the last turn of a launch of 2)
    each hold every class"""
    rooms, events = _timeline(True, 0)
    for turn in (0, 1):
        per_wave = _totals(rooms[turn])
        got = set().union(*(_classes(c) for c in per_wave))
        assert WANTED <= got, f"turn {turn} of the assembled batch lacks {sorted(WANTED - got)}; totals {[sum(c) for c in per_wave]}"
        # what acts is a subset of what was due (the oracle's events of that turn)
        for w, c in enumerate(per_wave):
            acted = sum(bin(int(x)).count("1") for x in events[turn]["acted_now"][64 * w:64 * w + 64])
            assert acted <= sum(c)
    # more than two rounds really run the second round's owners: of a wavefront of 145 due, more than 64 act
    w = ORDER.index("straddle128_by8")
    assert sum(bin(int(x)).count("1") for x in events[0]["acted_now"][64 * w:64 * w + 64]) > 64
    return True


def _check(b, state, what, first=FIRST):
    from oracle.summary import reference_summary_words
    orc = _oracle()
    assert_views_equal(b.read_rooms(), oracle_rooms_as_views(orc, state), what)
    assert_summary_equal(b.summary_words(), reference_summary_words([(orc.table, orc.n, state)], first, b.turn), what)


def _run(plan, restart=True, trace=False, human_mask=0):
    assert _checked_inputs()
    rooms, events = _timeline(restart, human_mask)
    what = f"restart={restart}, trace={trace}, humans={human_mask:#x}, launches {plan}"
    orc = _oracle()
    with RoomBatch([(GameTable(load_dsl(WW)), N, ROOMS, human_mask)], seed=SEED, first_room=FIRST, max_fuse=FUSE, restart=restart, trace=trace) as b:
        b.write_rooms(0, oracle_rooms_as_views(orc, rooms[0]))
        b.set_turn(T0)
        done = 0
        for k in plan:
            b.step(k)
            assert b.turn == T0 + done + k
            if trace:
                ev = b.read_events()
                assert ev.shape == (ROOMS, k)
                for t in range(k):
                    assert ev[:, t].tobytes() == events[done + t].tobytes(), f"{what}: events of turn {T0 + done + t} differ"
            done += k
            _check(b, rooms[done], f"{what}: behind {done} turns")


def test_the_assembled_wavefronts_hold_every_class():
    """(the oracle alone) and the buckets they are assembled from have rooms of seven and of eight due seats, now and one turn later"""
    now, nxt = _pool()
    assert {1, 2, 4, 5, 6, 7, 8} <= set(now) and {1, 2, 4, 5, 6, 7, 8} <= set(nxt), (sorted(now), sorted(nxt))
    assert _checked_inputs()


@pytest.mark.parametrize("plan", [(2,), (3,), (2, 3)], ids=["2", "3", "2+3"])
def test_rooms_equal_the_oracle(plan):
    """a launch of 2 (one turn of the loop, the peeled last turn), of 3, and two launches: the head stamps go on where the first stopped"""
    _run(plan)


def test_restart_off():
    _run((2, 3), restart=False)


def test_traced():
    _run((2, 3), trace=True)


def test_host_driven_seats():
    """players 3 and 6 of every room are left to people who never act: never queued - the totals are other totals (a room has six
    seats to be due at most), within one round, within two and past two in some wavefront-turn of the first two turns (the oracle
    alone, first)"""
    rooms, _ = _timeline(True, HUMANS)
    totals = [sum(c) for turn in (0, 1) for c in _totals(rooms[turn], ALL & ~HUMANS)]
    assert min(totals) <= 64 and any(64 < t <= 128 for t in totals) and max(totals) > 128, totals
    _run((2, 3), human_mask=HUMANS)


def test_two_segments_whose_boundary_falls_inside_a_wavefront():
    """the mixed lone kernel: 96 + 1 184 rooms as two segments of one batch.  The first segment's second wavefront ends in lanes past its
    end; the second segment starts a wavefront of its own, so its rooms are the assembled batch's from room 128 on, lane for lane"""
    assert _checked_inputs()
    orc, tb = _oracle(), GameTable(load_dsl(WW))
    sizes, starts = (96, 64 * 2 * len(WAVES) - 128), (0, 128)   # (rooms 96 .. 127 of the assembled batch are not in this one)
    lines = [_timeline(True, 0, first=FIRST + lo - at, n_rooms=r, lo=at) for r, lo, at in zip(sizes, (0, 96), starts)]
    per_wave = _totals(lines[1][0][0], waves=sizes[1] // 64)
    got = set().union(*(_classes(c) for c in per_wave))
    assert {"=65", "straddle64_by7", "straddle64_by8", "straddle128_by7", "straddle128_by8"} <= got, sorted(got)
    with RoomBatch([(tb, N, r) for r in sizes], seed=SEED, first_room=FIRST, max_fuse=FUSE, restart=True) as b:
        b.write_rooms(0, oracle_rooms_as_views(orc, np.concatenate([ln[0][0] for ln in lines])))
        b.set_turn(T0)
        done = 0
        for k in (2, 3):
            b.step(k)
            done += k
            got_rooms, lo = b.read_rooms(), 0
            for r, ln in zip(sizes, lines):
                assert_views_equal(got_rooms[lo:lo + r], oracle_rooms_as_views(orc, ln[0][done]), f"segment of {r} rooms at {lo}, behind {done} turns")
                lo += r

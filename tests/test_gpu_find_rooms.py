"""ge_batch_find_rooms (-m gpu): the device scan of a resident batch against tests/find_ref.py (the definition restated on the
oracle), hit for hit and in order - every layout and table kind, segment sizes at the wavefront's edges, windows inside a
wavefront and across segments -, truncation and resumption, `pending` against what inject_actions accepts on the GPU, that the
call only reads, a range beyond one pass of the scan kernel, the refusals in their order, and both hosts' forms of the call."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from find_ref import FIND_CASES, case_facts, expected_hits, hits_as_tuples
from game_engine_amd import GameTable, GeError, RoomBatch
from game_engine_amd.stepper import ROOM_HIT_DTYPE
from parity_util import oracle_rooms_as_views
from run_ref import END, PERSON, PHASE, SEED

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE_DIR = os.path.join(ROOT, "game_engine_amd", "node")
GE_ERR_ARG, GE_ERR_RANGE = -1, -6
SIZES = (1, 63, 64, 65, 130)       # rooms per segment: the wavefront's edge, one past it, a third wavefront partly filled
_U64P = C.POINTER(C.c_uint64)
_TABLES = {}


def _table(dsl):
    key = id(dsl)
    if key not in _TABLES:
        _TABLES[key] = (GameTable(dsl), dsl)                     # (the dsl is kept alive: its id is the key)
    return _TABLES[key][0]


def _batch(segs, restart, max_fuse=1, trace=False):
    """The start rooms written as views."""
    b = RoomBatch([(_table(dsl), n, len(rooms), mask) for _, dsl, n, mask, rooms in segs], seed=SEED, first_room=777,
                  max_fuse=max_fuse, restart=restart, trace=trace)
    base = 0
    for orc, _, _, _, rooms in segs:
        b.write_rooms(base, oracle_rooms_as_views(orc, rooms))
        base += len(rooms)
    return b


def _half_masks(segs, rng):
    """A random half of each segment's table's phase ids, as the call's mask words (ids a mask word can name: the shipped tables'
    terminal phases have ids of 98 and 99, which GE_FIND_END finds)."""
    masks = []
    for orc, _, _, _, _ in segs:
        ids = [p for p in orc.ids if p < len(orc.ids)]
        masks.append(sum(1 << int(p) for p in rng.choice(ids, size=len(ids) // 2, replace=False)))
    return masks


def _phases_arg(masks):
    return {g: [p for p in range(32) if (m >> p) & 1] for g, m in enumerate(masks)}


def _windows(per, n_seg):
    total = per * n_seg
    w = [(0, total), (5, 50), (60, 10), (63, 2), (1, total - 2), (70, 59), (total - 1, 1)]
    for k in range(1, n_seg):                                    # across each segment boundary (and the padding of the result words)
        w += [(k * per - 3, 7), (k * per - 1, 2), (k * per, 1), (max(0, k * per - 70), 140)]
    if n_seg > 1:
        w.append((per - 2, total - 2 * per + 4))                 # from the first segment's end into the last one
    return sorted({(f, c) for f, c in w if f >= 0 and c > 0 and f + c <= total})


@pytest.mark.parametrize("restart", [False, True])
@pytest.mark.parametrize("name", FIND_CASES)
def test_find_rooms_equals_the_reference_hit_for_hit(name, restart):
    assert _check_find_rooms(name, restart, SIZES) > 0


# the GENERIC builds of the Two-Truths x 8 and x 12 test, which no case above launches: 193 rooms - three full wavefronts and one
# with a single live lane
@pytest.mark.parametrize("name", ["tt8_generic_h1", "tt12_generic"])
def test_find_rooms_generic_two_truths_of_eight_and_twelve(name):
    assert _check_find_rooms(name, False, (193,)) > 0


def _check_find_rooms(name, restart, sizes):
    """Returns the number of hits compared."""
    rng = np.random.default_rng(len(name) + 2 * restart)
    seen = 0
    for per in sizes:
        segs, facts = case_facts(name, per, restart)
        masks = _half_masks(segs, rng)
        with _batch(segs, restart) as b:
            for want in range(1, 8):
                phases = _phases_arg(masks) if want & PHASE else None
                for first, count in _windows(per, len(segs)):
                    hits, n_match = b.find_rooms(want, phases, first, count)
                    ref = expected_hits(facts, want, masks, first, count)
                    what = (name, restart, per, want, first, count)
                    assert n_match == len(ref), (what, n_match, len(ref))
                    assert hits_as_tuples(hits) == ref, what
                    seen += len(ref)
    return seen


@pytest.mark.parametrize("name", ["ww8_h2", "tt4_h2"])
def test_truncation_keeps_a_prefix_and_a_scan_resumes(name):
    segs, facts = case_facts(name, 130, True)
    full = expected_hits(facts, PERSON | END)
    n = len(full)
    assert n > 8
    with _batch(segs, True) as b:
        for cap in (0, 1, n - 1, n, n + 5):
            buf = np.full(n + 8, 0xA5, dtype=np.uint8).repeat(16).view(ROOM_HIT_DTYPE)
            n_hits, n_match = np.full(1, 77, dtype=np.uint64), np.full(1, 77, dtype=np.uint64)
            st = b._lib.ge_batch_find_rooms(b._h, 0, 130, PERSON | END, None, buf.ctypes.data if cap else None, cap,
                                            n_hits.ctypes.data_as(_U64P), n_match.ctypes.data_as(_U64P))
            assert st == 0 and int(n_match[0]) == n and int(n_hits[0]) == min(n, cap), (cap, st, n_hits, n_match)
            assert hits_as_tuples(buf[: min(n, cap)]) == full[: min(n, cap)], cap
            assert set(buf[min(n, cap):].tobytes()) == {0xA5}, f"cap {cap}: slots past n_hits written"
        got, first = [], 0
        while True:
            hits, n_match = b.find_rooms(PERSON | END, first=first, cap=3)
            assert n_match == n - len(got)
            got += hits_as_tuples(hits)
            if len(hits) == n_match:
                break
            first = int(hits[-1]["room"]) + 1
        assert got == full


@pytest.mark.parametrize("name", ["ww8_h2", "tt4_h2"])
def test_pending_is_what_inject_actions_accepts(name):
    """Every room, every (human seat, choice) injected on a twin batch: some choice is accepted exactly when the seat's bit is set."""
    segs, _ = case_facts(name, 130, True)
    orc, _, n, mask, rooms = segs[0]
    views = oracle_rooms_as_views(orc, rooms)
    with _batch(segs, True) as b, _batch(segs, True) as twin:
        hits, _ = b.find_rooms("person")
        pending = np.zeros(130, dtype=np.uint32)
        pending[hits["room"].astype(np.int64)] = hits["pending"]
        assert (hits["why"] == PERSON).all() and (hits["pending"] != 0).all() and not (hits["pending"] & ~np.uint16(mask)).any()
        accepted = np.zeros(130, dtype=np.uint32)
        for seat in range(n):
            if not (mask >> seat) & 1:
                continue
            for choice in range(1, max(n, 3) + 1):
                twin.write_rooms(0, views)
                status = twin.inject_actions(np.arange(130), np.full(130, seat + 1), np.full(130, choice))
                accepted |= np.where(status == 0, np.uint32(1 << seat), np.uint32(0))
    assert np.array_equal(accepted, pending), np.flatnonzero(accepted != pending).tolist()
    assert (np.array([bin(int(p)).count("1") for p in pending]) >= 2).sum() >= 3


def _state(b):
    return (json.dumps(b.summary(), sort_keys=True, default=int), b.turn, b.read_events().tobytes() if b._trace else b"", b.read_rooms().tobytes())


@pytest.mark.parametrize("name", ["ww8_h2", "ww12_h2", "tt4_h2", "mixed"])
def test_the_call_only_reads(name):
    segs, _ = case_facts(name, 130, True)
    rng = np.random.default_rng(3)
    masks = _half_masks(segs, rng)
    with _batch(segs, True, trace=True) as b:
        b.step(1)
        before = _state(b)
        for want in range(1, 8):
            b.find_rooms(want, _phases_arg(masks) if want & PHASE else None)
            b.find_rooms(want, _phases_arg(masks) if want & PHASE else None, first=7, count=100, cap=2)
        assert _state(b) == before


@pytest.mark.parametrize("n_players,max_fuse", [(8, 0), (8, 1), (12, 1), (12, 0)])
def test_steps_with_scans_in_between_end_as_a_twin_that_never_scanned(dsl_ww, n_players, max_fuse):
    """Fused steps, single-turn launches, and a Werewolf x 12 batch with its deal side plane: prepared deals stay as they are."""
    tb = GameTable(dsl_ww)
    mk = lambda: RoomBatch([(tb, n_players, 700, 0b101)], seed=99, first_room=1 << 33, max_fuse=max_fuse, restart=True)
    with mk() as a, mk() as twin:
        matched = 0
        for k in (1, 3, 64, 1, 17, 65, 2):
            a.step(k)
            twin.step(k)
            hits, n = a.find_rooms(("person", "end", "phase"), phases=[0, 3])
            assert len(hits) == n
            matched += n
        assert matched > 0
        assert a.summary() == twin.summary() and a.turn == twin.turn
        assert a.read_rooms().tobytes() == twin.read_rooms().tobytes()
        a.step(40)
        twin.step(40)
        assert a.summary() == twin.summary()


def test_a_range_beyond_one_pass_of_the_scan(dsl_ww):
    """One pass of ge_find_scan covers 1 024 wavefront counts = 65 536 rooms (FIND_SCAN_WAVES, csrc/ge_find.inl): 70 000 rooms
    take a second pass, and the batch is above the 65 536 rooms at which the step kernels change build.  Against numpy over
    read_rooms of the same batch: the terminal phases from the table, and the mask."""
    n_rooms = 70_000
    tb = GameTable(dsl_ww)
    rows = tb.rows()
    terminal = np.zeros(256, dtype=bool)
    for r in rows:
        terminal[r["phase_id"]] = not r["branches"]
    ids = sorted(r["phase_id"] for r in rows)
    picked = [p for p in ids[1::2] if p < len(ids)]              # (the terminal phase's id, 99, is beyond a mask word: END finds it)
    in_mask = np.zeros(256, dtype=bool)
    in_mask[picked] = True
    with RoomBatch([(tb, 8, n_rooms)], seed=5, first_room=0) as b:
        b.step(48)
        phase = b.read_rooms()["phase_id"]
        why = np.where(terminal[phase], END, 0) | np.where(in_mask[phase], PHASE, 0)
        want_rooms = np.flatnonzero(why)
        hits, n_match = b.find_rooms(("end", "phase"), phases=picked)
        assert n_match == len(want_rooms) and 0 < n_match < n_rooms
        assert np.array_equal(hits["room"], want_rooms.astype(np.uint64))
        assert np.array_equal(hits["why"], why[want_rooms]) and np.array_equal(hits["phase_id"], phase[want_rooms])
        assert not hits["pending"].any() and not hits["segment"].any()
        assert (want_rooms > 65_536).any() and (why[:65_536] != 0).any()
        _, n_end = b.find_rooms("end", cap=0)
        assert n_end == b.summary()["finished"] == int(terminal[phase].sum()) and n_end > 0
        tail, n_tail = b.find_rooms(("end", "phase"), phases=picked, first=65_500, cap=40)
        assert n_tail == int((want_rooms >= 65_500).sum())
        assert np.array_equal(tail["room"], want_rooms[want_rooms >= 65_500][:40].astype(np.uint64))


def test_refusals_in_their_order_leave_every_output_untouched(dsl_ww, dsl_tt):
    with RoomBatch([(GameTable(dsl_ww), 8, 300, 1), (GameTable(dsl_tt), 4, 200, 2)], seed=1, max_fuse=1) as b:
        b.step(9)
        before = b.read_rooms().tobytes()
        n_ww, n_tt = GameTable(dsl_ww).n_phases, GameTable(dsl_tt).n_phases
        find = b._lib.ge_batch_find_rooms
        hits = np.full(16, 0x5A, dtype=np.uint8).repeat(16).view(ROOM_HIT_DTYPE)
        n_hits, n_match = np.full(1, 77, dtype=np.uint64), np.full(1, 78, dtype=np.uint64)
        good = np.array([1, 1], dtype=np.uint32)
        high = np.array([1, 1 << n_tt], dtype=np.uint32)          # a bit at the phase count of segment 1's table
        H, NH, NM = hits.ctypes.data, n_hits.ctypes.data_as(_U64P), n_match.ctypes.data_as(_U64P)
        calls = [
            # (first, count, want, masks, hits, cap, n_hits, n_match) -> status; later errors are present too where they can be
            ((0, 501, 0, None, None, 16, None, None), GE_ERR_ARG),                    # 1 want == 0 (and everything after it)
            ((0, 501, 8, None, None, 16, None, None), GE_ERR_ARG),                    # 1 unknown bits
            ((0, 501, 15, None, None, 16, None, None), GE_ERR_ARG),
            ((0, 501, 3, None, H, 16, None, NM), GE_ERR_ARG),                         # 2 n_hits NULL (range wrong as well)
            ((0, 501, 3, None, H, 16, NH, None), GE_ERR_ARG),                         # 2 n_match NULL
            ((0, 501, 3, None, None, 1, NH, NM), GE_ERR_ARG),                         # 3 hits NULL with cap > 0
            ((0, 501, 7, None, H, 16, NH, NM), GE_ERR_ARG),                           # 4 PHASE without masks
            ((0, 501, 4, high.ctypes.data, H, 16, NH, NM), GE_ERR_ARG),               # 5 mask bit >= phase count, before the range
            ((0, 501, 3, None, H, 16, NH, NM), GE_ERR_RANGE),                         # 6 beyond the batch
            ((500, 1, 3, None, H, 16, NH, NM), GE_ERR_RANGE),
            ((501, 0, 3, None, H, 16, NH, NM), GE_ERR_RANGE),                         # 6 before 7
            ((1 << 63, 1 << 63, 3, None, H, 16, NH, NM), GE_ERR_RANGE),               # first + count wraps
            ((0, 501, 4, good.ctypes.data, H, 16, NH, NM), GE_ERR_RANGE),
        ]
        for args, status in calls:
            first, count, want, masks, h, cap, nh, nm = args
            assert find(b._h, first, count, want, masks, h, cap, nh, nm) == status, args
            assert set(hits.tobytes()) == {0x5A} and int(n_hits[0]) == 77 and int(n_match[0]) == 78, args
        assert 1 << n_ww > 1                                     # (segment 0's table is checked by its own count)
        high0 = np.array([1 << n_ww, 1], dtype=np.uint32)
        if n_ww < 32:
            assert find(b._h, 0, 10, 4, high0.ctypes.data, H, 16, NH, NM) == GE_ERR_ARG
        assert find(b._h, 0, 10, 3, high.ctypes.data, H, 16, NH, NM) == 0    # masks are read only with PHASE
        n_hits[0], n_match[0] = 77, 78
        for first in (0, 17, 500):                               # 7 count == 0: GE_OK and zeros, nothing else written
            assert find(b._h, first, 0, 3, None, None, 0, NH, NM) == 0 and int(n_hits[0]) == 0 and int(n_match[0]) == 0
            n_hits[0], n_match[0] = 77, 78
        assert find(None, 0, 0, 3, None, None, 0, NH, NM) == GE_ERR_ARG
        with pytest.raises(GeError) as e:
            b.find_rooms(("person", "phase"))
        assert e.value.status == GE_ERR_ARG
        with pytest.raises(ValueError):
            b.find_rooms("person", phases=[1])
        with pytest.raises(GeError) as e:
            b.find_rooms("end", first=400, count=200)
        assert e.value.status == GE_ERR_RANGE
        hits0, n0 = b.find_rooms("end", first=500, count=0)
        assert len(hits0) == 0 and n0 == 0
        assert b.read_rooms().tobytes() == before


def test_kernel_time_includes_the_call(dsl_ww):
    with RoomBatch([(GameTable(dsl_ww), 8, 5000, 1)], seed=2, restart=True) as b:
        b.step(30)
        b.set_timing(True)
        b.kernel_time(reset=True)
        b.find_rooms(("person", "end"))
        ms, _ = b.kernel_time(reset=True)
        assert ms > 0.0


# ---- the hosts
needs_node = pytest.mark.skipif(shutil.which("node") is None or not os.path.exists(os.path.join(NODE_DIR, "ge_addon.node")),
                                reason="node or the built addon is not available")

FIND_SCRIPT = [dict(want=["person", "end"]), dict(want=["person"], first=40, count=200, cap=5), dict(want=["end"], cap=0),
               dict(want=["person", "end", "phase"], phases=[0, 2, 5]), dict(want=["phase"], phases={"0": [1, 3], "1": [0, 2]}, first=250, count=120),
               dict(want=["person", "phase"], phases=[4], first=299, count=2)]


def _python_find_script(dsl_ww, dsl_tt):
    from game_engine_amd.stepper import find_want_names, pending_seats
    out = []
    with RoomBatch([(GameTable(dsl_ww), 8, 300, 0b1001), (GameTable(dsl_tt), 4, 200, 0b10)], seed=11, first_room=5, restart=True) as b:
        b.step(37)
        for call in FIND_SCRIPT:
            kw = dict(call)
            if isinstance(kw.get("phases"), dict):
                kw["phases"] = {int(k): v for k, v in kw["phases"].items()}
            hits, n = b.find_rooms(**kw)
            out.append({"matched": n, "hits": [{"room": int(h["room"]), "why": find_want_names(int(h["why"])), "pending": pending_seats(h["pending"]),
                                                "phaseId": int(h["phase_id"]), "segment": int(h["segment"])} for h in hits]})
    return out


POOL_SPEC = dict(seed=21, chunkRooms=6, threads=10, humans=[1, 4], closed=["t1", "t4", "t7", "t8"], rounds=30)
GAME = "werewolf-(mafia)"


def _states_say(pool, live):
    """waiting / finished from the per-thread states alone: a seat waits when an inject_actions of it is accepted for some choice
    (the slot is put back afterwards), a thread has finished when its phase has no branch."""
    waiting, finished = {}, []
    for tid in live:
        room = pool._rooms[tid]
        chunk, slot = room["chunk"], room["slot"]
        view = chunk.read_rooms_at([slot])
        seats = []
        for s in room["human_seats"]:
            ok = False
            for c in range(1, 9):
                ok = ok or int(chunk.inject_actions([slot], [s], [c])[0]) == 0
                chunk.write_rooms_at([slot], view)
            if ok:
                seats.append(s)
        if seats:
            waiting[tid] = seats
        branches = {r["phase_id"]: r["branches"] for r in room["table"].rows()}
        if not branches[int(view["phase_id"][0])]:
            finished.append(tid)
    return waiting, sorted(finished)


def _python_pool_rounds(dsl_ww, check):
    from game_engine_amd import RoomPoolService
    p = POOL_SPEC
    pool = RoomPoolService(seed=p["seed"], chunk_rooms=p["chunkRooms"])
    rounds = []
    try:
        players = [{"name": f"P{i + 1}", "gamePlayerId": i + 1, "isBot": (i + 1) not in p["humans"]} for i in range(8)]
        ids = [f"t{k}" for k in range(p["threads"])]
        for tid in ids:
            pool.create_room(tid, GAME, players, dsl=dsl_ww)
        pool.run_rooms(ids, 64, ("person", "end"))
        closed_waiting = [t for t in p["closed"] if t in pool.waiting()]
        for tid in p["closed"]:                                  # two chunks of 6 slots: free slots in both, left as they stood
            pool.close(tid)
        live = [t for t in ids if t not in p["closed"]]
        for r in range(p["rounds"]):
            pool.run_rooms([t for k, t in enumerate(live) if (r + k) % 3 != 0], 1 + r % 3, ("person", "end"))
            waiting, finished = pool.waiting(), sorted(pool.finished())
            if check:
                assert (waiting, finished) == _states_say(pool, live), r
            answers = []
            for tid in sorted(waiting):
                for seat in waiting[tid]:
                    got = None
                    for c in range(1, 9):
                        try:
                            pool.human_action(tid, seat, c)
                            got = c
                            break
                        except GeError as e:
                            assert e.status == GE_ERR_ARG
                    answers.append([tid, seat, got])
            rounds.append({"waiting": waiting, "finished": finished, "answers": answers})
    finally:
        pool.close()
    return rounds, closed_waiting


def test_pool_waiting_and_finished_are_what_the_threads_states_say(dsl_ww):
    """Two chunks with closed slots in between: exactly the threads, and the seats, that the per-thread states give; a closed
    thread's slot still holds a room that waits for a person, and is never reported."""
    rounds, closed_waiting = _python_pool_rounds(dsl_ww, check=True)
    assert closed_waiting, "no closed slot was left waiting: the free-slot rule is not exercised"
    live = {f"t{k}" for k in range(POOL_SPEC["threads"])} - set(POOL_SPEC["closed"])
    assert all(set(r["waiting"]) | set(r["finished"]) <= live for r in rounds)
    assert sum(len(r["waiting"]) for r in rounds) > 0 and len(rounds[-1]["finished"]) > 0
    assert all(a[2] is not None for r in rounds for a in r["answers"]), "a waiting seat had no accepted choice"


@needs_node
def test_node_find_rooms_and_pool_are_the_python_hosts(dsl_ww, dsl_tt, tmp_path):
    want = _python_find_script(dsl_ww, dsl_tt)
    assert any(r["hits"] for r in want) and any(len(h["pending"]) for r in want for h in r["hits"])
    rounds, _ = _python_pool_rounds(dsl_ww, check=False)
    spec = tmp_path / "spec.json"
    spec.write_text(json.dumps({"ww": dsl_ww, "tt": dsl_tt, "script": FIND_SCRIPT, "pool": POOL_SPEC}))
    p = subprocess.run(["node", os.path.join(NODE_DIR, "selftest_find.js"), str(spec)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert got["finds"] == want
    assert got["pool"] == json.loads(json.dumps(rounds))

"""Every C-ABI call in random order against every other (-m gpu): the state-machine fuzz of tests/test_gpu_abi_sequences.py with
the indexed calls in it - ge_batch_step_rooms, read_rooms_at, write_rooms_at, run_rooms, run_rooms_playout, run_rooms_forecast,
step_rooms_playout (with and without halving) and the five rollouts - about half of each case's operations, the whole-batch calls
and the documented refusals the rest.  tests/abi_model.py draws the operations and holds the oracle-side model;
tests/test_abi_model_host.py proves on the model alone what the default seeds reach.

What the orders are for: the pinned staging buffer (io_stage) and the device scratch (pool_scratch) are shared by every call
and grow on demand, and the indexed calls lay several planes out in them and hold pointers across launches; a prepared role deal
is a cache tagged by the game index only, which an indexed turn under a foreign key must ignore and a whole-batch step must not
find in a record an indexed call stored; the indexed calls leave the turn counter (and its device mirror under graph replays),
the last step's trace and every unlisted room alone; an indexed call behind an unsynchronised multi-launch step follows it in
stream order.  After every indexed call: every returned array, the turn counter, read_rooms_at of the listed rooms and of a
sample of the others, and on traced batches the last step's events; at the end the whole read_rooms, the summary and the raw
records of every segment (no bit outside the view depends on which kernels wrote the record).  set_timing and kernel_time are
toggled along the way: timing turns graph replay off, so the same sequence must give the same rooms; three times a case the
launch count is read exactly over whole-batch steps alone (timed_steps), with timing on and off.  Hosted game threads
(inject_actions then step_rooms, round after round, each room on its own key and clock) run in slots the batch has recycled.

The seats-* scenarios put the seat plane, ge_batch_find_rooms and ge_batch_advise_seats into the same orders: set_seats (lists of
1, a few, 341 | 342 entries and the whole batch: 12 n staged bytes on either side of 4 096), get_seats, clear_seats with and
without a plane and a plane allocated again afterwards; find_rooms under all seven `want` sets, per-segment phase masks, ranges
across segments and of 192 | 193 rooms (3 888 | 4 176 B of scratch), cap 0, above and below n_match (the scan is resumed and the
concatenation compared), the slots from n_hits on pre-filled and untouched; advise_seats of seats that can act and seats that
cannot, both views; the serving loop (find who waits, advise, inject the advice, step_rooms) on a batch with a plane; the new
refusals with their statuses, and the playout bit a room's own mask allows where its segment's would not.  Every other kind runs
on batches with a plane as well: ge_batch_step then launches ge_seat_step_kernel plainly (one launch per segment and per max_fuse
turns, counted exactly), stores records without a prepared deal and leaves the Werewolf x 12 deal side plane and the graphs'
device turn word alone, and after clear_seats the cached graphs, the side plane and the flagship kernels take over again.  After
every operation on a batch that has or had a plane a sample of seats() is compared with the model, at the end all of it."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import abi_model as A
from find_ref import hits_as_tuples
from game_engine_amd import ROOM_HIT_DTYPE, GameTable, GeError, RoomBatch
from parity_util import assert_records_canonical, assert_views_equal

pytestmark = pytest.mark.gpu


def _events_equal(got, want, what):
    want = np.array(want).reshape(np.shape(got))
    for f in A.EV_FIELDS:
        assert np.array_equal(got[f], want[f]), (what, f, got[f].tolist(), want[f].tolist())


def _words_equal(got, want, what):
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    assert not len(bad), f"{what}: {len(bad)} words differ; first at {bad[0].tolist()}: got {int(np.asarray(got)[tuple(bad[0])])} want {int(np.asarray(want)[tuple(bad[0])])}"


def _run_equal(got, want, what, decided=None):
    """(played, stopped, events, views[, decided]) of a run call: events, views and decided masks below played[k]."""
    played, stopped, events, views = got[:4]
    assert played.tolist() == want[0].tolist(), (what, "played")
    assert stopped.tolist() == want[1].tolist(), (what, "stopped")
    for k, p in enumerate(played):
        _events_equal(events[k, :p], want[2][k], f"{what} entry {k}")
        assert_views_equal(np.ascontiguousarray(views[k, :p]), np.array(want[3][k]), f"{what} entry {k} views")
        if decided is not None:
            assert decided[0][k, :p].tolist() == [int(x) for x in decided[1][k]], (what, k, "decided")


def _refused(b, op):
    a = op.a
    n = len(a["rooms"])
    if a["call"] == "step_rooms":
        b.step_rooms(a["rooms"], a["keys"], a["turns"])
    elif a["call"] == "run_rooms":
        b.run_rooms(a["rooms"], a["keys"], a["turns"], max_turns=4)
    elif a["call"] == "step_rooms_playout":
        b.step_rooms_playout(a["rooms"], a["keys"], a["turns"], np.zeros(n, dtype=np.uint32), a["keys"], 4, 8)
    elif a["call"] == "read_rooms_at":
        b.read_rooms_at(a["rooms"])
    else:
        b.write_rooms_at(a["rooms"], a["views"])


_U64P = C.POINTER(C.c_uint64)


def _find_equal(b, c, what):
    """One drawn ge_batch_find_rooms call through the C ABI, the hit buffer pre-filled: hit for hit the model's, the slots from
    n_hits on untouched; a call that cap truncates is resumed behind its last hit until the scan is done."""
    got, first, left = [], c["first"], c["count"]
    while True:
        cap = c["cap"]
        buf = np.full(cap + 3, 0xA5, dtype=np.uint8).repeat(16).view(ROOM_HIT_DTYPE)
        n_hits, n_match = np.full(1, 77, dtype=np.uint64), np.full(1, 77, dtype=np.uint64)
        st = b._lib.ge_batch_find_rooms(b._h, first, left, c["want"], c["masks"].ctypes.data if c["masks"] is not None else None,
                                        buf.ctypes.data if cap else None, cap, n_hits.ctypes.data_as(_U64P), n_match.ctypes.data_as(_U64P))
        k = int(n_hits[0])
        assert st == 0 and int(n_match[0]) == c["n_match"] - len(got) and k == min(int(n_match[0]), cap, left), (what, st, n_hits, n_match, len(got))
        assert set(buf[k:].tobytes()) == {0xA5}, f"{what}: slots from n_hits on were written"
        got += hits_as_tuples(buf[:k])
        if cap == 0 or k == int(n_match[0]):
            break
        nxt = got[-1][0] + 1                                        # resume: first = hits[n_hits - 1].room + 1
        first, left = nxt, c["first"] + c["count"] - nxt
    assert got == (c["hits"] if c["cap"] else []), (what, got[:4], c["hits"][:4])


def _advice_equal(got, want, what):
    for f in ("status", "legal", "best", "phase_id"):
        assert got[f].tolist() == want[f].tolist(), (what, f, got[f].tolist(), want[f].tolist())
    for f in ("finished", "wins", "score"):
        assert got["policy"][f].tolist() == want["policy"][f].tolist(), (what, "policy", f)
        assert got["option"][f].tolist() == want["option"][f].tolist(), (what, "option", f)


def _seat_refusal(b, op, what):
    """A new refusal with its documented status (the after-call checks of apply show that nothing moved); refuse_playout_seat:
    and the accepted counterpart."""
    a, kind = op.a, op.kind
    if kind == "refuse_playout_seat":
        b.set_seats(*a["set"])
        r = a["refused"]
    with pytest.raises(GeError) as e:
        if kind == "refuse_set_seats":
            b.set_seats(a["rooms"], a["masks"])
        elif kind == "refuse_find_rooms":
            n_hits, n_match = C.c_uint64(77), C.c_uint64(78)
            buf = np.full(8, 0xA5, dtype=np.uint8).repeat(16).view(ROOM_HIT_DTYPE)
            st = b._lib.ge_batch_find_rooms(b._h, a["first"], a["count"], a["want"], a["masks"].ctypes.data if a["masks"] is not None else None,
                                            buf.ctypes.data, 8, C.byref(n_hits), C.byref(n_match))
            assert set(buf.tobytes()) == {0xA5} and (n_hits.value, n_match.value) == (77, 78), (what, "an output was written")
            raise GeError(st, "ge_batch_find_rooms") if st else AssertionError(what + ": accepted")
        elif kind == "refuse_advise_seats":
            b.advise_seats(a["rooms"], a["keys"], a["turns"], a["seats"], a["R"], a["M"])
        elif a["how"] == "step_rooms_playout":
            b.step_rooms_playout(r["rooms"], a["keys"], a["turns"], r["masks"], a["pkeys"], a["R"], a["M"])
        else:
            b.run_rooms_playout(r["rooms"], a["keys"], a["turns"], r["masks"], a["pkeys"], a["R"], a["M"], max_turns=2)
    assert e.value.status == op.status, (what, a["how"], e.value.status)
    if kind == "refuse_playout_seat":       # a seat of the segment's mask that the room has handed back to the policy plays out
        ev, decided = b.step_rooms_playout(a["rooms"], a["keys"], a["turns"], a["masks"], a["pkeys"], a["R"], a["M"], seed=a["seed"])
        assert decided.tolist() == op.want[1].tolist(), (what, "decided")
        _events_equal(ev, op.want[0], what)


def apply(b, op, d, what, check):
    """One drawn operation on batch b, compared with what the model (d.m, already moved) says it returns.  check: a generator of
    this test's own (never the operation stream's) for the samples of the checks."""
    m, a, kind = d.m, op.a, op.kind
    if kind == "step":
        for k in a["ks"]:
            b.step(k)
    elif kind == "read":
        assert_views_equal(b.read_rooms(), m.views(), what)
    elif kind == "read_part":
        if a["cnt"]:
            assert_views_equal(b.read_rooms(a["lo"], a["cnt"]), m.views(a["lo"], a["lo"] + a["cnt"]), what)
        else:
            assert len(b.read_rooms(a["lo"], 0)) == 0
    elif kind == "write":
        b.write_rooms(a["lo"], a["views"])
    elif kind == "inject":
        try:
            b.inject_action(a["room"], a["player"], a["choice"])
            got = 0
        except GeError as e:
            got = e.status
        assert got == op.want, what
    elif kind == "inject_many":
        assert b.inject_actions(a["rooms"], a["players"], a["choices"]).tolist() == op.want, what
    elif kind == "reset":
        b.reset()
    elif kind == "set_turn":
        b.set_turn(a["turn"])
    elif kind == "summary":
        got, want = b.summary(), m.summary()
        for key, v in want.items():
            assert got[key] == v, (what, key)
    elif kind == "events":
        if not d.trace:
            with pytest.raises(GeError) as e:
                b.read_events()
            assert e.value.status == -7
        elif "lo" in a:
            _events_equal(b.read_events(a["lo"], a["cnt"]), m.last_events[a["lo"]: a["lo"] + a["cnt"]], what)
    elif kind == "set_timing":
        b.set_timing(a["on"])
    elif kind == "kernel_time":
        ms, launches = b.kernel_time(reset=a["reset"])
        assert math.isfinite(ms) and ms >= 0, (what, ms)
        if a["exact"]:                                              # only whole-batch steps since the last reset of the count
            assert launches == a["launches"], (what, launches, a["launches"])
        assert launches >= a["launches"], (what, launches, a["launches"])
    elif kind == "timed_steps":
        ms, launches = b.kernel_time(reset=True)
        assert math.isfinite(ms) and ms >= 0 and launches >= a["before"], (what, ms, launches, a["before"])
        b.set_timing(a["on"])
        for k in a["ks"]:
            b.step(k)
        ms, launches = b.kernel_time(reset=a["reset"])
        # (with a seat plane: one launch per segment and per max_fuse turns)
        assert launches == a["total"] == a["per_launch"] * sum(-(-k // d.fuse) for k in a["ks"]), (what, a["ks"], launches, a["total"])
        assert math.isfinite(ms) and ms >= 0 and (ms > 0 or not a["on"]), (what, ms)
    elif kind == "step_rooms":
        _events_equal(b.step_rooms(a["rooms"], a["keys"], a["turns"]), op.want, what)
    elif kind == "hosted_threads":
        for t, (rooms, keys, turns, (ir, ip, ic), events) in enumerate(a["rounds"]):
            if len(ir):
                assert not b.inject_actions(ir, ip, ic).any(), (what, t, "a person's action was refused")
            _events_equal(b.step_rooms(rooms, keys, turns), events, f"{what} round {t}")
    elif kind == "read_rooms_at":
        assert_views_equal(b.read_rooms_at(a["rooms"]), op.want, what)
    elif kind == "write_rooms_at":
        b.write_rooms_at(a["rooms"], a["views"])
    elif kind == "run_rooms":
        _run_equal(b.run_rooms(a["rooms"], a["keys"], a["turns"], max_turns=a["max_turns"], until=a["until"]), op.want, what)
    elif kind == "run_rooms_playout":
        got = b.run_rooms_playout(a["rooms"], a["keys"], a["turns"], a["masks"], a["pkeys"], a["R"], a["M"], seed=a["seed"],
                                  full_view=a["full_view"], max_turns=a["max_turns"], until=a["until"])
        _run_equal(got, op.want, what, decided=(got[4], op.want[4]))
    elif kind == "run_rooms_forecast":
        got = b.run_rooms_forecast(a["rooms"], a["keys"], a["turns"], a["fkeys"], a["R"], a["M"], seats=a["seats"], seed=a["seed"],
                                   max_turns=a["max_turns"], until=a["until"])
        _run_equal(got, op.want, what)
        for k, p in enumerate(got[0]):
            _words_equal(got[4][k, :p + 1], op.want[4][k], f"{what} entry {k} stats")
    elif kind in ("step_rooms_playout", "step_rooms_playout_halving"):
        ev, decided = b.step_rooms_playout(a["rooms"], a["keys"], a["turns"], a["masks"], a["pkeys"], a["R"], a["M"], seed=a["seed"],
                                           full_view=a["full_view"], halving=a["halving"])
        assert decided.tolist() == op.want[1].tolist(), (what, "decided")
        _events_equal(ev, op.want[0], what)
    elif kind == "rollout_rooms":
        _words_equal(b.rollout_rooms(a["rooms"], a["keys"], a["turns"], a["R"], a["M"], seed=a["seed"]), op.want, what)
    elif kind.startswith("rollout_"):
        if kind == "rollout_actions":
            got = b.rollout_actions(a["rooms"], a["keys"], a["turns"], a["actions"], a["R"], a["M"], seed=a["seed"])
        elif kind == "rollout_seats":
            got = b.rollout_seats(a["rooms"], a["keys"], a["turns"], a["seats"], a["actions"], a["R"], a["M"], seed=a["seed"])
        elif kind == "rollout_compare":
            got = b.rollout_compare(a["rooms"], a["keys"], a["turns"], a["seats"], a["actions"], a["baseline"], a["subjects"], a["R"], a["M"],
                                    seed=a["seed"])
        else:
            got = b.rollout_beliefs(a["rooms"], a["keys"], a["turns"], a["seats"], a["actions"], a["beliefs"], a["R"], a["M"], seed=a["seed"],
                                    baseline=a.get("baseline"), subjects=a.get("subjects"))
        assert got[1].tolist() == op.want[1].tolist(), (what, "status")
        _words_equal(got[0], op.want[0], what)
        if len(got) == 3:
            _words_equal(got[2], op.want[2], what + " cmp")
    elif kind == "set_seats":
        b.set_seats(a["rooms"], a["masks"])
    elif kind == "get_seats":
        got = b.seats(a["first"], a["count"])
        assert got.dtype == np.uint32 and np.array_equal(got, op.want), what
    elif kind == "clear_seats":
        b.clear_seats()
    elif kind == "find_rooms":
        for j, c in enumerate(a["calls"]):
            _find_equal(b, c, f"{what} call {j}")
    elif kind == "advise_seats":
        _advice_equal(b.advise_seats(a["rooms"], a["keys"], a["turns"], a["seats"], a["R"], a["M"], seed=a["seed"], full_view=a["full_view"]),
                      op.want, what)
    elif kind == "served_rounds":
        for t, r in enumerate(a["rounds"]):
            hits, n_match = b.find_rooms("person")
            assert n_match == len(r["hits"]) and hits_as_tuples(hits) == r["hits"], f"{what} round {t}: who waits"
            if not len(r["rooms"]):                                 # nobody waits
                continue
            advice = b.advise_seats(r["rooms"], r["keys"], r["turns"], r["seats"], a["R"], a["M"], seed=a["seed"])
            _advice_equal(advice, r["advice"], f"{what} round {t}")
            assert not b.inject_actions(r["rooms"], r["seats"], advice["best"]).any(), (what, t, "an advised action was refused")
            _events_equal(b.step_rooms(r["rooms"], r["keys"], r["turns"]), r["events"], f"{what} round {t}")
    elif kind in A.SEAT_REFUSALS:
        _seat_refusal(b, op, what)
    elif kind in A.REFUSALS:
        with pytest.raises(GeError) as e:
            _refused(b, op)
        assert e.value.status == op.status, (what, a["call"], e.value.status)
        if kind == "refuse_view":
            assert str(a["rejected"]) in str(e.value), (what, str(e.value))
    else:
        raise AssertionError(kind)
    if d.had_plane:                                                 # the masks are configuration: only set_seats and clear_seats move them
        lo = int(check.integers(0, m.total))
        cnt = int(check.integers(0, min(96, m.total - lo) + 1))
        assert np.array_equal(b.seats(lo, cnt), m.get_seats(lo, cnt)), (what, "seats", lo, cnt)
    if op.listed is None:
        return
    # what an indexed call (and a refused one) must leave alone, and what it must have stored
    assert b.turn == m.turn, (what, "the turn counter moved")
    look = np.concatenate([op.listed[op.listed < m.total], check.integers(0, m.total, 24).astype(np.uint64)])
    assert_views_equal(b.read_rooms_at(look), m.views()[look.astype(np.int64)], what + ": listed and sampled rooms afterwards")
    if d.trace and m.last_events is not None:
        lo = int(check.integers(0, m.total))
        cnt = int(check.integers(1, min(64, m.total - lo) + 1))
        _events_equal(b.read_events(lo, cnt), m.last_events[lo: lo + cnt], what + ": the last step's trace")


def test_compare_refuses_a_subject_other_than_its_baselines():
    """What the fuzz found with subjects drawn per entry: a playout keeps one outcome byte, for its own entry's subject, so an
    entry compared with a baseline of another subject got sums that mixed two seats' outcomes (ww8-300-single seed 0: better 4
    against the reference's 1) where ge_step.h defined them for the entry's subject.  Such a call is refused now, nothing run;
    the same entries under one subject match the reference."""
    from compare_ref import reference_compare
    m = A.Model([(A.WW, 8, 64, 0)], 11, 5, False)
    m.step(9)                                                       # roles dealt, the first night under way
    with RoomBatch([(GameTable(A.dsl_for(A.WW)), 8, 64, 0)], seed=11, first_room=5, max_fuse=1) as b:
        b.step(9)
        rooms, keys, turns, seats = [3, 3, 3, 40, 40], [77, 77, 77, 2 ** 64 - 9, 2 ** 64 - 9], [9] * 5, [0, 0, 0, 2, 2]
        actions, baseline = [[], [], [], [], []], [0, 0, 1, 3, 3]
        for subjects in ([1, 2, 1, 4, 4], [1, 1, 2, 4, 4], [1, 1, 1, 4, 5]):
            with pytest.raises(GeError) as e:
                b.rollout_compare(rooms, keys, turns, seats, actions, baseline, subjects, 65, 40, seed=3)
            assert e.value.status == A.GE_ERR_ARG
            with pytest.raises(GeError) as e:
                b.rollout_beliefs(rooms, keys, turns, seats, actions, np.ones((5, 16), dtype=np.uint8) * (np.arange(16) < 8), 65, 40, seed=3,
                                  baseline=baseline, subjects=subjects)
            assert e.value.status == A.GE_ERR_ARG
        for subjects in ([1, 1, 1, 4, 4], [6, 6, 6, 8, 8]):
            words, status, cmp = b.rollout_compare(rooms, keys, turns, seats, actions, baseline, subjects, 65, 40, seed=3)
            want = reference_compare(m.orc_of, rooms, keys, turns, seats, actions, baseline, subjects, 65, 40, 3)
            assert status.tolist() == want[1].tolist()
            _words_equal(words, want[0], f"subjects {subjects}")
            _words_equal(cmp, want[2], f"subjects {subjects} cmp")
        assert_views_equal(b.read_rooms(), m.views(), "the batch is only read")


@pytest.mark.parametrize("name", A.SCENARIO_NAMES + A.SEAT_SCENARIO_NAMES)
@pytest.mark.parametrize("fuzz_seed", range(int(os.environ.get("GE_SEQ_FUZZ_SEEDS", "2"))))     # (a soak run sets more)
def test_abi_indexed_state_machine_fuzz(name, fuzz_seed):
    specs = dict(A.ALL_SCENARIOS)[name]
    tables = {g: GameTable(A.dsl_for(g)) for segs, _, _, _ in specs for g, _, _, _ in segs}
    check = np.random.default_rng(fuzz_seed)
    batches, draws = [], None
    try:
        for i, (op, draws) in enumerate(A.draw_ops(name, fuzz_seed)):
            if not batches:                                         # (the generator has built the models: same seeds, same keys)
                for d in draws:
                    batches.append(RoomBatch([(tables[g], n, r, mask) for g, n, r, mask in d.segs], seed=d.m.seed, first_room=d.m.first,
                                             max_fuse=d.fuse, restart=d.restart, trace=d.trace))
            apply(batches[op.bi], op, draws[op.bi], f"{name} fuzz {fuzz_seed} op {i} {op.kind} (batch {op.bi})", check)
        for j, (b, d) in enumerate(zip(batches, draws)):
            what = f"{name} fuzz {fuzz_seed} batch {j}"
            assert_views_equal(b.read_rooms(), d.m.views(), what + ": final read")
            got, want = b.summary(), d.m.summary()
            for key, v in want.items():
                assert got[key] == v, (what, key)
            for s, (o, rooms) in enumerate(zip(d.m.orcs, d.m.rooms)):
                assert_records_canonical(b, s, o, rooms, f"{what} segment {s}")
            assert np.array_equal(b.seats(), d.m.get_seats()), what + ": final seats"
    finally:
        for b in batches:
            b.close()

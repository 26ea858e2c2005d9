"""The indexed-call sequence fuzz reaches what it is for (no GPU): tests/abi_model.py's operation stream - the one
tests/test_gpu_abi_indexed_sequences.py replays against the library, same scenarios, same default seeds - is drawn on the
oracle model alone and measured.  These are properties of the generator, its seeds and its weights: a change that loses one of
them makes the GPU fuzz blind to the orders it exists for (a prepared deal of the batch's key under an indexed turn, a record
without one under a whole-batch step, stale staging pointers across a regrow, an indexed call behind an unsynchronised graph
replay), and shows here first.

The seats-* scenarios (the seat plane, find_rooms, advise_seats) are measured the same way: every new kind and refusal occurs,
entry counts and ranges lie on both sides of their byte thresholds, no find_rooms condition is answered by all or none of a
range, advice is mostly for seats that can act and not always the lowest choice, the rooms' own masks change what listed rooms
do, role deals meet records of the other step path, a game restarted under seat steps is dealt from the Werewolf x 12 side plane,
and a cached graph is replayed after seat steps moved the turn."""
import hashlib
import time
from collections import Counter

import numpy as np
import pytest

import abi_model as A

DEFAULT_SEEDS = (0, 1)
WEREWOLF = [n for n in A.SCENARIO_NAMES if n.startswith("ww") or n in ("mixed-4seg", "two-batches")]
_STATS = {}


def _masked(name):
    return any(mask for segs, _, _, _ in dict(A.SCENARIOS)[name] for _, _, _, mask in segs)


def stats_of(name):
    """What the default seeds of a scenario reach: operation counts, the models' coverage counters, the entry counts per call,
    the orders around multi-launch steps, and the oracle's wall time per case."""
    if name in _STATS:
        return _STATS[name]
    st = {"ops": Counter(), "cov": Counter(), "counts": {}, "step4_then_indexed": 0, "indexed_then_step4": 0, "seconds": [],
          "write_at_before_plane": 0, "indexed_before_plane": 0, "per_seed_ops": [], "step_ks": [], "timed": []}
    digest = hashlib.sha256()                                       # (kind, listed rooms) of every operation, both seeds
    for seed in DEFAULT_SEEDS:
        t0 = time.perf_counter()
        prev, plane, draws, n_ops = {}, {}, None, 0
        for op, draws in A.draw_ops(name, seed):
            n_ops += 1
            st["ops"][op.kind] += 1
            digest.update(op.kind.encode() + b"|" + (b"-" if op.listed is None else np.asarray(op.listed, dtype=np.uint64).tobytes()) + b";")
            if op.listed is not None and op.status is None:
                st["counts"].setdefault(op.kind, Counter())[len(op.listed)] += 1
            was = prev.get(op.bi)
            indexed = op.kind in A.INDEXED_OPS
            big = op.kind == "step" and op.a["launches"][-1] >= 4
            st["step4_then_indexed"] += int(indexed and was == "step4")
            st["indexed_then_step4"] += int(big and was == "indexed")
            prev[op.bi] = "step4" if big else "indexed" if indexed else op.kind
            fuse = draws[op.bi].fuse
            if op.kind == "timed_steps":
                st["timed"].append((op.a["on"], op.a["total"], any(n >= 4 and (k % fuse == 1 or fuse == 1) for k, n in zip(op.a["ks"], op.a["launches"]))))
            if op.kind == "kernel_time" and op.a["exact"] and op.a["launches"]:
                st["timed"].append((None, op.a["launches"], False))
            if op.kind == "step":
                st["step_ks"] += op.a["ks"]
            if op.kind == "step" and any(k % fuse == 1 or fuse == 1 for k in op.a["ks"]):
                plane[op.bi] = True                                 # a single-turn launch: the Werewolf x 12 side plane exists from here
            if not plane.get(op.bi):
                st["write_at_before_plane"] += int(op.kind == "write_rooms_at")
                st["indexed_before_plane"] += int(op.kind in A.MUTATING_INDEXED and op.kind != "write_rooms_at")
        for d in draws:
            st["cov"].update(d.m.cov)
        st["per_seed_ops"].append(n_ops)
        st["seconds"].append(time.perf_counter() - t0)
    st["digest"] = digest.hexdigest()
    _STATS[name] = st
    return st


@pytest.mark.parametrize("name", A.SCENARIO_NAMES)
def test_every_operation_kind_occurs(name):
    st = stats_of(name)
    print(f"{name}: {dict(sorted(st['ops'].items()))}  oracle seconds per case {[round(s, 2) for s in st['seconds']]}")
    assert all(60 <= n <= 84 for n in st["per_seed_ops"])
    kinds = list(A.OLD_OPS) + A.INDEXED_OPS + list(A.TIMING_OPS)
    few = {k: st["ops"][k] for k in kinds if st["ops"][k] < 3}
    assert not few, (name, few)
    indexed = sum(st["ops"][k] for k in A.INDEXED_OPS + A.REFUSALS)
    assert .4 <= indexed / sum(st["ops"].values()) <= .6


def test_every_refusal_kind_occurs():
    total = Counter()
    for name in A.SCENARIO_NAMES:
        total.update(stats_of(name)["ops"])
    assert all(total[k] >= 1 for k in A.REFUSALS), total


@pytest.mark.parametrize("name", WEREWOLF)
def test_role_deals_meet_the_other_kind_of_writer(name):
    """An indexed turn assigns roles in a record a whole-batch step wrote (it may carry a prepared deal of the batch's key), and
    a whole-batch step assigns roles in a record an indexed call wrote (it carries none)."""
    cov = stats_of(name)["cov"]
    print(name, dict(cov))
    assert cov["indexed_assigns_after_step"] >= 5, (name, dict(cov))
    assert cov["step_assigns_after_indexed"] >= 5, (name, dict(cov))


@pytest.mark.parametrize("name", ["ww8-300-single", "ww8-4096-fused", "ww8-generic-300"])
def test_a_kept_deal_would_be_dealt(name):
    """The whole chain that shows a Werewolf x 8 record stored with the prepared deal it was loaded with (instead of none): a
    single indexed turn (ge_pool_kernel: step_rooms, hosted threads, playout steps) deals game g over a record a whole-batch
    step wrote - its prepared deal is game g's, and with roles in the record it would now read as game g + 1's - only such
    turns and whole-batch steps touch the room until its game is over and the slot recycled, and a whole-batch step deals game
    g + 1 there: from the kept deal, so the next read differs in the players' roles."""
    assert stats_of(name)["cov"]["step_assigns_game_after_indexed_deal"] >= 3, (name, dict(stats_of(name)["cov"]))


@pytest.mark.parametrize("name", [n for n in A.SCENARIO_NAMES if _masked(n)])
def test_run_rooms_stops_for_every_reason(name):
    cov = stats_of(name)["cov"]
    for why in ("person", "end", "phase", "limit"):
        assert cov["run_stop_" + why] >= 1, (name, why, dict(cov))


@pytest.mark.parametrize("name", A.SCENARIO_NAMES)
def test_indexed_calls_restart_rooms(name):
    assert stats_of(name)["cov"]["indexed_restarted"] >= 1, name   # every scenario's batches restart


@pytest.mark.parametrize("name", A.SCENARIO_NAMES)
def test_playout_seats_decide(name):
    assert stats_of(name)["cov"]["playout_decisions"] >= 3, name


def test_playout_decisions_differ_from_the_policy():
    cov = Counter()
    for name in A.SCENARIO_NAMES:
        cov.update(stats_of(name)["cov"])
    print({k: v for k, v in cov.items() if k.startswith("playout")})
    assert cov["playout_not_policy"] >= 2 and cov["playout_decisions"] > cov["playout_not_policy"]


def test_entry_counts_lie_on_both_sides_of_each_threshold():
    seen = {}
    for name in A.SCENARIO_NAMES:
        for kind, c in stats_of(name)["counts"].items():
            seen.setdefault(kind, Counter()).update(c)
    for kind, sides in (("step_rooms", (113, 114)), ("read_rooms_at", (73, 74)), ("write_rooms_at", (73, 74)), ("run_rooms", (44, 45))):
        for n in (1,) + sides:
            assert seen[kind][n] >= 1, (kind, n, dict(seen[kind]))
    for kind in ("step_rooms", "read_rooms_at", "write_rooms_at"):
        assert seen[kind][A.LARGE] >= 1, (kind, dict(seen[kind]))      # (a smaller batch is listed whole instead)
        for name in A.SCENARIO_NAMES:
            assert max(stats_of(name)["counts"][kind]) >= 190, (name, kind)
    rollouts = Counter()
    for kind in A.INDEXED_OPS:
        if kind.startswith("rollout_"):
            rollouts.update(seen[kind])
            assert max(seen[kind]) <= 114
    assert min(rollouts) <= 6 and any(n >= 7 for n in rollouts), dict(rollouts)
    for kind in ("run_rooms", "run_rooms_playout", "run_rooms_forecast", "step_rooms_playout", "step_rooms_playout_halving"):
        assert max(seen[kind]) <= 114


def test_indexed_calls_follow_and_precede_multi_launch_steps():
    """A step of four or more launches (the graph replay, not yet synchronised) directly followed by an indexed call of the same
    batch - nothing in between that waits for the device - and the reverse order."""
    after = sum(stats_of(n)["step4_then_indexed"] for n in A.SCENARIO_NAMES)
    before = sum(stats_of(n)["indexed_then_step4"] for n in A.SCENARIO_NAMES)
    print("step >= 4 launches -> indexed:", after, " indexed -> step >= 4 launches:", before)
    assert after >= 3 and before >= 3


UNTRACED = [n for n in A.SCENARIO_NAMES if any(not trace for _, _, _, trace in dict(A.SCENARIOS)[n])]


@pytest.mark.parametrize("name", UNTRACED)
def test_each_untraced_scenario_has_indexed_calls_around_graph_replays(name):
    """The same per scenario - so on the Werewolf x 12 side-plane path, the GENERIC builds, the mixed batch, each form of Two-Truths."""
    st = stats_of(name)
    assert st["step4_then_indexed"] >= 3 and st["indexed_then_step4"] >= 3, (name, st["step4_then_indexed"], st["indexed_then_step4"])


@pytest.mark.parametrize("name", A.SCENARIO_NAMES)
def test_launch_counts_are_read_exactly_over_steps(name):
    """kernel_time(reset) -> only whole-batch steps -> kernel_time, the count compared exactly and not zero: at least five times
    a scenario, with timing on and with timing off, and where a batch is not traced over a step of four launches or more with a
    single-turn tail."""
    timed = stats_of(name)["timed"]
    assert sum(1 for _, total, _ in timed if total > 0) >= 5, (name, timed)
    assert {on for on, total, _ in timed if total > 0} >= {True, False}, (name, timed)
    if name in UNTRACED:
        assert sum(1 for on, _, graph in timed if graph) >= 2, (name, timed)
        assert any(graph and on is False for on, _, graph in timed) and any(graph and on for on, _, graph in timed), (name, timed)


# ---- the scenarios of the seat plane, find_rooms and advise_seats

SEAT_NAMES = A.SEAT_SCENARIO_NAMES
SEAT_WEREWOLF = [n for n in SEAT_NAMES if "ww" in n or n in ("seats-mixed-4seg", "seats-two-batches")]
SEAT_UNTRACED = [n for n in SEAT_NAMES if any(not trace for _, _, _, trace in dict(A.SEAT_SCENARIOS)[n])]
_SEAT_STATS = {}


def seat_stats_of(name):
    """What the default seeds of a seat-plane scenario reach: operation counts, refusal forms, the entry counts of set_seats, the
    ranges, wants and caps of find_rooms, the advice drawn, the coverage counters and the oracle's seconds per case."""
    if name in _SEAT_STATS:
        return _SEAT_STATS[name]
    st = {"ops": Counter(), "hows": Counter(), "cov": Counter(), "set_counts": Counter(), "find": [], "advice": [], "seconds": [],
          "get_counts": [], "clear_then_set": [], "views": set(), "advise_RM": set(), "timed_planes": Counter(),
          "served": [], "old_on_plane": Counter()}
    for seed in DEFAULT_SEEDS:
        t0 = time.perf_counter()
        draws, cleared, later_set = None, False, False
        for op, draws in A.draw_ops(name, seed):
            a = op.a
            st["ops"][op.kind] += 1
            if op.kind in A.SEAT_REFUSALS:
                st["hows"][(op.kind, a["how"])] += 1
            elif op.kind == "set_seats":
                st["set_counts"][len(a["rooms"])] += 1
                later_set |= cleared
            elif op.kind == "clear_seats":
                cleared |= a["plane"]
            elif op.kind == "get_seats":
                st["get_counts"].append(a["count"])
            elif op.kind == "find_rooms":
                st["find"] += a["calls"]
            elif op.kind == "advise_seats":
                st["advice"].append(op.want)
                st["views"].add(a["full_view"])
                st["advise_RM"].add((a["R"], a["M"]))
            elif op.kind == "served_rounds":
                st["served"] += a["rounds"]
            elif op.kind == "timed_steps":
                st["timed_planes"][a["per_launch"] if len(draws[op.bi].segs) > 1 else draws[op.bi].m.masks is not None] += 1
            if op.kind in A.INDEXED_OPS + ["step", "timed_steps"] and draws[op.bi].m.masks is not None:
                st["old_on_plane"][op.kind] += 1
        for d in draws:
            st["cov"].update(d.m.cov)
        st["clear_then_set"].append(later_set)
        st["seconds"].append(time.perf_counter() - t0)
    _SEAT_STATS[name] = st
    return st


@pytest.mark.parametrize("name", SEAT_NAMES)
def test_every_seat_kind_occurs(name):
    st = seat_stats_of(name)
    print(f"{name}: {dict(sorted(st['ops'].items()))}  oracle seconds per case {[round(s, 2) for s in st['seconds']]}")
    few = {k: st["ops"][k] for k in list(A.SEAT_OPS) + list(A.OLD_OPS) + A.INDEXED_OPS + list(A.TIMING_OPS) if st["ops"][k] < (3 if k in A.SEAT_OPS else 2)}
    assert not few, (name, few)
    # (the oracle's seconds are printed, not asserted: a new case is to stay below twice the slowest case of the other scenarios -
    # tests/README.md has the measured values)
    # a plane is allocated, freed by a clear_seats and allocated again by a later set_seats in every case; both kinds of clear
    assert st["cov"]["set_seats_allocates"] >= 4 and all(st["clear_then_set"]), (name, dict(st["cov"]), st["clear_then_set"])
    assert st["cov"]["clear_with_plane"] >= 2 and st["cov"]["clear_without_plane"] >= 1, (name, dict(st["cov"]))
    assert 0 in st["get_counts"] and max(st["get_counts"]) > 0, (name, st["get_counts"])


@pytest.mark.parametrize("name", SEAT_NAMES)
def test_the_other_kinds_run_on_batches_with_a_plane(name):
    """Steps, every indexed call, hosted threads and the exact launch counts also run while the batch has a plane."""
    on = seat_stats_of(name)["old_on_plane"]
    missing = [k for k in A.INDEXED_OPS + ["step", "timed_steps"] if not on[k]]
    # (seats-two-batches: about half of the operations go to the batch that never has a plane)
    assert len(missing) <= (8 if name == "seats-two-batches" else 3) and on["step"] >= 5, (name, missing, dict(on))


def test_every_indexed_kind_meets_a_plane_somewhere():
    on = Counter()
    for name in SEAT_NAMES:
        on.update(seat_stats_of(name)["old_on_plane"])
    assert all(on[k] >= 2 for k in A.INDEXED_OPS + ["step", "timed_steps"]), dict(on)


def test_every_new_refusal_occurs():
    hows = Counter()
    for name in SEAT_NAMES:
        hows.update(seat_stats_of(name)["hows"])
    for kind, forms in A.SEAT_REFUSALS.items():
        for how in forms:
            assert hows[(kind, how)] >= 1, (kind, how, dict(hows))


def test_seat_entry_counts_lie_on_both_sides_of_each_threshold():
    for name in SEAT_NAMES:
        st = seat_stats_of(name)
        total = sum(r for segs, _, _, _ in dict(A.SEAT_SCENARIOS)[name][:1] for _, _, r, _ in segs)
        for n in A.SET_SEATS_SIDES + (total,):
            assert st["set_counts"][n] >= 1, (name, n, dict(st["set_counts"]))
        assert min(st["set_counts"]) < 40, (name, dict(st["set_counts"]))
        if any(r >= 193 for segs, _, _, _ in dict(A.SEAT_SCENARIOS)[name][:1] for _, _, r, _ in segs):
            for n in A.FIND_SIDES:
                assert any(c["count"] == n and c["cap"] >= n for c in st["find"]), (name, n)


@pytest.mark.parametrize("name", SEAT_NAMES)
def test_find_rooms_is_not_answered_trivially(name):
    st = seat_stats_of(name)
    calls = st["find"]
    assert {c["want"] for c in calls} == set(range(1, 8)), name
    for bit in (A.PERSON, A.END, A.PHASE):                          # some rooms of the range match this bit and some do not
        assert any(c["want"] == bit and 0 < c["n_match"] < c["count"] for c in calls) or \
               any(c["want"] & bit and 0 < sum(1 for h in c["hits"] if h[1] & bit) < c["count"] for c in calls), (name, bit)
    assert any(0 < c["cap"] < c["n_match"] for c in calls), (name, "no truncated scan")
    assert any(c["cap"] == 0 and c["n_match"] for c in calls) and any(c["cap"] > c["n_match"] > 0 for c in calls), name
    assert any(c["first"] == 0 and c["count"] == sum(r for _, _, r, _ in dict(A.SEAT_SCENARIOS)[name][0][0]) for c in calls), name
    if len(dict(A.SEAT_SCENARIOS)[name][0][0]) > 1:
        lo = np.cumsum([0] + [r for _, _, r, _ in dict(A.SEAT_SCENARIOS)[name][0][0]])
        assert any(((lo[1:-1] > c["first"]) & (lo[1:-1] < c["first"] + c["count"])).any() and c["count"] < lo[-1] for c in calls), name
    assert any(c["masks"] is not None for c in calls)
    # the people the serving loop finds are the rooms' own
    assert sum(len(r["rooms"]) for r in st["served"]) >= 8, name


@pytest.mark.parametrize("name", SEAT_NAMES)
def test_advise_seats_is_not_a_call_of_refusals(name):
    st = seat_stats_of(name)
    for want in st["advice"]:
        assert 2 * int((want["legal"] != 0).sum()) >= len(want), (name, want["legal"].tolist())
    assert st["views"] == {False, True}, name
    assert {m for _, m in st["advise_RM"]} <= set(A.ADVISE_TURNS) and {r for r, _ in st["advise_RM"]} <= set(A.N_ROLLOUTS)


def test_some_advice_is_not_the_lowest_legal_choice():
    differs = decided = 0
    turns, rollouts = set(), set()
    for name in SEAT_NAMES:
        st = seat_stats_of(name)
        turns |= {m for _, m in st["advise_RM"]}
        rollouts |= {r for r, _ in st["advise_RM"]}
        for want in st["advice"] + [r["advice"] for r in st["served"]]:
            for w in want[want["legal"] != 0]:
                decided += 1
                differs += int(int(w["best"]) != (int(w["legal"]) & -int(w["legal"])).bit_length())
    print("advised entries", decided, "best other than the lowest legal choice", differs)
    assert differs >= 5 and decided > differs
    assert turns == set(A.ADVISE_TURNS) and len(rollouts) >= 2, (turns, rollouts)


@pytest.mark.parametrize("name", SEAT_NAMES)
def test_masks_matter(name):
    """Listed rooms whose turn under their own mask differs from the same turn under the segment's mask."""
    assert seat_stats_of(name)["cov"]["masks_matter"] >= 10, (name, dict(seat_stats_of(name)["cov"]))


@pytest.mark.parametrize("name", SEAT_WEREWOLF)
def test_role_deals_meet_the_other_step_path(name):
    """A plain step deals roles in a record a seat step stored (no prepared deal), and a seat step deals roles in a record a plain
    step stored (its prepared deal must be ignored)."""
    cov = seat_stats_of(name)["cov"]
    assert cov["plain_step_assigns_after_seat_step"] >= 3 and cov["seat_step_assigns_after_step"] >= 3, (name, dict(cov))


def test_a_game_restarted_under_seat_steps_is_dealt_from_the_side_plane():
    cov = seat_stats_of("seats-ww12-400-fused")["cov"]
    assert cov["restart_under_seat_step_then_plain_single_turn_deal"] >= 1, dict(cov)


@pytest.mark.parametrize("name", SEAT_UNTRACED)
def test_cached_graphs_are_replayed_after_seat_steps(name):
    cov = seat_stats_of(name)["cov"]
    assert cov["graph_replay_after_seat_steps"] >= 1 and cov["set_seats_behind_graph_step"] >= 1, (name, dict(cov))


def test_launch_counts_are_read_exactly_with_and_without_a_plane():
    """timed_steps on batches with a plane (one launch per segment and per max_fuse turns) and without one."""
    seen = Counter()
    for name in SEAT_NAMES:
        seen.update(seat_stats_of(name)["timed_planes"])
    assert seen[True] + seen[4] >= 2 and seen[False] + seen[1] >= 2, dict(seen)
    assert seat_stats_of("seats-mixed-4seg")["timed_planes"][4] >= 1, dict(seat_stats_of("seats-mixed-4seg")["timed_planes"])


STREAMS_DIGEST = "148c970e0b295cb0525ffe44d2dc61c8f7ebacbec3ba5087ba5ae6754fc3f0d2"


def test_the_old_scenarios_never_draw_a_seat_kind():
    """The operation streams of the nine older scenarios are what they were before the seat kinds existed: sha256 over the
    scenarios' own sha256 digests of (kind, listed rooms) per operation at seeds 0 and 1, taken from the model file as it was
    before SEAT_SCENARIOS was added.  A change that moves it has changed what those eighteen GPU cases run."""
    for name in A.SCENARIO_NAMES:
        assert not set(stats_of(name)["ops"]) & (set(A.SEAT_OPS) | set(A.SEAT_REFUSALS)), name
    assert hashlib.sha256("".join(stats_of(n)["digest"] for n in A.SCENARIO_NAMES).encode()).hexdigest() == STREAMS_DIGEST


def test_the_late_side_plane_comes_after_indexed_writes():
    st = stats_of("ww12-300-late-plane")
    assert st["write_at_before_plane"] >= 1 and st["indexed_before_plane"] >= 1, st
    assert any(k % 16 == 1 for k in st["step_ks"]), st["step_ks"]  # ... and it is allocated in the end

"""The indexed-call sequence fuzz reaches what it is for (no GPU): tests/abi_model.py's operation stream - the one
tests/test_gpu_abi_indexed_sequences.py replays against the library, same scenarios, same default seeds - is drawn on the
oracle model alone and measured.  These are properties of the generator, its seeds and its weights: a change that loses one of
them makes the GPU fuzz blind to the orders it exists for (a prepared deal of the batch's key under an indexed turn, a record
without one under a whole-batch step, stale staging pointers across a regrow, an indexed call behind an unsynchronised graph
replay), and shows here first."""
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
    for seed in DEFAULT_SEEDS:
        t0 = time.perf_counter()
        prev, plane, draws, n_ops = {}, {}, None, 0
        for op, draws in A.draw_ops(name, seed):
            n_ops += 1
            st["ops"][op.kind] += 1
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


def test_the_late_side_plane_comes_after_indexed_writes():
    st = stats_of("ww12-300-late-plane")
    assert st["write_at_before_plane"] >= 1 and st["indexed_before_plane"] >= 1, st
    assert any(k % 16 == 1 for k in st["step_ks"]), st["step_ks"]  # ... and it is allocated in the end

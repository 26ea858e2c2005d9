"""ge_batch_find_rooms between every other call that moves rooms (-m gpu): a seeded random interleaving of step, inject_actions,
write_rooms_at, step_rooms, run_rooms, reset, set_turn and find_rooms; every find_rooms result equals tests/find_ref.py evaluated
on the batch's own rooms (read_rooms, turned into oracle rooms) at that moment."""
import numpy as np
import pytest

from find_ref import case_facts, expected_hits, hits_as_tuples, room_facts
from game_engine_amd import GameTable, RoomBatch
from parity_util import oracle_rooms_as_views, views_as_oracle_rooms
from run_ref import PHASE, SEED

pytestmark = pytest.mark.gpu

PER, OPS = 130, 200


def _facts_now(b, segs):
    views = b.read_rooms()
    return [room_facts(orc, views_as_oracle_rooms(orc, views[g * PER:(g + 1) * PER]), mask) for g, (orc, _, _, mask, _) in enumerate(segs)]


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("name", ["ww8_h2", "mixed"])
def test_find_rooms_in_a_random_interleaving(name, seed):
    segs, _ = case_facts(name, PER, True)
    rng = np.random.default_rng(1000 * seed + len(name))
    total = PER * len(segs)
    finds = hits_seen = 0
    with RoomBatch([(GameTable(dsl), n, PER, mask) for _, dsl, n, mask, _ in segs], seed=SEED, first_room=31, max_fuse=int(rng.choice([0, 1, 4])),
                   restart=True) as b:
        def put_starts():
            for g, (orc, _, _, _, rooms) in enumerate(segs):
                b.write_rooms(g * PER, oracle_rooms_as_views(orc, rooms))

        put_starts()
        for op in range(OPS):
            kind = rng.choice(["step", "inject", "write_at", "step_rooms", "run_rooms", "reset", "set_turn", "find"],
                              p=[0.2, 0.15, 0.08, 0.12, 0.1, 0.02, 0.03, 0.3])
            listed = rng.permutation(total)[: int(rng.integers(1, 90))]
            if kind == "step":
                b.step(int(rng.choice([1, 2, 5, 9])))
            elif kind == "inject":                               # many are refused: what is accepted moves `acted`, and so `pending`
                seats = np.array([int(rng.integers(1, segs[int(r) // PER][2] + 1)) for r in listed])
                b.inject_actions(listed, seats, rng.integers(1, 5, len(listed)))
            elif kind == "write_at":                             # rooms of a segment copied over other rooms of it
                g = int(rng.integers(0, len(segs)))
                src = g * PER + rng.permutation(PER)[:20]
                b.write_rooms_at(g * PER + rng.permutation(PER)[:20], b.read_rooms_at(src))
            elif kind == "step_rooms":
                b.step_rooms(listed, rng.choice(1 << 40, size=len(listed), replace=False), rng.integers(0, 500, len(listed)))
            elif kind == "run_rooms":
                b.run_rooms(listed, rng.choice(1 << 40, size=len(listed), replace=False), rng.integers(0, 500, len(listed)),
                            max_turns=int(rng.integers(1, 12)), until=int(rng.integers(0, 8)), views=False)
            elif kind == "reset":
                b.reset()
                put_starts()
            elif kind == "set_turn":
                b.set_turn(int(rng.integers(0, 1000)))
            else:
                want = int(rng.integers(1, 8))
                masks = [int(rng.integers(0, 1 << len(orc.ids))) for orc, _, _, _, _ in segs]
                first = int(rng.integers(0, total))
                count = int(rng.integers(0, total - first + 1))
                cap = int(rng.choice([count, 3, 0]))
                phases = {g: [p for p in range(32) if (m >> p) & 1] for g, m in enumerate(masks)} if want & PHASE else None
                hits, n_match = b.find_rooms(want, phases, first, count, cap)
                ref = expected_hits(_facts_now(b, segs), want, masks, first, count)
                assert n_match == len(ref) and hits_as_tuples(hits) == ref[:cap], (name, seed, op, want, first, count, cap)
                finds += 1
                hits_seen += len(hits)
    assert finds > 30 and hits_seen > 0

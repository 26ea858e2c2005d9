"""The oracle side of the C-ABI sequence tests (tests only): Model, one room array per segment + the turn counter, with one method
per ABI call - the indexed calls composed from the references restated on the oracle (run_ref, playout_ref, halving_ref,
run_playout_ref, timeline_ref, rollout_*_ref, compare_ref), no rule logic of its own - and draw_ops, the seeded operation stream
tests/test_gpu_abi_indexed_sequences.py replays on the GPU and tests/test_abi_model_host.py measures on the model alone: every
operation is applied to the model when it is drawn and carries what the library must return for it.

The seat plane is part of the model: Model.masks is None or one mask per batch room, mask_of(room) what every indexed reference
plays a room under, and with a plane Model.step is the header's definition - room r takes ge_batch_step_rooms's entry (r, first
+ r, turn + t) under its own mask.  set_seats / get_seats / clear_seats, find_rooms (find_ref.find_ref over seats_ref.pending_of
under each room's own mask) and advise_seats (advise_ref.reference_advice on a copy of the room) are composed like the other
calls.  Their operation kinds (SEAT_OPS, SEAT_REFUSALS, the serving loop served_rounds and the switch of step paths around a
cached graph, seat_graph_sequence) are drawn only in SEAT_SCENARIOS; the streams of SCENARIOS are what they were before these
kinds existed."""
import zlib
from collections import Counter

import numpy as np

from conftest import load_dsl
from oracle import dsl_variants
from oracle.dsl_table import EFF_ASSIGN_ROLES
from oracle.oracle import Oracle
from parity_util import oracle_events, oracle_rooms_as_views, views_as_oracle_rooms

WW, TT, WW_GENERIC = "werewolf-(mafia)", "two-truths-and-a-lie", "ww_generic"
GE_ERR_ARG, GE_ERR_RANGE = -1, -6
PERSON, END, PHASE = 1, 2, 4
M64 = (1 << 64) - 1
EV_FIELDS = ("turn", "from_phase_id", "to_phase_id", "acted_now", "restarted", "choice")
NONE, BY_STEP, BY_INDEXED, BY_SEAT = 0, 1, 2, 3                  # what last changed a room (Model.last_mut); BY_SEAT: a whole-batch step with a plane


def dsl_for(game):
    """A segment's DSL: a committed fixture by its game name, or the GENERIC-table variant of Werewolf."""
    if game == WW_GENERIC:
        return dsl_variants.build("ww_generic", load_dsl(WW))
    return load_dsl(game)


class Model:
    """The oracle side of a batch: one room array per segment + the turn counter."""

    def __init__(self, segs, seed, first, restart):
        self.segs, self.seed, self.first, self.restart = segs, seed, first, restart
        self.orcs = [Oracle(dsl_for(g), n) for g, n, _, _ in segs]
        self.lo = np.cumsum([0] + [r for _, _, r, _ in segs]).tolist()
        self.total = self.lo[-1]
        self.masks = None                                           # the seat plane: None, or one uint32 mask per batch room
        self.reset()

    def reset(self):                                                # (the masks are configuration: a reset leaves them)
        self.rooms = [o.init_rooms(r) for o, (_, _, r, _) in zip(self.orcs, self.segs)]
        self.turn = 0
        self.last_events = None

    def mask_of(self, room):
        """The host-driven seats of a batch room: its own mask once a plane exists, else its segment's."""
        return int(self.masks[int(room)]) if self.masks is not None else self.segs[self.seg_of(int(room))[0]][3]

    def seg_of(self, room):
        k = int(np.searchsorted(self.lo, room, side="right")) - 1
        return k, room - self.lo[k]

    def views(self, lo=0, hi=None):
        hi = self.total if hi is None else hi
        parts = []
        for k, o in enumerate(self.orcs):
            a, z = max(lo, self.lo[k]), min(hi, self.lo[k + 1])
            if a < z:
                parts.append(oracle_rooms_as_views(o, self.rooms[k][a - self.lo[k]: z - self.lo[k]]))
        return np.concatenate(parts)

    def step(self, k):
        ev = []
        for t in range(k):                                          # turn by turn: the event trace is per turn
            row = []
            for s, o in enumerate(self.orcs):
                if self.masks is None:
                    o.run(self.rooms[s], self.seed, self.first + self.lo[s], self.turn, 1, threads=0, restart=self.restart,
                          human_mask=self.segs[s][3])
                else:                                               # with a plane: room r takes step_rooms's entry (r, first + r, turn) under its own mask
                    for i in range(len(self.rooms[s])):
                        o.run(self.rooms[s][i:i + 1], self.seed, self.first + self.lo[s] + i, self.turn, 1, threads=1, restart=self.restart,
                              human_mask=int(self.masks[self.lo[s] + i]))
                row.append(oracle_events(o, self.rooms[s], self.turn))
            ev.append(np.concatenate(row))
            self.turn += 1
        self.last_events = np.stack(ev, axis=1)                     # [room, turn]

    def inject(self, room, player, choice):
        if room >= self.total:
            return -6
        k, r = self.seg_of(room)
        return 0 if self.orcs[k].inject(self.rooms[k], r, player, choice) else -1

    def write(self, lo, views):
        for k, o in enumerate(self.orcs):
            a, z = max(lo, self.lo[k]), min(lo + len(views), self.lo[k + 1])
            if a < z:
                self.rooms[k][a - self.lo[k]: z - self.lo[k]] = views_as_oracle_rooms(o, views[a - lo: z - lo])

    def summary(self):
        s = {"rooms": self.total, "turn": self.turn, "finished": 0, "village_wins": 0, "wolf_wins": 0, "alive_players": 0,
             "sum_end_turn": 0, "end_turn_hist": np.zeros(16, dtype=np.int64), "score_hist": np.zeros(16, dtype=np.int64),
             "games_recycled": 0}
        for o, rooms, (_, n, _, _) in zip(self.orcs, self.rooms, self.segs):
            fin = rooms["end_turn"] >= 0
            s["finished"] += int(fin.sum())
            s["sum_end_turn"] += int(rooms["end_turn"][fin].sum())
            s["end_turn_hist"] += np.bincount(np.minimum(rooms["end_turn"][fin] // 8, 15), minlength=16)
            s["games_recycled"] += int(rooms["games"].sum())
            if o.table.pack == 1:
                alive = rooms["p"][:, :n, 2]
                wolves = ((rooms["p"][:, :n, 1] == 2) & (alive == 1)).sum(axis=1)
                s["alive_players"] += int(alive.sum())
                s["village_wins"] += int((fin & (wolves == 0)).sum())
                s["wolf_wins"] += int((fin & (wolves > 0)).sum())
            else:
                s["alive_players"] += n * len(rooms)                 # nobody is eliminated in Two-Truths
                s["score_hist"] += np.bincount(np.minimum(rooms["p"][:, :n, 7].ravel(), 15), minlength=16)
        s["end_turn_hist"], s["score_hist"] = s["end_turn_hist"].tolist(), s["score_hist"].tolist()
        return s

    # ---- the indexed calls: each composes the references of its call; the turn counter and last_events are never touched

    def orc_of(self, room):
        """(oracle, oracle record) of a batch room: what compare_ref / rollout_beliefs_ref ask for."""
        s, i = self.seg_of(int(room))
        return self.orcs[s], self.rooms[s][i]

    def step_rooms(self, listed, keys, turns):
        out = []
        for r, key, turn in zip(listed, keys, turns):
            s, i = self.seg_of(int(r))
            o, one = self.orcs[s], self.rooms[s][i:i + 1]
            o.run(one, self.seed, int(key), int(turn), 1, threads=1, restart=self.restart, human_mask=self.mask_of(r))
            out.append(oracle_events(o, one, int(turn))[0])
        return out

    def read_rooms_at(self, listed):
        return self.views()[np.asarray(listed, dtype=np.int64)]

    def write_rooms_at(self, listed, views):
        for r, v in zip(listed, views):
            s, i = self.seg_of(int(r))
            self.rooms[s][i] = views_as_oracle_rooms(self.orcs[s], np.asarray(v).reshape(1))[0]

    def run_rooms(self, listed, keys, turns, max_turns, until):
        from run_ref import run_ref
        played, stopped, events, views = [], [], [], []
        for r, key, turn in zip(listed, keys, turns):
            s, i = self.seg_of(int(r))
            p, why, ev, vw = run_ref(self.orcs[s], self.rooms[s], i, self.seed, int(key), int(turn), max_turns, until, self.restart,
                                     self.mask_of(r))
            played.append(p); stopped.append(why); events.append(ev); views.append(vw)
        return np.array(played, dtype=np.uint32), np.array(stopped, dtype=np.uint32), events, views

    def step_rooms_playout(self, listed, keys, turns, masks, pkeys, R, M, pseed, full_view, halving):
        from halving_ref import reference_step_playout_halving
        from playout_ref import reference_step_playout
        step = reference_step_playout_halving if halving else reference_step_playout
        events, decided = [], []
        for r, key, turn, mask, pkey in zip(listed, keys, turns, masks, pkeys):
            s, i = self.seg_of(int(r))
            o = self.orcs[s]
            d = step(o, self.rooms[s], i, self.seed, int(key), int(turn), int(mask), int(pkey), pseed, R, M, full_view, self.restart,
                     self.mask_of(r))
            events.append(oracle_events(o, self.rooms[s][i:i + 1], int(turn))[0])
            decided.append(d)
        return events, np.array(decided, dtype=np.uint32)

    def run_rooms_playout(self, listed, keys, turns, masks, pkeys, R, M, pseed, full_view, max_turns, until):
        from run_playout_ref import run_playout_ref
        played, stopped, events, views, decided = [], [], [], [], []
        for r, key, turn, mask, pkey in zip(listed, keys, turns, masks, pkeys):
            s, i = self.seg_of(int(r))
            p, why, ev, vw, dec = run_playout_ref(self.orcs[s], self.rooms[s], i, self.seed, int(key), int(turn), int(mask), int(pkey), pseed,
                                                  R, M, full_view, max_turns, until, self.restart, self.mask_of(r))
            played.append(p); stopped.append(why); events.append(ev); views.append(vw); decided.append(dec)
        return np.array(played, dtype=np.uint32), np.array(stopped, dtype=np.uint32), events, views, decided

    def run_rooms_forecast(self, listed, keys, turns, fkeys, seats, R, M, fseed, max_turns, until):
        from timeline_ref import timeline_of
        starts = [self.orc_of(r)[1].copy() for r in listed]
        played, stopped, events, views = self.run_rooms(listed, keys, turns, max_turns, until)
        stats = [timeline_of(self.orc_of(r)[0], starts[k], views[k], fseed, int(fkeys[k]), int(turns[k]), int(seats[k]), R, M)
                 for k, r in enumerate(listed)]
        return played, stopped, events, views, stats

    # the rollouts only read: each entry runs on a copy of the model's room
    def rollout_rooms(self, listed, keys, turns, R, M, pseed):
        from rollout_ref import reference_rollout
        return np.stack([reference_rollout(self.orc_of(r)[0], self.orc_of(r)[1].copy(), pseed, int(k), int(t), R, M)
                         for r, k, t in zip(listed, keys, turns)])

    def rollout_actions(self, listed, keys, turns, actions, R, M, pseed):
        from rollout_actions_ref import reference_rollout_actions
        got = [reference_rollout_actions(self.orc_of(r)[0], self.orc_of(r)[1].copy(), pseed, int(k), int(t), a, R, M)
               for r, k, t, a in zip(listed, keys, turns, actions)]
        return np.stack([w for w, _ in got]), np.array([s for _, s in got], dtype=np.int32)

    def rollout_seats(self, listed, keys, turns, seats, actions, R, M, pseed):
        from rollout_seats_ref import reference_rollout_seats
        got = [reference_rollout_seats(self.orc_of(r)[0], self.orc_of(r)[1].copy(), pseed, int(k), int(t), int(s), a, R, M)
               for r, k, t, s, a in zip(listed, keys, turns, seats, actions)]
        return np.stack([w for w, _ in got]), np.array([s for _, s in got], dtype=np.int32)

    def rollout_beliefs(self, listed, keys, turns, seats, actions, beliefs, R, M, pseed):
        from rollout_beliefs_ref import reference_beliefs
        words, status, _ = reference_beliefs(self.orc_of, listed, keys, turns, seats, actions, beliefs, R, M, pseed)
        return words, status

    def rollout_compare(self, listed, keys, turns, seats, actions, baseline, subjects, R, M, pseed):
        from compare_ref import reference_compare
        return reference_compare(self.orc_of, listed, keys, turns, seats, actions, baseline, subjects, R, M, pseed)

    # ---- the seat plane (ge_step.h, "Per-room host-driven seats"): configuration, which reset, write, write_rooms_at and the turn
    # counter leave alone

    def set_seats(self, rooms, masks):
        """ge_batch_set_seats: the status; a refused call changes nothing, the first accepted one of n > 0 allocates the plane."""
        rooms = [int(r) for r in rooms]
        if not rooms:
            return 0
        if any(r >= self.total for r in rooms):
            return GE_ERR_RANGE
        if len(set(rooms)) != len(rooms):
            return GE_ERR_ARG
        if any(int(k) >> self.segs[self.seg_of(r)[0]][1] for r, k in zip(rooms, masks)):
            return GE_ERR_ARG
        if self.masks is None:
            self.masks = np.concatenate([np.full(r, mask, dtype=np.uint32) for _, _, r, mask in self.segs])
        self.masks[rooms] = np.asarray(masks, dtype=np.uint32)
        return 0

    def get_seats(self, first=0, count=None):
        count = self.total - first if count is None else count
        return np.array([self.mask_of(r) for r in range(first, first + count)], dtype=np.uint32)

    def clear_seats(self):
        self.masks = None

    def find_rooms(self, first, count, want, phase_masks, cap):
        """ge_batch_find_rooms: (the first cap hits as (room, why, pending, phase_id, segment), n_match) - find_ref.find_ref over
        each room's facts, `pending` by seats_ref.pending_of under the room's own mask."""
        from find_ref import find_ref
        from run_ref import is_terminal
        from seats_ref import pending_of
        hits = []
        for r in range(first, first + count):
            s, i = self.seg_of(r)
            o, one = self.orcs[s], self.rooms[s][i:i + 1]
            fact = (pending_of(o, one, self.mask_of(r)) if want & PERSON else 0, bool(is_terminal(o, one)), int(o.ids[int(one["phase"][0])]))
            why, pending, pid = find_ref([fact], want, int(phase_masks[s]) if phase_masks is not None else 0)[0]
            if why:
                hits.append((r, why, pending, pid, s))
        return hits[:cap], len(hits)

    def advise_seats(self, listed, keys, turns, seats, R, M, aseed, full_view):
        """ge_batch_advise_seats: advise_ref.reference_advice of each entry on a copy of its room."""
        from advise_ref import ADVICE_REF_DTYPE, reference_advice
        return np.array([reference_advice(self.orc_of(r)[0], self.orc_of(r)[1].copy(), aseed, int(k), int(t), int(s), R, M, full_view)
                         for r, k, t, s in zip(listed, keys, turns, seats)], dtype=ADVICE_REF_DTYPE)


class TrackedModel(Model):
    """Model + what the operation stream needs to know about its own past (tests/test_abi_model_host.py reads cov): which kind
    of call last wrote each room, and how often the orders the sequence fuzz exists for were reached.  Nothing here changes what
    a call returns."""

    def __init__(self, segs, seed, first, restart):
        # the phase ids whose entry deals the roles (Werewolf), per segment
        orcs = [Oracle(dsl_for(g), n) for g, n, _, _ in segs]
        self.assign_ids = [{o.ids[i] for i, ph in enumerate(o.table.phases) if ph.effect == EFF_ASSIGN_ROLES} for o in orcs]
        self.cov = Counter()
        self.fuse, self.had_plane_now = 1, False                    # (fuse: the batch's max_fuse, set by the generator)
        super().__init__(segs, seed, first, restart)

    def reset(self):
        super().reset()
        self.last_mut = np.zeros(self.total, dtype=np.uint8)
        # rooms whose game ended and was recycled under a seat step and has not been dealt since: their next deal is the first that
        # the other step path makes for them
        self.seat_restarted = np.zeros(self.total, dtype=bool)
        # rooms in which a single indexed turn (ge_pool_kernel) dealt the roles over a record a whole-batch step wrote: were that
        # record's prepared deal - of the game just dealt - stored back, the next game's whole-batch deal would take it
        self.kept_deal = np.zeros(self.total, dtype=bool)

    def _assigned(self, s, ev):
        """Which of segment s's events moved their room into a role-assignment phase."""
        if not self.assign_ids[s]:
            return np.zeros(len(ev), dtype=bool)
        return np.isin(ev["to_phase_id"], list(self.assign_ids[s])) & (ev["to_phase_id"] != ev["from_phase_id"])

    def step(self, k):
        turns = []
        for t in range(k):
            super().step(1)
            e = self.last_events[:, 0]
            hit = np.concatenate([self._assigned(s, e[self.lo[s]: self.lo[s + 1]]) for s in range(len(self.orcs))])
            if self.masks is not None:
                # a seat step (ge_seat_step_kernel): the record's prepared deal is ignored, roles are dealt on the spot, the record is
                # stored without a deal and the Werewolf x 12 side plane is not touched
                self.cov["seat_step_assigns_after_step"] += int((hit & (self.last_mut == BY_STEP)).sum())
                self.seat_restarted = (self.seat_restarted | (e["restarted"] != 0)) & ~hit
                self.kept_deal[:] = False
                self.last_mut[:] = BY_SEAT
                turns.append(e)
                continue
            self.cov["step_assigns_after_indexed"] += int((hit & (self.last_mut == BY_INDEXED)).sum())
            self.cov["plain_step_assigns_after_seat_step"] += int((hit & (self.last_mut == BY_SEAT)).sum())
            self.cov["step_assigns_game_after_indexed_deal"] += int((hit & self.kept_deal).sum())
            if self.fuse == 1 or (t == k - 1 and k % self.fuse == 1):   # a single-turn launch: Werewolf x 12 deals come from the side plane
                for s, (_, n, _, _) in enumerate(self.segs):
                    if n == 12 and self.assign_ids[s]:
                        self.cov["restart_under_seat_step_then_plain_single_turn_deal"] += int((hit & self.seat_restarted)[self.lo[s]: self.lo[s + 1]].sum())
            self.seat_restarted &= ~hit
            self.kept_deal &= ~hit
            self.last_mut[:] = BY_STEP
            turns.append(e)
        self.last_events = np.stack(turns, axis=1)

    def set_seats(self, rooms, masks):
        st = super().set_seats(rooms, masks)
        self.cov["set_seats_allocates"] += int(st == 0 and len(rooms) > 0 and not self.had_plane_now)
        self.had_plane_now = self.masks is not None
        return st

    def clear_seats(self):
        self.cov["clear_with_plane" if self.masks is not None else "clear_without_plane"] += 1
        super().clear_seats()
        self.had_plane_now = False

    def write(self, lo, views):
        super().write(lo, views)
        self.last_mut[lo: lo + len(views)] = NONE
        self.kept_deal[lo: lo + len(views)] = False
        self.seat_restarted[lo: lo + len(views)] = False

    def write_rooms_at(self, listed, views):
        super().write_rooms_at(listed, views)
        idx = np.asarray(listed, dtype=np.int64)
        self.last_mut[idx] = BY_INDEXED
        self.kept_deal[idx] = False
        self.seat_restarted[idx] = False

    def _note(self, room, events, call):
        """The turns indexed call `call` played on a room.  indexed_assigns_after_step counts a step_rooms entry or a run whose
        first turn - the one that loaded the record a whole-batch step wrote, with whatever prepared deal of the batch's own key it
        carries - moved the room into role assignment.  A single indexed turn (ge_pool_kernel: step_rooms, a hosted thread's
        round, a playout step) keeps the record's other bits as they are; the run kernels store a record of their own."""
        room = int(room)
        s, _ = self.seg_of(room)
        ev = np.array(events).reshape(-1)
        single = call in ("step_rooms", "hosted_threads", "step_rooms_playout", "served_rounds")
        first = bool(self._assigned(s, ev[:1])[0])
        if self.last_mut[room] == BY_STEP and first:
            self.cov["indexed_assigns_after_step"] += int(call in ("step_rooms", "run_rooms", "run_rooms_playout"))
            self.kept_deal[room] = single
        if not single:
            self.kept_deal[room] = False
        self.cov["indexed_restarted"] += int(ev["restarted"].sum())
        if self._assigned(s, ev).any():
            self.seat_restarted[room] = False
        self.last_mut[room] = BY_INDEXED

    def step_rooms(self, listed, keys, turns, call="step_rooms"):
        if self.masks is not None:                                  # masks_matter: the same turn under the segment's mask gives another record
            for r, key, turn in zip(listed, keys, turns):
                s, i = self.seg_of(int(r))
                if self.mask_of(r) != self.segs[s][3]:
                    own, seg = self.rooms[s][i:i + 1].copy(), self.rooms[s][i:i + 1].copy()
                    self.orcs[s].run(own, self.seed, int(key), int(turn), 1, threads=1, restart=self.restart, human_mask=self.mask_of(r))
                    self.orcs[s].run(seg, self.seed, int(key), int(turn), 1, threads=1, restart=self.restart, human_mask=self.segs[s][3])
                    self.cov["masks_matter"] += int(own.tobytes() != seg.tobytes())
        out = super().step_rooms(listed, keys, turns)
        for r, e in zip(listed, out):
            self._note(r, [e], call)
        return out

    def run_rooms(self, listed, keys, turns, max_turns, until):
        got = super().run_rooms(listed, keys, turns, max_turns, until)
        for r, why, ev in zip(listed, got[1], got[2]):
            self._note(r, ev, "run_rooms")
            for bit, name in ((PERSON, "person"), (END, "end"), (PHASE, "phase")):
                self.cov["run_stop_" + name] += int(bool(int(why) & bit))
            self.cov["run_stop_limit"] += int(why == 0)
        return got

    def step_rooms_playout(self, listed, keys, turns, *rest):
        from playout_ref import policy_choice
        before = [self.orc_of(r)[1].copy() for r in listed]
        events, decided = super().step_rooms_playout(listed, keys, turns, *rest)
        for r, key, turn, rec, e, dmask in zip(listed, keys, turns, before, events, decided):
            o = self.orc_of(r)[0]
            for seat in range(1, o.n + 1):
                if (int(dmask) >> (seat - 1)) & 1:
                    self.cov["playout_decisions"] += 1
                    self.cov["playout_not_policy"] += int(int(e["choice"][seat - 1]) != policy_choice(o, rec, self.seed, int(key), int(turn), seat))
            self._note(r, [e], "step_rooms_playout")
        return events, decided

    def run_rooms_playout(self, listed, *rest):
        got = super().run_rooms_playout(listed, *rest)
        for r, ev in zip(listed, got[2]):
            self._note(r, ev, "run_rooms_playout")
        return got


# ---- the scenarios: (name, [batch, ...]); a batch is (segments, max_fuse, restart, trace), a segment (game, players, rooms, mask)
SCENARIOS = [
    # the record's prepared deal (word 7's upper half) is in play on every launch
    ("ww8-300-single", [([(WW, 8, 300, 0b1)], 1, True, True)]),
    # steps of {1, 2, 4, 13} turns: 13 = four launches, the graph path, its tail a single turn
    ("ww8-4096-fused", [([(WW, 8, 4096, 0b101)], 4, True, False)]),
    # the side plane of prepared deals exists from the first step
    ("ww12-300-single", [([(WW, 12, 300, 0b1)], 1, True, False)]),
    # ... and here only from the first step of 16 k + 1 turns, which comes after indexed calls and a write_rooms_at
    ("ww12-300-late-plane", [([(WW, 12, 300, 0b1)], 16, True, False)]),
    ("tt4-600", [([(TT, 4, 600, 0b10)], 3, True, True)]),          # no action queue: no dynamic LDS in the indexed kernels
    ("tt7-600", [([(TT, 7, 600, 0b1000000)], 8, True, False)]),    # the queue form
    # one launch per segment in every indexed call; 40-, 24- and 32-byte records at the 4 KB threshold of rooms_io
    ("mixed-4seg", [([(WW, 12, 102, 0b1), (TT, 4, 170, 0b11), (WW, 8, 128, 0b10), (TT, 7, 150, 0)], 2, True, False)]),
    ("ww8-generic-300", [([(WW_GENERIC, 8, 300, 0b10)], 2, True, False)]),   # the GENERIC builds of every indexed kernel
    # two batches alive together: buffers, graph caches and the rejected room are per batch or per thread
    ("two-batches", [([(WW, 8, 256, 0b1)], 4, True, True),
                     ([(WW, 12, 90, 0b1), (TT, 4, 120, 0b10), (WW, 8, 100, 0)], 1, True, False)]),
]
SCENARIO_NAMES = [s[0] for s in SCENARIOS]

# ---- the scenarios of the seat plane, ge_batch_find_rooms and ge_batch_advise_seats: the operation kinds of SEAT_OPS and
# SEAT_REFUSALS are drawn only here, next to every kind above.  400 rooms: a partial last wavefront, set_seats lists on both sides
# of 341 | 342 entries and a find_rooms range of 192 | 193 rooms inside one segment
MIXED_SEGS = [(WW, 12, 102, 0b1), (TT, 4, 170, 0b11), (WW, 8, 128, 0b10), (TT, 7, 150, 0)]
SEAT_SCENARIOS = [
    ("seats-ww8-400-traced", [([(WW, 8, 400, 0b1)], 1, True, True)]),
    ("seats-ww12-400-fused", [([(WW, 12, 400, 0b1)], 4, True, False)]),       # graphs and the deal side plane on the other step path
    ("seats-tt4-400", [([(TT, 4, 400, 0b10)], 3, True, True)]),
    ("seats-tt7-400", [([(TT, 7, 400, 0b1000000)], 8, True, False)]),         # the queue form: a wavefront probes the union of its lanes' masks
    ("seats-mixed-4seg", [(MIXED_SEGS, 2, True, False)]),
    ("seats-ww8-generic-400", [([(WW_GENERIC, 8, 400, 0b10)], 2, True, False)]),   # the GENERIC seat-step, find and advise kernels
    # the first batch gets a plane; the second, alive beside it, never does and behaves as before
    ("seats-two-batches", [([(WW, 8, 400, 0b1)], 4, True, False), ([(TT, 4, 120, 0b10), (WW, 12, 90, 0b1)], 1, True, True)]),
]
SEAT_SCENARIO_NAMES = [s[0] for s in SEAT_SCENARIOS]
ALL_SCENARIOS = SCENARIOS + SEAT_SCENARIOS

OLD_OPS = {"step": 6, "read": 2, "read_part": 2, "write": 3, "inject": 2, "inject_many": 3, "reset": 2, "set_turn": 2, "summary": 2,
           "events": 2}
INDEXED_OPS = ["step_rooms", "read_rooms_at", "write_rooms_at", "run_rooms", "run_rooms_playout", "run_rooms_forecast",
               "step_rooms_playout", "step_rooms_playout_halving", "rollout_rooms", "rollout_actions", "rollout_seats",
               "rollout_beliefs", "rollout_compare", "hosted_threads"]
REFUSALS = ["refuse_repeat", "refuse_range", "refuse_turn", "refuse_view"]
TIMING_OPS = {"set_timing": 3, "kernel_time": 2, "timed_steps": 3}
SEAT_OLD_OPS = {"step": 5, "read": 1, "read_part": 1, "write": 2, "inject": 1, "inject_many": 2, "reset": 1, "set_turn": 1, "summary": 1,
                "events": 1}
SEAT_TIMING_OPS = {"set_timing": 2, "kernel_time": 1, "timed_steps": 2}
SEAT_OPS = {"set_seats": 4, "get_seats": 2, "clear_seats": 2, "find_rooms": 5, "advise_seats": 3, "served_rounds": 2}
# the new refusals, one call of each kind a case; which of its forms a case draws goes round with the case
SEAT_REFUSALS = {"refuse_set_seats": ("range", "repeat", "mask_bit"),
                 "refuse_find_rooms": ("want_zero", "unknown_bit", "beyond", "phase_bit"),
                 "refuse_advise_seats": ("seat_zero", "seat_above", "turn_overflow"),
                 "refuse_playout_seat": ("step_rooms_playout", "run_rooms_playout")}
MUTATING_INDEXED = {"hosted_threads", "step_rooms", "write_rooms_at", "run_rooms", "run_rooms_playout", "run_rooms_forecast", "step_rooms_playout",
                    "step_rooms_playout_halving"}


def deck():
    """The operations of one case, before the seeded shuffle: 66, of which 32 are indexed calls (each kind twice, each refusal
    once), so that the two default fuzz seeds hold every kind at least three times and every refusal.  (timed_steps holds
    steps of its own; draw_ops adds two multi-launch steps between indexed calls where a batch is not traced.)"""
    d = []
    for k, c in OLD_OPS.items():
        d += [k] * c
    for k in INDEXED_OPS:
        d += [k] * 2
    d += REFUSALS
    for k, c in TIMING_OPS.items():
        d += [k] * c
    return d


def seat_deck(rng, fuzz_seed):
    """The operations of a seat-plane case before the shuffle: every kind of deck() (the whole-batch kinds and the indexed calls
    fewer times: they have their own scenarios), the kinds of SEAT_OPS, one of each new refusal and one seat_graph_sequence
    (draw_ops).  Shuffled here, then the set_seats and clear_seats put in an order in which the first of
    them allocates the plane, a clear_seats meets a plane and the last set_seats allocates a plane again."""
    d = []
    for k, c in list(SEAT_OLD_OPS.items()) + list(SEAT_TIMING_OPS.items()) + list(SEAT_OPS.items()):
        d += [k] * c
    d += INDEXED_OPS + REFUSALS[fuzz_seed % 2::2] + list(SEAT_REFUSALS) + ["seat_graph_sequence"]
    rng.shuffle(d)
    at = [i for i, k in enumerate(d) if k in ("set_seats", "clear_seats")]
    order = ["set_seats"] + [str(k) for k in rng.permutation(["set_seats", "set_seats", "clear_seats"])] + ["clear_seats", "set_seats"]
    for i, k in zip(at, order):
        d[i] = k
    return d


# Entry counts on both sides of the device scratch's first size, 4 096 B (pool_scratch; the pinned staging grows with the same
# totals), from the staging layouts of the calls:
#   step_rooms      up16(20 n) + 16 n           113: 2 272 + 1 808 = 4 080 | 114: 2 288 + 1 824 = 4 112
#   read_rooms_at   56 n                         73: 4 088                 |  74: 4 144
#   write_rooms_at  up16(8 n) + 48 n             73: 592 + 3 504 = 4 096 (fits) | 74: 592 + 3 552 = 4 144
#   run_rooms       up16(up16(20 n) + 8 n) + 64 n T; at T = 1   44: 1 232 + 2 816 = 4 048 | 45: 1 280 + 2 880 = 4 160
#   rollout_*       >= up16(20 n) + 640 n (80 accumulator words an entry)   6: 128 + 3 840 = 3 968 | 7: 144 + 4 480 = 4 624
#   step_rooms_playout / run_rooms_playout: a playout seat takes its candidates' entries of 640 B each: above 4 096 from the first
# LARGE (about 1 500, or the whole batch where it is smaller) regrows both buffers while every earlier pointer is stale; it is
# for step_rooms, read_rooms_at (repeats allowed: always 1 500) and write_rooms_at only - their references cost one oracle call
# an entry.
LARGE = 1500
COUNTS = {"step_rooms": (1, 113, 114, LARGE), "read_rooms_at": (1, 73, 74, LARGE), "write_rooms_at": (1, 73, 74, LARGE),
          "rollout": (1, 6, 7, 113, 114), "playout": (1, 2, 5, 20, 54)}
N_ROLLOUTS = (1, 33, 64, 65)                                        # either side of one wavefront of replicas


class Op:
    """One drawn operation: kind, the batch it goes to (bi), its arguments (a), what the library must return (want), the rooms
    it lists (listed; None for the whole-batch calls) and, for a refusal, the status it must raise."""

    def __init__(self, kind, bi, **a):
        self.kind, self.bi, self.a, self.want, self.listed, self.status = kind, bi, a, None, None, None


class _Draw:
    """The generator's state of one batch: its model, snapshots for write-backs and the launch arithmetic of the timing calls."""

    def __init__(self, spec, seed, first, fuzz_seed):
        self.segs, self.fuse, self.restart, self.trace = spec
        self.m = TrackedModel(self.segs, seed, first, self.restart)
        self.m.fuse = self.fuse
        self.seatable, self.had_plane = True, False                 # may get a seat plane; has or had one
        self.graphs, self.seat_moved, self.prev_big = [], False, False   # the n_turns replayed as graphs; seat steps since the last replay
        self.snapshots = []
        self.nmax = max(n for _, n, _, _ in self.segs)
        self.timing = False
        self.launches, self.pure = 0, False                        # since the last kernel_time(reset=True); pure: only steps
        self.fuzz_seed, self.runs, self.calls = fuzz_seed, 0, Counter()
        self.plane_ready = False                                    # ww12-300-late-plane: a write_rooms_at and an indexed turn were seen
        self.seen = set()


def _terminal(m):
    """Per batch room: its phase is terminal."""
    return np.concatenate([np.array([not ph.branches for ph in o.table.phases])[r["phase"]] for o, r in zip(m.orcs, m.rooms)])


def _ends_soon(rng, m, turns):
    """Rooms (of a sample of 1 024 a segment) that the oracle brings to a terminal phase within `turns` turns without their people."""
    out = []
    for s, o in enumerate(m.orcs):
        idx = rng.permutation(len(m.rooms[s]))[:1024]
        trial = m.rooms[s][idx].copy()
        if m.masks is None:
            o.run(trial, m.seed, 0, 0, turns, threads=0, restart=False, human_mask=m.segs[s][3])
        else:                                                       # each room without its own people
            for j, i in enumerate(idx):
                o.run(trial[j:j + 1], m.seed, j, 0, turns, threads=1, restart=False, human_mask=m.mask_of(m.lo[s] + int(i)))
        done = np.array([not ph.branches for ph in o.table.phases])[trial["phase"]]
        out.append(m.lo[s] + idx[done & ~_terminal(m)[m.lo[s] + idx]])
    return np.concatenate(out)


def _count(rng, d, kind):
    """The entry count of a step_rooms, read_rooms_at or write_rooms_at: the case's calls of a kind go round the large count, the
    two sides of the threshold and one entry or a few, so that the default seeds of every scenario hold all four."""
    one, lo, hi, large = COUNTS[kind]
    at = (2 * d.fuzz_seed + d.calls[kind]) % 4
    d.calls[kind] += 1
    return [large, lo, hi, int(rng.choice([one, int(rng.integers(2, 40))]))][at]


def _entries(rng, m, n, distinct=True, last_fit=None, far=True, ends_within=0):
    """n listed rooms (shuffled, segments interleaved), distinct keys below and above 2^32 with one near 2^64, turns below 300
    with - for the run calls - entry 0 at the last turns that fit."""
    n = min(n, m.total) if distinct else n
    listed = rng.choice(m.total, size=n, replace=False) if distinct else rng.integers(0, m.total, n)
    if distinct:
        # up to a quarter of the entries: rooms a whole-batch step has just recycled (in phase 0, last written by a step), whose
        # next turns deal roles - the records that may carry a prepared deal of the batch's own key; up to another quarter:
        # finished rooms, which an indexed turn of a restarting batch recycles
        # (a run call: and up to half that can reach their end within its turns without their people)
        phase = np.concatenate([r["phase"] for r in m.rooms])
        fresh = np.nonzero((m.last_mut == BY_STEP) & (phase == 0))[0]
        take = np.concatenate([rng.permutation(fresh)[: n // 4], rng.permutation(np.nonzero(_terminal(m))[0])[: n // 4]])
        if ends_within:
            take = np.unique(np.concatenate([take, rng.permutation(_ends_soon(rng, m, ends_within))[: max(1, n // 2)]]))[:n]
        rest = [r for r in listed.tolist() if r not in set(take.tolist())]
        listed = rng.permutation(np.concatenate([take, rest[: n - len(take)]]).astype(np.int64))
    keys = rng.choice(1 << 40, size=n, replace=False).astype(np.uint64)
    keys[::2] = rng.choice(1 << 20, size=len(keys[::2]), replace=False)
    keys[int(rng.integers(n))] = np.uint64(M64 - int(rng.integers(0, 40)))
    turns = rng.integers(0, 300, n).astype(np.uint32)
    if last_fit is not None:
        turns[0] = last_fit
    elif far and rng.random() < .5:
        turns[int(rng.integers(n))] = 0xFFFFFFFE                    # the last turn a single step can take
    return listed.astype(np.uint64), keys, turns


def _bots(m, room):
    n, mask = m.segs[m.seg_of(int(room))[0]][1], m.mask_of(room)    # (the room's own people once the batch has a seat plane)
    return [c for c in range(n) if not (mask >> c) & 1]


def _masks(rng, m, listed, whole=(), none_every=4):
    """Per listed room a playout mask of 1 - 2 seats no person plays, or of all of them (every fourth room: none; the entries
    of `whole`: all)."""
    out = np.zeros(len(listed), dtype=np.uint32)
    for k, r in enumerate(listed):
        if k % none_every != none_every - 1 or k in whole:
            bots = _bots(m, r)
            if not bots:                                            # (a room whose every seat is a person's: no playout seat)
                continue
            for c in rng.choice(bots, size=len(bots) if k % 2 or k in whole else min(len(bots), int(rng.integers(1, 3))), replace=False):
                out[k] |= np.uint32(1 << int(c))
    return out


def _prefer_deciders(rng, d, listed, keys, turns):
    """Every second entry's room (of five entries or fewer: every entry's) exchanged, where sixteen tries find one, for a room in which a seat is due to act under the
    entry's key and turn with a choice to make (playout_ref.due_seats, candidates); returns those entries: most rooms of a batch wait for a person, every other seat having acted."""
    from playout_ref import candidates, due_seats
    m = d.m
    found = set()
    used = set(int(r) for r in listed)
    for k in range(0, len(listed), 1 if len(listed) <= 5 else 2):
        for r in rng.integers(0, m.total, 16):
            o, rec = m.orc_of(r)
            due = [] if int(r) in used else due_seats(o, rec, m.seed, int(keys[k]), int(turns[k]), d.restart, m.mask_of(r))
            if any(len(candidates(o, rec, seat)) >= 2 for seat in due):
                used.add(int(r))
                found.add(k)
                listed[k] = r
                break
    return found


def _fresh(m):
    """The rooms a whole-batch step has just recycled: in phase 0 and last written by a step."""
    return np.nonzero((m.last_mut == BY_STEP) & (np.concatenate([r["phase"] for r in m.rooms]) == 0))[0]


def _hosted_threads(rng, d, n=12, max_rounds=70):
    """Game threads hosted in slots of the batch, the way a service runs them: each of up to n rooms - first the rooms a
    whole-batch step has just recycled, whose records may carry a prepared deal of the batch's key - on its own key and clock,
    round after round one inject_actions for the people of the rooms that wait for one (a choice the model accepts) and one
    step_rooms of the rooms still going.  A thread ends when its game has ended and its slot has been recycled (or after
    max_rounds turns): the next game in that slot is dealt by a whole-batch step.  Returns per round (rooms, keys, turns,
    (inject rooms, players, choices), events)."""
    m = d.m
    fresh = rng.permutation(_fresh(m))[:n]
    rest = [r for r in rng.permutation(m.total).tolist() if r not in set(fresh.tolist())]
    rooms = np.concatenate([fresh, rest[: n - len(fresh)]]).astype(np.uint64)
    keys = rng.choice(1 << 40, size=len(rooms), replace=False).astype(np.uint64)
    keys[0] = np.uint64(M64 - int(rng.integers(0, 40)))
    turns = rng.integers(0, 300, len(rooms)).astype(np.uint32)
    dealt, live = np.zeros(len(rooms), dtype=bool), np.ones(len(rooms), dtype=bool)
    rounds = []
    for t in range(max_rounds):
        if not live.any():
            break
        idx = np.nonzero(live)[0]
        inj = ([], [], [])
        for r in rooms[idx]:
            s, i = m.seg_of(int(r))
            o, mask = m.orcs[s], m.mask_of(r)
            for seat in [c + 1 for c in range(o.n) if (mask >> c) & 1]:
                for choice in rng.permutation(max(o.n, 3)) + 1:
                    if o.inject(m.rooms[s][i:i + 1].copy(), 0, seat, int(choice)):
                        assert m.inject(int(r), seat, int(choice)) == 0
                        inj[0].append(int(r)); inj[1].append(seat); inj[2].append(int(choice))
                        break
        ev = m.step_rooms(rooms[idx], keys[idx], turns[idx] + t, call="hosted_threads")
        rounds.append((rooms[idx], keys[idx], (turns[idx] + t).astype(np.uint32),
                       (np.array(inj[0], dtype=np.uint64), np.array(inj[1], dtype=np.uint32), np.array(inj[2], dtype=np.uint32)), ev))
        for j, e in zip(idx, ev):
            s, _ = m.seg_of(int(rooms[j]))
            if dealt[j] and e["restarted"]:
                live[j] = False                                     # the thread's game is over and its slot recycled
            dealt[j] |= bool(m._assigned(s, np.array([e]))[0]) or m.orcs[s].table.pack != 1
    return rounds


def _actions(rng, m, listed):
    """Per entry no action, a legal one (found on the model) or a random one (refused on the device, entry by entry)."""
    from rollout_actions_ref import inject_all
    out = []
    for r in listed:
        o, rec = m.orc_of(r)
        hi = o.n if o.table.pack == 1 else 3
        x = rng.random()
        if x < .4:
            out.append([])
            continue
        tries = [(int(rng.integers(1, o.n + 1)), int(rng.integers(1, hi + 1))) for _ in range(12)]
        legal = [a for a in tries if inject_all(o, rec, [a])[1] == 0]
        out.append([legal[0]] if legal and x < .9 else [(int(rng.integers(0, o.n + 2)), int(rng.integers(0, hi + 2)))])
    return out


def _seats(rng, m, listed):
    return np.array([int(rng.integers(0, m.orc_of(r)[0].n + 1)) for r in listed], dtype=np.uint32)


def _until_and_turns(rng, n, budget):
    """(until, max_turns) of a run call: every stop condition and none; max_turns <= 24, n * max_turns within the budget."""
    until = int(rng.choice([PERSON | END, PERSON, END | PHASE, 0, PHASE, END, PERSON | END | PHASE]))
    T = int(rng.choice([t for t in (1, 3, 8, 24) if n * t <= budget] or [1]))
    return until, T


def _pairs(rng, choices, budget, n_of=lambda n: n):
    """(entry count, n_rollouts) with the oracle's work n_of(count) * n_rollouts within the budget."""
    while True:
        n, R = int(rng.choice(choices)), int(rng.choice(N_ROLLOUTS))
        if n_of(n) * R <= budget:
            return n, R


def draw_ops(name, fuzz_seed):
    """The operations of case (scenario, fuzz seed), in order, each already applied to the model of its batch.  Yields
    (op, draws): draws[op.bi].m is that model as the operation left it."""
    for op, draws in _draw_stream(name, fuzz_seed):
        d = draws[op.bi]
        # a set_seats directly behind a multi-launch step that nothing has waited for
        d.m.cov["set_seats_behind_graph_step"] += int(op.kind == "set_seats" and d.prev_big)
        d.prev_big = op.kind == "step" and op.a["launches"][-1] >= 4
        d.had_plane |= d.m.masks is not None
        yield op, draws


def _draw_stream(name, fuzz_seed):
    specs = dict(ALL_SCENARIOS)[name]
    seat = name in SEAT_SCENARIO_NAMES
    rng = np.random.default_rng(zlib.crc32(name.encode()) + fuzz_seed)
    draws = [_Draw(spec, 777 + fuzz_seed + 1000 * j, (1 << 30) + 3 + (j << 33), fuzz_seed) for j, spec in enumerate(specs)]
    if seat:
        kinds = seat_deck(rng, fuzz_seed)
        for d in draws[1:]:
            d.seatable = False                                      # seats-two-batches: the second batch never has a plane
        case = 2 * SEAT_SCENARIO_NAMES.index(name) + fuzz_seed
        for d in draws:
            d.case = case
    else:
        kinds = deck()
        rng.shuffle(kinds)
    untraced = [j for j, d in enumerate(draws) if not d.trace]
    if untraced:
        # twice a case: indexed call -> step of four launches or more (the graph replay, not waited for) -> indexed call, all
        # three on one untraced batch, between two indexed calls that the shuffle has put side by side
        for _ in range(2):
            at = [i for i in range(len(kinds) - 1) if kinds[i] in INDEXED_OPS and kinds[i + 1] in INDEXED_OPS
                  and "graph_step" not in kinds[max(0, i - 2): i + 3]]
            if at:
                kinds.insert(int(rng.choice(at)) + 1, "graph_step")
    for bi, d in enumerate(draws):                                  # every batch starts with its rooms all over their games
        yield _adopt_played(rng, bi, d), draws
        yield _advance(rng, name, bi, d, int(rng.integers(1, 4))), draws
    hold = 0
    for i, kind in enumerate(kinds):
        if kinds[i + 1: i + 2] == ["graph_step"]:
            bi, hold = int(rng.choice(untraced)), 3
        elif not hold:
            bi = int(rng.integers(len(draws)))
        hold = max(0, hold - 1)
        if (kind in SEAT_OPS or kind in SEAT_REFUSALS or kind == "seat_graph_sequence") and not draws[bi].seatable:
            bi = 0
        d = draws[bi]
        if kind == "seat_graph_sequence":
            # the switch of step paths around a cached graph: a step of K turns (four launches or more, timing off, no plane: a graph
            # replay) -> set_seats directly behind it -> steps with the plane, which move the turn counter and not the graphs'
            # device turn word -> clear_seats -> single turns (a Werewolf x 12 deal then comes from the side plane) -> K turns again
            if d.m.masks is not None:
                yield _draw_seat(rng, "clear_seats", bi, d), draws
            if d.timing:
                yield _draw_one(rng, name, "set_timing", bi, d), draws
            K = max(4, 3 * d.fuse + 1)
            parts = ([K], "set_seats", [d.fuse + 1, int(rng.integers(1, d.fuse + 1))], "clear_seats", [1, 1, 1], [K])
            if d.trace:
                # a traced batch (a step holds one launch, no graphs): games all over their course, a turn without a plane, turns
                # with one - roles dealt over records the other path stored -, and turns without one again
                parts = ("adopt", [d.fuse], "set_seats", [d.fuse] * -(-6 // d.fuse), "clear_seats", [d.fuse] * -(-6 // d.fuse))
            for part in parts:
                if part == "adopt":
                    yield _adopt_played(rng, bi, d), draws
                elif isinstance(part, str):
                    yield _draw_seat(rng, part, bi, d), draws
                else:
                    op = Op("step", bi)
                    _apply_steps(op, d, part)
                    d.pure = False
                    yield op, draws
            continue
        if kind == "served_rounds" and d.m.masks is None:          # the serving loop runs on a batch with a plane
            yield _draw_seat(rng, "set_seats", bi, d), draws
        if seat and kind in INDEXED_OPS and d.seatable and d.m.masks is None and rng.random() < .6:
            yield _draw_seat(rng, "set_seats", bi, d), draws        # the indexed calls of these scenarios mostly meet a plane
        if kind == "find_rooms" and _terminal(d.m).sum() < 3:      # GE_FIND_END has something to find
            yield _write_ended(rng, bi, d), draws
        if kind in SEAT_OPS or kind in SEAT_REFUSALS:
            op = _draw_seat(rng, kind, bi, d)
            yield op, draws
            if kind == "clear_seats" and op.a["plane"]:             # ... and once more, now without a plane: nothing to do
                yield _draw_seat(rng, "clear_seats", bi, d), draws
            if kind in ("set_seats", "clear_seats"):                # the step path just switched: a few turns on the other one
                yield _advance(rng, name, bi, d, int(rng.integers(2, 6))), draws
            continue
        if kind == "graph_step":
            late = name == "ww12-300-late-plane" and not d.plane_ready
            op = Op("step", bi)
            _apply_steps(op, d, [4 * d.fuse if late else max(4, 3 * d.fuse + 1)])
            d.pure = False
            yield op, draws
            continue
        if kind == "hosted_threads" and len(_fresh(d.m)) < 6 and kinds[max(0, i - 1)] != "graph_step":
            # threads start in slots a whole-batch step has just recycled; where there are too few (every game at its start, or
            # waiting for its people), games under way are adopted first and the batch steps on: those at their end are recycled
            yield _adopt_played(rng, bi, d), draws
            yield _advance(rng, name, bi, d, 1), draws
        op = _draw_one(rng, name, kind, bi, d)
        d.seen.add(kind)
        yield op, draws
        if kind == "hosted_threads" and kinds[i + 1: i + 2] != ["graph_step"]:   # the slots handed back: their next games are the batch's own
            yield _advance(rng, name, bi, d, int(rng.integers(1, 4))), draws
        if kind == "reset":                                         # a reset is followed by the opening turns, or by games under way
            if rng.random() < .5:
                yield _adopt_played(rng, bi, d), draws
            yield _advance(rng, name, bi, d, int(rng.integers(1, 4))), draws


def _played_views(rng, d):
    """Views of a whole batch of rooms the oracle played from the initial state for 0 .. 99 turns, eight groups a segment, every
    seat by the policy (under a batch's human mask the games wait for their people: no ends, no restarts)."""
    m = d.m
    parts = []
    for o, (_, _, r, _) in zip(m.orcs, m.segs):
        rooms = o.init_rooms(r)
        for lo in range(0, r, -(-r // 8)):
            o.run(rooms[lo: lo + -(-r // 8)], m.seed, int(rng.integers(0, 1 << 40)), 0, int(rng.integers(0, 100)), threads=0, restart=d.restart,
                  human_mask=0)
        parts.append(oracle_rooms_as_views(o, rooms))
    return np.concatenate(parts)


def _write_ended(rng, bi, d):
    """A write_rooms_at of a few rooms with their own games played to the end on the oracle (every seat by the policy, nothing
    recycled): finished games that wait for the next turn of a restarting batch."""
    m = d.m
    rooms, views = [], []
    for r in rng.permutation(m.total)[:8]:
        o, rec = m.orc_of(r)
        one = np.array([rec])
        o.run(one, m.seed, int(rng.integers(0, 1 << 40)), int(rng.integers(0, 300)), 600, threads=1, restart=False, human_mask=0)
        if not o.table.phases[int(one["phase"][0])].branches:
            rooms.append(int(r))
            views.append(oracle_rooms_as_views(o, one)[0])
    assert rooms
    op = Op("write_rooms_at", bi, rooms=np.array(rooms, dtype=np.uint64), views=np.ascontiguousarray(np.array(views, dtype=views[0].dtype)))
    m.write_rooms_at(op.a["rooms"], op.a["views"])
    op.listed = op.a["rooms"]
    return op


def _adopt_played(rng, bi, d):
    """A write_rooms of the whole batch with _played_views."""
    op = Op("write", bi, lo=0, views=_played_views(rng, d))
    d.m.write(0, op.a["views"])
    return op


def _advance(rng, name, bi, d, turns):
    """A step operation of about `turns` turns: one call (at four launches or more: the graph path), on a traced batch - whose
    step holds one launch - call after call; before ww12-300-late-plane has its side plane, in whole launches only."""
    op = Op("step", bi)
    if d.trace:
        ks = [d.fuse] * -(-turns // d.fuse)
    elif name == "ww12-300-late-plane" and not d.plane_ready:
        ks = [d.fuse * -(-turns // d.fuse)]
    else:
        ks = [turns]
    _apply_steps(op, d, ks)
    return op


def _apply_steps(op, d, ks):
    op.a["ks"] = ks
    op.a["launches"] = [-(-k // d.fuse) for k in ks]
    # with a seat plane a step launches once per segment and per max_fuse turns (ge_step.h), plainly; without one, a call of four
    # launches or more replays a graph cached by its n_turns (eight of them, the oldest evicted) unless timing is on
    op.a["per_launch"] = len(d.segs) if d.m.masks is not None else 1
    for k in ks:
        if d.m.masks is not None:
            d.seat_moved = True
        elif -(-k // d.fuse) >= 4 and not d.timing:
            d.m.cov["graph_replay_after_seat_steps"] += int(d.seat_moved and k in d.graphs)
            if k not in d.graphs:
                d.graphs = (d.graphs + [k])[-8:]
            d.seat_moved = False
        d.m.step(k)
    d.launches += sum(op.a["launches"]) * op.a["per_launch"]


def _draw_one(rng, name, kind, bi, d):
    m = d.m
    op = Op(kind, bi)
    a = op.a
    if kind == "step":
        k = int(rng.integers(1, d.fuse + 1)) if d.trace else int(rng.choice([1, 2, d.fuse, 3 * d.fuse + 1]))
        if name == "ww12-300-late-plane" and not d.plane_ready:
            k = int(rng.choice([2, 16, 32]))                        # no single-turn launch yet: the side plane is not allocated
        _apply_steps(op, d, [k])
    elif kind in ("read", "summary"):
        if kind == "read" and rng.random() < .5:
            d.snapshots.append(m.views())
    elif kind == "read_part":
        a["lo"] = int(rng.integers(0, m.total))
        a["cnt"] = int(rng.integers(0, m.total - a["lo"] + 1))
    elif kind == "write":
        x = rng.random()                                            # games under way, an earlier state (no turn change), or the present one
        views = _played_views(rng, d) if x < .4 else d.snapshots[int(rng.integers(len(d.snapshots)))] if d.snapshots and x < .8 else m.views()
        lo = int(rng.integers(0, m.total))
        cnt = int(rng.integers(1, m.total - lo + 1))
        a["lo"], a["views"] = lo, np.ascontiguousarray(views[lo: lo + cnt])
        m.write(lo, a["views"])
    elif kind == "inject":
        a["room"], a["player"], a["choice"] = int(rng.integers(0, m.total)), int(rng.integers(0, d.nmax + 2)), int(rng.integers(0, d.nmax + 2))
        op.want = m.inject(a["room"], a["player"], a["choice"])
    elif kind == "inject_many":
        # 170 | 171 actions: 4 084 | 4 108 bytes of scratch, either side of its first size; 3 000: a regrow
        k = int(rng.choice([1, 50, 170, 171, 3000]))
        a["rooms"] = rng.integers(0, m.total + (3 if rng.random() < .3 else 0), size=k).astype(np.uint64)
        a["players"] = rng.integers(0, d.nmax + 2, size=k).astype(np.uint32)
        a["choices"] = rng.integers(0, d.nmax + 2, size=k).astype(np.uint32)
        op.want = [m.inject(int(r), int(p), int(c)) for r, p, c in zip(a["rooms"], a["players"], a["choices"])]
    elif kind == "reset":
        m.reset()
        d.snapshots = []
        d.launches, d.pure = 0, False                               # (whatever a reset does to the count, the steps behind it stay a lower bound)
    elif kind == "set_turn":
        a["turn"] = int(rng.integers(0, 500))
        m.turn = a["turn"]
    elif kind == "events":
        if d.trace and m.last_events is not None:
            a["lo"] = int(rng.integers(0, m.total))
            a["cnt"] = int(rng.integers(1, m.total - a["lo"] + 1))
    elif kind == "set_timing":
        d.timing = not d.timing
        a["on"] = d.timing
    elif kind == "kernel_time":
        a["reset"] = bool(rng.random() < .7)
        a["launches"], a["exact"] = d.launches, d.pure
        if a["reset"]:
            d.launches, d.pure = 0, True
    elif kind == "timed_steps":
        # the launch count as a unit: kernel_time(reset) -> timing on or off (off: a step of four launches replays a graph) -> one
        # to three whole-batch steps, a multi-launch one with a single-turn tail among them -> kernel_time: exactly the sum of
        # ceil(k / max_fuse)
        a["before"], a["on"] = d.launches, bool((d.fuzz_seed + d.calls[kind]) % 2)
        d.calls[kind] += 1
        late = name == "ww12-300-late-plane" and not d.plane_ready
        if d.trace:
            ks = [int(rng.integers(1, d.fuse + 1)) for _ in range(int(rng.integers(1, 4)))]
        elif late:
            ks = [d.fuse * int(x) for x in rng.choice([1, 2, 4], size=int(rng.integers(1, 4)))]
        else:
            ks = [int(x) for x in rng.permutation([max(4, 3 * d.fuse + 1)] + [int(y) for y in rng.choice([1, 2, d.fuse, d.fuse + 1], size=int(rng.integers(0, 3)))])]
        d.timing, d.launches = a["on"], 0
        _apply_steps(op, d, ks)
        a["reset"] = bool(rng.random() < .5)
        a["total"] = d.launches
        d.pure = True
        if a["reset"]:
            d.launches = 0
    elif kind == "step_rooms":
        listed, keys, turns = _entries(rng, m, _count(rng, d, kind))
        a.update(rooms=listed, keys=keys, turns=turns)
        op.want = m.step_rooms(listed, keys, turns)
    elif kind == "hosted_threads":
        a["rounds"] = _hosted_threads(rng, d)
        a["rooms"] = a["rounds"][0][0]
    elif kind == "read_rooms_at":
        n = _count(rng, d, kind)
        a["rooms"] = rng.integers(0, m.total, n).astype(np.uint64)  # any order, repeats allowed
        op.want = m.read_rooms_at(a["rooms"])
    elif kind == "write_rooms_at":
        n = min(_count(rng, d, kind), m.total)
        listed = rng.choice(m.total, size=n, replace=False).astype(np.uint64)
        a["rooms"], a["views"] = listed, _views_for(rng, d, listed)
        m.write_rooms_at(listed, a["views"])
    elif kind == "run_rooms":
        # the case's run_rooms calls go round four shapes, so that the default seeds of every scenario hold each stop reason: many
        # rooms for a few turns under every condition; a few rooms for 24 turns under none (the limit; games end and restart
        # inside the call); either side of the scratch threshold for one turn; some rooms until a person is needed or the game ends
        shape = (2 * d.fuzz_seed + d.runs) % 4
        d.runs += 1
        n, T, until = [(int(rng.choice([113, 114])), 3, PERSON | END | PHASE), (int(rng.integers(8, 30)), 24, 0),
                       (int(rng.choice([44, 45])), 1, END | PHASE), (int(rng.choice([1, int(rng.integers(2, 30))])), 8, PERSON | END)][shape]
        listed, keys, turns = _entries(rng, m, n, last_fit=0xFFFFFFFF - T, ends_within=T)
        a.update(rooms=listed, keys=keys, turns=turns, max_turns=T, until=until)
        op.want = m.run_rooms(listed, keys, turns, T, until)
    elif kind == "run_rooms_forecast":
        R = int(rng.choice(N_ROLLOUTS))
        n = int(rng.integers(1, 5)) if R > 1 else int(rng.choice([1, 6, 7, 20]))
        until, T = _until_and_turns(rng, n * R, 300)
        M = int(rng.choice([4, 12, 24]))
        listed, keys, turns = _entries(rng, m, n, last_fit=0xFFFFFFFF - T - M)
        fkeys = rng.integers(0, 1 << 62, len(listed)).astype(np.uint64)
        seats = _seats(rng, m, listed)
        fseed = int(rng.integers(0, 1 << 40))
        a.update(rooms=listed, keys=keys, turns=turns, fkeys=fkeys, seats=seats, R=R, M=M, seed=fseed, max_turns=T, until=until)
        op.want = m.run_rooms_forecast(listed, keys, turns, fkeys, seats, R, M, fseed, T, until)
    elif kind in ("step_rooms_playout", "step_rooms_playout_halving", "run_rooms_playout"):
        run = kind == "run_rooms_playout"
        # the oracle's work: entries with a playout seat x its candidates x n_rollouts re-dealt replicas (x the run's turns)
        n, R = _pairs(rng, COUNTS["playout"], 100 if run else 220)
        M = int(rng.choice([4, 12, 24]))
        until, T = _until_and_turns(rng, n * R, 400) if run else (0, 1)
        listed, keys, turns = _entries(rng, m, n, last_fit=0xFFFFFFFF - T + 1 - M)
        masks = _masks(rng, m, listed, whole=_prefer_deciders(rng, d, listed, keys, turns))
        pkeys = rng.integers(0, 1 << 63, len(listed)).astype(np.uint64)
        pkeys[0] = np.uint64(M64 - 3)                               # the replica keys wrap
        pseed, full = int(rng.integers(0, 1 << 40)), bool(rng.random() < .3)
        a.update(rooms=listed, keys=keys, turns=turns, masks=masks, pkeys=pkeys, R=R, M=M, seed=pseed, full_view=full)
        if run:
            a.update(max_turns=T, until=until)
            op.want = m.run_rooms_playout(listed, keys, turns, masks, pkeys, R, M, pseed, full, T, until)
        else:
            a["halving"] = kind.endswith("halving")
            op.want = m.step_rooms_playout(listed, keys, turns, masks, pkeys, R, M, pseed, full, a["halving"])
    elif kind.startswith("rollout_"):
        n, R = _pairs(rng, COUNTS["rollout"] + (int(rng.integers(2, 13)),), 520)
        M = int(rng.choice([0, 5, 24]))
        pseed = int(rng.integers(0, 1 << 40))
        if kind == "rollout_compare" or (kind == "rollout_beliefs" and rng.random() < .5):
            # groups of 2 - 3 entries of one room under one key, turn and seat: common random numbers against the group's first
            g = max(1, n // 3)
            base, keys0, turns0 = _entries(rng, m, g, last_fit=0xFFFFFFFF - M)
            seats0 = _seats(rng, m, base)
            rep = rng.integers(2, 4, len(base))
            idx = np.repeat(np.arange(len(base)), rep)
            listed, keys, turns, seats = base[idx], keys0[idx], turns0[idx], seats0[idx]
            first_of = np.concatenate([[0], np.cumsum(rep)[:-1]])
            a["baseline"] = first_of[idx].astype(np.uint32)
            # (one subject a group: an entry is compared with its baseline for the same seat)
            a["subjects"] = np.array([int(rng.integers(1, m.orc_of(r)[0].n + 1)) for r in base], dtype=np.uint32)[idx]
        else:
            listed, keys, turns = _entries(rng, m, n, distinct=False, last_fit=0xFFFFFFFF - M)
            seats = _seats(rng, m, listed)
        a.update(rooms=listed, keys=keys, turns=turns, R=R, M=M, seed=pseed)
        if kind != "rollout_rooms":
            a["actions"] = _actions(rng, m, listed)
        if kind in ("rollout_seats", "rollout_beliefs", "rollout_compare"):
            a["seats"] = seats
        if kind == "rollout_beliefs":
            bel = np.zeros((len(listed), 16), dtype=np.uint8)
            for k, r in enumerate(listed):
                o = m.orc_of(r)[0]
                slots = o.n if o.table.pack == 1 else 3
                x = k % 4
                bel[k, :slots] = 0 if x == 0 else 7 if x == 1 else rng.integers(0, 256, slots)
            a["beliefs"] = bel
        if kind == "rollout_rooms":
            op.want = m.rollout_rooms(listed, keys, turns, R, M, pseed)
        elif kind == "rollout_actions":
            op.want = m.rollout_actions(listed, keys, turns, a["actions"], R, M, pseed)
        elif kind == "rollout_seats":
            op.want = m.rollout_seats(listed, keys, turns, seats, a["actions"], R, M, pseed)
        elif kind == "rollout_compare":
            op.want = m.rollout_compare(listed, keys, turns, seats, a["actions"], a["baseline"], a["subjects"], R, M, pseed)
        elif "baseline" in a:
            from rollout_beliefs_ref import reference_beliefs
            op.want = reference_beliefs(m.orc_of, listed, keys, turns, seats, a["actions"], a["beliefs"], R, M, pseed, a["baseline"], a["subjects"])
        else:
            op.want = m.rollout_beliefs(listed, keys, turns, seats, a["actions"], a["beliefs"], R, M, pseed)
    elif kind in REFUSALS:
        # the ABI's documented error returns, checked before anything is launched: the model does not move
        call = str(rng.choice(["write_rooms_at"] if kind == "refuse_view" else ["step_rooms", "run_rooms", "step_rooms_playout"]
                              if kind == "refuse_turn" else ["step_rooms", "write_rooms_at", "run_rooms", "step_rooms_playout", "read_rooms_at"]
                              if kind == "refuse_range" else ["step_rooms", "write_rooms_at", "run_rooms", "step_rooms_playout"]))
        listed, keys, turns = _entries(rng, m, int(rng.integers(3, 9)), far=False)
        j = int(rng.integers(len(listed)))
        a.update(call=call, keys=keys, turns=turns)
        views = _views_for(rng, d, listed)
        op.status = GE_ERR_ARG
        if kind == "refuse_repeat":
            listed[j] = listed[(j + 1) % len(listed)]
        elif kind == "refuse_range":
            listed[j] = m.total
            op.status = GE_ERR_RANGE
        elif kind == "refuse_turn":
            turns[j] = 0xFFFFFFFF
            op.status = GE_ERR_RANGE
        else:
            bad = int(rng.integers(3))
            if bad == 0:
                views["n_players"][j] += 1
            elif bad == 1:
                views["phase_id"][j] = 4242
            else:
                views["pack"][j] ^= 3
            a["rejected"] = int(listed[j])
        a.update(rooms=listed, views=views)
    else:
        raise AssertionError(kind)
    if kind in INDEXED_OPS or kind in REFUSALS:
        op.listed = np.asarray(a["rooms"], dtype=np.uint64)
        d.pure = False
        if kind in MUTATING_INDEXED and "write_rooms_at" in d.seen | {kind} and (d.seen | {kind}) & (MUTATING_INDEXED - {"write_rooms_at"}):
            d.plane_ready = True
    elif kind not in ("step", "set_timing", "kernel_time", "timed_steps"):
        d.pure = False
    return op


def _views_for(rng, d, listed):
    """A view for each listed room: some room of its own segment (it fits) as it is now, as it was at an earlier read, as a
    game under way, or as a new game (a thread adopted into the slot)."""
    m = d.m
    srcs = [np.concatenate([oracle_rooms_as_views(o, o.init_rooms(r)) for o, (_, _, r, _) in zip(m.orcs, m.segs)]), _played_views(rng, d),
            d.snapshots[int(rng.integers(len(d.snapshots)))] if d.snapshots else m.views(), m.views()]
    out = []
    for r in listed:
        s, _ = m.seg_of(int(min(int(r), m.total - 1)))
        out.append(srcs[int(rng.choice(4, p=[.35, .25, .2, .2]))][int(rng.integers(m.lo[s], m.lo[s + 1]))])
    return np.ascontiguousarray(np.array(out, dtype=srcs[0].dtype))


# ---- the kinds of the seat-plane scenarios

# ge_batch_set_seats stages 12 n bytes (8 n of rooms, 4 n of masks): 341: 4 092 | 342: 4 104, either side of the scratch's first size.
# ge_batch_find_rooms over one segment's range with cap >= count, by the layout in find_rooms_impl (result words and wavefront
# counts padded to whole wavefronts, offsets, a total, 16 B a hit): 192 rooms: 768 + 12 -> 784, + 24 = 808, + 8 -> 816, + 3 072 =
# 3 888 | 193 rooms: 1 024 + 16 = 1 040, + 32 = 1 072, + 8 -> 1 088, + 3 088 = 4 176
SET_SEATS_SIDES, FIND_SIDES = (341, 342), (192, 193)
ADVISE_TURNS = (0, 5, 24)
ROLLOUT_BUDGET = 520                                               # the oracle's playouts a call, as the rollout_* kinds


def _seat_masks_for(rng, m, rooms):
    """seats_ref.seat_masks over each segment (the six forms from lane to lane, rotated by a drawn offset), read at the rooms."""
    from seats_ref import seat_masks
    whole = np.concatenate([np.roll(seat_masks(n, r, rng), int(rng.integers(0, 6))) for _, n, r, _ in m.segs])
    return whole[np.asarray(rooms, dtype=np.int64)].astype(np.uint32)


def _phase_masks(rng, m):
    """A mask word per segment: about half of the phase ids its rooms stand in and one id of the table that no room is in (ids
    a mask word may name: below 32 and below the table's phase count)."""
    out = []
    for o, rooms in zip(m.orcs, m.rooms):
        ok = [int(p) for p in o.ids if p < min(32, len(o.table.phases))]
        here = sorted({int(o.ids[int(r)]) for r in np.unique(rooms["phase"])} & set(ok))
        absent = [p for p in ok if p not in here]
        pick = [int(p) for p in rng.permutation(here)[: max(1, len(here) // 2)]] + [int(p) for p in rng.permutation(absent)[:1]]
        out.append(sum(1 << p for p in pick))
    return np.array(out, dtype=np.uint32)


def _find_range(rng, m, shape, side):
    """(first, count): 0 the whole batch; 1 inside one segment, 192 | 193 rooms in turn (where none is that large: as 2); 2 across a
    segment boundary (one segment: as 3); 3 a random range."""
    if shape == 0:
        return 0, m.total
    big = [s for s in range(len(m.segs)) if m.segs[s][2] >= FIND_SIDES[1]]
    if shape == 1 and big:
        s, n = int(rng.choice(big)), FIND_SIDES[side % 2]
        return m.lo[s] + int(rng.integers(0, m.segs[s][2] - n + 1)), n
    if shape in (1, 2) and len(m.segs) > 1:
        s = int(rng.integers(1, len(m.segs)))
        first = m.lo[s] - int(rng.integers(1, min(70, m.segs[s - 1][2]) + 1))
        return first, int(rng.integers(m.lo[s] - first + 1, min(m.total - first, 200) + 1))
    first = int(rng.integers(0, m.total - 1))
    return first, int(rng.integers(1, m.total - first + 1))


def _advise_entries(rng, m, n):
    """n (room, seat) pairs, repeats allowed: at least half of them seats that can act now (advise_ref.legal_mask on the model, as
    _prefer_deciders looks for deciders), those with a choice to make first; the others drawn blindly (most are refused)."""
    from advise_ref import legal_mask
    some, many = [], []
    for r in rng.permutation(m.total)[:48]:
        o, rec = m.orc_of(r)
        for seat in range(1, o.n + 1):
            legal = legal_mask(o, rec, seat)
            if legal:
                (many if bin(legal).count("1") >= 2 else some).append((int(r), seat))
    found = [many[int(i)] for i in rng.permutation(len(many))] + [some[int(i)] for i in rng.permutation(len(some))]
    pairs = found[: -(-n // 2)]
    while len(pairs) < n:
        r = int(rng.integers(0, m.total))
        pairs.append(pairs[0] if pairs and rng.random() < .2 else (r, int(rng.integers(1, m.orc_of(r)[0].n + 1))))
    return [pairs[int(i)] for i in rng.permutation(len(pairs))]


def _n_choices(m, room):
    o = m.orc_of(room)[0]
    return o.n if o.table.pack == 1 else 3


def _draw_seat(rng, kind, bi, d):
    m = d.m
    op = Op(kind, bi)
    a = op.a
    call = d.calls[kind]
    d.calls[kind] += 1
    d.pure = False
    if kind == "set_seats":
        # the case's calls go round: the whole batch in shuffled order, the two sides of the threshold, one entry or a few
        n = [m.total, SET_SEATS_SIDES[0], SET_SEATS_SIDES[1], int(rng.choice([1, int(rng.integers(2, 40))]))][(2 * d.fuzz_seed + call) % 4]
        rooms = rng.permutation(m.total)[: min(n, m.total)].astype(np.uint64)
        a.update(rooms=rooms, masks=_seat_masks_for(rng, m, rooms), allocates=m.masks is None)
        assert m.set_seats(rooms, a["masks"]) == 0
        op.listed = rooms
    elif kind == "get_seats":
        first = int(rng.integers(0, m.total))
        count = [int(rng.integers(1, m.total - first + 1)), 0, m.total - first][(d.fuzz_seed + call) % 3]
        a.update(first=first, count=count)
        op.want = m.get_seats(first, count)
        op.listed = np.zeros(0, dtype=np.uint64)
    elif kind == "clear_seats":
        a["plane"] = m.masks is not None
        m.clear_seats()
    elif kind == "find_rooms":
        a["calls"] = []
        rooms = []
        for j in range(2):
            q = 2 * call + j + d.fuzz_seed
            want = (3 * q + d.fuzz_seed) % 7 + 1                    # all seven combinations within seven calls
            shape = q % 4
            first, count = _find_range(rng, m, shape, q // 4 + d.fuzz_seed)
            masks = _phase_masks(rng, m) if want & PHASE else None
            hits, n_match = m.find_rooms(first, count, want, masks, count)
            # cap: at least count (always so for the 192 | 193 ranges), above n_match, below it (the scan is resumed), 0
            mode = 0 if shape == 1 else 1 + (q // 4 + q) % 3
            cap = [count + int(rng.integers(0, 3)), n_match + int(rng.integers(1, 4)), max(1, -(-n_match // 3)) if n_match >= 2 else 0, 0][mode]
            a["calls"].append(dict(first=first, count=count, want=want, masks=masks, cap=cap, hits=hits, n_match=n_match))
            rooms += [h[0] for h in hits[:16]]
        op.listed = np.array(rooms, dtype=np.uint64)
    elif kind == "advise_seats":
        M = int(ADVISE_TURNS[(d.fuzz_seed + call) % 3])
        full = bool((d.fuzz_seed + call) % 2)
        cmax = max(n if g != TT else 3 for g, n, _, _ in m.segs) + 1   # the most entries of work one listed entry can cost
        R = int(rng.choice([r for r in N_ROLLOUTS if cmax * r <= ROLLOUT_BUDGET]))
        n = int(rng.integers(1, min(40, ROLLOUT_BUDGET // (cmax * R)) + 1))
        pairs = _advise_entries(rng, m, n)
        rooms = np.array([r for r, _ in pairs], dtype=np.uint64)
        seats = np.array([s for _, s in pairs], dtype=np.uint32)
        keys = rng.integers(0, 1 << 40, n).astype(np.uint64)
        keys[int(rng.integers(n))] = np.uint64(M64 - int(rng.integers(0, 40)))
        turns = rng.integers(0, 300, n).astype(np.uint32)
        turns[0] = 0xFFFFFFFF - M                                    # the last turn that fits
        aseed = int(rng.integers(0, 1 << 40))
        a.update(rooms=rooms, keys=keys, turns=turns, seats=seats, R=R, M=M, seed=aseed, full_view=full)
        op.want = m.advise_seats(rooms, keys, turns, seats, R, M, aseed, full)
        op.listed = rooms
    elif kind == "served_rounds":
        # find who waits, advise them, inject the advice, step them: each served room under a key and a clock of its own
        a.update(R=1, M=int(rng.choice([5, 24])), seed=int(rng.integers(0, 1 << 40)), rounds=[])
        keys, clocks, served = {}, {}, []
        for _ in range(3):
            hits, n_match = m.find_rooms(0, m.total, PERSON, None, m.total)
            pick = sorted(int(i) for i in rng.permutation(len(hits))[:8])
            rooms = np.array([hits[i][0] for i in pick], dtype=np.uint64)
            seats = np.array([(hits[i][2] & -hits[i][2]).bit_length() for i in pick], dtype=np.uint32)   # the lowest pending seat
            for r in rooms:
                keys.setdefault(int(r), int(rng.integers(0, 1 << 40)))
                clocks.setdefault(int(r), int(rng.integers(0, 300)))
            k = np.array([keys[int(r)] for r in rooms], dtype=np.uint64)
            t = np.array([clocks[int(r)] for r in rooms], dtype=np.uint32)
            advice = m.advise_seats(rooms, k, t, seats, a["R"], a["M"], a["seed"], False)
            for r, seat, adv in zip(rooms, seats, advice):
                assert adv["status"] == 0 and m.inject(int(r), int(seat), int(adv["best"])) == 0, (int(r), int(seat), adv)
                clocks[int(r)] += 1
            events = m.step_rooms(rooms, k, t, call="served_rounds")
            a["rounds"].append(dict(hits=hits, rooms=rooms, keys=k, turns=t, seats=seats, advice=advice, events=events))
            served += rooms.tolist()
        op.listed = np.array(sorted(set(served)), dtype=np.uint64)
    else:
        how = SEAT_REFUSALS[kind][d.case % len(SEAT_REFUSALS[kind])]
        a["how"] = how
        op.status = GE_ERR_ARG
        op.listed = np.zeros(0, dtype=np.uint64)
        if kind == "refuse_set_seats":
            rooms = rng.permutation(m.total)[: int(rng.integers(3, 9))].astype(np.uint64)
            masks = _seat_masks_for(rng, m, rooms)
            j = int(rng.integers(len(rooms)))
            if how == "range":
                rooms[j] = m.total
                op.status = GE_ERR_RANGE
            elif how == "repeat":
                rooms[j] = rooms[(j + 1) % len(rooms)]
            else:
                masks[j] |= np.uint32(1 << m.segs[m.seg_of(int(rooms[j]))[0]][1])
            a.update(rooms=rooms, masks=masks)
            assert m.set_seats(rooms, masks) == op.status
            op.listed = rooms[rooms < m.total]
        elif kind == "refuse_find_rooms":
            a.update(first=int(rng.integers(0, m.total - 8)), count=8, want=PERSON | END, masks=None)
            if how == "want_zero":
                a["want"] = 0
            elif how == "unknown_bit":
                a["want"] = 8 | int(rng.integers(0, 8))
            elif how == "beyond":
                a.update(first=m.total - 7)
                op.status = GE_ERR_RANGE
            else:
                masks = _phase_masks(rng, m)
                s = int(rng.integers(len(m.segs)))
                assert len(m.orcs[s].table.phases) < 32
                masks[s] |= np.uint32(1 << len(m.orcs[s].table.phases))
                a.update(want=PHASE | END, masks=masks)
        elif kind == "refuse_advise_seats":
            pairs = _advise_entries(rng, m, int(rng.integers(2, 6)))
            rooms = np.array([r for r, _ in pairs], dtype=np.uint64)
            seats = np.array([s for _, s in pairs], dtype=np.uint32)
            turns = rng.integers(0, 300, len(rooms)).astype(np.uint32)
            j = int(rng.integers(len(rooms)))
            if how == "seat_zero":
                seats[j] = 0
            elif how == "seat_above":
                seats[j] = m.orc_of(rooms[j])[0].n + 1
            else:
                turns[j] = 0xFFFFFFFF - 5 + 1
                op.status = GE_ERR_RANGE
            a.update(rooms=rooms, keys=rng.integers(0, 1 << 40, len(rooms)).astype(np.uint64), turns=turns, seats=seats, R=4, M=5)
            op.listed = rooms
        else:
            # room y: a seat handed to a person -> a playout bit on it is refused; room x: a seat of the segment's mask handed back to
            # the policy -> a playout bit on it is accepted (the host mirror of the room's own mask decides, not the segment's)
            segs = [s for s in range(len(m.segs)) if m.segs[s][3]]
            s = int(rng.choice(segs))
            x = m.lo[s] + int(rng.integers(0, m.segs[s][2]))
            y = int(rng.choice([r for r in rng.integers(0, m.total, 8) if int(r) != x]))
            seat_y = int(rng.integers(0, m.segs[m.seg_of(y)[0]][1]))
            bit_x = m.segs[s][3] & -m.segs[s][3]
            a["set"] = (np.array([x, y], dtype=np.uint64), np.array([0, m.mask_of(y) | (1 << seat_y)], dtype=np.uint32))
            assert m.set_seats(*a["set"]) == 0
            keys, turns = rng.integers(0, 1 << 40, 1).astype(np.uint64), rng.integers(0, 300, 1).astype(np.uint32)
            pkeys, pseed = rng.integers(0, 1 << 62, 1).astype(np.uint64), int(rng.integers(0, 1 << 40))
            a.update(refused=dict(rooms=np.array([y], dtype=np.uint64), masks=np.array([1 << seat_y], dtype=np.uint32)),
                     rooms=np.array([x], dtype=np.uint64), keys=keys, turns=turns, masks=np.array([bit_x], dtype=np.uint32), pkeys=pkeys,
                     R=4, M=4, seed=pseed)
            op.want = m.step_rooms_playout(a["rooms"], keys, turns, a["masks"], pkeys, 4, 4, pseed, False, False)
            op.listed = np.array([x, y], dtype=np.uint64)
    return op

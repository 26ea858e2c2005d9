"""Host side of the batch stepper, mirroring the reference's interface for this path.

Reference surface kept (same names / argument meaning):
  load_dsl_by_gamename(gamename)            agent/tools/utils.py:557-581  (YAML -> dict)
  AgentState fields returned by agent_state current_phase_id, current_phase_name, player_states
                                            {"1": {<declared fields>}}  agent/game_agent_v2.py:97-117
  player ids "1".."N"                       agent/tools/utils.py:642-647
What is new: rooms are stepped in batches on the GPU (RoomBatch), one turn = one graph run.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import re
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib

ROOM_VIEW_DTYPE = np.dtype([("phase_id", "<i4"), ("prev_phase_id", "<i4"), ("end_turn", "<i4"), ("games", "<i4"),
                            ("phase0_done", "u1"), ("n_players", "u1"), ("pack", "u1"), ("pad", "u1"),
                            ("players", "u1", (16, 12)), ("det", "u1", (16,))])

EVENT_DTYPE = np.dtype([("turn", "<u4"), ("from_phase_id", "<i4"), ("to_phase_id", "<i4"), ("acted_now", "<u2"),
                        ("restarted", "u1"), ("pad", "u1"), ("choice", "u1", (16,))])

PACK_WEREWOLF, PACK_TWO_TRUTHS = 1, 2
WW_FIELDS = ["role", "team", "is_alive", "role_revealed", "can_vote", "has_secret_role",
             "night_action_eligible", "night_action_submitted", "selected_target_id"]
TT_FIELDS = ["is_speaker", "statements_submitted", "lie_index", "lie_revealed", "can_vote",
             "vote_choice", "has_voted", "total_score", "rounds_as_speaker"]
_TEAMS = ["", "villagers", "werewolves"]
# slots that are not ge_room_view columns (include/ge_step.h GE_WW_DET_MEMORY, GE_WW_WOLF_CHAT, GE_TT_STATEMENTS)
SLOT_DET_MEMORY, SLOT_WOLF_CHAT, SLOT_STATEMENTS = 9, 10, 9


GE_ERR_ARG = -1                           # include/ge_step.h ge_status
GE_MAX_PLAYERS = 12                       # include/ge_step.h


RUN_UNTIL = {"person": 1, "end": 2, "phase": 4}   # include/ge_step.h GE_RUN_UNTIL_*


def _named_bits(value, names: Dict[str, int], what: str) -> int:
    """A sequence of names of `names`, one of them, or the bits themselves, as the ABI's bit set."""
    if isinstance(value, (int, np.integer)):
        return int(value)
    if isinstance(value, str):
        value = (value,)
    bits = 0
    for name in value:
        if name not in names:
            raise ValueError(f"{what} {name!r}")
        bits |= names[name]
    return bits


def run_until_bits(until) -> int:
    """`until` of run_rooms / run_room as the ABI's bit set: a sequence of "person" / "end" / "phase", or the bits themselves."""
    return _named_bits(until, RUN_UNTIL, "until: unknown stop condition")


def run_until_names(bits: int) -> List[str]:
    return [name for name, bit in RUN_UNTIL.items() if bits & bit]


RUN_SEATS_UNTIL = dict(RUN_UNTIL, seat=8)         # include/ge_step.h GE_RUN_UNTIL_SEAT: run_seats alone takes it


FIND_WANT = {"person": 1, "end": 2, "phase": 4}   # include/ge_step.h GE_FIND_*
# include/ge_step.h ge_room_hit
ROOM_HIT_DTYPE = np.dtype([("room", "<u8"), ("why", "<u4"), ("pending", "<u2"), ("phase_id", "u1"), ("segment", "u1")])
# ge_advice (224 B) and its ge_advice_option (16 B)
ADVICE_OPTION_DTYPE = np.dtype([("finished", "<u4"), ("wins", "<u4"), ("score", "<u8")])
ADVICE_DTYPE = np.dtype([("status", "<i4"), ("legal", "<u4"), ("best", "<u4"), ("phase_id", "<u4"), ("policy", ADVICE_OPTION_DTYPE),
                         ("option", ADVICE_OPTION_DTYPE, (12,))])
ADVICE_BYTES = ADVICE_DTYPE.itemsize              # 224
# ge_seat_obs (192 B): what ge_batch_observe_seats stores per (room, seat)
SEAT_OBS_DTYPE = np.dtype([("seat", "u1"), ("n_players", "u1"), ("pack", "u1"), ("act", "u1"), ("phase_row", "u1"), ("done", "u1"), ("won", "u1"),
                           ("pad0", "u1"), ("legal", "<u2"), ("unknown", "<u2"), ("phase_id", "<i4"), ("prev_phase_id", "<i4"), ("end_turn", "<i4"),
                           ("games", "<i4"), ("pad1", "<u4"), ("players", "u1", (12, 12)), ("det", "u1", (12,)), ("pad2", "u1", (4,))])


def _device_buffer(obj) -> Tuple[int, int]:
    """(device pointer, bytes) of a torch tensor or of any object with data_ptr() and a byte size"""
    ptr = int(obj.data_ptr())
    if hasattr(obj, "nbytes"):
        return ptr, int(obj.nbytes)
    return ptr, int(obj.numel()) * int(obj.element_size())


def find_want_bits(want) -> int:
    """`want` of find_rooms as the ABI's bit set: a sequence of "person" / "end" / "phase", or the bits themselves."""
    return _named_bits(want, FIND_WANT, "want: unknown condition")


def find_want_names(bits: int) -> List[str]:
    return [name for name, bit in FIND_WANT.items() if bits & bit]


def pending_seats(pending: int) -> List[int]:
    """the seats (1-based) of a hit's `pending` mask"""
    return [i + 1 for i in range(GE_MAX_PLAYERS) if (int(pending) >> i) & 1]


class GeError(RuntimeError):
    def __init__(self, status: int, what: str = ""):
        msg = _lib.load().ge_strerror(status).decode()
        super().__init__(f"{what}: {msg} ({status})" if what else f"{msg} ({status})")
        self.status = status


def library_path() -> str:
    return _lib.LIB_PATH


def _check(status: int, what: str = ""):
    if status != 0:
        raise GeError(status, what)


def load_dsl_by_gamename(gamename: str, games_dir: Optional[str] = None) -> dict:
    """Same contract as the reference's loader (utils.py:557-581): '<games_dir>/<gamename>.yaml'
    -> dict, {} when the name is empty or the file is missing.  Also accepts the JSON form of
    the same document ('<gamename>.json')."""
    if not gamename:
        return {}
    games_dir = games_dir or os.environ.get("GE_GAMES_DIR", "games")
    ypath = os.path.join(games_dir, f"{gamename}.yaml")
    jpath = os.path.join(games_dir, f"{gamename}.json")
    if os.path.exists(ypath):
        import yaml
        with open(ypath, encoding="utf-8") as f:
            return yaml.safe_load(f) or {}
    if os.path.exists(jpath):
        with open(jpath, encoding="utf-8") as f:
            return json.load(f)
    return {}


def initialize_player_states_from_dsl(dsl_content: dict, room_players: list) -> dict:
    """Same contract as the reference's helper (agent/tools/utils.py:584-653; TS twin
    src/app/api/games/initialize-players/route.ts:83-166): every room player gets a copy of
    declaration.player_states_template.player_states[<first id>] with its own `name`; ids "1".."N".
    Falls back to defaults derived from declaration.player_states when there is no template."""
    decl = (dsl_content or {}).get("declaration") or {}
    tmpl_all = (decl.get("player_states_template") or {}).get("player_states") or {}
    template = tmpl_all.get("1") or tmpl_all.get(1) or (tmpl_all[next(iter(tmpl_all))] if tmpl_all else {})
    if not template:
        defaults = {"string": "", "num": 0, "number": 0, "array": [], "list": [], "object": {}, "dict": {}}
        for name, spec in (decl.get("player_states") or {}).items():
            ftype, example = spec.get("type", "string"), spec.get("example")
            if ftype == "boolean":
                template[name] = example if example is not None else True
            else:
                template[name] = example or defaults.get(ftype)
    if not template:
        return {}
    return {str(i + 1): {**template, "name": p.get("name", f"Player {i + 1}")} for i, p in enumerate(room_players)}


class GameTable:
    """A game DSL compiled by ge_table_compile_json."""

    def __init__(self, dsl: dict, rounds: int = 1):
        if not isinstance(dsl, dict) or not dsl:
            raise GeError(-2, "empty DSL")
        self.dsl = dsl
        # declared fields the rule packs do not model: constants from the template (nobody writes them under the fixed policy)
        tmpl_all = ((dsl.get("declaration") or {}).get("player_states_template") or {}).get("player_states") or {}
        tmpl = tmpl_all.get("1") or tmpl_all.get(1) or (tmpl_all[next(iter(tmpl_all))] if tmpl_all else {})
        text = json.dumps(dsl, ensure_ascii=False).encode("utf-8")   # int phase keys become strings
        self.c = _lib.Table()
        err = C.create_string_buffer(512)
        st = _lib.load().ge_table_compile_json(text, len(text), rounds, C.byref(self.c), err, len(err))
        if st != 0:
            raise GeError(st, err.value.decode("utf-8", "replace"))
        # slot -> the DSL's own name for it ("" = the DSL does not declare the slot); include/ge_step.h GE_WW_* / GE_TT_*
        self.field_names: List[str] = [self.c.field_names[s].value.decode("utf-8", "replace") for s in range(_lib.GE_MAX_SLOTS)]
        modelled = set(n for n in self.field_names if n) | {"name"}
        self.extra_fields = {k: v for k, v in (tmpl or {}).items() if k not in modelled and isinstance(v, (bool, int, str))}

    @classmethod
    def from_gamename(cls, gamename: str, games_dir: Optional[str] = None, rounds: int = 1) -> "GameTable":
        return cls(load_dsl_by_gamename(gamename, games_dir), rounds)

    @property
    def pack(self) -> int:
        return self.c.pack

    @property
    def n_phases(self) -> int:
        return self.c.n_phases

    def rows(self) -> List[dict]:
        out = []
        for i in range(self.c.n_phases):
            r = self.c.rows[i]
            out.append({"phase_id": r.phase_id, "name": r.name.decode("utf-8", "replace"),
                        "completion": r.completion, "act": r.act, "effect": r.effect,
                        "terms": [(r.term_base[j], r.term_neg[j]) for j in range(r.n_terms)],
                        "generic": bool(r.generic),
                        # the condition in clause form: OR of AND-clauses of (kind, neg, bases bit set, num_field, lo, hi)
                        "clauses": [[(l.kind, l.neg, l.bases, l.num_field, l.lo, l.hi) for l in list(r.clause[c])[: r.clause_len[c]]]
                                    for c in range(r.n_clauses)],
                        "branches": [(r.br_res[j], r.br_target[j]) for j in range(r.n_branches)]})
        return out

    def dev_row(self, n_players: int, row: int) -> List[int]:
        """The 8 words of row `row` in the device phase table of a segment of `n_players` players (csrc/ge_layout.h DevRow)."""
        out = (C.c_uint32 * 8)()
        _check(_lib.load().ge_table_dev_row(C.byref(self.c), n_players, row, out), "ge_table_dev_row")
        return list(out)

    def phase_name(self, phase_id: int) -> str:
        for i in range(self.c.n_phases):
            if self.c.rows[i].phase_id == phase_id:
                return self.c.rows[i].name.decode("utf-8", "replace")
        return f"Phase {phase_id}"        # utils.py:30 fallback

    def role_name(self, cls_idx: int) -> str:
        return self.c.role_names[cls_idx].value.decode("utf-8", "replace")


Segment = Tuple                            # (table, n_players, n_rooms[, human_mask])


class RoomBatch:
    """A batch of independent rooms resident in HBM.  One `step()` = one turn of every room
    (= one LangGraph run per room in the reference)."""

    def __init__(self, segments: Sequence[Segment], seed: int = 0, first_room: int = 0,
                 device: int = 0, max_fuse: int = 0, restart: bool = False, trace: bool = False):
        lib = _lib.load()
        if not 1 <= len(segments) <= _lib.GE_MAX_SEGMENTS:
            raise GeError(-1, "segments")
        self.segments = list(segments)
        d = _lib.BatchDesc()
        d.seed, d.first_room, d.n_segments, d.device, d.max_fuse = seed, first_room, len(segments), device, max_fuse
        d.flags = (1 if restart else 0) | (2 if trace else 0)
        for k, seg in enumerate(segments):
            tb, n_players, n_rooms = seg[:3]
            d.seg[k].table = C.pointer(tb.c)
            d.seg[k].n_players, d.seg[k].n_rooms = n_players, n_rooms
            d.seg[k].human_mask = seg[3] if len(seg) > 3 else 0      # bit i: player i+1 is host-driven
        h = C.c_void_p()
        _check(lib.ge_batch_create(C.byref(d), C.byref(h)), "ge_batch_create")
        self._h = h
        self._lib = lib
        self._seed, self._first_room, self._max_fuse, self._restart, self._trace = seed, first_room, max_fuse, restart, trace
        self.device = device
        self.n_rooms = sum(s[2] for s in segments)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.ge_batch_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- stepping
    def step(self, n_turns: int = 1, stream: int = 0):
        _check(self._lib.ge_batch_step(self._h, n_turns, C.c_void_p(stream or None)), "ge_batch_step")

    def reset(self):
        _check(self._lib.ge_batch_reset(self._h), "ge_batch_reset")

    def sync(self):
        _check(self._lib.ge_batch_sync(self._h), "ge_batch_sync")

    @property
    def turn(self) -> int:
        t = C.c_uint64()
        _check(self._lib.ge_batch_turn(self._h, C.byref(t)))
        return t.value

    def set_turn(self, turn: int):
        """Restore the turn counter of a checkpoint (the RNG and end_turn are keyed by it)."""
        _check(self._lib.ge_batch_set_turn(self._h, turn), "ge_batch_set_turn")

    def set_timing(self, on: bool):
        _check(self._lib.ge_batch_set_timing(self._h, int(on)))

    def kernel_time(self, reset: bool = True) -> Tuple[float, int]:
        ms, n = C.c_double(), C.c_uint64()
        _check(self._lib.ge_batch_kernel_time(self._h, int(reset), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    # ---- state access
    def read_rooms(self, first: int = 0, count: Optional[int] = None, out: Optional[np.ndarray] = None) -> np.ndarray:
        """Canonical views of `count` rooms from `first` on.  `out`: an array of a previous call to fill again (a fresh
        228-byte-per-room array costs its page faults on top of the read)."""
        count = self.n_rooms - first if count is None else count
        if out is None:
            out = np.empty(count, dtype=ROOM_VIEW_DTYPE)        # the library writes every byte of every view
        assert out.dtype == ROOM_VIEW_DTYPE and out.flags.c_contiguous and len(out) == count
        _check(self._lib.ge_batch_read_rooms(self._h, first, count, out.ctypes.data, out.nbytes), "ge_batch_read_rooms")
        return out

    def write_rooms(self, first: int, views: np.ndarray):
        assert views.dtype == ROOM_VIEW_DTYPE and views.flags.c_contiguous
        st = self._lib.ge_batch_write_rooms(self._h, first, len(views), views.ctypes.data)
        if st == -1 and len(views):             # all-or-nothing: say which view did not fit its segment (pack / players / phase ids / role class)
            bad = int(self._lib.ge_last_rejected_room())
            if first <= bad < first + len(views):
                raise GeError(st, f"ge_batch_write_rooms: room {bad} does not fit its segment (nothing was written)")
        _check(st, "ge_batch_write_rooms")

    def inject_action(self, room: int, player_id: int, choice: int):
        """Log an action of a host-driven (human) player in the room's current phase."""
        _check(self._lib.ge_batch_inject_action(self._h, room, player_id, choice), "ge_batch_inject_action")

    def inject_actions(self, rooms, player_ids, choices) -> np.ndarray:
        """Log many host-driven players' actions at once (one kernel).  Returns the per-action status
        (0 = applied, negative ge_status = refused and nothing changed for that action)."""
        rooms = np.ascontiguousarray(rooms, dtype=np.uint64)
        player_ids = np.ascontiguousarray(player_ids, dtype=np.uint32)
        choices = np.ascontiguousarray(choices, dtype=np.uint32)
        if not (len(rooms) == len(player_ids) == len(choices)):
            raise GeError(-1, "inject_actions: arrays differ in length")
        status = np.zeros(len(rooms), dtype=np.int32)
        st = self._lib.ge_batch_inject_actions(self._h, len(rooms), rooms.ctypes.data, player_ids.ctypes.data,
                                               choices.ctypes.data, status.ctypes.data)
        # the return value is the first refused action's status - or a failure of the call itself (closed handle,
        # allocation, HIP error), which leaves the status array untouched: that one must not read as "all applied"
        if st != 0 and not status.any():
            _check(st, "ge_batch_inject_actions")
        return status

    def read_events(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """[count, n_turns] events of the most recent step() call (batch created with trace=True)."""
        count = self.n_rooms - first if count is None else count
        n = C.c_uint32()
        st = self._lib.ge_batch_read_events(self._h, first, 0, C.byref(n), None, 0)
        _check(st, "ge_batch_read_events")
        out = np.zeros((count, max(n.value, 1)), dtype=EVENT_DTYPE)
        _check(self._lib.ge_batch_read_events(self._h, first, count, C.byref(n), out.ctypes.data, out.nbytes),
               "ge_batch_read_events")
        return out[:, : n.value]

    def step_rooms(self, rooms, keys, turns) -> np.ndarray:
        """One turn of each listed room (local indices, pairwise distinct), room k keyed as global room keys[k] at turn
        turns[k]: what a lone batch with first_room = keys[k] and turn counter turns[k] does to it in one step(1).  The
        batch's turn counter, its trace and every unlisted room are untouched.  Returns event k of room k (EVENT_DTYPE).
        All-or-nothing: a room outside the batch, turn 0xFFFFFFFF or a repeated room raises and steps nothing."""
        rooms = np.ascontiguousarray(rooms, dtype=np.uint64)
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        turns = np.ascontiguousarray(turns, dtype=np.uint32)
        if not (len(rooms) == len(keys) == len(turns)):
            raise GeError(-1, "step_rooms: arrays differ in length")
        out = np.zeros(len(rooms), dtype=EVENT_DTYPE)
        _check(self._lib.ge_batch_step_rooms(self._h, len(rooms), rooms.ctypes.data, keys.ctypes.data, turns.ctypes.data,
                                             out.ctypes.data), "ge_batch_step_rooms")
        return out

    def step_rooms_playout(self, rooms, keys, turns, masks, playout_keys, n_rollouts: int, max_turns: int = 256,
                           seed: Optional[int] = None, full_view: bool = False, halving: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """step_rooms with playout seats (POLICY.md §3d): bit i of masks[k] makes seat i+1 of room k a playout bot.  Such a seat,
        when the policy has it act in this turn with at least 2 candidates, takes the candidate whose rollout_seats entry
        (room k as it stands, playout_keys[k], turns[k], the seat - or 0 with full_view -, that one action, n_rollouts,
        max_turns, seed) has the highest seat_wins of the seat; ties go to the policy's own pick among the tied.  Returns
        (events, decided): events as step_rooms (the decided seats listed as acted), decided[k] bit i = seat i+1 chose by
        playouts.  seed None: the batch's seed.  All-or-nothing (GeError, nothing run): step_rooms's checks, rollout_seats's
        caps, a mask bit at or above the room's player count or on a host-driven seat, or sum of popcount(mask) x n_players x
        n_rollouts over the rooms above 2^26.  halving (GE_PLAYOUT_HALVING, POLICY.md §3h): a seat's candidates are valued in
        ceil(log2 c) rounds of growing replica ranges, the worse half leaving after each, so that only the finalists play all
        n_rollouts playouts; fewer playouts but more launches per turn, and slower at every shape measured on an MI355X (x 0.38 .. 0.71 of the unflagged call's speed): DESIGN.md §4."""
        rooms = np.ascontiguousarray(rooms, dtype=np.uint64)
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        turns = np.ascontiguousarray(turns, dtype=np.uint32)
        masks = np.ascontiguousarray(masks, dtype=np.uint32)
        pkeys = np.ascontiguousarray(playout_keys, dtype=np.uint64)
        if not (len(rooms) == len(keys) == len(turns) == len(masks) == len(pkeys)):
            raise GeError(-1, "step_rooms_playout: arrays differ in length")
        events = np.zeros(len(rooms), dtype=EVENT_DTYPE)
        decided = np.zeros(len(rooms), dtype=np.uint32)
        flags = (1 if full_view else 0) | (4 if halving else 0)  # GE_PLAYOUT_FULL_VIEW | GE_PLAYOUT_HALVING
        _check(self._lib.ge_batch_step_rooms_playout(self._h, len(rooms), rooms.ctypes.data, keys.ctypes.data, turns.ctypes.data,
                                                     masks.ctypes.data, pkeys.ctypes.data, n_rollouts, max_turns,
                                                     self._seed if seed is None else seed, flags, events.ctypes.data,
                                                     decided.ctypes.data), "ge_batch_step_rooms_playout")
        return events, decided

    def run_rooms(self, rooms, keys, turns, max_turns: int = 64, until=("person", "end"),
                  views: bool = True) -> Tuple[np.ndarray, np.ndarray, np.ndarray, Optional[np.ndarray]]:
        """Play each listed room on until a person is needed (POLICY.md §3f): room k takes step_rooms's entries (rooms[k], keys[k],
        turns[k] + t), t = 0, 1, ..., and stops after the first turn that leaves it in a state named in `until` - "person": a
        host-driven seat of its segment is a pending target (an inject_action of it would be accepted); "end": a terminal phase;
        "phase": the turn moved the phase - or after max_turns turns; the first turn is always played.  `until` is a sequence of
        those names or the ABI's bit set.  Returns (played, stopped, events, views): played[k] turns were played, stopped[k] has
        the RUN_UNTIL bits that held after the last one (0: the limit), events / views have shape (n, max_turns) and hold, below
        played[k], each turn's step_rooms event and the read_rooms_at view after it (index them only there; views=False: None).
        All-or-nothing like step_rooms; also max_turns outside 1 .. 4096, n * max_turns above 2^20 or turns[k] + max_turns
        above 0xFFFFFFFF raise and run nothing."""
        rooms = np.ascontiguousarray(rooms, dtype=np.uint64)
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        turns = np.ascontiguousarray(turns, dtype=np.uint32)
        if not (len(rooms) == len(keys) == len(turns)):
            raise GeError(-1, "run_rooms: arrays differ in length")
        bits = run_until_bits(until)
        if int(max_turns) < 0 or int(max_turns) > 0xFFFFFFFF:   # no uint32 at all (0 and values above the cap go to the library's checks)
            raise GeError(GE_ERR_ARG, "run_rooms: max_turns")
        n, cap = len(rooms), int(max_turns)
        if n * cap > 1 << 20 or cap > 4096:                      # the library refuses these (after its entry checks): no arrays for them
            cap = 0
        played = np.zeros(n, dtype=np.uint32)
        stopped = np.zeros(n, dtype=np.uint32)
        events = np.zeros((n, cap), dtype=EVENT_DTYPE)
        out = np.zeros((n, cap), dtype=ROOM_VIEW_DTYPE) if views else None
        _check(self._lib.ge_batch_run_rooms(self._h, n, rooms.ctypes.data, keys.ctypes.data, turns.ctypes.data, max_turns, bits,
                                            played.ctypes.data, stopped.ctypes.data, events.ctypes.data,
                                            out.ctypes.data if views else None, out.nbytes if views else 0), "ge_batch_run_rooms")
        return played, stopped, events, out

    def run_rooms_playout(self, rooms, keys, turns, masks, playout_keys, n_rollouts: int, playout_max_turns: int = 256,
                          seed: Optional[int] = None, full_view: bool = False, max_turns: int = 64, until=("person", "end"),
                          views: bool = True, halving: bool = False) -> Tuple[np.ndarray, np.ndarray, np.ndarray, Optional[np.ndarray], np.ndarray]:
        """run_rooms with playout seats (POLICY.md §3g): room k takes step_rooms_playout's entries (rooms[k], keys[k], turns[k] + t,
        masks[k], playout_keys[k]; n_rollouts, playout_max_turns, seed, full_view, halving), t = 0, 1, ..., and stops as run_rooms stops it.
        Between the turns of the call the host does not wait for the device.  Returns (played, stopped, events, views, decided):
        the first four as run_rooms returns them, events being step_rooms_playout's (the decided seats listed as acted);
        decided has shape (n, max_turns) and holds, below played[k], each turn's decided mask.  All-or-nothing: run_rooms's checks,
        then step_rooms_playout's, with the cost cap per turn and turns[k] + max_turns - 1 + playout_max_turns within 0xFFFFFFFF."""
        rooms = np.ascontiguousarray(rooms, dtype=np.uint64)
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        turns = np.ascontiguousarray(turns, dtype=np.uint32)
        masks = np.ascontiguousarray(masks, dtype=np.uint32)
        pkeys = np.ascontiguousarray(playout_keys, dtype=np.uint64)
        if not (len(rooms) == len(keys) == len(turns) == len(masks) == len(pkeys)):
            raise GeError(-1, "run_rooms_playout: arrays differ in length")
        bits = run_until_bits(until)
        if int(max_turns) < 0 or int(max_turns) > 0xFFFFFFFF:   # no uint32 at all (0 and values above the cap go to the library's checks)
            raise GeError(GE_ERR_ARG, "run_rooms_playout: max_turns")
        n, cap = len(rooms), int(max_turns)
        if n * cap > 1 << 20 or cap > 4096:                      # the library refuses these (after its entry checks): no arrays for them
            cap = 0
        played = np.zeros(n, dtype=np.uint32)
        stopped = np.zeros(n, dtype=np.uint32)
        decided = np.zeros((n, cap), dtype=np.uint32)
        events = np.zeros((n, cap), dtype=EVENT_DTYPE)
        out = np.zeros((n, cap), dtype=ROOM_VIEW_DTYPE) if views else None
        flags = (1 if full_view else 0) | (4 if halving else 0)  # GE_PLAYOUT_FULL_VIEW | GE_PLAYOUT_HALVING
        _check(self._lib.ge_batch_run_rooms_playout(self._h, n, rooms.ctypes.data, keys.ctypes.data, turns.ctypes.data, masks.ctypes.data,
                                                    pkeys.ctypes.data, n_rollouts, playout_max_turns, self._seed if seed is None else seed,
                                                    flags, max_turns, bits, played.ctypes.data, stopped.ctypes.data, decided.ctypes.data,
                                                    events.ctypes.data, out.ctypes.data if views else None, out.nbytes if views else 0),
               "ge_batch_run_rooms_playout")
        return played, stopped, events, out, decided

    def run_rooms_forecast(self, rooms, keys, turns, forecast_keys, n_rollouts: int, playout_max_turns: int = 1024, seats=None,
                           seed: Optional[int] = 0, max_turns: int = 64, until=("person", "end")):
        """run_rooms with a forecast of every turn it played (POLICY.md §3i): (played, stopped, events, views) are run_rooms's for
        the same (rooms, keys, turns, max_turns, until), and stats, a (n, max_turns + 1, 77) uint64 array, holds for point
        p = 0 .. played[k] the rollout_seats words of room k as it stood there - point 0 before the call, point p after its turn
        p - 1 - under (forecast_keys[k], turns[k] + p, seats[k], no actions; n_rollouts, playout_max_turns, seed).  seats None: the
        full view for every entry; seed None: the batch's seed.  Rows past played[k] are not written (zero here).  All-or-nothing:
        run_rooms's checks, then 1 <= n_rollouts <= 2^20, playout_max_turns <= 4096, n * (max_turns + 1) <= 2^16, n * (max_turns + 1)
        * n_rollouts <= 2^26, seats within their rooms' player counts, turns[k] + max_turns + playout_max_turns within 0xFFFFFFFF."""
        rooms = np.ascontiguousarray(rooms, dtype=np.uint64)
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        turns = np.ascontiguousarray(turns, dtype=np.uint32)
        fkeys = np.ascontiguousarray(forecast_keys, dtype=np.uint64)
        seat_arr = None if seats is None else np.ascontiguousarray(seats, dtype=np.uint32)
        if not (len(rooms) == len(keys) == len(turns) == len(fkeys)) or (seat_arr is not None and len(seat_arr) != len(rooms)):
            raise GeError(-1, "run_rooms_forecast: arrays differ in length")
        bits = run_until_bits(until)
        if int(max_turns) < 0 or int(max_turns) > 0xFFFFFFFF:   # no uint32 at all (0 and values above the cap go to the library's checks)
            raise GeError(GE_ERR_ARG, "run_rooms_forecast: max_turns")
        n, cap = len(rooms), int(max_turns)
        if n * cap > 1 << 20 or cap > 4096:                      # the library refuses these (after its entry checks): no arrays for them
            cap = 0
        pts = cap + 1 if n * (cap + 1) <= 1 << 16 else 0         # (likewise)
        played = np.zeros(n, dtype=np.uint32)
        stopped = np.zeros(n, dtype=np.uint32)
        events = np.zeros((n, cap), dtype=EVENT_DTYPE)
        out = np.zeros((n, cap), dtype=ROOM_VIEW_DTYPE)
        stats = np.zeros((n, pts, _lib.ROLLOUT_WORDS), dtype=np.uint64)
        _check(self._lib.ge_batch_run_rooms_forecast(self._h, n, rooms.ctypes.data, keys.ctypes.data, turns.ctypes.data, max_turns, bits,
                                                     fkeys.ctypes.data, None if seat_arr is None else seat_arr.ctypes.data, n_rollouts,
                                                     playout_max_turns, self._seed if seed is None else seed, played.ctypes.data,
                                                     stopped.ctypes.data, events.ctypes.data, out.ctypes.data, out.nbytes,
                                                     stats.ctypes.data, stats.nbytes), "ge_batch_run_rooms_forecast")
        return played, stopped, events, out, stats

    def find_rooms(self, want=("person", "end"), phases=None, first: int = 0, count: Optional[int] = None,
                   cap: Optional[int] = None) -> Tuple[np.ndarray, int]:
        """The rooms of first .. first + count - 1 that need attention, as they stand (POLICY.md §3k; the batch is only read).
        `want` is a sequence of "person" (a host-driven seat of the room's segment is a pending target: run_rooms's test), "end"
        (a terminal phase) and "phase" (the room's phase id is in `phases`), or the ABI's bit set.  phases: a list of phase ids
        for every segment, or a dict segment -> list; it requires "phase" in `want`.  Returns (hits, n_match): hits
        (ROOM_HIT_DTYPE: room, why, pending, phase_id, segment) are the first min(n_match, cap) matches in ascending room order,
        `why` the FIND_WANT bits that hold, `pending` bit i = host-driven seat i+1 could act now (pending_seats); n_match counts
        every match of the range.  count None: to the end of the batch; cap None: count; cap 0 counts only.  A truncated scan
        goes on from first = hits[-1]["room"] + 1."""
        bits = find_want_bits(want)
        masks = None
        if phases is not None:
            if not bits & FIND_WANT["phase"]:
                raise ValueError('find_rooms: phases requires "phase" in want')
            masks = np.zeros(len(self.segments), dtype=np.uint32)
            for g in range(len(self.segments)):
                for pid in (phases.get(g, ()) if isinstance(phases, dict) else phases):
                    if not 0 <= int(pid) < 32:
                        raise GeError(GE_ERR_ARG, "find_rooms: phase id")
                    masks[g] |= np.uint32(1 << int(pid))
        count = self.n_rooms - first if count is None else count
        cap = count if cap is None else cap
        if min(int(first), int(count), int(cap)) < 0:
            raise GeError(GE_ERR_ARG, "find_rooms: first / count / cap")
        hits = np.zeros(max(0, min(int(cap), int(count))), dtype=ROOM_HIT_DTYPE)
        n_hits, n_match = C.c_uint64(), C.c_uint64()
        _check(self._lib.ge_batch_find_rooms(self._h, first, count, bits, masks.ctypes.data if masks is not None else None,
                                             hits.ctypes.data if len(hits) else None, len(hits), C.byref(n_hits), C.byref(n_match)),
               "ge_batch_find_rooms")
        return hits[: n_hits.value], int(n_match.value)

    def set_seats(self, rooms, masks):
        """Per-room host-driven seats (POLICY.md §3l): masks[k] (bit i = seat i+1 is host-driven) becomes the seat mask of room
        rooms[k] (local indices, pairwise distinct).  From then on every call that honours the segment's human_mask - step,
        step_rooms, the run-ons, find_rooms, the playout-seat check - honours the room's own mask instead.  All-or-nothing: a room
        outside the batch, a repeated room or a mask bit at or above the room's player count raises and changes nothing.  The mask
        is configuration: reset, set_turn, record writes and restarts leave it; a change takes effect with the next turn played."""
        rooms = np.ascontiguousarray(rooms, dtype=np.uint64)
        masks = np.ascontiguousarray(masks, dtype=np.uint32)
        if len(rooms) != len(masks):
            raise GeError(-1, "set_seats: rooms and masks differ in length")
        _check(self._lib.ge_batch_set_seats(self._h, len(rooms), rooms.ctypes.data, masks.ctypes.data), "ge_batch_set_seats")

    def seats(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """The seat masks of rooms first .. first + count - 1 (uint32; the segment's human_mask where none was ever set), from the
        library's host mirror: no device synchronisation.  count None: to the end of the batch."""
        count = self.n_rooms - first if count is None else count
        if min(int(first), int(count)) < 0:
            raise GeError(GE_ERR_ARG, "seats: first / count")
        out = np.zeros(int(count), dtype=np.uint32)
        _check(self._lib.ge_batch_get_seats(self._h, first, count, out.ctypes.data if len(out) else None), "ge_batch_get_seats")
        return out

    def clear_seats(self):
        """Every room back to its segment's human_mask; the seat plane is freed."""
        _check(self._lib.ge_batch_clear_seats(self._h), "ge_batch_clear_seats")

    def read_rooms_at(self, rooms) -> np.ndarray:
        """Canonical views of the listed rooms, out[k] = room rooms[k] (any order, repeats allowed)."""
        rooms = np.ascontiguousarray(rooms, dtype=np.uint64)
        out = np.empty(len(rooms), dtype=ROOM_VIEW_DTYPE)        # the library writes every byte of every view
        _check(self._lib.ge_batch_read_rooms_at(self._h, len(rooms), rooms.ctypes.data, out.ctypes.data, out.nbytes),
               "ge_batch_read_rooms_at")
        return out

    def write_rooms_at(self, rooms, views):
        """Store views[k] into room rooms[k] (local indices, pairwise distinct): the indexed twin of write_rooms, one copy and
        one device scatter.  A record is stored exactly as write_rooms stores it.  All-or-nothing: a room outside the batch, a
        repeated room or a view that does not fit its room's segment raises and writes nothing."""
        rooms = np.ascontiguousarray(rooms, dtype=np.uint64)
        views = np.ascontiguousarray(np.asarray(views, dtype=ROOM_VIEW_DTYPE).reshape(-1))
        if len(rooms) != len(views):
            raise GeError(-1, "write_rooms_at: rooms and views differ in length")
        st = self._lib.ge_batch_write_rooms_at(self._h, len(rooms), rooms.ctypes.data, views.ctypes.data)
        if st == -1 and len(rooms) and len(np.unique(rooms)) == len(rooms):
            bad = int(self._lib.ge_last_rejected_room())
            if bad in set(int(r) for r in rooms):
                raise GeError(st, f"ge_batch_write_rooms_at: room {bad} does not fit its segment (nothing was written)")
        _check(st, "ge_batch_write_rooms_at")

    def rollout_rooms(self, rooms, keys, turns, n_rollouts: int, max_turns: int = 1024, seed: Optional[int] = None) -> np.ndarray:
        """Playouts: entry k is played n_rollouts times from room rooms[k] as it stands, replica r as global room keys[k] + r
        (mod 2^64) under `seed` (None: the batch's seed) at turns turns[k] .. turns[k] + max_turns - 1, every seat played by the
        policy and a finished game left finished.  Returns the raw (n, 77) uint64 words of ge_rollout_stats (rollout_to_dict reads
        one row): row k's first 41 words are what summary_words() of a fresh batch of n_rollouts copies of the room, keyed from
        keys[k], would give after set_turn(turns[k]) and step(max_turns).  The batch is only read.  Caps (GeError otherwise,
        nothing run): 1 <= n_rollouts <= 2^20, n * n_rollouts <= 2^26, max_turns <= 4096, turns[k] + max_turns < 2^32."""
        return self._rollout("rollout_rooms", rooms, keys, turns, None, None, n_rollouts, max_turns, seed)[0]

    def rollout_actions(self, rooms, keys, turns, actions, n_rollouts: int, max_turns: int = 1024,
                        seed: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        """Playouts after given actions: entry k is rollout_rooms's entry (rooms[k], keys[k], turns[k]) with actions[k], a
        sequence of (player_id, choice) pairs, logged in every replica, in that order, before its first turn (what
        inject_actions would log).  Legality is decided per entry on the device: an entry any of whose actions is refused is not
        played.  Returns (words (n, 77) uint64, status (n,) int32): status[k] = 0 and words[k] as rollout_rooms would give for
        the room after those actions, or status[k] = the refused action's status and words[k] = 0.  An entry without actions is
        rollout_rooms's entry word for word.  The batch is only read.  GeError only for a structural error (rollout_rooms's caps,
        more than 12 actions in one entry), before anything runs."""
        return self._rollout("rollout_actions", rooms, keys, turns, None, actions, n_rollouts, max_turns, seed)

    def rollout_seats(self, rooms, keys, turns, seats, actions=None, n_rollouts: int = 4096, max_turns: int = 1024,
                      seed: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        """Playouts from a seat's view (POLICY.md §3c): entry k is rollout_actions's entry (rooms[k], keys[k], turns[k],
        actions[k]) with every replica's copy re-dealt, after the actions, over what seat seats[k] (1-based) cannot see - the
        hidden roles of the seats it cannot rule out (Werewolf), the speaker's unrevealed lie (Two-Truths).  seats[k] = 0: the
        full view, rollout_actions's entry word for word.  actions None: no actions in any entry.  Returns (words (n, 77)
        uint64, status (n,) int32) as rollout_actions.  The batch is only read.  GeError only for a structural error
        (rollout_actions's, or a seat above its room's player count), before anything runs."""
        return self._rollout("rollout_seats", rooms, keys, turns, seats, actions, n_rollouts, max_turns, seed)

    def rollout_compare(self, rooms, keys, turns, seats, actions, baseline, subjects, n_rollouts: int = 4096, max_turns: int = 1024,
                        seed: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """rollout_seats with every entry also compared, playout by playout, against its baseline entry (POLICY.md §3e):
        baseline[k] is an index into this call (the same room), subjects[k] the seat (1-based) whose outcome is compared -
        Werewolf: its team has won, Two-Truths: its total_score.  Returns (words (n, 77) uint64, status (n,) int32, cmp (n, 6)
        uint64): words and status are rollout_seats's for the same entries word for word; cmp[k] = (compared, better, worse,
        gain, loss, diff_sq) of ge_compare_stats, all zero when entry k or its baseline was refused.  Only equal keys, turns
        and seats of an entry and its baseline make it a comparison on common random numbers.  At most 65 536 entries.  The
        batch is only read.  GeError only for a structural error (rollout_seats's, a baseline outside the call or of another
        room, a subject outside 1 .. n_players or other than its baseline's), before anything runs."""
        extra = (np.ascontiguousarray(baseline, dtype=np.uint32), np.ascontiguousarray(subjects, dtype=np.uint32))
        return self._rollout("rollout_compare", rooms, keys, turns, seats, actions, n_rollouts, max_turns, seed, extra)

    def rollout_beliefs(self, rooms, keys, turns, seats, actions, beliefs, n_rollouts: int = 4096, max_turns: int = 1024,
                        seed: Optional[int] = None, baseline=None, subjects=None):
        """rollout_seats - with baseline and subjects, rollout_compare - under the caller's beliefs (POLICY.md §3j): beliefs is
        (n, 16) uint8, byte c of row k how much entry k's caller suspects seat c + 1 of being a werewolf (Werewolf) or statement
        c + 1 of being the lie (Two-Truths), as prior odds 0 .. 255.  The wolf seats among the seats seats[k] cannot rule out,
        and a redrawn lie, are drawn by these weights instead of uniformly; what the seat knows is never overridden.  Equal
        weights give rollout_seats's entry word for word; nothing in the engine derives the weights.  Returns (words, status),
        or with baseline and subjects (words, status, cmp), as those methods.  The batch is only read.  GeError only for a
        structural error (theirs, a non-zero byte at a slot the room does not have, baseline without subjects or the reverse),
        before anything runs."""
        bel = np.ascontiguousarray(beliefs, dtype=np.uint8)
        if bel.ndim != 2 or bel.shape[1] != _lib.BELIEF_SLOTS:
            raise GeError(-1, f"rollout_beliefs: beliefs must be (n, {_lib.BELIEF_SLOTS}) bytes")
        if (baseline is None) != (subjects is None):
            raise GeError(-1, "rollout_beliefs: baseline and subjects go together")
        extra = None
        if baseline is not None:
            extra = (np.ascontiguousarray(baseline, dtype=np.uint32), np.ascontiguousarray(subjects, dtype=np.uint32))
        return self._rollout("rollout_beliefs", rooms, keys, turns, seats, actions, n_rollouts, max_turns, seed, extra, bel)

    def advise_seats(self, rooms, keys, turns, seats, n_rollouts: int, max_turns: int = 1024, seed: Optional[int] = None,
                     full_view: bool = False) -> np.ndarray:
        """Advice for listed seats, found, played and ranked on the device (POLICY.md §3m).  Entry k is seat seats[k] (1-based,
        any seat: no human mask is consulted) of room rooms[k].  Returns an ADVICE_DTYPE array: `legal` bit c-1 is set exactly
        when inject_action(rooms[k], seats[k], c) would be accepted now; for each such c, option[c-1] = (finished, wins, score)
        are summary.finished, seat_wins[seat-1] and seat_score[seat-1] of rollout_seats's entry (rooms[k], keys[k], turns[k],
        seats[k] - 0 with full_view -, [(seats[k], c)]; n_rollouts, max_turns, seed); `policy` the same of that entry without
        actions; `best` the legal choice with the most wins (Werewolf) or the highest score (Two-Truths), the lowest on a tie;
        `phase_id` the room's phase.  A seat that could not act now gets status GE_ERR_ARG and zeros: that is an answer, not an
        error.  The batch is only read.  GeError only for a structural error (NULL-free here: n_rollouts outside 1 .. 2^20,
        max_turns > 4096, a room outside the batch, a seat outside 1 .. its room's player count, turns[k] + max_turns beyond
        0xFFFFFFFF, more than 2^26 playouts reserved), before anything runs."""
        rooms = np.ascontiguousarray(rooms, dtype=np.uint64)
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        turns = np.ascontiguousarray(turns, dtype=np.uint32)
        seats = np.ascontiguousarray(seats, dtype=np.uint32)
        if not len(rooms) == len(keys) == len(turns) == len(seats):
            raise GeError(-1, "advise_seats: arrays differ in length")
        out = np.zeros(len(rooms), dtype=ADVICE_DTYPE)
        _check(self._lib.ge_batch_advise_seats(self._h, len(rooms), rooms.ctypes.data, keys.ctypes.data, turns.ctypes.data,
                                               seats.ctypes.data, n_rollouts, max_turns, self._seed if seed is None else seed,
                                               _lib.ADVISE_FULL_VIEW if full_view else 0, out.ctypes.data), "ge_batch_advise_seats")
        return out

    def observe_seats(self, seats, out, first: int = 0, count: Optional[int] = None, stream: int = 0):
        """What each listed seat (1-based, pairwise distinct) is shown of rooms first .. first + count - 1, into DEVICE memory the
        caller owns (POLICY.md §3n): `out` is a torch tensor, or any object with data_ptr() and a byte size (nbytes, or numel()
        and element_size()), of at least count * len(seats) * 192 bytes; record (r - first) * len(seats) + j is room r as seat
        seats[j] sees it (SEAT_OBS_DTYPE).  Launched on `stream` (a hipStream_t handle; torch: current_stream().cuda_stream),
        asynchronous, ordered behind the batch's earlier work as step() is; nothing crosses to the host.  The batch is only read."""
        seats = np.ascontiguousarray(seats, dtype=np.uint32)
        count = self.n_rooms - first if count is None else count
        ptr, nbytes = _device_buffer(out)
        _check(self._lib.ge_batch_observe_seats(self._h, first, count, len(seats), seats.ctypes.data if len(seats) else None, ptr, nbytes,
                                                C.c_void_p(stream or None)), "ge_batch_observe_seats")

    def act_seats(self, seats, choices, status=None, first: int = 0, count: Optional[int] = None, stream: int = 0):
        """inject_actions over a range of rooms with the choices read from DEVICE memory: `choices` (int32, count * len(seats)
        entries, same kinds of object as observe_seats's `out`) holds at (r - first) * len(seats) + j the choice of seat seats[j]
        in room r, 0 = no action.  `status` (int32, same shape, optional) gets 0 for a zero or an applied choice and GE_ERR_ARG
        for a refused one, which changes nothing.  Launched on `stream`, asynchronous, ordered as step() is."""
        seats = np.ascontiguousarray(seats, dtype=np.uint32)
        count = self.n_rooms - first if count is None else count
        need = 4 * int(count) * len(seats)
        ptr, nbytes = _device_buffer(choices)
        st_ptr, st_bytes = _device_buffer(status) if status is not None else (None, need)
        if nbytes < need or st_bytes < need:
            raise GeError(GE_ERR_ARG, "act_seats: choices / status hold fewer than count * len(seats) int32 entries")
        _check(self._lib.ge_batch_act_seats(self._h, first, count, len(seats), seats.ctypes.data if len(seats) else None, ptr, st_ptr,
                                            C.c_void_p(stream or None)), "ge_batch_act_seats")

    def run_seats(self, seats, played, stopped=None, max_turns: int = 16, until=("seat", "end"), first: int = 0, count: Optional[int] = None,
                  stream: int = 0):
        """Play every room of first .. first + count - 1 on until a listed seat (1-based, pairwise distinct) must act, with the
        results in DEVICE memory the caller owns (POLICY.md §3p): room r takes run_rooms's entry (r, its global index, the batch's
        turn) under max_turns and `until` - a sequence of "person" / "end" / "phase" / "seat", or the bit set; "seat": some listed
        seat is a pending target of the record the turn left (its observation's `legal` is not 0).  The turn is step_rooms's: the
        room's own seat mask decides whom the policy plays, the seat list plays no part in it.  `played` (uint32 or int32, count
        entries, the kinds of object observe_seats takes) gets the turns each room played, `stopped` (optional, the same) the
        RUN_SEATS_UNTIL bits that held after its last turn (0: the limit).  The batch's turn advances by max_turns whatever the
        rooms played.  Launched on `stream`, asynchronous, ordered behind the batch's earlier work as step() is; nothing crosses
        to the host."""
        seats = np.ascontiguousarray(seats, dtype=np.uint32)
        count = self.n_rooms - first if count is None else count
        bits = _named_bits(until, RUN_SEATS_UNTIL, "until: unknown stop condition")
        if int(max_turns) < 0 or int(max_turns) > 0xFFFFFFFF:   # no uint32 at all (0 and values above the cap go to the library's checks)
            raise GeError(GE_ERR_ARG, "run_seats: max_turns")
        need = 4 * int(count)
        ptr, nbytes = _device_buffer(played) if played is not None else (None, need)
        st_ptr, st_bytes = _device_buffer(stopped) if stopped is not None else (None, need)
        if nbytes < need or st_bytes < need:
            raise GeError(GE_ERR_ARG, "run_seats: played / stopped hold fewer than count 4-byte entries")
        _check(self._lib.ge_batch_run_seats(self._h, first, count, len(seats), seats.ctypes.data if len(seats) else None, max_turns, bits,
                                            ptr, st_ptr, C.c_void_p(stream or None)), "ge_batch_run_seats")

    def gather_seats(self, seats, out, entries, n, want=("seat", "end"), first: int = 0, count: Optional[int] = None, cap: Optional[int] = None,
                     stream: int = 0):
        """The decision list of rooms first .. first + count - 1 into DEVICE memory the caller owns (POLICY.md §3q): of the
        count * len(seats) records observe_seats would store, those that are due - `want` "seat": legal != 0, "end": done != 0;
        a sequence of the names, one of them, or the GATHER_WANT bit set - in ascending entry order.  `out` (192 bytes per
        entry) gets the first min(M, cap) due records byte for byte, `entries` (uint32 or int32) their entry indices
        (r - first) * len(seats) + j, and `n` (two 4-byte words) min(M, cap) and M, the number of due entries.  Nothing beyond
        the list is written: rows at and behind n[0] keep what they held.  cap None: what `out` and `entries` both hold; cap = 0
        counts only (out and entries may then be None).  The kinds of object observe_seats takes.  Launched on `stream`,
        asynchronous, ordered behind the batch's earlier work as step() is; nothing crosses to the host (a call of a larger
        shape than any before it grows the batch's scratch, which may wait for the device).  The batch is only read."""
        seats = np.ascontiguousarray(seats, dtype=np.uint32)
        count = self.n_rooms - first if count is None else count
        bits = _named_bits(want, _lib.GATHER_WANT, "want: unknown condition")
        o_ptr, o_bytes = _device_buffer(out) if out is not None else (None, 0)
        e_ptr, e_bytes = _device_buffer(entries) if entries is not None else (None, 0)
        n_ptr, n_bytes = _device_buffer(n) if n is not None else (None, 8)
        cap = min(o_bytes // _lib.SEAT_OBS_BYTES, e_bytes // 4) if cap is None else int(cap)
        if cap < 0 or o_bytes < cap * _lib.SEAT_OBS_BYTES or e_bytes < 4 * cap or n_bytes < 8:
            raise GeError(GE_ERR_ARG, "gather_seats: out / entries hold fewer than cap entries, or n fewer than two words")
        _check(self._lib.ge_batch_gather_seats(self._h, first, count, len(seats), seats.ctypes.data if len(seats) else None, bits, o_ptr, e_ptr,
                                               cap, n_ptr, C.c_void_p(stream or None)), "ge_batch_gather_seats")

    def act_listed(self, seats, n, entries, choices, status=None, first: int = 0, count: Optional[int] = None, cap: Optional[int] = None,
                   stream: int = 0):
        """act_seats from a list in DEVICE memory (POLICY.md §3q): with D the dense count * len(seats) choices that are 0 except
        D[entries[i]] = choices[i] for i < min(n[0], cap) - n[0] read on the device -, the call is act_seats(seats, D), and
        status[i] (int32, optional) that call's verdict at entries[i].  `n`, `entries`, `choices` as gather_seats left them or in
        any order (choices int32); an entry at or above count * len(seats) gets GE_ERR_ARG and touches nothing; status behind the
        list is not written; of an entry named twice one choice is applied and every copy reports its verdict.  cap None: what
        entries, choices and status all hold.  Launched on `stream`, asynchronous, ordered as step() is."""
        seats = np.ascontiguousarray(seats, dtype=np.uint32)
        count = self.n_rooms - first if count is None else count
        n_ptr, n_bytes = _device_buffer(n) if n is not None else (None, 4)
        e_ptr, e_bytes = _device_buffer(entries) if entries is not None else (None, 0)
        c_ptr, c_bytes = _device_buffer(choices) if choices is not None else (None, 0)
        s_ptr, s_bytes = _device_buffer(status) if status is not None else (None, None)
        holds = min(e_bytes, c_bytes, c_bytes if s_bytes is None else s_bytes) // 4
        cap = holds if cap is None else int(cap)
        if cap < 0 or cap > holds or n_bytes < 4:
            raise GeError(GE_ERR_ARG, "act_listed: entries / choices / status hold fewer than cap 4-byte entries, or n no word")
        _check(self._lib.ge_batch_act_listed(self._h, first, count, len(seats), seats.ctypes.data if len(seats) else None, n_ptr, cap, e_ptr,
                                             c_ptr, s_ptr, C.c_void_p(stream or None)), "ge_batch_act_listed")

    def teach_seats(self, seats, out, n_rollouts: int, max_turns: int = 1024, *, first: int = 0, count: Optional[int] = None, keys=None,
                    key0: int = 0, turn: Optional[int] = None, seed: Optional[int] = None, full_view: bool = False, stream: int = 0):
        """advise_seats for each listed seat (1-based, pairwise distinct) of rooms first .. first + count - 1, into DEVICE memory the
        caller owns (POLICY.md §3o): `out` (the kinds of object observe_seats takes, at least count * len(seats) * 224 bytes) gets
        at (r - first) * len(seats) + j, byte for byte, the ADVICE_DTYPE record advise_seats returns for (room r, key(r), turn,
        seats[j]) under the same n_rollouts, max_turns, seed and full_view.  key(r) = keys[r - first] where `keys` (uint64 on the
        device, count entries) is given, else key0 + (r << 20) mod 2^64.  turn None: the batch's turn; seed None: the batch's seed.
        Launched on `stream`, asynchronous, ordered behind the batch's earlier work as step() is; nothing crosses to the host (a
        call of a larger shape than any before it grows the batch's scratch, which may wait for the device).  The batch is only
        read."""
        seats = np.ascontiguousarray(seats, dtype=np.uint32)
        count = self.n_rooms - first if count is None else count
        ptr, nbytes = _device_buffer(out)
        k_ptr = None
        if keys is not None:
            k_ptr, k_bytes = _device_buffer(keys)
            if k_bytes < 8 * int(count):
                raise GeError(GE_ERR_ARG, "teach_seats: keys hold fewer than count uint64 entries")
        _check(self._lib.ge_batch_teach_seats(self._h, first, count, len(seats), seats.ctypes.data if len(seats) else None, k_ptr,
                                              int(key0) & 0xFFFFFFFFFFFFFFFF, self.turn if turn is None else turn, n_rollouts, max_turns,
                                              self._seed if seed is None else seed, _lib.ADVISE_FULL_VIEW if full_view else 0, ptr, nbytes,
                                              C.c_void_p(stream or None)), "ge_batch_teach_seats")

    def _rollout(self, method: str, rooms, keys, turns, seats, actions, n_rollouts: int, max_turns: int,
                 seed: Optional[int], compare=None, beliefs=None):
        """The rollout_* methods: one call of ge_batch_<method> (seats and actions are read where the method has them;
        actions None: every entry's slice empty, passed as NULL).  Returns (words, status) - with compare, rollout_compare's
        (baseline, subjects), (words, status, cmp); GeError naming the method when the lengths differ, or naming the symbol when
        it fails without a verdict written."""
        rooms = np.ascontiguousarray(rooms, dtype=np.uint64)
        args = [rooms, np.ascontiguousarray(keys, dtype=np.uint64), np.ascontiguousarray(turns, dtype=np.uint32)]
        if method in ("rollout_seats", "rollout_compare", "rollout_beliefs"):
            args.append(np.ascontiguousarray(seats, dtype=np.uint32))
        if method == "rollout_actions" or actions is not None:
            actions = [list(a) for a in actions]
        if len({len(x) for x in args + list(compare or ()) + ([] if beliefs is None else [beliefs])}
               | ({len(rooms)} if actions is None else {len(actions)})) > 1:
            raise GeError(-1, f"{method}: arrays differ in length")
        out = np.zeros((len(rooms), _lib.ROLLOUT_WORDS), dtype=np.uint64)
        status = None
        if method != "rollout_rooms":
            first = players = choices = None
            if actions is not None:                              # CSR: entry k's actions are [first[k], first[k + 1])
                first = np.zeros(len(actions) + 1, dtype=np.uint32)
                first[1:] = np.cumsum([len(a) for a in actions])
                flat = [pc for a in actions for pc in a]
                players = np.ascontiguousarray([int(p) for p, _ in flat], dtype=np.uint32)
                choices = np.ascontiguousarray([int(c) for _, c in flat], dtype=np.uint32)
            status = np.full(len(rooms), 1, dtype=np.int32)      # 1: untouched (no ge_status is positive)
            args += [first, players, choices, status]
            if beliefs is not None:
                args.append(beliefs)
        sym = "ge_batch_" + method
        tail = []
        if compare is not None:
            cmp = np.zeros((len(rooms), _lib.COMPARE_WORDS), dtype=np.uint64)
            tail = [compare[0].ctypes.data, compare[1].ctypes.data, cmp.ctypes.data]
        elif beliefs is not None:
            tail = [None, None, None]
        st = getattr(self._lib, sym)(self._h, len(rooms), *[x if x is None else x.ctypes.data for x in args], n_rollouts, max_turns,
                                     self._seed if seed is None else seed, out.ctypes.data, *tail)
        # a refused entry returns its status with every entry's verdict written; a structural error or a failure of the call
        # leaves the verdicts untouched (ge_batch_rollout_rooms writes none)
        if st != 0 and (status is None or (status == 1).any()):
            _check(st, sym)
        if compare is not None:
            return out, status, cmp
        return out, status

    def write_agent_state(self, room: int, state: Dict[str, Any], visit_actions: Optional[Dict[Any, int]] = None) -> Dict[str, Any]:
        """Adopt a reference AgentState into one room (agent_state_to_view); returns its host-side fields."""
        return self.write_agent_states([room], [state], None if visit_actions is None else [visit_actions])[0]

    def write_agent_states(self, rooms, states: Sequence[Dict[str, Any]],
                           visit_actions: Optional[Sequence[Optional[Dict[Any, int]]]] = None) -> List[Dict[str, Any]]:
        """Adopt many AgentStates at once: every state is converted (and refused, ValueError) before one write_rooms_at."""
        rooms = [int(r) for r in rooms]
        if len(rooms) != len(states) or (visit_actions is not None and len(visit_actions) != len(states)):
            raise ValueError("write_agent_states: rooms, states and visit_actions differ in length")
        views, hosts = [], []
        for k, (room, st) in enumerate(zip(rooms, states)):
            tb, n = self._segment_of(room)
            v, host = agent_state_to_view(tb, st, n, None if visit_actions is None else visit_actions[k])
            views.append(v)
            hosts.append(host)
        self.write_rooms_at(rooms, views)
        return hosts

    def summary(self) -> Dict[str, Any]:
        s = _lib.Summary()
        _check(self._lib.ge_batch_summary(self._h, C.byref(s)), "ge_batch_summary")
        return summary_to_dict(np.frombuffer(bytes(s), dtype="<u8"))

    def summary_words(self) -> np.ndarray:
        s = _lib.Summary()
        _check(self._lib.ge_batch_summary(self._h, C.byref(s)), "ge_batch_summary")
        return np.frombuffer(bytes(s), dtype="<u8").copy()

    # ---- checkpoint / resume (the reference delegates this to LangGraph thread persistence; here a batch
    # ---- is its room records + the turn counter, and the RNG is counter-based, so a resumed batch continues bit-exact)
    def save_checkpoint(self, path: str) -> None:
        """Self-contained, layout-independent checkpoint: every room as a ge_room_view, the turn counter, the batch
        description and the games' DSLs (numpy .npz; `load_checkpoint` rebuilds the batch from it alone)."""
        meta = {"abi": _lib.GE_ABI_VERSION, "seed": self._seed, "first_room": self._first_room, "turn": self.turn,
                "max_fuse": self._max_fuse, "restart": self._restart, "trace": self._trace,
                "segments": [{"dsl": seg[0].dsl, "rounds": int(seg[0].c.rounds), "n_players": int(seg[1]), "n_rooms": int(seg[2]),
                              "human_mask": int(seg[3]) if len(seg) > 3 else 0} for seg in self.segments]}
        with open(path, "wb") as f:
            np.savez_compressed(f, views=self.read_rooms(), meta=np.frombuffer(json.dumps(meta).encode("utf-8"), dtype=np.uint8))

    @classmethod
    def load_checkpoint(cls, path: str, device: int = 0) -> "RoomBatch":
        with np.load(path, allow_pickle=False) as z:
            meta = json.loads(bytes(z["meta"]).decode("utf-8"))
            views = np.ascontiguousarray(z["views"])
        if meta["abi"] != _lib.GE_ABI_VERSION:
            raise GeError(-1, f"checkpoint written by ABI {meta['abi']}, this library is ABI {_lib.GE_ABI_VERSION}")
        segs = [(GameTable(sg["dsl"], sg["rounds"]), sg["n_players"], sg["n_rooms"], sg["human_mask"]) for sg in meta["segments"]]
        b = cls(segs, seed=meta["seed"], first_room=meta["first_room"], device=device, max_fuse=meta["max_fuse"],
                restart=meta["restart"], trace=meta["trace"])
        b.write_rooms(0, views.astype(ROOM_VIEW_DTYPE, copy=False))
        b.set_turn(meta["turn"])
        return b

    def state(self, segment: int = 0) -> Tuple[int, int, int]:
        p, nbytes, bpr = C.c_void_p(), C.c_size_t(), C.c_uint32()
        _check(self._lib.ge_batch_state(self._h, segment, C.byref(p), C.byref(nbytes), C.byref(bpr)))
        return p.value, nbytes.value, bpr.value

    def bytes_per_room(self, segment: int = 0) -> int:
        return self.state(segment)[2]

    def _segment_of(self, room: int) -> Tuple[GameTable, int]:
        base = 0
        for seg in self.segments:
            tb, n, rooms = seg[:3]
            if room < base + rooms:
                return tb, n
            base += rooms
        raise IndexError(room)

    def agent_state(self, room: int) -> Dict[str, Any]:
        """AgentState-shaped dict of one room (agent/game_agent_v2.py:97-117): what the TS
        frontend's useCoAgent sync receives (src/lib/canvas/types.ts:338-360)."""
        tb, _ = self._segment_of(room)
        return view_to_agent_state(tb, self.read_rooms(room, 1)[0])


class RoomGroup:
    """One host process, several GPUs: the rooms of `segments` (the WHOLE job) sharded over `devices`, stepped
    concurrently, with one RCCL all-gather of the per-device summaries inside the native library (ge_group_*,
    include/ge_step.h).  Results equal those of one RoomBatch with the same arguments, for any number of devices.
    (The multi-process form, one rank per GPU over torch.distributed, is game_engine_amd.dist.)"""

    def __init__(self, segments: Sequence[Segment], devices: Sequence[int], seed: int = 0, first_room: int = 0,
                 max_fuse: int = 0, restart: bool = False, trace: bool = False):
        lib = _lib.load()
        if not 1 <= len(segments) <= _lib.GE_MAX_SEGMENTS:
            raise GeError(-1, "segments")
        self.segments = list(segments)
        d = self._desc = _job_desc(segments, seed, first_room, max_fuse, restart, trace)
        devs = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        _check(lib.ge_group_create(C.byref(d), devs, len(devices), C.byref(h)), "ge_group_create")
        self._h, self._lib = h, lib
        self.n_devices = len(devices)
        self.n_rooms = sum(s[2] for s in segments)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.ge_group_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def step(self, n_turns: int = 1):
        _check(self._lib.ge_group_step(self._h, n_turns), "ge_group_step")

    def sync(self):
        _check(self._lib.ge_group_sync(self._h), "ge_group_sync")

    def summary(self) -> Dict[str, Any]:
        s = _lib.Summary()
        _check(self._lib.ge_group_summary(self._h, C.byref(s)), "ge_group_summary")
        return summary_to_dict(np.frombuffer(bytes(s), dtype="<u8"))

    def shard_summaries(self) -> List[Dict[str, Any]]:
        """Each device's own ge_batch_summary (host-side cross-check of the collective: they add up to summary())."""
        out = []
        for i in range(self.n_devices):
            b, s = C.c_void_p(), _lib.Summary()
            _check(self._lib.ge_group_shard(self._h, i, C.byref(b)), "ge_group_shard")
            _check(self._lib.ge_batch_summary(b, C.byref(s)), "ge_batch_summary")
            out.append(summary_to_dict(np.frombuffer(bytes(s), dtype="<u8")))
        return out

    def read_rooms(self) -> np.ndarray:
        """All rooms in the order of one RoomBatch with the same segments (segment-major)."""
        shards = []
        for i in range(self.n_devices):
            b = C.c_void_p()
            _check(self._lib.ge_group_shard(self._h, i, C.byref(b)), "ge_group_shard")
            shards.append(b)
        return reassemble_rooms(self._lib, shards, self._desc)


def _job_desc(segments: Sequence[Segment], seed: int, first_room: int, max_fuse: int, restart: bool, trace: bool) -> "_lib.BatchDesc":
    d = _lib.BatchDesc()
    d.seed, d.first_room, d.n_segments, d.device, d.max_fuse = seed, first_room, len(segments), 0, max_fuse
    d.flags = (1 if restart else 0) | (2 if trace else 0)
    for k, seg in enumerate(segments):
        tb, n_players, n_rooms = seg[:3]
        d.seg[k].table = C.pointer(tb.c)
        d.seg[k].n_players, d.seg[k].n_rooms = n_players, n_rooms
        d.seg[k].human_mask = seg[3] if len(seg) > 3 else 0
    return d


def partition(desc: "_lib.BatchDesc", n_parts: int, part: int):
    """(shard desc, [global index of the part's first room of each segment]) - ge_group_partition, the arithmetic
    ge_group_create shards a job with: the part-th of n_parts contiguous parts of every segment.  No device is touched."""
    lib = _lib.load()
    shard = _lib.BatchDesc()
    first = (C.c_uint64 * _lib.GE_MAX_SEGMENTS)()
    _check(lib.ge_group_partition(C.byref(desc), n_parts, part, C.byref(shard), first), "ge_group_partition")
    return shard, [int(first[k]) for k in range(desc.n_segments)]


def reassemble_rooms(lib, shard_handles, desc: "_lib.BatchDesc") -> np.ndarray:
    """Every room of a sharded job in the order of ONE batch of `desc` (segment-major): shard i holds, segment by segment,
    the i-th part of each; read each part and put segment k's parts side by side.  Used by RoomGroup (devices of a node)
    and RoomShards (shards placed by the host)."""
    n = len(shard_handles)
    per_seg: List[List[np.ndarray]] = [[] for _ in range(desc.n_segments)]
    for i, b in enumerate(shard_handles):
        sd, _ = partition(desc, n, i)
        first = 0
        for k in range(desc.n_segments):
            cnt = int(sd.seg[k].n_rooms)
            out = np.empty(cnt, dtype=ROOM_VIEW_DTYPE)          # the library writes every byte of every view
            _check(lib.ge_batch_read_rooms(b, first, cnt, out.ctypes.data, out.nbytes), "ge_batch_read_rooms")
            per_seg[k].append(out)
            first += cnt
    return np.concatenate([x for seg in per_seg for x in seg])


class RoomShards:
    """The same sharding as RoomGroup, with the shards placed by the host: `devices[i]` is where part i of len(devices) lives -
    devices may repeat (several shards on one GPU) and no collective library is involved; summary() adds the shards' own
    summaries on the host (every field is a sum over rooms).  For hosts that schedule shards themselves, and the way the n > 1
    partition is exercised on a one-GPU box (tests/test_gpu_group.py)."""

    def __init__(self, segments: Sequence[Segment], devices: Sequence[int], seed: int = 0, first_room: int = 0,
                 max_fuse: int = 0, restart: bool = False, trace: bool = False):
        lib = _lib.load()
        if not 1 <= len(segments) <= _lib.GE_MAX_SEGMENTS:
            raise GeError(-1, "segments")
        self.segments, self._lib = list(segments), lib
        self._desc = _job_desc(segments, seed, first_room, max_fuse, restart, trace)
        self._h: List[C.c_void_p] = []
        self.firsts: List[List[int]] = []
        for i, dev in enumerate(devices):
            sd, first = partition(self._desc, len(devices), i)
            sd.device = dev
            h = C.c_void_p()
            arr = (C.c_uint64 * _lib.GE_MAX_SEGMENTS)(*(first + [0] * (_lib.GE_MAX_SEGMENTS - len(first))))
            st = lib.ge_batch_create_shard(C.byref(sd), arr, C.byref(h))
            if st != 0:
                self.close()
                _check(st, "ge_batch_create_shard")
            self._h.append(h)
            self.firsts.append(first)
        self.n_rooms = sum(s[2] for s in segments)

    def close(self):
        for h in getattr(self, "_h", []):
            self._lib.ge_batch_destroy(h)
        self._h = []

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def step(self, n_turns: int = 1):
        for h in self._h:                                  # asynchronous: shards on different devices step concurrently
            _check(self._lib.ge_batch_step(h, n_turns, None), "ge_batch_step")

    def shard_summaries(self) -> List[Dict[str, Any]]:
        out = []
        for h in self._h:
            s = _lib.Summary()
            _check(self._lib.ge_batch_summary(h, C.byref(s)), "ge_batch_summary")
            out.append(summary_to_dict(np.frombuffer(bytes(s), dtype="<u8")))
        return out

    def summary(self) -> Dict[str, Any]:
        return sum_summaries(self.shard_summaries())

    def read_rooms(self) -> np.ndarray:
        return reassemble_rooms(self._lib, self._h, self._desc)


def sum_summaries(parts: List[Dict[str, Any]]) -> Dict[str, Any]:
    """Whole-job summary from the shards' (what the all-gather + sum of ge_group_summary computes): sums mod 2^64; `turn` is common."""
    out: Dict[str, Any] = {}
    for k, v in parts[0].items():
        if isinstance(v, list):
            out[k] = [sum(p[k][j] for p in parts) & 0xFFFFFFFFFFFFFFFF for j in range(len(v))]
        else:
            out[k] = v if k == "turn" else sum(p[k] for p in parts) & 0xFFFFFFFFFFFFFFFF
    return out


def summary_to_dict(w: np.ndarray) -> Dict[str, Any]:
    w = [int(x) for x in w]
    return {"rooms": w[0], "finished": w[1], "village_wins": w[2], "wolf_wins": w[3], "alive_players": w[4],
            "sum_end_turn": w[5], "end_turn_hist": w[6:22], "score_hist": w[22:38], "checksum": w[38], "turn": w[39], "games_recycled": w[40]}


def rollout_to_dict(w: np.ndarray) -> Dict[str, Any]:
    """One row of RoomBatch.rollout_rooms: {"summary": summary_to_dict(...), "seat_alive", "seat_wins", "seat_score"} (12 each)."""
    w = [int(x) for x in w]
    return {"summary": summary_to_dict(w[:_lib.SUMMARY_WORDS]), "seat_alive": w[41:53], "seat_wins": w[53:65], "seat_score": w[65:77]}


def project_view(view, table: Optional["GameTable"] = None) -> List[int]:
    """Canonical integer projection of one room: [phase, prev_phase, phase0_done, end_turn]
    + 11 ints per player (+ detective memory per player, werewolf) — the form the parity
    tests compare (tests/golden/*.json 'layout').  With `table`: only what the DSL declares (a slot it does not
    declare reads 0, as it does in a reference-run room, whose player_states have no such field)."""
    n = int(view["n_players"])
    out = [int(view["phase_id"]), int(view["prev_phase_id"]), int(view["phase0_done"]), int(view["end_turn"])]
    names = table.field_names if table is not None else None
    shown = [1 if (names is None or names[s]) else 0 for s in range(9)] + [1, 1]
    for i in range(n):
        out += [int(x) * k for x, k in zip(view["players"][i][:11], shown)]
    if int(view["pack"]) == PACK_WEREWOLF:
        det = 1 if (names is None or names[SLOT_DET_MEMORY]) else 0
        out += [int(x) * det for x in view["det"][:n]]
    return out


def slot_values(tb: GameTable, view, i: int) -> List[Any]:
    """Player i's state, one value per slot of the pack (GE_WW_* / GE_TT_* order), whether or not the DSL declares it."""
    f = [int(x) for x in view["players"][i]]
    if int(view["pack"]) == PACK_WEREWOLF:
        n = int(view["n_players"])
        mem = {str(k + 1): _TEAMS[int(d)] for k, d in enumerate(view["det"][:n]) if d} if f[0] == 4 else {}
        return [tb.role_name(f[0]), _TEAMS[f[1]], bool(f[2]), bool(f[3]), bool(f[4]), bool(f[5]), bool(f[6]), bool(f[7]), f[8],
                mem, f[1] == 2]
    return [bool(f[0]), bool(f[1]), f[2], bool(f[3]), bool(f[4]), f[5], bool(f[6]), f[7], f[8]]


def view_to_agent_state(tb: GameTable, view) -> Dict[str, Any]:
    """player_states hold exactly the fields the DSL declares, under the DSL's own names (GameTable.field_names)."""
    n = int(view["n_players"])
    ps: Dict[str, Dict[str, Any]] = {}
    for i in range(n):
        vals = slot_values(tb, view, i)
        ps[str(i + 1)] = {tb.field_names[s]: v for s, v in enumerate(vals) if tb.field_names[s]}
        ps[str(i + 1)].update(tb.extra_fields)             # declared fields no rule writes: the template's values
    pid = int(view["phase_id"])
    return {"current_phase_id": pid, "current_phase_name": tb.phase_name(pid), "player_states": ps,
            "previous_phase_id": int(view["prev_phase_id"]), "end_turn": int(view["end_turn"])}


# ---- AgentState -> room view: the inverse of view_to_agent_state / RoomLog.agent_state, for threads handed over mid-game
_ACTION_TAG = re.compile(r"^\[t=(\d+)\|c=(\d+)\]")
# integer slots and the largest value the record holds for them (None: the player count); the rest are booleans
_WW_INTS = {8: None}
_TT_INTS = {2: 3, 5: 3, 7: 255, 8: 15}


def _phase_of(entry, where: str) -> int:
    pid = entry.get("phase_id") if isinstance(entry, dict) else None
    if not isinstance(pid, int) or isinstance(pid, bool):
        raise ValueError(f"{where}: phase_history entries need an integer phase_id, got {entry!r}")
    return pid


_ACT_NIGHT = (1, 2, 3)                      # include/ge_step.h GE_ACT_WOLF_TARGET, GE_ACT_DOCTOR_PROTECT, GE_ACT_DETECTIVE
_EFF_NIGHT_BEGIN = 2                       # GE_EFF_NIGHT_BEGIN


def _derive_undeclared_ww(table: GameTable, v, n: int, pa: Dict[str, Any], hist_ids: List[int], visit: Dict[int, int], cur: int):
    """Werewolf slots a DSL may leave undeclared (the reference's draft declares no has_secret_role, night_action_submitted or
    selected_target_id) still drive the rules.  Their state then lives where the reference keeps it: in the role and the action
    log.  has_secret_role = any role but Villager once roles are dealt; night_action_submitted / selected_target_id = the latest
    night action (wolf target, protection, investigation) since the room last entered a night-begin phase, as the record effects
    write and the night-begin effect clears them (POLICY.md 3)."""
    names = table.field_names
    if names[5] and names[7] and names[8]:
        return
    rows = {r["phase_id"]: r for r in table.rows()}
    name_act = {r["name"]: r["act"] for r in rows.values()}
    since = -1                                 # the last turn that entered a night-begin phase
    for t, pid in enumerate(hist_ids):
        if rows.get(pid, {}).get("effect") == _EFF_NIGHT_BEGIN and (t == 0 or hist_ids[t - 1] != pid):
            since = t
    night: Dict[int, Tuple[int, int]] = {}
    for key, rec in pa.items():
        try:
            pid = int(key)
        except (TypeError, ValueError):
            continue
        acts = (rec or {}).get("actions") or {} if isinstance(rec, dict) else {}
        for a in (acts.values() if isinstance(acts, dict) else acts):
            if not isinstance(a, dict) or name_act.get(a.get("phase")) not in _ACT_NIGHT:
                continue
            m = _ACTION_TAG.match(str(a.get("action", "")))
            if m and since < int(m.group(1)) < len(hist_ids) and 1 <= pid <= n and int(m.group(1)) >= night.get(pid, (-1, 0))[0]:
                night[pid] = (int(m.group(1)), int(m.group(2)))
    if rows[cur]["act"] in _ACT_NIGHT:
        for pid, c in visit.items():
            night[pid] = (len(hist_ids), c)
    for i in range(n):
        f = v["players"][i]
        if not names[5] and f[0] >= 2:
            f[5] = 1
        if i + 1 in night:
            if not names[7]:
                f[7] = 1
            if not names[8]:
                f[8] = night[i + 1][1]


def agent_state_to_view(table: GameTable, state: Dict[str, Any], n_players: Optional[int] = None,
                        visit_actions: Optional[Dict[Any, int]] = None) -> Tuple[np.ndarray, Dict[str, Any]]:
    """The room view of a reference AgentState (agent/game_agent_v2.py:97-117: current_phase_id, player_states, playerActions,
    phase_history) under the DSL's own field names: the exact inverse of view_to_agent_state and RoomLog.agent_state.

    Returns (view, host_side).  host_side holds what the record does not carry and a host renders back: per player the `name`,
    the Two-Truths `statements` text, and every key the record does not model ({"names", "statements", "extra"}, keyed "1".."n").
    A modelled field the state leaves out takes the template's value (player_states_template).  Phase fields:
      prev_phase_id  state["previous_phase_id"], else the phase of the phase_history entry before the trailing run of the current
                     phase (the phase the room last left: phase_history[-2] when the last turn moved), else a fresh room's;
      phase0_done    some phase_history entry is phase 0 (the guard of v2:1025-1052);
      end_turn       state["end_turn"], else for a terminal phase the history index where its trailing run began, else -1;
      games          state.get("games", 0).
    acted / choice (this visit's log) come from the playerActions entries tagged "[t=<turn>|c=<choice>]" (as
    toolcalls.turn_tool_calls writes them) filed under the current phase's name at a turn of the current visit; untagged entries
    (a person's messages) are ignored.  visit_actions={player_id: choice} overrides that: how a host passes a human seat's
    pending action.  The thread's next turn is len(phase_history) (one entry per run, v2:1207-1215).
    Anything that does not fit, or that would not read back unchanged through view_to_agent_state, raises ValueError naming the
    player and field; no library call is made."""
    if not isinstance(state, dict):
        raise ValueError("state must be a dict")
    ww = table.pack == PACK_WEREWOLF
    names = table.field_names
    ps = state.get("player_states")
    if not isinstance(ps, dict) or not ps:
        raise ValueError("state['player_states'] must be a non-empty dict")
    n = len(ps) if n_players is None else int(n_players)
    if not 1 <= n <= GE_MAX_PLAYERS:
        raise ValueError(f"{n} players: a room holds 1..{GE_MAX_PLAYERS}")
    by_id: Dict[int, Dict[str, Any]] = {}
    for key, rec in ps.items():
        try:
            pid = int(key)
        except (TypeError, ValueError):
            raise ValueError(f"player_states key {key!r} is not a player id") from None
        if pid in by_id or not isinstance(rec, dict):
            raise ValueError(f"player {key!r}: repeated or not a dict")
        by_id[pid] = rec
    if sorted(by_id) != list(range(1, n + 1)):
        raise ValueError(f"player_states must name players 1..{n} exactly, got {sorted(by_id)}")
    rows = table.rows()
    ids = [r["phase_id"] for r in rows]
    cur = state.get("current_phase_id")
    if not isinstance(cur, int) or isinstance(cur, bool) or cur not in ids:
        raise ValueError(f"current_phase_id {cur!r} is not a phase of the table")
    hist = state.get("phase_history") or []
    if not isinstance(hist, list):
        raise ValueError("phase_history must be a list")
    hist_ids = [_phase_of(e, "phase_history") for e in hist]
    s = len(hist_ids)                                          # the trailing run of the current phase: hist[s:]
    while s > 0 and hist_ids[s - 1] == cur:
        s -= 1

    v = np.zeros(1, dtype=ROOM_VIEW_DTYPE)[0]
    v["n_players"], v["pack"] = n, table.pack
    v["phase_id"] = cur
    prev = state.get("previous_phase_id")
    if prev is None:
        prev = hist_ids[s - 1] if s > 0 else 0                 # a fresh room holds phase 0 as its previous phase
    if not isinstance(prev, int) or isinstance(prev, bool) or prev not in ids:
        raise ValueError(f"previous_phase_id {prev!r} is not a phase of the table")
    v["prev_phase_id"] = prev
    v["phase0_done"] = 1 if 0 in hist_ids else 0
    end = state.get("end_turn")
    if end is None:
        end = min(s, 0xFFFE) if not rows[ids.index(cur)]["branches"] else -1
    if not isinstance(end, int) or isinstance(end, bool) or not -1 <= end <= 0xFFFE:
        raise ValueError(f"end_turn {end!r} is out of range (-1 .. 65534)")
    v["end_turn"] = end
    games = state.get("games", 0)
    if not isinstance(games, int) or isinstance(games, bool) or not 0 <= games <= 0xFFFF:
        raise ValueError(f"games {games!r} is out of range (0 .. 65535)")
    v["games"] = games

    roles = [table.role_name(c) for c in range(5)] if ww else []
    teams = {t: k for k, t in enumerate(_TEAMS)}
    ints = _WW_INTS if ww else _TT_INTS
    n_slots = 9
    modelled = {names[k] for k in range(_lib.GE_MAX_SLOTS) if names[k]} | {"name"}
    host: Dict[str, Any] = {"names": {}, "statements": {}, "extra": {}}
    for pid in range(1, n + 1):
        rec, where = by_id[pid], f"player {pid}"
        f = [int(x) for x in table.c.init_fields[:12]]
        f[9] = f[10] = f[11] = 0
        for k in range(n_slots):
            name = names[k]
            if not name or name not in rec:
                continue
            val = rec[name]
            if ww and k == 0:
                if val not in roles:
                    raise ValueError(f"{where}: field {name!r}: unknown role {val!r} (the DSL declares {roles[1:]})")
                f[k] = roles.index(val)
            elif ww and k == 1:
                if val not in teams:
                    raise ValueError(f"{where}: field {name!r}: team {val!r} is not one of {_TEAMS}")
                f[k] = teams[val]
            elif k in ints:
                hi = n if ints[k] is None else ints[k]
                if not isinstance(val, int) or isinstance(val, bool) or not 0 <= val <= hi:
                    raise ValueError(f"{where}: field {name!r}: {val!r} is not an integer in 0..{hi}")
                f[k] = val
            else:
                if not isinstance(val, bool):
                    raise ValueError(f"{where}: field {name!r}: {val!r} is not a boolean")
                f[k] = int(val)
        v["players"][pid - 1] = f
        if ww and names[SLOT_DET_MEMORY] in rec:
            mem = rec[names[SLOT_DET_MEMORY]]
            field = names[SLOT_DET_MEMORY]
            if not isinstance(mem, dict):
                raise ValueError(f"{where}: field {field!r} must be a dict")
            if mem and f[0] != 4:
                raise ValueError(f"{where}: field {field!r}: only the {roles[4]} holds investigation results")
            for q, team in mem.items():
                try:
                    qi = int(q)
                except (TypeError, ValueError):
                    qi = 0
                if not 1 <= qi <= n or team not in ("villagers", "werewolves"):
                    raise ValueError(f"{where}: field {field!r}: entry {q!r}: {team!r} must name a player 1..{n} and a team")
                v["det"][qi - 1] = teams[team]
        host["names"][str(pid)] = rec.get("name", f"Player {pid}")
        if not ww and names[SLOT_STATEMENTS]:
            st = rec.get(names[SLOT_STATEMENTS], {})
            if not isinstance(st, dict):
                raise ValueError(f"{where}: field {names[SLOT_STATEMENTS]!r} must be a dict")
            host["statements"][str(pid)] = dict(st)
        extra = {k: val for k, val in rec.items() if k not in modelled}
        if extra:
            host["extra"][str(pid)] = extra

    # acted / choice: this visit's latest tagged action per player (turns past the one that entered the phase; a room that
    # never left phase 0 has been in it since turn 0)
    cur_name = table.phase_name(cur)
    first = 0 if (s == 0 and cur == 0) else s + 1
    latest: Dict[int, Tuple[int, int]] = {}
    pa = state.get("playerActions") or {}
    if not isinstance(pa, dict):
        raise ValueError("playerActions must be a dict")
    for key, rec in pa.items():
        try:
            pid = int(key)
        except (TypeError, ValueError):
            continue
        acts = (rec or {}).get("actions") or {} if isinstance(rec, dict) else {}
        for a in (acts.values() if isinstance(acts, dict) else acts):
            if not isinstance(a, dict) or a.get("phase") != cur_name:
                continue
            m = _ACTION_TAG.match(str(a.get("action", "")))
            if not m:
                continue
            t, c = int(m.group(1)), int(m.group(2))
            if first <= t < len(hist_ids) and 1 <= pid <= n and t >= latest.get(pid, (-1, 0))[0]:
                latest[pid] = (t, c)
    acted = {pid: c for pid, (_, c) in latest.items()}
    for key, c in (visit_actions or {}).items():
        acted[int(key)] = c
    top = n if ww else 3
    for pid, c in acted.items():
        if not 1 <= pid <= n or not isinstance(c, int) or isinstance(c, bool) or not 1 <= c <= top:
            raise ValueError(f"player {pid}: visit action {c!r} is not a choice in 1..{top}")
        v["players"][pid - 1][9], v["players"][pid - 1][10] = 1, c
    if ww:
        _derive_undeclared_ww(table, v, n, pa, hist_ids, {int(k): c for k, c in (visit_actions or {}).items()}, cur)

    # self-check: every modelled field reads back as given
    back = view_to_agent_state(table, v)["player_states"]
    for pid in range(1, n + 1):
        rec, got = by_id[pid], back[str(pid)]
        for k in range(_lib.GE_MAX_SLOTS):
            name = names[k]
            if not name or name not in rec or name not in got:
                continue
            want = rec[name]
            if ww and k == SLOT_DET_MEMORY:
                want = {str(q): t for q, t in want.items()}
            if got[name] != want or type(got[name]) is not type(want):
                raise ValueError(f"player {pid}: field {name!r} = {want!r} does not fit the record (it reads back as {got[name]!r})")
    return v, host

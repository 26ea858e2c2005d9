"""RoomPoolService — many game threads hosted in a few resident batches (twin of node/room_pool.js).

RoomService gives every thread its own N = 1 batch: its own device allocations, table upload and staging buffers, and
per message one launch, one read of the room, one read of the events and a synchronisation for each.  Here threads of the
same (game, player count, human seats) share a pool of fixed-capacity batch chunks; a thread owns one slot of one chunk.
Its RNG stream is keyed by `room_index_of(thread_id)` (or the `room_index` it was created with) and its turn counter is its
own, so a thread plays exactly the game it plays on a RoomService: `RoomBatch.step_rooms` moves a slot by one turn keyed
as that global room at that turn.  `handle_messages` is one tick for many threads: per chunk touched, one injection round
per candidate seat, one `step_rooms` and one `read_rooms_at` - against about three synchronising calls per message.

Same per-thread API and outputs as RoomService (create_room / human_action / continue_room / handle_message / close).
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import messages as M
from .room_service import (PLAYOUT_CAP, HintRequest, RolloutRequest, adopted_output, advise_candidates, advise_output, advise_seat, belief_bytes,
                           check_forecast_args, check_forecast_seat, check_playout_options, check_run_args, check_run_forecast, check_run_thread, check_view,
                           forecast_key, forecast_seed, hint_output, playout_mask, playout_max_cands, prepare_adoption, room_index_of, neutral_beliefs, run_forecast_per_call,
                           run_forecasts, run_hints, run_output, run_rollouts, run_turn, seat_forecast_output, seats_mask)
from .stepper import GE_ERR_ARG, PACK_WEREWOLF, GeError, GameTable, RoomBatch, load_dsl_by_gamename, pending_seats, slot_values
from .toolcalls import WW_IS_ALIVE, RoomLog, turn_tool_calls
from .ui_script import ui_tool_calls


class _Pool:
    """The chunks of one (game, n_players, human_mask) and their free slots."""

    def __init__(self, table: GameTable, n_players: int, human_mask: int):
        self.table, self.n_players, self.human_mask = table, n_players, human_mask
        self.chunks: List[Any] = []
        self.free: List[Tuple[int, int]] = []      # (chunk, slot), popped from the end
        self.used: set = set()                     # slots a thread has held: written back to the template when reused
        self.seated: set = set()                   # slots whose seat mask set_human_seats changed: set back to human_mask when reused
        self.template = None                       # the initial room view (player_states_template, phase 0)


class RoomPoolService:
    def __init__(self, games_dir: str = "games", seed: int = 0, device: int = 0, chunk_rooms: int = 1024, playout_rollouts: int = 256,
                 playout_max_turns: int = 256, playout_view: str = "seat", playout_halving: bool = False):
        """playout_*: as RoomService's."""
        if chunk_rooms < 1:
            raise ValueError("chunk_rooms must be >= 1")
        self.playout_full = check_playout_options(playout_rollouts, playout_max_turns, playout_view, playout_halving)
        self.playout_halving = playout_halving
        self._halving_kw = {"halving": True} if playout_halving else {}   # (off: no keyword, so a stand-in batch written before the option existed still serves)
        self.playout_rollouts, self.playout_max_turns = int(playout_rollouts), int(playout_max_turns)
        self.games_dir, self.seed, self.device, self.chunk_rooms = games_dir, seed, device, chunk_rooms
        self._tables: Dict[str, GameTable] = {}
        self._pools: Dict[Tuple[str, int, int], _Pool] = {}
        self._rooms: Dict[str, Dict[str, Any]] = {}

    def table(self, game_name: str, dsl: Optional[dict] = None) -> GameTable:
        if game_name not in self._tables:
            self._tables[game_name] = GameTable(dsl if dsl else load_dsl_by_gamename(game_name, self.games_dir))
        return self._tables[game_name]

    def _new_chunk(self, tb: GameTable, n_players: int, human_mask: int, n_rooms: int):
        """One chunk of a pool: an untraced batch whose slots are stepped only through step_rooms (the device is required)."""
        return RoomBatch([(tb, n_players, n_rooms, human_mask)], seed=self.seed, first_room=0, device=self.device, max_fuse=1)

    # ---- slots
    def _acquire(self, pool: _Pool, template: bool = True) -> Tuple[Any, int, int]:
        if not pool.free:
            ci = len(pool.chunks)
            chunk = self._new_chunk(pool.table, pool.n_players, pool.human_mask, self.chunk_rooms)
            pool.chunks.append(chunk)
            if pool.template is None:
                pool.template = chunk.read_rooms_at([0])[0].copy()
            pool.free.extend((ci, s) for s in reversed(range(self.chunk_rooms)))
        ci, slot = pool.free.pop()
        chunk = pool.chunks[ci]
        if template and (ci, slot) in pool.used:  # a reused slot starts from the template (which also drops any prepared deal)
            chunk.write_rooms(slot, np.array([pool.template], dtype=pool.template.dtype))
        if (ci, slot) in pool.seated:             # ... and with the pool's own seating (set_human_seats changed the slot's mask)
            chunk.set_seats([slot], [pool.human_mask])
            pool.seated.discard((ci, slot))
        pool.used.add((ci, slot))
        return chunk, ci, slot

    def create_room(self, thread_id: str, game_name: str, players: List[Dict[str, Any]], dsl: Optional[dict] = None,
                    room_index: Optional[int] = None, playout_seats=()) -> Dict[str, Any]:
        """As RoomService.create_room: `isBot: False` marks a human seat; room_index = the global room index the thread's RNG
        is keyed by (default: derived from the thread id); playout_seats = bot seats that choose by playouts."""
        tb = self.table(game_name, dsl)
        human_mask = sum(1 << i for i, p in enumerate(players) if p.get("isBot") is False)
        pmask = playout_mask(len(players), human_mask, playout_seats)
        if thread_id in self._rooms:
            self.close(thread_id)
        key = (game_name, len(players), human_mask)
        pool = self._pools.get(key)
        if pool is None:
            pool = self._pools[key] = _Pool(tb, len(players), human_mask)
        chunk, ci, slot = self._acquire(pool)
        names = [p.get("name") or f"Player {i + 1}" for i, p in enumerate(players)]
        room = {"pool": pool, "chunk": chunk, "ci": ci, "slot": slot, "turn": 0,
                "key": room_index_of(thread_id) if room_index is None else int(room_index),
                "table": tb, "gameName": game_name, "names": names, "panel": None,
                "human_seats": [i + 1 for i in range(len(players)) if (human_mask >> i) & 1], "playout_mask": pmask,
                "view": pool.template.copy(), "log": RoomLog(tb, names, game_name)}
        self._rooms[thread_id] = room
        return self._agent_state(room)

    def adopt_room(self, thread_id: str, game_name: str, state: Dict[str, Any], **kw) -> Dict[str, Any]:
        """As RoomService.adopt_room, into a pool slot."""
        return self.adopt_rooms([(thread_id, game_name, state, kw)])[0]

    def adopt_rooms(self, entries: Sequence[Tuple]) -> List[Dict[str, Any]]:
        """Take over many threads that are already mid-game: [(thread_id, game_name, state[, options]), ...] with the options of
        RoomService.adopt_room as a dict (players, human_seats, dsl, room_index, turn, visit_actions, playout_seats).  Every state is converted
        first (ValueError, before any slot is taken); then one write_rooms_at per chunk touched.  A reused slot is written over
        directly (no template write first).  Returns, in order, what RoomService.adopt_room returns for each."""
        prepared, seen = [], set()
        for e in entries:
            tid, game, state = e[0], e[1], e[2]
            kw = dict(e[3]) if len(e) > 3 and e[3] else {}
            if tid in seen:
                raise ValueError(f"thread {tid!r} is named twice")
            seen.add(tid)
            tb = self.table(game, kw.get("dsl"))
            a = prepare_adoption(tb, state, kw.get("players"), kw.get("human_seats", ()), kw.get("turn"), kw.get("visit_actions"))
            a["playout_mask"] = playout_mask(a["n"], a["human_mask"], kw.get("playout_seats", ()))
            prepared.append((tid, game, tb, state, kw, a))
        # slots next (new chunks may be created); a failure gives them back, and no thread has been touched yet
        taken: List[Tuple[_Pool, Any, int, int]] = []
        try:
            for tid, game, tb, state, kw, a in prepared:
                key = (game, a["n"], a["human_mask"])
                pool = self._pools.get(key)
                if pool is None:
                    pool = self._pools[key] = _Pool(tb, a["n"], a["human_mask"])
                taken.append((pool,) + self._acquire(pool, template=False))
            by_chunk: Dict[int, Tuple[Any, List[int]]] = {}
            for k, (_, chunk, _, _) in enumerate(taken):
                by_chunk.setdefault(id(chunk), (chunk, []))[1].append(k)
            views = [None] * len(taken)
            for chunk, ks in by_chunk.values():
                slots = [taken[k][3] for k in ks]
                chunk.write_rooms_at(slots, [prepared[k][5]["view"] for k in ks])
                for k, v in zip(ks, chunk.read_rooms_at(slots)):     # the canonical views, as RoomService reads its room back
                    views[k] = v
        except BaseException:
            for pool, _, ci, slot in taken:
                pool.free.append((ci, slot))
            raise
        rooms = []
        for (tid, game, tb, state, kw, a), (pool, chunk, ci, slot), view in zip(prepared, taken, views):
            if tid in self._rooms:
                self.close(tid)
            room = {"pool": pool, "chunk": chunk, "ci": ci, "slot": slot, "turn": a["turn"],
                    "key": room_index_of(tid) if kw.get("room_index") is None else int(kw["room_index"]),
                    "table": tb, "gameName": game, "names": a["names"], "panel": None,
                    "human_seats": a["human_seats"], "playout_mask": a["playout_mask"], "view": view, "log": RoomLog(tb, a["names"], game)}
            room["log"].adopt(state, a["host"])
            self._rooms[tid] = room
            rooms.append(room)
        return [adopted_output(room, room["turn"]) for room in rooms]

    def _agent_state(self, room: Dict[str, Any]) -> Dict[str, Any]:
        return room["log"].agent_state(room["view"])

    def human_action(self, thread_id: str, player_id: int, choice: int) -> Dict[str, Any]:
        room = self._rooms[thread_id]
        st = room["chunk"].inject_actions([room["slot"]], [player_id], [choice])
        if int(st[0]) != 0:
            raise GeError(int(st[0]), "ge_batch_inject_actions")
        room["view"] = room["chunk"].read_rooms_at([room["slot"]])[0]
        return self._agent_state(room)

    def set_human_seats(self, thread_id: str, seats) -> List[int]:
        """As RoomService.set_human_seats: from the next turn on exactly `seats` (player ids) of the thread are played by people
        (POLICY.md §3l).  The thread stays in its slot and its pool (pools stay keyed by the seating threads are created with); the
        slot's seat mask goes back to the pool's when the slot is reused.  ValueError for an unknown thread or a seat outside
        1..n, before anything changes."""
        room = self._rooms.get(thread_id)
        if room is None:
            raise ValueError(f"unknown thread {thread_id!r}")
        pool = room["pool"]
        mask = seats_mask(thread_id, pool.n_players, seats)
        room["chunk"].set_seats([room["slot"]], [mask])
        pool.seated.add((room["ci"], room["slot"]))
        room["human_seats"] = [i + 1 for i in range(pool.n_players) if (mask >> i) & 1]
        room["playout_mask"] &= ~mask
        return list(room["human_seats"])

    def continue_room(self, thread_id: str, items: Optional[List[Dict[str, Any]]] = None) -> Dict[str, Any]:
        """One turn of one thread: {"state", "toolCalls", "uiCalls"}, as RoomService.continue_room."""
        room = self._rooms[thread_id]
        return self._turns([room], [items])[0]

    def handle_message(self, thread_id: str, text: str, items: Optional[List[Dict[str, Any]]] = None) -> Dict[str, Any]:
        """As RoomService.handle_message (one message of one thread)."""
        return self.handle_messages([(thread_id, text, items)])[0]

    def handle_messages(self, msgs: Sequence[Tuple]) -> List[Dict[str, Any]]:
        """One tick: [(thread_id, text[, items]), ...] -> [output, ...] in the same order, each what handle_message returns
        for it.  A thread may appear once per tick (ValueError otherwise, before anything runs)."""
        entries = []
        seen = set()
        for m in msgs:
            tid, text, items = m[0], m[1], (m[2] if len(m) > 2 else None)
            if tid in seen:
                raise ValueError(f"thread {tid!r} is named twice in one tick")
            seen.add(tid)
            entries.append((self._rooms[tid], text, items))       # KeyError for an unknown thread, before anything runs
        out: List[Optional[Dict[str, Any]]] = [None] * len(entries)
        play, pending = [], []                                  # indices into entries; (index, candidates) of action messages
        for i, (room, text, _) in enumerate(entries):
            kind = M.classify(text)
            if kind == M.CHAT:
                out[i] = {"state": self._agent_state(room), "toolCalls": [], "uiCalls": [], "played": False, "kind": kind}
                continue
            play.append((i, kind))
            if kind == M.ACTION:
                room["log"].person_message(text)
                view, tb = room["view"], room["table"]
                n = int(view["n_players"])
                pid = int(view["phase_id"])
                act = next((r["act"] for r in tb.rows() if r["phase_id"] == pid), 0)
                alive = [bool(slot_values(tb, view, j)[WW_IS_ALIVE]) for j in range(n)] if tb.pack == PACK_WEREWOLF else [True] * n
                cands = list(M.resolve(text, room["panel"], act, tb.pack, room["names"], alive, room["human_seats"]))
                if cands:
                    pending.append((i, cands))
        # injection rounds: a thread's next candidate seat is tried only where the previous one was refused with GE_ERR_ARG
        # (not a living pending target of this phase: logged, no game effect), as RoomService.handle_message's loop
        r = 0
        while pending:
            by_chunk: Dict[int, List[Tuple[int, List]]] = {}
            for i, cands in pending:
                by_chunk.setdefault(id(entries[i][0]["chunk"]), []).append((i, cands))
            nxt = []
            for group in by_chunk.values():
                chunk = entries[group[0][0]][0]["chunk"]
                st = chunk.inject_actions([entries[i][0]["slot"] for i, _ in group], [c[r][0] for _, c in group],
                                          [c[r][1] for _, c in group])
                for (i, cands), s in zip(group, st):
                    if int(s) == 0:
                        continue
                    if int(s) != GE_ERR_ARG:
                        raise GeError(int(s), "ge_batch_inject_actions")
                    if r + 1 < len(cands):
                        nxt.append((i, cands))
            pending, r = nxt, r + 1
        res = self._turns([entries[i][0] for i, _ in play], [entries[i][2] for i, _ in play])
        for (i, kind), o in zip(play, res):
            o.update(played=True, kind=kind)
            out[i] = o
        return out

    def _turns(self, rooms: List[Dict[str, Any]], items: List[Optional[List[Dict[str, Any]]]]) -> List[Dict[str, Any]]:
        """One turn of each room (distinct threads): one step_rooms and one read_rooms_at per chunk touched; a chunk holding a
        thread with playout seats is stepped by step_rooms_playout instead (mask 0 for its other threads; more calls only when
        the playouts would pass the call's cap)."""
        by_chunk: Dict[int, List[int]] = {}
        for j, room in enumerate(rooms):
            by_chunk.setdefault(id(room["chunk"]), []).append(j)
        events, afters = [None] * len(rooms), [None] * len(rooms)
        for js in by_chunk.values():
            chunk = rooms[js[0]]["chunk"]
            slots = np.array([rooms[j]["slot"] for j in js], dtype=np.uint64)
            keys = np.array([rooms[j]["key"] for j in js], dtype=np.uint64)
            turns = np.array([rooms[j]["turn"] for j in js], dtype=np.uint32)
            if any(rooms[j]["playout_mask"] for j in js):
                ev = self._step_playout(chunk, [rooms[j] for j in js], slots, keys, turns)
            else:
                ev = chunk.step_rooms(slots, keys, turns)
            views = chunk.read_rooms_at(slots)
            for k, j in enumerate(js):
                events[j], afters[j] = ev[k], views[k]
                rooms[j]["turn"] += 1
        return [self._finish(room, afters[j], events[j], items[j]) for j, room in enumerate(rooms)]

    def run_room(self, thread_id: str, max_turns: int = 64, until=("person", "end"),
                 items: Optional[List[Dict[str, Any]]] = None, playout: bool = False, forecast: bool = False, forecast_rollouts: int = 4096,
                 forecast_max_turns: int = 1024, forecast_seat: Optional[int] = None) -> Dict[str, Any]:
        """As RoomService.run_room (same turns, forecasts and output), from the thread's pool slot."""
        return self.run_rooms([thread_id], max_turns, until, None if items is None else [items], playout, forecast, forecast_rollouts,
                              forecast_max_turns, None if forecast_seat is None else [forecast_seat])[0]

    def run_rooms(self, thread_ids: Sequence[str], max_turns: int = 64, until=("person", "end"),
                  items: Optional[Sequence[Optional[List[Dict[str, Any]]]]] = None, playout: bool = False, forecast: bool = False,
                  forecast_rollouts: int = 4096, forecast_max_turns: int = 1024,
                  forecast_seats: Optional[Sequence[Optional[int]]] = None) -> List[Dict[str, Any]]:
        """Play many threads on, each until a person is needed in it (RoomService.run_room's conditions and output, in order):
        one RoomBatch.run_rooms call per chunk touched, every thread under its own key and from its own turn.  items[j]: thread
        j's canvas items.  A thread may be named once (ValueError); unknown threads (KeyError), threads with playout seats and
        bad arguments (ValueError) are refused before anything runs.  playout=True: threads with playout seats are run too - a
        chunk holding one takes one RoomBatch.run_rooms_playout call (POLICY.md §3g; mask 0 for its other threads; more calls
        only where the playouts of one turn would pass the call's cap), under the keys, seed and options continue_room gives
        its playout bots.  Every chunk's call is made before any turn is folded: if
        one of them raises (a device error), the threads of the chunks already run have moved on the device while no thread's
        turn or log has - such a service is to be closed, not continued.
        forecast=True: every thread's output gains "forecasts" (RoomService.run_room's; forecast_seats[j]: the seat thread j's
        are seen from, None: the full view), from one RoomBatch.run_rooms_forecast call per chunk touched (POLICY.md §3i; more
        calls only where the points of one call would pass its caps); the options are checked as forecasts checks them and a
        thread with playout seats is refused (ValueError), before anything runs."""
        bits = check_run_args(max_turns, until)
        if len(set(thread_ids)) != len(thread_ids):
            raise ValueError("run_rooms: a thread is named twice")
        rooms = [self._rooms[tid] for tid in thread_ids]          # KeyError for an unknown thread, before anything runs
        its = list(items) if items is not None else [None] * len(rooms)
        if len(its) != len(rooms):
            raise ValueError("run_rooms: thread_ids and items differ in length")
        fseats = list(forecast_seats) if forecast_seats is not None else [None] * len(rooms)
        if len(fseats) != len(rooms):
            raise ValueError("run_rooms: thread_ids and forecast_seats differ in length")
        for tid, room, fs in zip(thread_ids, rooms, fseats):
            check_run_thread(tid, room, playout)
            if forecast:
                check_run_forecast(tid, room, max_turns, forecast_rollouts, forecast_max_turns, fs, room["turn"])
            if int(room["turn"]) + int(max_turns) + (self.playout_max_turns - 1 if room["playout_mask"] else 0) > 0xFFFFFFFF:
                raise ValueError(f"thread {tid!r}: the turn counter would overflow")
        by_chunk: Dict[int, List[int]] = {}
        for j, room in enumerate(rooms):
            by_chunk.setdefault(id(room["chunk"]), []).append(j)
        per_call = max(1, (1 << 20) // int(max_turns))             # the call's cap on n x max_turns
        if forecast:
            per_call = run_forecast_per_call(max_turns, forecast_rollouts)
        got: List[Any] = [None] * len(rooms)
        for all_js in by_chunk.values():
            with_bots = any(rooms[j]["playout_mask"] for j in all_js)
            parts = self._playout_parts([rooms[j] for j in all_js], per_call) if with_bots else \
                [(lo, min(lo + per_call, len(all_js))) for lo in range(0, len(all_js), per_call)]
            for a, b in parts:
                js = all_js[a:b]
                chunk, slots, keys = rooms[js[0]]["chunk"], [rooms[j]["slot"] for j in js], [rooms[j]["key"] for j in js]
                turns = [rooms[j]["turn"] for j in js]
                stats = None
                if forecast:
                    played, stopped, events, views, stats = chunk.run_rooms_forecast(
                        slots, keys, turns, [forecast_key(k) for k in keys], forecast_rollouts, forecast_max_turns,
                        seats=[fseats[j] or 0 for j in js], seed=forecast_seed(self.seed), max_turns=max_turns, until=bits)
                elif with_bots:
                    played, stopped, events, views, _ = chunk.run_rooms_playout(
                        slots, keys, turns, [rooms[j]["playout_mask"] for j in js], [forecast_key(k) for k in keys], self.playout_rollouts,
                        self.playout_max_turns, seed=forecast_seed(self.seed), full_view=self.playout_full, max_turns=max_turns, until=bits,
                        **self._halving_kw)
                else:
                    played, stopped, events, views = chunk.run_rooms(slots, keys, turns, max_turns, bits)
                for k, j in enumerate(js):
                    got[j] = (int(played[k]), int(stopped[k]), events[k], views[k], None if stats is None else stats[k])
        out = []
        for tid, room, (played, stopped, events, views, stats), it, fs in zip(thread_ids, rooms, got, its, fseats):
            fc = None if stats is None else run_forecasts(room["table"], room["names"], tid, room["turn"], played, forecast_rollouts,
                                                          forecast_max_turns, fs, stats)
            room["turn"] += played
            out.append(run_output([run_turn(self._finish(room, views[t], events[t], it)) for t in range(played)], stopped, fc))
        return out

    def _playout_parts(self, rooms: List[Dict[str, Any]], most: Optional[int] = None) -> List[Tuple[int, int]]:
        """Runs [a, b) of one chunk's rooms whose playouts of one turn stay under the call's cap (and of at most `most` rooms)."""
        cost = [bin(int(r["playout_mask"])).count("1") * playout_max_cands(r["table"].pack, r["pool"].n_players) * self.playout_rollouts
                for r in rooms]
        parts, lo, acc = [], 0, 0
        for k, c in enumerate(cost):
            if (acc + c > PLAYOUT_CAP or (most is not None and k - lo >= most)) and k > lo:
                parts.append((lo, k)); lo, acc = k, 0
            acc += c
        parts.append((lo, len(rooms)))
        return parts

    def _step_playout(self, chunk, rooms: List[Dict[str, Any]], slots, keys, turns) -> np.ndarray:
        """step_rooms_playout of one chunk's rooms under advise's keys and seed, in runs under the call's cap."""
        masks = np.array([r["playout_mask"] for r in rooms], dtype=np.uint32)
        pkeys = np.array([forecast_key(r["key"]) for r in rooms], dtype=np.uint64)
        parts = self._playout_parts(rooms)
        evs = [chunk.step_rooms_playout(slots[a:b], keys[a:b], turns[a:b], masks[a:b], pkeys[a:b], self.playout_rollouts,
                                        self.playout_max_turns, seed=forecast_seed(self.seed), full_view=self.playout_full,
                                        **self._halving_kw)[0]
               for a, b in parts]
        return np.concatenate(evs)

    def _finish(self, room: Dict[str, Any], after, event, items) -> Dict[str, Any]:
        # as RoomService._turn: `before` is the view before any action injected with this message
        before = room["view"]
        calls = turn_tool_calls(room["table"], before, after, event)
        room["log"].fold(calls, after)
        room["view"] = after
        state = self._agent_state(room)
        deaths = [c["args"]["player_id"] for c in calls if c["name"] == "update_player_state"
                  and c["args"]["state_name"] == "is_alive" and c["args"]["state_value"] is False]
        ui = ui_tool_calls(room["table"].dsl, state, room["table"], turn=int(event["turn"]), deaths=deaths, items=items)
        room["panel"] = M.newest_panel(ui)
        return {"state": state, "toolCalls": calls, "uiCalls": ui}

    def forecast(self, thread_id: str, n_rollouts: int = 4096, max_turns: int = 1024, seat: Optional[int] = None,
                 beliefs: Optional[Dict[Any, int]] = None) -> Dict[str, Any]:
        """As RoomService.forecast (same keys, seed, seat view, beliefs and output), from the thread's pool slot."""
        return self.forecasts([thread_id], n_rollouts, max_turns, None if seat is None else [seat], None if beliefs is None else [beliefs])[0]

    def forecasts(self, thread_ids: Sequence[str], n_rollouts: int = 4096, max_turns: int = 1024,
                  seats: Optional[Sequence[Optional[int]]] = None,
                  beliefs: Optional[Sequence[Optional[Dict[Any, int]]]] = None) -> List[Dict[str, Any]]:
        """Forecasts of many threads, in order: one rollout_rooms call per chunk touched (replica r of a thread is global room
        (thread_key << 16) + r under seed service seed ^ 0x9E3779B97F4A7C15, from the thread's own turn).  seats[j] (1 .. n):
        thread j's forecast from that seat's view, as RoomService.forecast(seat=...); with seats, one rollout_seats call per
        chunk touched (seat 0 there for the threads without one: their full view).  beliefs[j] (None, or a mapping as
        RoomService.forecast's, for a thread with a seat): a chunk any of whose threads has beliefs gets one rollout_beliefs
        call instead, its other threads under equal weights - their unweighted deal exactly.  No thread changes."""
        check_forecast_args(n_rollouts, max_turns)
        rooms = [self._rooms[tid] for tid in thread_ids]          # KeyError for an unknown thread, before anything runs
        sv = list(seats) if seats is not None else [None] * len(rooms)
        if len(sv) != len(rooms):
            raise ValueError("forecasts: thread_ids and seats differ in length")
        bv = list(beliefs) if beliefs is not None else [None] * len(rooms)
        if len(bv) != len(rooms):
            raise ValueError("forecasts: thread_ids and beliefs differ in length")
        for tid, room, st in zip(thread_ids, rooms, sv):
            check_forecast_seat(tid, len(room["names"]), st)
        bel = [belief_bytes(tid, room["table"], len(room["names"]), bm, st is not None) for tid, room, st, bm in zip(thread_ids, rooms, sv, bv)]
        res = run_rollouts([RolloutRequest(room["chunk"], room["slot"], room["key"], room["turn"], st, None, bl,
                                           neutral_beliefs(room["table"], len(room["names"])))
                            for room, st, bl in zip(rooms, sv, bel)], seats is not None, n_rollouts, max_turns, self.seed)
        return [seat_forecast_output(room["table"], room["names"], tid, room["turn"], n_rollouts, max_turns, sv[j], res[j][0][0], bel[j])
                for j, (tid, room) in enumerate(zip(thread_ids, rooms))]

    def advise(self, thread_id: str, player_id: Optional[int] = None, n_rollouts: int = 4096, max_turns: int = 1024,
               view: str = "full", compare: bool = False, beliefs: Optional[Dict[Any, int]] = None) -> Dict[str, Any]:
        """As RoomService.advise (same candidates, keys, seed, views, compare, beliefs and output), from the thread's pool slot."""
        return self.advises([thread_id], None if player_id is None else [player_id], n_rollouts, max_turns, view, compare,
                            None if beliefs is None else [beliefs])[0]

    def advises(self, thread_ids: Sequence[str], player_ids: Optional[Sequence[Optional[int]]] = None, n_rollouts: int = 4096,
                max_turns: int = 1024, view: str = "full", compare: bool = False,
                beliefs: Optional[Sequence[Optional[Dict[Any, int]]]] = None) -> List[Dict[str, Any]]:
        """Advice for many threads, in order (player_ids[j] None or absent: thread j's lowest human seat): one rollout_actions
        call per chunk touched - rollout_seats in the "seat" view, every thread from its advised seat's view - each thread's
        entries as RoomService.advise's.  compare: one rollout_compare call per chunk touched instead, and every option gains
        "versus" as RoomService.advise's.  beliefs[j] (view "seat" only): thread j's advised seat's suspicions, as
        RoomService.advise's; a chunk any of whose threads has some gets one rollout_beliefs call instead.  No thread changes."""
        check_forecast_args(n_rollouts, max_turns)
        seat_view = check_view(view)
        rooms = [self._rooms[tid] for tid in thread_ids]          # KeyError for an unknown thread, before anything runs
        pids = list(player_ids) if player_ids is not None else [None] * len(rooms)
        if len(pids) != len(rooms):
            raise ValueError("advises: thread_ids and player_ids differ in length")
        seats = [advise_seat(tid, room["human_seats"], pid) for tid, room, pid in zip(thread_ids, rooms, pids)]
        cands = [advise_candidates(room["table"], room["view"]) for room in rooms]
        bv = list(beliefs) if beliefs is not None else [None] * len(rooms)
        if len(bv) != len(rooms):
            raise ValueError("advises: thread_ids and beliefs differ in length")
        bel = [belief_bytes(tid, room["table"], len(room["names"]), bm, seat_view) for tid, room, bm in zip(thread_ids, rooms, bv)]
        res = run_rollouts([RolloutRequest(room["chunk"], room["slot"], room["key"], room["turn"], seat, c, bl,
                                           neutral_beliefs(room["table"], len(room["names"])))
                            for room, seat, c, bl in zip(rooms, seats, cands, bel)], seat_view, n_rollouts, max_turns, self.seed, compare)
        return [advise_output(room["table"], room["names"], tid, room["turn"], seats[j], room["view"], cands[j], n_rollouts, max_turns,
                              res[j][0], res[j][1], seat_view, res[j][2] if compare else None, bel[j])
                for j, (tid, room) in enumerate(zip(thread_ids, rooms))]

    def hints(self, thread_ids: Optional[Sequence[str]] = None, player_ids: Optional[Sequence[Optional[int]]] = None,
              n_rollouts: int = 4096, max_turns: int = 1024, view: str = "seat") -> List[Dict[str, Any]]:
        """Hints for many (thread, seat) pairs, each as RoomService.hint's: one advise_seats call per chunk touched (POLICY.md §3m).
        thread_ids None: every thread waiting() reports, in the order the threads were created, and each of its pending seats
        ascending - the tick "find who waits, tell each what their choices lead to" in two device calls per chunk.  With
        thread_ids: player_ids[j] (None or absent: thread j's lowest human seat).  No thread changes."""
        check_forecast_args(n_rollouts, max_turns)
        seat_view = check_view(view)
        if thread_ids is None:
            if player_ids is not None:
                raise ValueError("hints: player_ids need thread_ids")
            wait = self.waiting()
            pairs = [(tid, seat) for tid in self._rooms if tid in wait for seat in wait[tid]]
        else:
            pids = list(player_ids) if player_ids is not None else [None] * len(thread_ids)
            if len(pids) != len(thread_ids):
                raise ValueError("hints: thread_ids and player_ids differ in length")
            pairs = [(tid, advise_seat(tid, self._rooms[tid]["human_seats"], pid)) for tid, pid in zip(thread_ids, pids)]
        rooms = [self._rooms[tid] for tid, _ in pairs]
        advs = run_hints([HintRequest(room["chunk"], room["slot"], room["key"], room["turn"], seat,
                                      playout_max_cands(room["table"].pack, len(room["names"])) + 1)
                          for room, (_, seat) in zip(rooms, pairs)], seat_view, n_rollouts, max_turns, self.seed)
        return [hint_output(room["table"], room["names"], tid, room["turn"], seat, room["view"], n_rollouts, max_turns, adv, seat_view)
                for room, (tid, seat), adv in zip(rooms, pairs, advs)]

    def _scan(self, want) -> List[Tuple[str, Any]]:
        """One find_rooms per chunk that holds a thread; (thread_id, hit) of the slots a thread owns - a free slot holds a template
        room or what its last thread left, and is never reported."""
        owner: Dict[int, Tuple[Any, Dict[int, str]]] = {}
        for tid, room in self._rooms.items():
            owner.setdefault(id(room["chunk"]), (room["chunk"], {}))[1][room["slot"]] = tid
        out = []
        for chunk, slots in owner.values():
            hits, _ = chunk.find_rooms(want)
            out.extend((slots[int(h["room"])], h) for h in hits if int(h["room"]) in slots)
        return out

    def waiting(self) -> Dict[str, List[int]]:
        """The threads that wait for a person, and for whom: {thread_id: [seats that could act now]} - from one find_rooms per
        chunk (POLICY.md §3k) instead of a walk over the threads' states."""
        return {tid: pending_seats(h["pending"]) for tid, h in self._scan(("person",))}

    def finished(self) -> List[str]:
        """The threads whose game stands in a terminal phase."""
        return [tid for tid, _ in self._scan(("end",))]

    def close(self, thread_id: Optional[str] = None):
        """Close one thread (its slot goes back to the pool's free list) or, without an id, every thread and every chunk."""
        if thread_id is not None:
            room = self._rooms.pop(thread_id)
            room["pool"].free.append((room["ci"], room["slot"]))
            return
        self._rooms.clear()
        for pool in self._pools.values():
            for chunk in pool.chunks:
                chunk.close()
        self._pools.clear()

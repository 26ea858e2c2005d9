"""RoomService — the single-room drop-in for Python hosts (twin of node/room_service.js).

In the reference one LangGraph thread is one room, and every "Continue" message is one run of the
graph (agent/game_agent_v2.py:1571-1587) that returns the AgentState (v2:97-117) plus an AIMessage
whose tool calls drive the frontend.  `continue_room(thread_id)` is that run without the LLM: an N=1
traced batch advances the room by one turn; the turn comes back as the reference's backend tool
calls (toolcalls.turn_tool_calls, agent/tools/backend_tools.py:10-157) and the phase now showing as
frontend tool calls (ui_script.ui_tool_calls); the log-shaped parts of AgentState the packed state
does not carry — playerActions (bt:285-344), game_notes (bt:163-202), phase_history (v2:1207-1215) —
are folded from those calls exactly as the reference's `_execute_*` functions would.
"""
from __future__ import annotations

import copy
import re
from typing import Any, Dict, List, NamedTuple, Optional, Sequence, Tuple

from . import messages as M
from .stepper import (GE_ERR_ARG, PACK_WEREWOLF, GeError, GameTable, RoomBatch, agent_state_to_view, load_dsl_by_gamename, rollout_to_dict,
                      run_until_bits, run_until_names, slot_values, view_to_agent_state)
from .toolcalls import WW_IS_ALIVE, RoomLog, turn_tool_calls
from .ui_script import ui_tool_calls


def room_index_of(thread_id: str) -> int:
    """Stable 48-bit global room index of a thread id (FNV-1a 64, low 48 bits; same as the JS host):
    the RNG is keyed by it, so a thread replays identically on any host."""
    h = 0xCBF29CE484222325
    for ch in str(thread_id).encode("utf-8"):
        h ^= ch
        h = (h * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h & 0xFFFFFFFFFFFF


def _human_mask(players: Optional[List[Dict[str, Any]]], human_seats, n: int) -> int:
    mask = sum(1 << i for i, p in enumerate(players or []) if p.get("isBot") is False)
    for seat in human_seats or ():
        if not 1 <= int(seat) <= n:
            raise ValueError(f"human seat {seat} is not a player 1..{n}")
        mask |= 1 << (int(seat) - 1)
    return mask


def prepare_adoption(tb: GameTable, state: Dict[str, Any], players, human_seats, turn, visit_actions) -> Dict[str, Any]:
    """agent_state_to_view of an adoption request and what follows from it (both services; nothing is created here)."""
    view, host = agent_state_to_view(tb, state, len(players) if players else None, visit_actions)
    n = int(view["n_players"])
    mask = _human_mask(players, human_seats, n)
    names = [(players[i].get("name") if players else None) or host["names"][str(i + 1)] for i in range(n)]
    return {"view": view, "n": n, "human_mask": mask, "names": names,
            "turn": len(state.get("phase_history") or []) if turn is None else int(turn),
            "human_seats": [i + 1 for i in range(n) if (mask >> i) & 1],
            "host": dict(host, names={str(i + 1): nm for i, nm in enumerate(names)})}


_DEATH_NOTE = re.compile(r"CRITICAL: Player (\d+) \(.*\) eliminated")


def last_turn_deaths(notes: List[str], turn: int) -> List[str]:
    """The players eliminated by `turn`, as its notes report them (the CRITICAL notes after its "[t=<turn>]" phase note):
    what that turn's UI marked dead."""
    at = max((i for i, x in enumerate(notes) if f"PHASE_STATUS: [t={turn}] " in x), default=-1)
    if at < 0:
        return []
    out = []
    for x in notes[at + 1:]:
        if "PHASE_STATUS: " in x:
            break
        m = _DEATH_NOTE.search(x)
        if m:
            out.append(m.group(1))
    return out


def adopted_output(room: Dict[str, Any], turn: int) -> Dict[str, Any]:
    """What adopting a thread returns: its state and the UI of the phase now showing, as the last turn (turn - 1) rendered it."""
    state = room["log"].agent_state(room["view"])
    last = max(turn - 1, 0)
    ui = ui_tool_calls(room["table"].dsl, state, room["table"], turn=last, deaths=last_turn_deaths(room["log"].game_notes, last))
    room["panel"] = M.newest_panel(ui)
    return {"state": state, "toolCalls": [], "uiCalls": ui}


FORECAST_SEED_XOR = 0x9E3779B97F4A7C15     # forecast seed = service seed ^ this: no forecast stream is ever a game stream
FORECAST_MAX_ROLLOUTS = 1 << 16             # replicas of a thread are keyed thread_key << 16 .. + (n_rollouts - 1)


def forecast_key(thread_key: int) -> int:
    """Base key of a thread's forecast replicas: replica r is global room (thread_key << 16) + r (mod 2^64)."""
    return (int(thread_key) << 16) & 0xFFFFFFFFFFFFFFFF


def forecast_seed(seed: int) -> int:
    return (int(seed) ^ FORECAST_SEED_XOR) & 0xFFFFFFFFFFFFFFFF


def playout_mask(n_players: int, human_mask: int, playout_seats) -> int:
    """Bit i = seat i+1 is a playout bot (POLICY.md §3d).  A playout seat must be a bot seat 1..n (ValueError otherwise)."""
    mask = 0
    for seat in playout_seats or ():
        if not 1 <= int(seat) <= n_players:
            raise ValueError(f"playout seat {seat} is not a player 1..{n_players}")
        if (human_mask >> (int(seat) - 1)) & 1:
            raise ValueError(f"playout seat {seat} is a human seat")
        mask |= 1 << (int(seat) - 1)
    return mask


def seats_mask(thread_id: str, n_players: int, seats) -> int:
    """set_human_seats: the seats (player ids 1..n) as the room's seat mask (POLICY.md §3l); ValueError for an id outside 1..n."""
    mask = 0
    for seat in seats or ():
        if isinstance(seat, bool) or int(seat) != seat or not 1 <= int(seat) <= n_players:
            raise ValueError(f"thread {thread_id!r}: seat {seat!r} is not a player 1..{n_players}")
        mask |= 1 << (int(seat) - 1)
    return mask


def check_playout_options(n_rollouts: int, max_turns: int, view: str, halving: bool = False) -> bool:
    """The services' playout-bot options; returns True for the full view."""
    check_forecast_args(n_rollouts, max_turns)
    if not isinstance(halving, bool):
        raise ValueError("playout_halving must be True or False")
    return not check_view(view)


PLAYOUT_CAP = 1 << 26                       # ge_batch_step_rooms_playout: sum of popcount(mask) x max_cands x n_rollouts per call


def playout_max_cands(pack: int, n_players: int) -> int:
    """The most candidates one playout seat can have (the call's cost unit): Werewolf n, Two-Truths max(n, 3)."""
    return n_players if pack == PACK_WEREWOLF else max(n_players, 3)


def check_forecast_args(n_rollouts: int, max_turns: int) -> None:
    if not 1 <= int(n_rollouts) <= FORECAST_MAX_ROLLOUTS:
        raise ValueError(f"n_rollouts must be 1 .. {FORECAST_MAX_ROLLOUTS} (replica keys are thread_key << 16 + r)")
    if not 0 <= int(max_turns) <= 4096:
        raise ValueError("max_turns must be 0 .. 4096")


def forecast_output(table: GameTable, names: List[str], thread_id: str, turn: int, n_rollouts: int, max_turns: int, words) -> Dict[str, Any]:
    """The forecast of one thread from its ge_rollout_stats words: JSON integers only (clients divide by `rollouts`), the same
    bytes as room_service.js / room_pool.js produce."""
    d = rollout_to_dict(words)
    sm = d["summary"]
    out: Dict[str, Any] = {"threadId": thread_id, "turn": int(turn), "rollouts": int(n_rollouts), "maxTurns": int(max_turns),
                           "finished": sm["finished"], "endTurnSum": sm["sum_end_turn"], "ended": sum(sm["end_turn_hist"])}
    if table.pack == PACK_WEREWOLF:
        out["sides"] = {"villagers": sm["village_wins"], "werewolves": sm["wolf_wins"]}
        out["players"] = {str(i + 1): {"name": nm, "alive": d["seat_alive"][i], "wins": d["seat_wins"][i]} for i, nm in enumerate(names)}
    else:
        out["players"] = {str(i + 1): {"name": nm, "scoreSum": d["seat_score"][i], "topScore": d["seat_wins"][i]} for i, nm in enumerate(names)}
    return out


def check_view(view: str) -> bool:
    """advise's `view`: "full" (every playout from the true record) or "seat" (from what the advised seat knows, POLICY.md
    §3c); True for the seat view."""
    if view not in ("full", "seat"):
        raise ValueError('view must be "full" or "seat"')
    return view == "seat"


def check_forecast_seat(thread_id: str, n_players: int, seat: Optional[int]) -> None:
    if seat is not None and not 1 <= int(seat) <= int(n_players):
        raise ValueError(f"thread {thread_id!r}: seat must be 1 .. {n_players}")


BELIEF_SLOTS = 16                                           # GE_BELIEF_SLOTS
BELIEF_NEUTRAL = 16                                         # an unnamed slot: a caller can go below neutral as well as above


def belief_slots(table: GameTable, n_players: int) -> int:
    """The slots a thread's beliefs can name: its seats (Werewolf) or the three statements (Two-Truths)."""
    return int(n_players) if table.pack == PACK_WEREWOLF else 3


def belief_bytes(thread_id: str, table: GameTable, n_players: int, beliefs, seat_view: bool) -> Optional[bytes]:
    """The 16 bytes of POLICY.md §3j from a mapping seat number (Werewolf) / statement number 1-3 (Two-Truths) -> integer
    0..255 (keys may be the decimal strings JSON makes of them); unnamed slots get 16, slots the thread does not have 0.
    None stays None (today's path).  ValueError for a value out of range, a key that is no seat or statement of the thread,
    or beliefs without a seat view - the same bytes as room_service.js's beliefBytes."""
    if beliefs is None:
        return None
    if not seat_view:
        raise ValueError(f"thread {thread_id!r}: beliefs need a seat's view (forecast: seat=..., advise: view=\"seat\")")
    if not isinstance(beliefs, dict):
        raise ValueError(f"thread {thread_id!r}: beliefs must map seat or statement numbers to 0..255")
    slots = belief_slots(table, n_players)
    out = [BELIEF_NEUTRAL] * slots + [0] * (BELIEF_SLOTS - slots)
    for k, v in beliefs.items():
        if isinstance(k, bool) or not (isinstance(k, int) or (isinstance(k, str) and k.isascii() and k.isdigit())) or not 1 <= int(k) <= slots:
            raise ValueError(f"thread {thread_id!r}: beliefs key {k!r} is not 1 .. {slots}")
        if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= 255:
            raise ValueError(f"thread {thread_id!r}: beliefs[{k!r}] must be an integer 0 .. 255")
        out[int(k) - 1] = v
    return bytes(out)


def neutral_beliefs(table: GameTable, n_players: int) -> bytes:
    """Equal weights: the unweighted deal exactly (a thread without beliefs in a call where another has some)."""
    slots = belief_slots(table, n_players)
    return bytes([BELIEF_NEUTRAL] * slots + [0] * (BELIEF_SLOTS - slots))


def seat_forecast_output(table: GameTable, names: List[str], thread_id: str, turn: int, n_rollouts: int, max_turns: int, seat: Optional[int],
                         words, beliefs: Optional[bytes] = None) -> Dict[str, Any]:
    """forecast's JSON; from a seat's view it gains "seat", under beliefs "beliefs" - the 16 bytes used (the default output is
    unchanged)."""
    out = forecast_output(table, names, thread_id, turn, n_rollouts, max_turns, words)
    if seat is not None:
        out["seat"] = int(seat)
    if beliefs is not None:
        out["beliefs"] = list(beliefs)
    return out


def advise_candidates(table: GameTable, view) -> List[int]:
    """The choices a seat may make in the room's current phase, as messages.resolve can read them: Werewolf every seat id
    1..n, Two-Truths [1] in the statements phase and [1, 2, 3] otherwise.  The device decides which are legal."""
    n = int(view["n_players"])
    if table.pack == PACK_WEREWOLF:
        return list(range(1, n + 1))
    pid = int(view["phase_id"])
    act = next((r["act"] for r in table.rows() if r["phase_id"] == pid), 0)
    return [1] if act == M.ACT_TT_STATEMENTS else [1, 2, 3]


def advise_seat(thread_id: str, human_seats: List[int], player_id: Optional[int]) -> int:
    if player_id is not None:
        return int(player_id)
    if not human_seats:
        raise ValueError(f"thread {thread_id!r} has no human seat: name the player to advise")
    return min(human_seats)


class RolloutRequest(NamedTuple):
    """One thread of a forecast or advise call: its batch, slot, thread key and turn; seat: the advised seat, or the seat a
    forecast is seen from (None: the full view); cands: advise's candidates (None: a forecast)."""
    batch: Any
    slot: int
    key: int
    turn: int
    seat: Optional[int] = None
    cands: Optional[List[int]] = None
    beliefs: Optional[bytes] = None                        # the 16 bytes of POLICY.md §3j, or the request has none
    neutral: bytes = bytes(BELIEF_SLOTS)                   # what it gets in a call where another request has beliefs


def run_rollouts(reqs: Sequence[RolloutRequest], seat_view: bool, n_rollouts: int, max_turns: int, seed: int,
                 compare: bool = False) -> List[Tuple[Any, ...]]:
    """The playouts of a forecast or advise call, as (words, status) per request (status None after rollout_rooms).  A forecast
    is one entry, an advise one per candidate then the policy's (no action), all under the thread's forecast key and the forecast
    seed.  One call per batch, in the order the batches first appear, split only where the library's cap on entries x rollouts
    needs it: rollout_rooms for a forecast, rollout_actions for an advise, rollout_seats in the seat view (seat 0 for a thread
    without a seat: its full view).  compare (an advise): the one call is rollout_compare instead (seat 0 entries in the full
    view) - every entry's baseline is its thread's policy entry, the subject the advised seat - and each result is (words, status,
    cmp); a thread's entries stay in one call and a call at or below 65 536 entries.  A call any of whose requests carries
    beliefs is rollout_beliefs instead (with or without the comparison); its other requests get their neutral bytes - equal
    weights, the unweighted deal exactly.  Without beliefs nothing changes."""
    per_call = max(1, (1 << 26) // int(n_rollouts))
    if compare:
        per_call = min(per_call, 65536)
    calls: Dict[int, List[List[int]]] = {}                 # per batch, in first-appearance order: its calls' requests
    n_ent: Dict[int, int] = {}                             # entries in the batch's last call
    for j, r in enumerate(reqs):
        k = 1 if r.cands is None else len(r.cands) + 1
        b = id(r.batch)
        if b not in calls:
            calls[b], n_ent[b] = [[]], 0
        elif n_ent[b] + k > per_call:
            calls[b].append([])
            n_ent[b] = 0
        calls[b][-1].append(j)
        n_ent[b] += k
    seed = forecast_seed(seed)
    out: List[Tuple[Any, Any]] = [(None, None)] * len(reqs)
    for part in (part for parts in calls.values() for part in parts):
        rooms: list = []
        keys: list = []
        turns: list = []
        seats: list = []
        acts: list = []
        base: list = []
        subj: list = []
        bel: list = []
        weighted = any(reqs[j].beliefs is not None for j in part)
        for j in part:
            r = reqs[j]
            k = 1 if r.cands is None else len(r.cands) + 1
            bel += [list(r.neutral if r.beliefs is None else r.beliefs)] * k
            base += [len(rooms) + k - 1] * k
            subj += [r.seat] * k
            rooms += [r.slot] * k
            keys += [forecast_key(r.key)] * k
            turns += [r.turn] * k
            seats += [r.seat or 0] * k
            if r.cands is not None:
                acts += [[(r.seat, c)] for c in r.cands] + [[]]
        batch = reqs[part[0]].batch
        cmp = None
        if weighted:
            res = batch.rollout_beliefs(rooms, keys, turns, seats if seat_view else [0] * len(rooms), acts or None, bel, n_rollouts,
                                        max_turns, seed=seed, **({"baseline": base, "subjects": subj} if compare else {}))
            words, status = res[0], res[1]
            cmp = res[2] if compare else None
        elif compare:
            words, status, cmp = batch.rollout_compare(rooms, keys, turns, seats if seat_view else [0] * len(rooms), acts, base, subj,
                                                       n_rollouts, max_turns, seed=seed)
        elif seat_view:
            words, status = batch.rollout_seats(rooms, keys, turns, seats, acts or None, n_rollouts, max_turns, seed=seed)
        elif acts:
            words, status = batch.rollout_actions(rooms, keys, turns, acts, n_rollouts, max_turns, seed=seed)
        else:
            words, status = batch.rollout_rooms(rooms, keys, turns, n_rollouts, max_turns, seed=seed), None
        at = 0
        for j in part:
            k = 1 if reqs[j].cands is None else len(reqs[j].cands) + 1
            out[j] = (words[at:at + k], None if status is None else status[at:at + k]) + (() if cmp is None else (cmp[at:at + k],))
            at += k
    return out


def advise_output(table: GameTable, names: List[str], thread_id: str, turn: int, seat: int, view, cands: List[int], n_rollouts: int,
                  max_turns: int, words, status, seat_view: bool = False, cmp=None, beliefs: Optional[bytes] = None) -> Dict[str, Any]:
    """advise's JSON from the words and verdicts of an advise's entries (run_rollouts; the same bytes as room_service.js /
    room_pool.js); from the seat's view it gains "view": "seat"; with cmp (the entries' ge_compare_stats words) "compare": true
    and per option "versus": the option against the policy's entry, playout by playout, for the advised seat; under beliefs
    "beliefs": the 16 bytes used."""
    options = []
    for j, c in enumerate(cands):
        if int(status[j]) != 0:
            continue
        label = names[c - 1] if table.pack == PACK_WEREWOLF else str(c)
        options.append({"choice": c, "label": label,
                        "forecast": forecast_output(table, names, thread_id, turn, n_rollouts, max_turns, words[j])})
        if cmp is not None:
            options[-1]["versus"] = dict(zip(("compared", "better", "worse", "gain", "loss", "diffSq"), (int(x) for x in cmp[j])))
    return {"threadId": thread_id, "turn": int(turn), "playerId": int(seat), "phaseId": int(view["phase_id"]),
            "rollouts": int(n_rollouts), "maxTurns": int(max_turns),
            "policy": forecast_output(table, names, thread_id, turn, n_rollouts, max_turns, words[len(cands)]), "options": options,
            **({"view": "seat"} if seat_view else {}), **({"compare": True} if cmp is not None else {}),
            **({"beliefs": list(beliefs)} if beliefs is not None else {})}


ADVISE_CAP = 1 << 26                        # ge_batch_advise_seats: sum of (max_cands + 1) x n_rollouts per call


class HintRequest(NamedTuple):
    """One (thread, seat) of a hint call: its batch, slot, thread key and turn, the advised seat, and the entries the library
    reserves for it (playout_max_cands + 1)."""
    batch: Any
    slot: int
    key: int
    turn: int
    seat: int
    cost: int


def run_hints(reqs: Sequence[HintRequest], seat_view: bool, n_rollouts: int, max_turns: int, seed: int) -> List[Any]:
    """The advice records of a hint call, one per request: RoomBatch.advise_seats (POLICY.md §3m) under the thread's forecast key
    and the forecast seed - advise's keys and seed, so a hint's numbers are those inside advise's option forecasts.  One call per
    batch, in the order the batches first appear, split only where the library's cap on reserved playouts needs it."""
    calls: Dict[int, List[List[int]]] = {}
    cost: Dict[int, int] = {}
    for j, r in enumerate(reqs):
        b = id(r.batch)
        if b not in calls:
            calls[b], cost[b] = [[]], 0
        elif (cost[b] + r.cost) * int(n_rollouts) > ADVISE_CAP:
            calls[b].append([])
            cost[b] = 0
        calls[b][-1].append(j)
        cost[b] += r.cost
    out: List[Any] = [None] * len(reqs)
    for part in (part for parts in calls.values() for part in parts):
        adv = reqs[part[0]].batch.advise_seats([reqs[j].slot for j in part], [forecast_key(reqs[j].key) for j in part],
                                               [reqs[j].turn for j in part], [reqs[j].seat for j in part], n_rollouts, max_turns,
                                               seed=forecast_seed(seed), full_view=not seat_view)
        for k, j in enumerate(part):
            out[j] = adv[k]
    return out


def hint_output(table: GameTable, names: List[str], thread_id: str, turn: int, seat: int, view, n_rollouts: int, max_turns: int, adv,
                seat_view: bool = True) -> Dict[str, Any]:
    """hint's JSON from one advice record (ADVICE_DTYPE; the same bytes as room_service.js / room_pool.js): integers, names and
    labels only.  `best` and `policy` are None when the seat has nothing to do now (then options is [])."""
    ok = int(adv["status"]) == 0
    options = []
    for c in range(1, 13):
        if ok and (int(adv["legal"]) >> (c - 1)) & 1:
            o = adv["option"][c - 1]
            options.append({"choice": c, "label": names[c - 1] if table.pack == PACK_WEREWOLF else str(c), "wins": int(o["wins"]),
                            "score": int(o["score"]), "finished": int(o["finished"])})
    p = adv["policy"]
    return {"threadId": thread_id, "turn": int(turn), "playerId": int(seat), "phaseId": int(view["phase_id"]),
            "rollouts": int(n_rollouts), "maxTurns": int(max_turns), "best": int(adv["best"]) if ok else None,
            "policy": {"finished": int(p["finished"]), "wins": int(p["wins"]), "score": int(p["score"])} if ok else None,
            "options": options, **({"view": "seat"} if seat_view else {})}


RUN_MAX_TURNS = 4096                                        # ge_batch_run_rooms's cap on max_turns


def check_run_args(max_turns: int, until) -> int:
    """run_room's max_turns and until, before anything runs; returns `until` as ge_batch_run_rooms's bit set."""
    if not 1 <= int(max_turns) <= RUN_MAX_TURNS:
        raise ValueError(f"max_turns must be 1 .. {RUN_MAX_TURNS}")
    return run_until_bits(until)


def check_run_thread(thread_id: str, room: Dict[str, Any], playout: bool = False) -> None:
    if room["playout_mask"] and not playout:
        raise ValueError(f"thread {thread_id!r} has playout seats: run_room does not run playout bots, use continue_room "
                         "(or run it with playout=True)")


TIMELINE_MAX_POINTS = 1 << 16                               # ge_batch_run_rooms_forecast: n x (max_turns + 1) per call
TIMELINE_CAP = 1 << 26                                      # ... and n x (max_turns + 1) x n_rollouts


def check_run_forecast(thread_id: str, room: Dict[str, Any], max_turns: int, n_rollouts: int, forecast_max_turns: int,
                       seat: Optional[int], turn: int) -> None:
    """run_room's forecast options for one thread standing at `turn` (POLICY.md §3i), before anything runs."""
    check_forecast_args(n_rollouts, forecast_max_turns)
    check_forecast_seat(thread_id, len(room["names"]), seat)
    if room["playout_mask"]:
        raise ValueError(f"thread {thread_id!r} has playout seats: run_room gives no forecasts of a run with playout bots")
    if (int(max_turns) + 1) * int(n_rollouts) > TIMELINE_CAP:
        raise ValueError(f"(max_turns + 1) x forecast_rollouts must be at most {TIMELINE_CAP}")
    if int(turn) + int(max_turns) + int(forecast_max_turns) > 0xFFFFFFFF:
        raise ValueError(f"thread {thread_id!r}: the turn counter would overflow")


def run_forecast_per_call(max_turns: int, n_rollouts: int) -> int:
    """The most threads one run_rooms_forecast call takes under the library's caps."""
    pts = int(max_turns) + 1
    return max(1, min((1 << 20) // int(max_turns), TIMELINE_MAX_POINTS // pts, TIMELINE_CAP // (pts * int(n_rollouts))))


def run_forecasts(table: GameTable, names: List[str], thread_id: str, turn: int, played: int, n_rollouts: int, max_turns: int,
                  seat: Optional[int], stats) -> List[Dict[str, Any]]:
    """run_room's "forecasts": element p is forecast()'s JSON of the thread as it stood after p of the call's turns."""
    return [seat_forecast_output(table, names, thread_id, int(turn) + p, n_rollouts, max_turns, seat, stats[p]) for p in range(int(played) + 1)]


def run_turn(out: Dict[str, Any]) -> Dict[str, Any]:
    """One turn's output as run_room keeps it: the state of a continue_room output shares the thread's growing log
    (playerActions, phase_history, game_notes), and here later turns are folded before the caller sees the earlier ones - so
    those three are copied.  The copy grows with the log: host work per turn that a continue_room caller does not pay."""
    out["state"] = {**out["state"], **{k: copy.deepcopy(out["state"][k]) for k in ("playerActions", "phase_history", "game_notes")}}
    return out


def run_output(turns: List[Dict[str, Any]], stopped: int, forecasts: Optional[List[Dict[str, Any]]] = None) -> Dict[str, Any]:
    return {"turns": turns, "played": len(turns), "stopped": run_until_names(stopped), **({} if forecasts is None else {"forecasts": forecasts})}


class RoomService:
    def __init__(self, games_dir: str = "games", seed: int = 0, device: int = 0, playout_rollouts: int = 256,
                 playout_max_turns: int = 256, playout_view: str = "seat", playout_halving: bool = False):
        """playout_*: how the playout bots of threads created with playout_seats choose (POLICY.md §3d): n_rollouts and
        max_turns of each candidate's playouts, and "seat" (from what the bot knows) or "full" (from the true record - a
        cheating bot in a game with people).  playout_halving: the bots spend each decision's playouts by sequential halving
        (POLICY.md §3h): 1.3 - 2.5 x fewer playouts, but more launches per turn, and slower at every shape measured on an MI355X (x 0.38 .. 0.71 of the unflagged call's speed): DESIGN.md §4; off by default;
        a bot's candidate values are then advise's option forecasts for the finalists only."""
        self.playout_full = check_playout_options(playout_rollouts, playout_max_turns, playout_view, playout_halving)
        self.playout_halving = playout_halving
        self._halving_kw = {"halving": True} if playout_halving else {}   # (off: no keyword, so a stand-in batch written before the option existed still serves)
        self.playout_rollouts, self.playout_max_turns = int(playout_rollouts), int(playout_max_turns)
        self.games_dir, self.seed, self.device = games_dir, seed, device
        self._tables: Dict[str, GameTable] = {}
        self._rooms: Dict[str, Dict[str, Any]] = {}

    def table(self, game_name: str, dsl: Optional[dict] = None) -> GameTable:
        if game_name not in self._tables:
            self._tables[game_name] = GameTable(dsl if dsl else load_dsl_by_gamename(game_name, self.games_dir))
        return self._tables[game_name]

    def create_room(self, thread_id: str, game_name: str, players: List[Dict[str, Any]], dsl: Optional[dict] = None,
                    room_index: Optional[int] = None, playout_seats=()) -> Dict[str, Any]:
        """players: roomSession.players as the lobby builds it; `isBot: False` marks a human seat, which
        the bot policy never acts for (bot_behavior_system_prompt.txt:3) — use human_action for it.
        room_index: the global room index the RNG is keyed by (default: derived from the thread id).
        playout_seats: bot seats that choose each action by playouts (POLICY.md §3d; ValueError for a human seat or an id
        outside 1..n, before anything is created)."""
        tb = self.table(game_name, dsl)
        human_mask = sum(1 << i for i, p in enumerate(players) if p.get("isBot") is False)
        pmask = playout_mask(len(players), human_mask, playout_seats)
        key = room_index_of(thread_id) if room_index is None else int(room_index)
        batch = self._new_batch(tb, len(players), human_mask, key)
        if thread_id in self._rooms:
            self.close(thread_id)
        names = [p.get("name") or f"Player {i + 1}" for i, p in enumerate(players)]
        room = {"batch": batch, "key": key, "table": tb, "gameName": game_name, "names": names, "panel": None,
                "human_seats": [i + 1 for i in range(len(players)) if (human_mask >> i) & 1], "playout_mask": pmask,
                "view": batch.read_rooms(0, 1)[0], "log": RoomLog(tb, names, game_name)}
        self._rooms[thread_id] = room
        return self._agent_state(room)

    def adopt_room(self, thread_id: str, game_name: str, state: Dict[str, Any], players: Optional[List[Dict[str, Any]]] = None,
                   human_seats=(), dsl: Optional[dict] = None, room_index: Optional[int] = None, turn: Optional[int] = None,
                   visit_actions: Optional[Dict[Any, int]] = None, playout_seats=()) -> Dict[str, Any]:
        """Take over a thread that is already mid-game: `state` is its AgentState (current_phase_id, player_states, playerActions,
        phase_history, game_notes - what update_complete_player_states replaces wholesale in the reference).  The room continues
        from it exactly as the thread would have gone on.  players (optional, roomSession.players): `isBot: False` marks a human
        seat, as does human_seats (player ids); the names default to the state's.  turn: the thread's next turn (default
        len(phase_history), one entry per run); visit_actions={player_id: choice}: a human seat's action already logged in this
        visit (see stepper.agent_state_to_view).  Returns {"state", "toolCalls": [], "uiCalls"}: the UI of the phase now showing,
        rendered for the last turn, so that a person's next vote resolves against the panel the thread showed.
        A state that does not fit raises ValueError before anything is created, as do playout_seats (see create_room) that
        are not bot seats."""
        tb = self.table(game_name, dsl)
        a = prepare_adoption(tb, state, players, human_seats, turn, visit_actions)
        pmask = playout_mask(a["n"], a["human_mask"], playout_seats)
        key = room_index_of(thread_id) if room_index is None else int(room_index)
        batch = self._new_batch(tb, a["n"], a["human_mask"], key)
        try:
            batch.write_rooms_at([0], [a["view"]])
            batch.set_turn(a["turn"])
            view = batch.read_rooms(0, 1)[0]
        except BaseException:
            batch.close()
            raise
        if thread_id in self._rooms:                      # only now: a refused state leaves an existing thread of this id alone
            self.close(thread_id)
        room = {"batch": batch, "key": key, "table": tb, "gameName": game_name, "names": a["names"], "panel": None,
                "human_seats": a["human_seats"], "playout_mask": pmask, "view": view, "log": RoomLog(tb, a["names"], game_name)}
        room["log"].adopt(state, a["host"])
        self._rooms[thread_id] = room
        return adopted_output(room, a["turn"])

    def _new_batch(self, tb: GameTable, n_players: int, human_mask: int, first_room: int) -> RoomBatch:
        """The room's N=1 traced batch on the device (there is no other stepper: without the HIP library this raises)."""
        return RoomBatch([(tb, n_players, 1, human_mask)], seed=self.seed, first_room=first_room,
                         device=self.device, max_fuse=1, trace=True)

    def _agent_state(self, room: Dict[str, Any]) -> Dict[str, Any]:
        return room["log"].agent_state(room["view"])

    def human_action(self, thread_id: str, player_id: int, choice: int) -> Dict[str, Any]:
        """A human's vote / choice (logged by process_human_action_if_needed, agent/tools/utils.py:310-358)."""
        room = self._rooms[thread_id]
        room["batch"].inject_action(0, player_id, choice)
        room["view"] = room["batch"].read_rooms(0, 1)[0]
        return self._agent_state(room)

    def set_human_seats(self, thread_id: str, seats) -> List[int]:
        """A seat changes hands mid-game (POLICY.md §3l): from the next turn on exactly `seats` (player ids) are played by people,
        every other seat by the policy - a person who leaves, a person who takes over a bot's seat.  The thread's human_seats
        (what handle_message resolves against and advise defaults to) follow, and a seat given to a person leaves the thread's
        playout seats.  ValueError for an unknown thread or a seat outside 1..n, before anything changes.  Returns the seats."""
        room = self._rooms.get(thread_id)
        if room is None:
            raise ValueError(f"unknown thread {thread_id!r}")
        mask = seats_mask(thread_id, int(room["view"]["n_players"]), seats)
        room["batch"].set_seats([0], [mask])
        room["human_seats"] = [i + 1 for i in range(int(room["view"]["n_players"])) if (mask >> i) & 1]
        room["playout_mask"] &= ~mask
        return list(room["human_seats"])

    def continue_room(self, thread_id: str, items: Optional[List[Dict[str, Any]]] = None) -> Dict[str, Any]:
        """One turn (one graph run): {"state": AgentState, "toolCalls": [...], "uiCalls": [...]}.
        items: the frontend's canvas items (AgentState.items, [{id, type, ...}]) when the caller has them:
        clearCanvas then names the ids to keep (exemptList)."""
        return self._turn(self._rooms[thread_id], items)

    def handle_message(self, thread_id: str, text: str, items: Optional[List[Dict[str, Any]]] = None) -> Dict[str, Any]:
        """The drop-in's message-level entry: what the reference's graph does with ONE message of the browser
        (src/app/page.tsx:183-259 -> agent/game_agent_v2.py:198-349, agent/tools/utils.py:310-358; POLICY.md 3b).
          chat ("... in game chat: ..." / "... to Bot k: ...")  -> ChatBotNode: no turn, no state change;
          control ("Start game.", "Continue")                    -> one turn;
          anything else -> logged verbatim under Player 1 (first 200 characters, phase 0's name - the reference's own quirk),
                           read as a seat's action where it is one (a vote on the newest panel, an input for the
                           statements phase: ge_batch_inject_action), then one turn.
        Returns {"state", "toolCalls", "uiCalls", "played", "kind"}; an action message that is no valid game action is still
        logged and still plays the turn, as in the reference."""
        room = self._rooms[thread_id]
        kind = M.classify(text)
        if kind == M.CHAT:
            return {"state": self._agent_state(room), "toolCalls": [], "uiCalls": [], "played": False, "kind": kind}
        if kind == M.ACTION:
            room["log"].person_message(text)
            view, tb = room["view"], room["table"]
            n = int(view["n_players"])
            pid = int(view["phase_id"])
            act = next((r["act"] for r in tb.rows() if r["phase_id"] == pid), 0)
            alive = [bool(slot_values(tb, view, i)[WW_IS_ALIVE]) for i in range(n)] if tb.pack == PACK_WEREWOLF else [True] * n
            for seat, choice in M.resolve(text, room["panel"], act, tb.pack, room["names"], alive, room["human_seats"]):
                try:
                    room["batch"].inject_action(0, seat, choice)
                    break
                except GeError as e:                     # not a living pending target of this phase: logged, no game effect
                    if e.status != GE_ERR_ARG:
                        raise
        out = self._turn(room, items)
        out.update(played=True, kind=kind)
        return out

    def _turn(self, room: Dict[str, Any], items: Optional[List[Dict[str, Any]]] = None) -> Dict[str, Any]:
        # `before` is the view BEFORE any injected action of this message: the person's record writes (night target, vote
        # choice, ...) then show up among the turn's update_player_state calls, where the reference's Referee issues them
        batch, before = room["batch"], room["view"]
        if room["playout_mask"]:                            # playout bots: advise's keys and seed, so a bot's values are its advice
            turn = batch.turn
            ev, _ = batch.step_rooms_playout([0], [room["key"]], [turn], [room["playout_mask"]], [forecast_key(room["key"])],
                                             self.playout_rollouts, self.playout_max_turns, seed=forecast_seed(self.seed),
                                             full_view=self.playout_full, **self._halving_kw)
            batch.set_turn(turn + 1)
            event = ev[0]
        else:
            batch.step(1)
            event = batch.read_events(0, 1)[0][0]
        return self._finish(room, batch.read_rooms(0, 1)[0], event, items)

    def _finish(self, room: Dict[str, Any], after, event, items) -> Dict[str, Any]:
        """Fold one played turn - its event and the view after it - into the thread: the turn's tool calls, log, state and UI."""
        before = room["view"]
        calls = turn_tool_calls(room["table"], before, after, event)
        room["log"].fold(calls, after)                      # playerActions / game_notes / phase_history, as bt:163-202, 285-344 would
        room["view"] = after
        state = self._agent_state(room)
        deaths = [c["args"]["player_id"] for c in calls if c["name"] == "update_player_state"
                  and c["args"]["state_name"] == "is_alive" and c["args"]["state_value"] is False]
        ui = ui_tool_calls(room["table"].dsl, state, room["table"], turn=int(event["turn"]), deaths=deaths, items=items)
        room["panel"] = M.newest_panel(ui)                # what a person's next vote message can answer
        return {"state": state, "toolCalls": calls, "uiCalls": ui}

    def run_room(self, thread_id: str, max_turns: int = 64, until=("person", "end"),
                 items: Optional[List[Dict[str, Any]]] = None, playout: bool = False, forecast: bool = False, forecast_rollouts: int = 4096,
                 forecast_max_turns: int = 1024, forecast_seat: Optional[int] = None) -> Dict[str, Any]:
        """Play the thread on until a person is needed: one RoomBatch.run_rooms call (POLICY.md §3f) instead of a continue_room
        per turn.  until: "person" (a human seat of the thread has an action to give), "end" (the game is over), "phase" (the
        turn moved the phase); the first turn is always played, at most max_turns are.  Returns {"turns": [{state, toolCalls,
        uiCalls}, ...], "played": p, "stopped": [...]}: element t is exactly what continue_room would have returned for that
        turn (items goes to every turn's UI builder as given), "stopped" names the conditions that held after the last turn
        ([]: the limit), and the thread's turn and panel end where p calls of continue_room would have left them.  A thread
        with playout seats is refused (ValueError) before anything runs, unless playout=True: then it is run by one
        RoomBatch.run_rooms_playout call (POLICY.md §3g) with the keys, seed and options continue_room gives its playout bots.
        Every turn's state carries its own copy of the thread's log (run_turn): host work that grows with the log, per turn.
        forecast=True: a win-odds timeline of the run (POLICY.md §3i), from one RoomBatch.run_rooms_forecast call instead: the
        output gains "forecasts", a list of played + 1 objects - element p is exactly what forecast(thread_id, forecast_rollouts,
        forecast_max_turns, forecast_seat) would have returned after p of the call's turns (element 0: before the call), every
        point under the same keys and seed, so the difference of two neighbours is that turn's effect on the odds.  The forecast
        options are checked as forecast checks them, before anything runs; a thread with playout seats is refused (ValueError)."""
        room = self._rooms[thread_id]
        bits = check_run_args(max_turns, until)
        check_run_thread(thread_id, room, playout)
        batch, turn = room["batch"], room["batch"].turn
        if forecast:
            check_run_forecast(thread_id, room, max_turns, forecast_rollouts, forecast_max_turns, forecast_seat, turn)
            played, stopped, events, views, stats = batch.run_rooms_forecast(
                [0], [room["key"]], [turn], [forecast_key(room["key"])], forecast_rollouts, forecast_max_turns, seats=[forecast_seat or 0],
                seed=forecast_seed(self.seed), max_turns=max_turns, until=bits)
            batch.set_turn(turn + int(played[0]))
            turns = [run_turn(self._finish(room, views[0, t], events[0, t], items)) for t in range(int(played[0]))]
            return run_output(turns, int(stopped[0]), run_forecasts(room["table"], room["names"], thread_id, turn, int(played[0]), forecast_rollouts,
                                                                    forecast_max_turns, forecast_seat, stats[0]))
        if room["playout_mask"]:
            played, stopped, events, views, _ = batch.run_rooms_playout(
                [0], [room["key"]], [turn], [room["playout_mask"]], [forecast_key(room["key"])], self.playout_rollouts, self.playout_max_turns,
                seed=forecast_seed(self.seed), full_view=self.playout_full, max_turns=max_turns, until=bits, **self._halving_kw)
        else:
            played, stopped, events, views = batch.run_rooms([0], [room["key"]], [turn], max_turns, bits)
        batch.set_turn(turn + int(played[0]))
        return run_output([run_turn(self._finish(room, views[0, t], events[0, t], items)) for t in range(int(played[0]))], int(stopped[0]))

    def forecast(self, thread_id: str, n_rollouts: int = 4096, max_turns: int = 1024, seat: Optional[int] = None,
                 beliefs: Optional[Dict[Any, int]] = None) -> Dict[str, Any]:
        """How the thread ends from where it stands: n_rollouts playouts of its room (RoomBatch.rollout_rooms), each played for
        up to max_turns turns from the thread's next turn, every seat - human seats too - played by the policy.  Replica r is
        global room (thread_key << 16) + r, so n_rollouts <= 65 536 (ValueError above), under seed (service seed ^
        0x9E3779B97F4A7C15): no forecast stream is a game stream, and two forecasts at the same turn are identical.  The thread
        is not changed.  Returns JSON integers: threadId, turn, rollouts, maxTurns, finished, endTurnSum, ended, and per seat
        (Werewolf: sides {villagers, werewolves}, players {"1": {name, alive, wins}}; Two-Truths: players {"1": {name,
        scoreSum, topScore}}); divide by rollouts for odds.  seat (1 .. n): the playouts start from what that seat knows
        (RoomBatch.rollout_seats, POLICY.md §3c: what it cannot see is dealt again in every replica), and the JSON gains
        "seat" - the form to show a player; the default is the full view.  beliefs (with seat): what that seat suspects, a
        mapping seat number (Werewolf) or statement number 1-3 (Two-Truths) -> 0..255, unnamed ones 16; the re-deal is weighted
        by it (RoomBatch.rollout_beliefs, POLICY.md §3j) and the JSON gains "beliefs", the 16 bytes used.  ValueError, before
        anything runs, for a value out of range, a key the thread does not have, or beliefs without a seat."""
        check_forecast_args(n_rollouts, max_turns)
        room = self._rooms[thread_id]
        check_forecast_seat(thread_id, len(room["names"]), seat)
        bel = belief_bytes(thread_id, room["table"], len(room["names"]), beliefs, seat is not None)
        turn = room["batch"].turn
        (words, _), = run_rollouts([RolloutRequest(room["batch"], 0, room["key"], turn, seat, None, bel)], seat is not None, n_rollouts,
                                   max_turns, self.seed)
        return seat_forecast_output(room["table"], room["names"], thread_id, turn, n_rollouts, max_turns, seat, words[0], bel)

    def advise(self, thread_id: str, player_id: Optional[int] = None, n_rollouts: int = 4096, max_turns: int = 1024,
               view: str = "full", compare: bool = False, beliefs: Optional[Dict[Any, int]] = None) -> Dict[str, Any]:
        """What each choice the seat can make now leads to: for every candidate (advise_candidates) the forecast of the thread
        given that the seat logs it before the next turn, and the forecast with the policy's own choice ("policy", equal to
        forecast(thread_id)).  One rollout_actions call; every entry uses forecast's keys and seed, so replica r of every option
        draws the same stream.  player_id defaults to the lowest human seat (ValueError if there is none).  Returns JSON
        integers, names and labels: threadId, turn, playerId, phaseId, rollouts, maxTurns, policy, options [{choice, label,
        forecast}] for the accepted candidates in ascending order ([] when the seat has nothing to do now).  The thread is not
        changed.  view "seat": every playout starts from what the advised seat knows (RoomBatch.rollout_seats, POLICY.md §3c)
        - the form to show that player - and the JSON gains "view": "seat"; "full" (the default) plays from the true record and
        is for spectators and debugging.  compare: the one call is rollout_compare; the JSON gains "compare": true and per option
        "versus" {compared, better, worse, gain, loss, diffSq}: the option against the policy's entry, playout by playout, for
        the advised seat (INTEGRATION.md "Is this choice really better?"); everything else is byte for byte the same.
        beliefs (view "seat" only): what the advised seat suspects, as forecast's; every entry of the call is dealt under it
        (INTEGRATION.md "Advising a seat from what it suspects") and the JSON gains "beliefs"."""
        check_forecast_args(n_rollouts, max_turns)
        seat_view = check_view(view)
        room = self._rooms[thread_id]
        seat = advise_seat(thread_id, room["human_seats"], player_id)
        bel = belief_bytes(thread_id, room["table"], len(room["names"]), beliefs, seat_view)
        rv, turn = room["view"], room["batch"].turn
        cands = advise_candidates(room["table"], rv)
        res, = run_rollouts([RolloutRequest(room["batch"], 0, room["key"], turn, seat, cands, bel)], seat_view, n_rollouts, max_turns,
                            self.seed, compare)
        return advise_output(room["table"], room["names"], thread_id, turn, seat, rv, cands, n_rollouts, max_turns, res[0], res[1],
                             seat_view, res[2] if compare else None, bel)

    def hint(self, thread_id: str, player_id: Optional[int] = None, n_rollouts: int = 4096, max_turns: int = 1024,
             view: str = "seat") -> Dict[str, Any]:
        """advise in 224 bytes: which choices the seat can make now, what each leads to for that seat, and the best of them - found,
        played and ranked on the device (RoomBatch.advise_seats, POLICY.md §3m), under advise's keys and seed, so every number is
        the advised seat's own inside advise(..., view=...)'s option forecasts (wins = players[seat].wins or topScore, score =
        scoreSum, finished).  player_id defaults to the lowest human seat.  Returns JSON integers and labels: threadId, turn,
        playerId, phaseId, rollouts, maxTurns, best (the choice with the most wins - Two-Truths: the highest score -, the lowest
        on a tie), policy {finished, wins, score} (the policy plays the seat), options [{choice, label, wins, score, finished}]
        ascending, and "view": "seat" in the default view ("full" plays from the true record: spectators and debugging).  best
        and policy are None and options [] when the seat has nothing to do now.  The thread is not changed.  advise stays the
        call for the full per-option forecast."""
        check_forecast_args(n_rollouts, max_turns)
        seat_view = check_view(view)
        room = self._rooms[thread_id]
        seat = advise_seat(thread_id, room["human_seats"], player_id)
        turn = room["batch"].turn
        cost = playout_max_cands(room["table"].pack, len(room["names"])) + 1
        adv, = run_hints([HintRequest(room["batch"], 0, room["key"], turn, seat, cost)], seat_view, n_rollouts, max_turns, self.seed)
        return hint_output(room["table"], room["names"], thread_id, turn, seat, room["view"], n_rollouts, max_turns, adv, seat_view)

    def close(self, thread_id: Optional[str] = None):
        for tid in ([thread_id] if thread_id else list(self._rooms)):
            self._rooms.pop(tid)["batch"].close()

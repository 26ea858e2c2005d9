'use strict';
/**
 * RoomService — the single-room drop-in: one LangGraph thread (= one room) served by an N=1
 * batch through the same C ABI as the big batches.
 *
 * In the reference, src/app/api/copilotkit/route.ts:22-47 binds each request's X-Thread-ID to a
 * LangGraphAgent and every "Continue" / "Start game." message (src/app/page.tsx:2774, 2962) is one
 * run of the Python graph.  `continueRoom(threadId)` is that run: it advances the room by one turn
 * and returns what the graph returns to CopilotKit — the AgentState (agent/game_agent_v2.py:97-117)
 * plus the AIMessage's tool calls: here the backend calls that describe the turn
 * (turnToolCalls) and the frontend calls of the phase now showing (uiToolCalls).
 * A handler that wants this instead of the LLM graph calls it in place of constructing the
 * LangGraphAgent (route.ts:30-39); `serve()` exposes the same over plain HTTP for a quick try.
 */
const http = require('http');
const { GameTable, RoomBatch, RoomLog, agentStateToView, loadDslByGamename, turnToolCalls, uiToolCalls, runUntilBits, runUntilNames } = require('./index.js');
const M = require('./messages.js');

/** stable 48-bit room index from a thread id (the RNG is keyed by it) */
function roomIndexOf(threadId) {
  let h = 0xcbf29ce484222325n;
  for (const ch of Buffer.from(String(threadId), 'utf8')) { h ^= BigInt(ch); h = (h * 0x100000001b3n) & 0xffffffffffffffffn; }
  return h & 0xffffffffffffn;
}

/** humanSeats / players' isBot === false -> the segment's human mask */
function humanMaskOf(players, humanSeats, n) {
  let mask = (players || []).reduce((m, p, i) => (p.isBot === false ? m | (1 << i) : m), 0);
  for (const seat of humanSeats || []) {
    if (!(Number.isInteger(seat) && seat >= 1 && seat <= n)) throw new RangeError(`human seat ${seat} is not a player 1..${n}`);
    mask |= 1 << (seat - 1);
  }
  return mask;
}

/** The players eliminated by the turn that the last "[t=<turn>]" phase note reports (its CRITICAL notes): what that turn's UI marked. */
function lastTurnDeaths(notes, turn) {
  let at = -1;
  notes.forEach((x, i) => { if (x.includes(`PHASE_STATUS: [t=${turn}] `)) at = i; });
  if (at < 0) return [];
  const out = [];
  for (let i = at + 1; i < notes.length && !notes[i].includes('PHASE_STATUS: '); i++) {
    const m = /CRITICAL: Player (\d+) \(.*\) eliminated/.exec(notes[i]);
    if (m) out.push(m[1]);
  }
  return out;
}

/** What adopting a thread returns: its state and the UI of the phase now showing, as its last turn (turn - 1) rendered it. */
function adoptedOutput(room, turn) {
  const state = room.log.agentState(room.state);
  const last = Math.max(turn - 1, 0);
  const uiCalls = uiToolCalls(room.table.dsl, state, { table: room.table, turn: last, deaths: lastTurnDeaths(room.log.gameNotes, last) });
  room.panel = M.newestPanel(uiCalls);
  return { state, toolCalls: [], uiCalls };
}

/** agentStateToView of an adoption request and what follows from it (both services) */
function prepareAdoption(table, { state, players, humanSeats, turn, visitActions }) {
  const { view, hostSide } = agentStateToView(table, state, { nPlayers: players ? players.length : undefined, visitActions });
  const n = new Uint8Array(view)[17];
  const humanMask = humanMaskOf(players, humanSeats, n);
  const t = turn === undefined || turn === null ? (state.phase_history || []).length : Number(turn);
  const names = Array.from({ length: n }, (_, i) => (players && players[i] && players[i].name) || hostSide.names[String(i + 1)]);
  const seats = Array.from({ length: n }, (_, i) => i + 1).filter((i) => (humanMask >> (i - 1)) & 1);
  return { view, hostSide, n, humanMask, turn: t, names, humanSeats: seats };
}

const FORECAST_SEED_XOR = 0x9e3779b97f4a7c15n;   // forecast seed = service seed ^ this: no forecast stream is a game stream
const FORECAST_MAX_ROLLOUTS = 65536;             // replicas of a thread are keyed threadKey << 16 .. + (nRollouts - 1)
const forecastKey = (threadKey) => BigInt.asUintN(64, BigInt(threadKey) << 16n);
const forecastSeed = (seed) => BigInt.asUintN(64, BigInt(seed) ^ FORECAST_SEED_XOR);
function checkForecastArgs(nRollouts, maxTurns) {
  if (!(Number.isInteger(nRollouts) && nRollouts >= 1 && nRollouts <= FORECAST_MAX_ROLLOUTS))
    throw new RangeError(`nRollouts must be 1 .. ${FORECAST_MAX_ROLLOUTS} (replica keys are threadKey << 16 + r)`);
  if (!(Number.isInteger(maxTurns) && maxTurns >= 0 && maxTurns <= 4096)) throw new RangeError('maxTurns must be 0 .. 4096');
}
/** The forecast of one thread from its 77 ge_rollout_stats words (w[off ..]): JSON integers only, the bytes the Python hosts print. */
function forecastOutput(table, names, threadId, turn, nRollouts, maxTurns, w, off = 0) {
  const at = (i) => Number(w[off + i]);
  let ended = 0;
  for (let i = 6; i < 22; i++) ended += at(i);
  const out = { threadId, turn: Number(turn), rollouts: nRollouts, maxTurns, finished: at(1), endTurnSum: at(5), ended };
  const players = {};
  if (table.info.pack === 1) {
    out.sides = { villagers: at(2), werewolves: at(3) };
    names.forEach((name, i) => { players[String(i + 1)] = { name, alive: at(41 + i), wins: at(53 + i) }; });
  } else {
    names.forEach((name, i) => { players[String(i + 1)] = { name, scoreSum: at(65 + i), topScore: at(53 + i) }; });
  }
  out.players = players;
  return out;
}

/** forecast's JSON; from a seat's view it gains "seat", under beliefs "beliefs" - the 16 bytes used (twin of room_service.py
 * seat_forecast_output). */
function seatForecastOutput(table, names, threadId, turn, nRollouts, maxTurns, seat, w, off = 0, beliefs = null) {
  const out = forecastOutput(table, names, threadId, turn, nRollouts, maxTurns, w, off);
  if (seat !== undefined && seat !== null) out.seat = Number(seat);
  if (beliefs) out.beliefs = Array.from(beliefs);
  return out;
}
const BELIEF_SLOTS = 16, BELIEF_NEUTRAL = 16;        // GE_BELIEF_SLOTS; an unnamed slot: a caller can go below neutral as well as above
/** The slots a thread's beliefs can name: its seats (Werewolf, pack 1) or the three statements (Two-Truths). */
const beliefSlots = (pack, nPlayers) => (pack === 1 ? nPlayers : 3);
/** Equal weights: the unweighted deal exactly (a thread without beliefs in a call where another has some). */
function neutralBeliefs(pack, nPlayers) {
  const out = new Array(BELIEF_SLOTS).fill(0);
  return out.fill(BELIEF_NEUTRAL, 0, beliefSlots(pack, nPlayers));
}
/** The 16 bytes of POLICY.md §3j from an object seat number (Werewolf) / statement number 1-3 (Two-Truths) -> integer 0..255; unnamed
 * slots get 16, slots the thread does not have 0.  undefined / null stays null (today's path).  RangeError for a value out of range,
 * a key that is no seat or statement of the thread, or beliefs without a seat view (twin of room_service.py belief_bytes). */
function beliefBytes(threadId, pack, nPlayers, beliefs, seatView) {
  if (beliefs === undefined || beliefs === null) return null;
  if (!seatView) throw new RangeError(`thread ${threadId}: beliefs need a seat's view (forecast: seat, advise: view "seat")`);
  if (typeof beliefs !== 'object' || Array.isArray(beliefs)) throw new RangeError(`thread ${threadId}: beliefs must map seat or statement numbers to 0..255`);
  const slots = beliefSlots(pack, nPlayers);
  const out = neutralBeliefs(pack, nPlayers);
  const entries = beliefs instanceof Map ? Array.from(beliefs.entries()) : Object.entries(beliefs);
  for (const [k, v] of entries) {
    const key = typeof k === 'number' ? k : /^[0-9]+$/.test(String(k)) ? Number(k) : NaN;
    if (!(Number.isInteger(key) && key >= 1 && key <= slots)) throw new RangeError(`thread ${threadId}: beliefs key ${k} is not 1 .. ${slots}`);
    if (!(typeof v === 'number' && Number.isInteger(v) && v >= 0 && v <= 255)) throw new RangeError(`thread ${threadId}: beliefs[${k}] must be an integer 0 .. 255`);
    out[key - 1] = v;
  }
  return out;
}
function checkForecastSeat(threadId, n, seat) {
  if (seat !== undefined && seat !== null && !(Number.isInteger(seat) && seat >= 1 && seat <= n))
    throw new RangeError(`thread ${threadId}: seat must be 1 .. ${n}`);
}
/** bit i = seat i+1 is a playout bot (POLICY.md §3d); a playout seat must be a bot seat 1..n (RangeError otherwise) */
function playoutMaskOf(n, humanMask, playoutSeats) {
  let mask = 0;
  for (const seat of playoutSeats || []) {
    if (!(Number.isInteger(seat) && seat >= 1 && seat <= n)) throw new RangeError(`playout seat ${seat} is not a player 1..${n}`);
    if ((humanMask >> (seat - 1)) & 1) throw new RangeError(`playout seat ${seat} is a human seat`);
    mask |= 1 << (seat - 1);
  }
  return mask;
}
/** the services' playout-bot options (twin of room_service.py check_playout_options); returns true for the full view */
function checkPlayoutOptions(nRollouts, maxTurns, view, halving = false) {
  checkForecastArgs(nRollouts, maxTurns);
  if (typeof halving !== 'boolean') throw new RangeError('playoutHalving must be true or false');
  if (view !== 'full' && view !== 'seat') throw new RangeError('playoutView must be "full" or "seat"');
  return view === 'full';
}
const PLAYOUT_CAP = 1 << 26;                     // stepRoomsPlayout: sum of popcount(mask) x maxCands x nRollouts per call
/** the most candidates one playout seat can have (the call's cost unit): Werewolf n, Two-Truths max(n, 3) */
const playoutMaxCands = (pack, n) => (pack === 1 ? n : Math.max(n, 3));
function checkView(view) {
  if (view !== undefined && view !== 'full' && view !== 'seat') throw new RangeError('view must be "full" or "seat"');
  return view === 'seat';
}

/** The choices a seat may make in the room's current phase, as messages.resolve can read them (twin of room_service.py
 * advise_candidates): Werewolf every seat id 1..n, Two-Truths [1] in the statements phase and [1, 2, 3] otherwise. */
function adviseCandidates(table, st) {
  const n = st.slots.length;
  if (st.pack === 1) return Array.from({ length: n }, (_, i) => i + 1);
  const phase = table.info.phases.find((x) => x.id === st.current_phase_id);
  return phase && phase.act === 5 ? [1] : [1, 2, 3];             // 5: GE_ACT_TT_STATEMENTS
}
/** setHumanSeats: the seats (player ids 1..n) as the room's seat mask (POLICY.md §3l); RangeError for an id outside 1..n */
function seatsMask(threadId, n, seats) {
  let mask = 0;
  for (const seat of seats || []) {
    if (!Number.isInteger(seat) || seat < 1 || seat > n) throw new RangeError(`thread ${threadId}: seat ${seat} is not a player 1..${n}`);
    mask |= 1 << (seat - 1);
  }
  return mask;
}

function adviseSeat(threadId, humanSeats, playerId) {
  if (playerId !== undefined && playerId !== null) return Number(playerId);
  if (!humanSeats.length) throw new RangeError(`thread ${threadId} has no human seat: name the player to advise`);
  return Math.min(...humanSeats);
}
/** The playouts of a forecast or advise call (twin of room_service.py run_rollouts): reqs [{ batch, slot, key, turn, seat, cands }]
 * - seat: the advised seat, or the seat a forecast is seen from (undefined / null: the full view); cands: advise's candidates
 * (undefined: a forecast).  A forecast is one entry, an advise one per candidate then the policy's (no action), all under the
 * thread's forecast key and the forecast seed.  One call per batch, in the order the batches first appear, split only where the
 * library's cap on entries x rollouts needs it: rolloutRooms for a forecast, rolloutActions for an advise, rolloutSeats in the
 * seat view (seat 0 for a thread without a seat: its full view).  Returns per request { words, status } (status null after
 * rolloutRooms), views into the call's results.  compare (an advise): the one call is rolloutCompare instead (seat 0 entries in
 * the full view) - every entry's baseline is its thread's policy entry, the subject the advised seat - and each result gains
 * cmp; a thread's entries stay in one call and a call at or below 65 536 entries.  A call any of whose requests carries beliefs
 * (16 bytes, POLICY.md §3j) is rolloutBeliefs instead, with or without the comparison; its other requests get their `neutral`
 * bytes - equal weights, the unweighted deal exactly.  Without beliefs nothing changes. */
function runRollouts(reqs, seatView, nRollouts, maxTurns, seed, compare = false) {
  const byBatch = new Map();
  reqs.forEach((r, j) => {
    if (!byBatch.has(r.batch)) byBatch.set(r.batch, []);
    byBatch.get(r.batch).push(j);
  });
  const size = reqs.map((r) => (r.cands ? r.cands.length + 1 : 1));
  const perCall = Math.min(Math.max(1, Math.floor(2 ** 26 / nRollouts)), compare ? 65536 : Infinity);
  const parts = [];
  for (const js of byBatch.values()) {
    let nEnt = 0;
    parts.push([]);
    for (const j of js) {
      if (parts[parts.length - 1].length && nEnt + size[j] > perCall) { parts.push([]); nEnt = 0; }
      parts[parts.length - 1].push(j);
      nEnt += size[j];
    }
  }
  const out = new Array(reqs.length);
  const fseed = forecastSeed(seed);
  for (const part of parts) {
    const rooms = [], keys = [], turns = [], seats = [], base = [], subj = [];
    const acts = part.some((j) => reqs[j].cands) ? [] : null;
    const weighted = part.some((j) => reqs[j].beliefs);
    const bel = [];
    for (const j of part) {
      const r = reqs[j];
      for (let i = 0; i < size[j]; i++) bel.push(r.beliefs || r.neutral || new Array(BELIEF_SLOTS).fill(0));
      for (let i = 0; i < size[j]; i++) { base.push(rooms.length + size[j] - 1); subj.push(r.seat); }
      for (let i = 0; i < size[j]; i++) { rooms.push(r.slot); keys.push(forecastKey(r.key)); turns.push(r.turn); seats.push(r.seat || 0); }
      if (acts) acts.push(...r.cands.map((c) => [[r.seat, c]]), []);
    }
    const batch = reqs[part[0]].batch;
    const res = weighted ? batch.rolloutBeliefs(rooms, keys, turns, seatView ? seats : seats.map(() => 0), acts, bel, nRollouts, maxTurns, fseed,
                                                compare ? base : null, compare ? subj : null)
      : compare ? batch.rolloutCompare(rooms, keys, turns, seatView ? seats : seats.map(() => 0), acts, base, subj, nRollouts, maxTurns, fseed)
      : seatView ? batch.rolloutSeats(rooms, keys, turns, seats, acts, nRollouts, maxTurns, fseed)
      : acts ? batch.rolloutActions(rooms, keys, turns, acts, nRollouts, maxTurns, fseed)
        : { words: batch.rolloutRooms(rooms, keys, turns, nRollouts, maxTurns, fseed), status: null };
    let at = 0;
    for (const j of part) {
      out[j] = { words: res.words.subarray(77 * at, 77 * (at + size[j])), status: res.status && res.status.subarray(at, at + size[j]) };
      if (res.cmp) out[j].cmp = res.cmp.subarray(6 * at, 6 * (at + size[j]));
      at += size[j];
    }
  }
  return out;
}
/** advise's JSON from the words and verdicts of an advise's entries (runRollouts) at entry offset `at`: the bytes the Python hosts print. */
function adviseOutput(table, names, threadId, turn, seat, st, cands, nRollouts, maxTurns, res, at = 0, seatView = false, beliefs = null) {
  const options = [];
  cands.forEach((c, j) => {
    if (res.status[at + j] !== 0) return;
    options.push({ choice: c, label: st.pack === 1 ? names[c - 1] : String(c),
                   forecast: forecastOutput(table, names, threadId, turn, nRollouts, maxTurns, res.words, 77 * (at + j)) });
    if (res.cmp) {                                           // the option against the policy's entry, for the advised seat
      const v = (i) => Number(res.cmp[6 * (at + j) + i]);
      options[options.length - 1].versus = { compared: v(0), better: v(1), worse: v(2), gain: v(3), loss: v(4), diffSq: v(5) };
    }
  });
  const out = { threadId, turn: Number(turn), playerId: seat, phaseId: st.current_phase_id, rollouts: nRollouts, maxTurns,
                policy: forecastOutput(table, names, threadId, turn, nRollouts, maxTurns, res.words, 77 * (at + cands.length)), options };
  if (seatView) out.view = 'seat';
  if (res.cmp) out.compare = true;
  if (beliefs) out.beliefs = Array.from(beliefs);
  return out;
}

const ADVISE_CAP = 2 ** 26;                         // ge_batch_advise_seats: sum of (maxCands + 1) x nRollouts per call
/** The advice records of a hint call, one per request (twin of room_service.py run_hints): reqs [{ batch, slot, key, turn, seat, cost }]
 * - cost: the entries the library reserves for it (playoutMaxCands + 1).  RoomBatch.adviseSeats (POLICY.md §3m) under the thread's
 * forecast key and the forecast seed - advise's keys and seed.  One call per batch, in the order the batches first appear, split
 * only where the library's cap on reserved playouts needs it. */
function runHints(reqs, seatView, nRollouts, maxTurns, seed) {
  const byBatch = new Map();
  reqs.forEach((r, j) => {
    if (!byBatch.has(r.batch)) byBatch.set(r.batch, []);
    byBatch.get(r.batch).push(j);
  });
  const parts = [];
  for (const js of byBatch.values()) {
    let cost = 0;
    parts.push([]);
    for (const j of js) {
      if (parts[parts.length - 1].length && (cost + reqs[j].cost) * nRollouts > ADVISE_CAP) { parts.push([]); cost = 0; }
      parts[parts.length - 1].push(j);
      cost += reqs[j].cost;
    }
  }
  const out = new Array(reqs.length);
  for (const part of parts) {
    const adv = reqs[part[0]].batch.adviseSeats(part.map((j) => reqs[j].slot), part.map((j) => forecastKey(reqs[j].key)), part.map((j) => reqs[j].turn),
                                                part.map((j) => reqs[j].seat), nRollouts, maxTurns, forecastSeed(seed), !seatView);
    part.forEach((j, k) => { out[j] = adv[k]; });
  }
  return out;
}
/** hint's JSON from one advice record of RoomBatch.adviseSeats: the bytes the Python hosts print. */
function hintOutput(table, names, threadId, turn, seat, st, nRollouts, maxTurns, adv, seatView = true) {
  const ok = adv.status === 0;
  const options = ok ? adv.options.map((o) => ({ choice: o.choice, label: st.pack === 1 ? names[o.choice - 1] : String(o.choice), wins: o.wins,
                                                 score: o.score, finished: o.finished })) : [];
  const out = { threadId, turn: Number(turn), playerId: seat, phaseId: st.current_phase_id, rollouts: nRollouts, maxTurns, best: ok ? adv.best : null,
                policy: ok ? { finished: adv.policy.finished, wins: adv.policy.wins, score: adv.policy.score } : null, options };
  if (seatView) out.view = 'seat';
  return out;
}

const RUN_MAX_TURNS = 4096;                         // ge_batch_run_rooms's cap on maxTurns
/** runRoom's maxTurns and until, before anything runs; returns `until` as ge_batch_run_rooms's bit set. */
function checkRunArgs(maxTurns, until) {
  if (!Number.isInteger(maxTurns) || maxTurns < 1 || maxTurns > RUN_MAX_TURNS) throw new RangeError(`maxTurns must be 1 .. ${RUN_MAX_TURNS}`);
  return runUntilBits(until);
}
function checkRunThread(threadId, room, playout) {
  if (room.playoutMask && !playout) {
    throw new RangeError(`thread ${threadId} has playout seats: runRoom does not run playout bots, use continueRoom (or run it with { playout: true })`);
  }
}
/** One turn's output as runRoom keeps it: the state of a continueRoom output shares the thread's growing log (playerActions,
 * phase_history, game_notes), and here later turns are folded before the caller sees the earlier ones - so those three are copied. */
function runTurn(out) {
  const st = out.state;
  out.state = Object.assign({}, st, JSON.parse(JSON.stringify({ playerActions: st.playerActions, phase_history: st.phase_history, game_notes: st.game_notes })));
  return out;
}
function runOutput(turns, stopped, forecasts) {
  const out = { turns, played: turns.length, stopped: runUntilNames(stopped) };
  if (forecasts) out.forecasts = forecasts;
  return out;
}
const TIMELINE_MAX_POINTS = 1 << 16, TIMELINE_CAP = 2 ** 26;    // ge_batch_run_rooms_forecast: n x (maxTurns + 1) per call, and x nRollouts
/** runRoom's forecast options { forecast: true, rollouts = 4096, maxTurns = 1024, seat } (POLICY.md §3i; twin of room_service.py
 * check_run_forecast), before anything runs; returns null without `forecast`. */
function checkRunForecast(threadId, room, maxTurns, options) {
  if (!options || !options.forecast) return null;
  const f = { rollouts: options.rollouts === undefined ? 4096 : options.rollouts, maxTurns: options.maxTurns === undefined ? 1024 : options.maxTurns,
              seat: options.seat === null ? undefined : options.seat };
  checkForecastArgs(f.rollouts, f.maxTurns);
  checkForecastSeat(threadId, room.names.length, f.seat);
  if (room.playoutMask) throw new RangeError(`thread ${threadId} has playout seats: runRoom gives no forecasts of a run with playout bots`);
  if ((maxTurns + 1) * f.rollouts > TIMELINE_CAP) throw new RangeError(`(maxTurns + 1) x rollouts must be at most ${TIMELINE_CAP}`);
  if (room.turn + maxTurns + f.maxTurns > 0xFFFFFFFF) throw new RangeError(`thread ${threadId}: the turn counter would overflow`);
  return f;
}
/** The most threads one runRoomsForecast call takes under the library's caps. */
function runForecastPerCall(maxTurns, nRollouts) {
  const pts = maxTurns + 1;
  return Math.max(1, Math.min(Math.floor((1 << 20) / maxTurns), Math.floor(TIMELINE_MAX_POINTS / pts), Math.floor(TIMELINE_CAP / (pts * nRollouts))));
}
/** runRoom's "forecasts": element p is forecast()'s JSON of the thread as it stood after p of the call's turns. */
function runForecasts(table, names, threadId, turn, f, stats) {
  return stats.map((w, p) => seatForecastOutput(table, names, threadId, turn + p, f.rollouts, f.maxTurns, f.seat, w));
}

class RoomService {
  /** playoutRollouts / playoutMaxTurns / playoutView: how the playout bots of threads created with playoutSeats choose
   * (POLICY.md §3d): nRollouts and maxTurns of each candidate's playouts, and "seat" (from what the bot knows) or "full" (from
   * the true record - a cheating bot in a game with people).  playoutHalving: the bots spend each decision's playouts by
   * sequential halving (POLICY.md §3h): fewer playouts but more launches per turn, and slower at every shape measured on an MI355X (x 0.38 .. 0.71 of the unflagged call's speed), so off by default; a
   * bot's candidate values are then advise's option forecasts for the finalists only. */
  constructor({ gamesDir = 'games', seed = 0n, device = 0, playoutRollouts = 256, playoutMaxTurns = 256, playoutView = 'seat',
                playoutHalving = false } = {}) {
    this.playoutFull = checkPlayoutOptions(playoutRollouts, playoutMaxTurns, playoutView, playoutHalving);
    this.playoutHalving = playoutHalving;
    this.playoutRollouts = playoutRollouts; this.playoutMaxTurns = playoutMaxTurns;
    this.gamesDir = gamesDir; this.seed = BigInt(seed); this.device = device;
    this.tables = new Map();       // gameName -> GameTable
    this.rooms = new Map();        // threadId -> { batch, table, state, phaseHistory, playerActions, gameNotes, names }
  }
  table(gameName, dsl) {
    if (!this.tables.has(gameName)) this.tables.set(gameName, dsl ? new GameTable(dsl) : GameTable.fromGamename(gameName, this.gamesDir));
    return this.tables.get(gameName);
  }
  /** roomSession.players as the lobby builds it (src/app/game-library/[game]/room/page.tsx:261-369). */
  /** players[i].isBot === false marks a human seat: the bot policy never acts for it (humanAction does). */
  /** playoutSeats: bot seats that choose each action by playouts (RangeError for a human seat or an id outside 1..n, before
   * anything is created). */
  createRoom({ threadId, gameName, players, dsl, roomIndex, playoutSeats }) {
    const table = this.table(gameName, dsl);
    const humanMask = players.reduce((m, p, i) => (p.isBot === false ? m | (1 << i) : m), 0);
    const playoutMask = playoutMaskOf(players.length, humanMask, playoutSeats);
    const key = roomIndex === undefined ? roomIndexOf(threadId) : BigInt(roomIndex);
    const batch = new RoomBatch({ segments: [{ table, nPlayers: players.length, nRooms: 1, humanMask }], seed: this.seed,
                                  firstRoom: key,   // the RNG is keyed by it
                                  device: this.device, maxFuse: 1, trace: true });
    if (this.rooms.has(threadId)) this.close(threadId);
    const names = players.map((p, i) => p.name || `Player ${i + 1}`);
    const humanSeats = players.map((p, i) => (p.isBot === false ? i + 1 : 0)).filter((x) => x);
    const room = { batch, key, turn: 0, table, gameName, names, humanSeats, playoutMask, panel: null, state: batch.readRoom(0), log: new RoomLog(table, names, gameName), queue: Promise.resolve() };
    this.rooms.set(threadId, room);
    return this.agentState(room);
  }
  /**
   * Take over a thread that is already mid-game (twin of the Python RoomService.adopt_room): `state` is its AgentState
   * (current_phase_id, player_states, playerActions, phase_history, game_notes).  players (optional): isBot === false marks a
   * human seat, as does humanSeats (player ids); names default to the state's.  turn: the thread's next turn (default
   * phase_history.length); visitActions {playerId: choice}: a human seat's action already logged in this visit.  Returns
   * { state, toolCalls: [], uiCalls } - the UI of the phase now showing, as the last turn rendered it.  A state that does not
   * fit throws (TypeError / RangeError) before anything is created or closed.
   */
  adoptRoom({ threadId, gameName, state, players, humanSeats, dsl, roomIndex, turn, visitActions, playoutSeats }) {
    const table = this.table(gameName, dsl);
    const a = prepareAdoption(table, { state, players, humanSeats, turn, visitActions });
    const playoutMask = playoutMaskOf(a.n, a.humanMask, playoutSeats);
    const key = roomIndex === undefined ? roomIndexOf(threadId) : BigInt(roomIndex);
    const batch = new RoomBatch({ segments: [{ table, nPlayers: a.n, nRooms: 1, humanMask: a.humanMask }], seed: this.seed,
                                  firstRoom: key, device: this.device, maxFuse: 1, trace: true });
    try {
      batch.writeRoomsAt([0], [a.view]);
      batch.setTurn(a.turn);
    } catch (e) { batch.close(); throw e; }
    if (this.rooms.has(threadId)) this.close(threadId);
    const room = { batch, key, turn: a.turn, table, gameName, names: a.names, humanSeats: a.humanSeats, playoutMask, panel: null, state: batch.readRoom(0),
                   log: new RoomLog(table, a.names, gameName), queue: Promise.resolve() };
    room.log.adopt(state, Object.assign({}, a.hostSide, { names: Object.fromEntries(a.names.map((nm, i) => [String(i + 1), nm])) }));
    this.rooms.set(threadId, room);
    return adoptedOutput(room, a.turn);
  }
  agentState(room) { return room.log.agentState(room.state); }
  /** A seat changes hands mid-game (twin of the Python RoomService.set_human_seats, POLICY.md §3l): from the next turn on exactly
   * `seats` (player ids) are played by people, every other seat by the policy.  The thread's humanSeats (what handleMessage
   * resolves against and advise defaults to) follow, and a seat given to a person leaves the thread's playout seats.  Rejects for an
   * unknown thread or a seat outside 1..n, before anything changes; resolves with the seats. */
  setHumanSeats(threadId, seats) {
    const room = this.rooms.get(threadId);
    if (!room) return Promise.reject(new Error(`unknown thread ${threadId}`));
    let mask;
    try { mask = seatsMask(threadId, room.names.length, seats); } catch (e) { return Promise.reject(e); }
    return this._serial(room, () => {
      room.batch.setSeats([0], [mask]);
      room.humanSeats = room.names.map((_, i) => i + 1).filter((i) => (mask >> (i - 1)) & 1);
      room.playoutMask &= ~mask;
      return room.humanSeats.slice();
    });
  }
  /** Requests of one thread run strictly one after the other (the reference's LangGraph server queues
   * runs per thread the same way): overlapping /continue and /action calls neither race on the batch
   * handle nor see a half-updated log. */
  _serial(room, fn) {
    const p = room.queue.then(fn);
    room.queue = p.catch(() => {});
    return p;
  }
  /** How the thread ends from where it stands (twin of the Python RoomService.forecast): nRollouts playouts of its room, each for
   * up to maxTurns turns from its next turn, every seat - human seats too - played by the policy.  Replica r is global room
   * (threadKey << 16) + r, so nRollouts <= 65 536 (RangeError above), under seed (service seed ^ 0x9E3779B97F4A7C15); two forecasts
   * at the same turn are identical and the thread is not changed.  Resolves with JSON integers: threadId, turn, rollouts, maxTurns,
   * finished, endTurnSum, ended, and per seat (Werewolf: sides {villagers, werewolves}, players {"1": {name, alive, wins}};
   * Two-Truths: players {"1": {name, scoreSum, topScore}}).  seat (1 .. n): the playouts start from what that seat knows
   * (rolloutSeats, POLICY.md §3c) and the JSON gains "seat" - the form to show a player; the default is the full view.  beliefs
   * (with seat): what that seat suspects, { seat number (Werewolf) or statement number 1-3 (Two-Truths): 0..255 }, unnamed ones 16;
   * the re-deal is weighted by it (rolloutBeliefs, POLICY.md §3j) and the JSON gains "beliefs", the 16 bytes used.  RangeError,
   * before anything runs, for a value out of range, a key the thread does not have, or beliefs without a seat. */
  forecast(threadId, nRollouts = 4096, maxTurns = 1024, seat, beliefs) {
    checkForecastArgs(nRollouts, maxTurns);
    const room = this.rooms.get(threadId);
    if (!room) return Promise.reject(new Error(`unknown thread ${threadId}`));
    checkForecastSeat(threadId, room.names.length, seat);
    const bel = beliefBytes(threadId, room.table.info.pack, room.names.length, beliefs, seat !== undefined && seat !== null);
    return this._serial(room, () => {
      const [res] = runRollouts([{ batch: room.batch, slot: 0, key: room.key, turn: room.turn, seat, beliefs: bel }], seat !== undefined && seat !== null,
                                nRollouts, maxTurns, this.seed);
      return seatForecastOutput(room.table, room.names, threadId, room.turn, nRollouts, maxTurns, seat, res.words, 0, bel);
    });
  }
  /** What each choice the seat can make now leads to (twin of the Python RoomService.advise): for every candidate the forecast given
   * that the seat logs it before the next turn, and the policy's own ("policy", equal to forecast(threadId)).  One rolloutActions
   * call under forecast's keys and seed.  playerId defaults to the lowest human seat (RangeError if there is none).  Resolves with
   * { threadId, turn, playerId, phaseId, rollouts, maxTurns, policy, options: [{ choice, label, forecast }] } for the accepted
   * candidates in ascending order.  The thread is not changed.  view "seat": every playout starts from what the advised seat knows
   * (rolloutSeats) - the form to show that player - and the JSON gains "view": "seat"; "full" (the default) is for spectators.
   * compare: the one call is rolloutCompare; the JSON gains "compare": true and per option "versus" { compared, better, worse, gain,
   * loss, diffSq }: the option against the policy's entry, playout by playout, for the advised seat; the rest is the same bytes.
   * beliefs (view "seat" only): what the advised seat suspects, as forecast's; every entry of the call is dealt under it and the
   * JSON gains "beliefs". */
  advise(threadId, playerId, nRollouts = 4096, maxTurns = 1024, view = 'full', compare = false, beliefs) {
    checkForecastArgs(nRollouts, maxTurns);
    const seatView = checkView(view);
    const room = this.rooms.get(threadId);
    if (!room) return Promise.reject(new Error(`unknown thread ${threadId}`));
    const seat = adviseSeat(threadId, room.humanSeats, playerId);
    const bel = beliefBytes(threadId, room.table.info.pack, room.names.length, beliefs, seatView);
    return this._serial(room, () => {
      const cands = adviseCandidates(room.table, room.state);
      const [res] = runRollouts([{ batch: room.batch, slot: 0, key: room.key, turn: room.turn, seat, cands, beliefs: bel }], seatView, nRollouts, maxTurns,
                                this.seed, !!compare);
      return adviseOutput(room.table, room.names, threadId, room.turn, seat, room.state, cands, nRollouts, maxTurns, res, 0, seatView, bel);
    });
  }
  /** advise in 224 bytes (twin of the Python RoomService.hint): which choices the seat can make now, what each leads to for that
   * seat, and the best of them - found, played and ranked on the device (RoomBatch.adviseSeats, POLICY.md §3m) under advise's keys
   * and seed, so every number is the advised seat's own inside advise's option forecasts.  playerId defaults to the lowest human
   * seat.  Resolves with { threadId, turn, playerId, phaseId, rollouts, maxTurns, best, policy: { finished, wins, score }, options:
   * [{ choice, label, wins, score, finished }], view: "seat" } (no `view` key for view "full"); best and policy are null and options
   * [] when the seat has nothing to do now.  The thread is not changed. */
  hint(threadId, playerId, nRollouts = 4096, maxTurns = 1024, view = 'seat') {
    checkForecastArgs(nRollouts, maxTurns);
    const seatView = checkView(view);
    const room = this.rooms.get(threadId);
    if (!room) return Promise.reject(new Error(`unknown thread ${threadId}`));
    const seat = adviseSeat(threadId, room.humanSeats, playerId);
    return this._serial(room, () => {
      const cost = playoutMaxCands(room.table.info.pack, room.names.length) + 1;
      const [adv] = runHints([{ batch: room.batch, slot: 0, key: room.key, turn: room.turn, seat, cost }], seatView, nRollouts, maxTurns, this.seed);
      return hintOutput(room.table, room.names, threadId, room.turn, seat, room.state, nRollouts, maxTurns, adv, seatView);
    });
  }
  /** Forget a thread and free its device memory (after queued requests have finished). */
  close(threadId) {
    const room = this.rooms.get(threadId);
    if (!room) return Promise.resolve(false);
    this.rooms.delete(threadId);
    return this._serial(room, () => { room.batch.close(); return true; });
  }
  /** A human's vote / choice (the frontend's "Player X voted ..." message, src/app/page.tsx:302-305). */
  humanAction(threadId, playerId, choice) {
    const room = this.rooms.get(threadId);
    if (!room) return Promise.reject(new Error(`unknown thread ${threadId}`));
    return this._serial(room, () => {
      room.batch.injectAction(0, playerId, choice);
      room.state = room.batch.readRoom(0);
      return this.agentState(room);
    });
  }
  /** One turn (one graph run).  Returns { state, toolCalls, uiCalls }. */
  /** items: the frontend's canvas items (AgentState.items) when the caller has them (clearCanvas exemptList). */
  continueRoom(threadId, items) {
    const room = this.rooms.get(threadId);
    if (!room) return Promise.reject(new Error(`unknown thread ${threadId}`));
    return this._serial(room, () => this._continue(room, items));
  }
  /** Play the thread on until a person is needed (twin of the Python RoomService.run_room): one RoomBatch.runRooms call (POLICY.md
   * §3f) instead of a continueRoom per turn.  until: "person" (a human seat of the thread has an action to give), "end" (the game
   * is over), "phase" (the turn moved the phase); the first turn is always played, at most maxTurns are.  Resolves { turns:
   * [{ state, toolCalls, uiCalls }, ...], played, stopped }: element t is exactly what continueRoom would have resolved for that
   * turn (items goes to every turn's UI builder as given), stopped names the conditions that held after the last turn ([]: the
   * limit), and the thread's turn and panel end where `played` calls of continueRoom would have left them.  A thread with playout
   * seats or bad arguments are refused (RangeError) before anything runs; with options { playout: true } a thread with playout seats
   * is run by one RoomBatch.runRoomsPlayout call (POLICY.md §3g) under the keys, seed and options continueRoom gives its playout
   * bots.  Every turn's state carries its own copy of the thread's log (runTurn): host work that grows with the log, per turn.
   * options { forecast: true, rollouts, maxTurns, seat }: a win-odds timeline of the run (POLICY.md §3i), from one
   * RoomBatch.runRoomsForecast call instead - the result gains forecasts, played + 1 objects: element p is exactly what
   * forecast(threadId, rollouts, maxTurns, seat) would have resolved after p of the call's turns, every point under the same keys
   * and seed.  The options are checked as forecast checks them and a thread with playout seats is refused, before anything runs. */
  runRoom(threadId, maxTurns = 64, until = ['person', 'end'], items, options) {
    const room = this.rooms.get(threadId);
    if (!room) return Promise.reject(new Error(`unknown thread ${threadId}`));
    return this._serial(room, () => {
      const bits = checkRunArgs(maxTurns, until);
      checkRunThread(threadId, room, !!(options && options.playout));
      const f = checkRunForecast(threadId, room, maxTurns, options);
      if (f) {
        const turn = room.turn;
        const q = room.batch.runRoomsForecast([0], [room.key], [turn], [forecastKey(room.key)], f.rollouts, f.maxTurns, [f.seat || 0],
                                              forecastSeed(this.seed), maxTurns, bits);
        room.turn += q.played[0];
        room.batch.setTurn(room.turn);
        return runOutput(q.events[0].map((ev, t) => runTurn(this._finish(room, q.views[0][t], ev, items))), q.stopped[0],
                         runForecasts(room.table, room.names, threadId, turn, f, q.stats[0]));
      }
      const r = room.playoutMask
        ? room.batch.runRoomsPlayout([0], [room.key], [room.turn], [room.playoutMask], [forecastKey(room.key)], this.playoutRollouts,
                                     this.playoutMaxTurns, forecastSeed(this.seed), this.playoutFull, maxTurns, bits, true,
                                     this.playoutHalving)
        : room.batch.runRooms([0], [room.key], [room.turn], maxTurns, bits);
      room.turn += r.played[0];
      room.batch.setTurn(room.turn);
      return runOutput(r.events[0].map((ev, t) => runTurn(this._finish(room, r.views[0][t], ev, items))), r.stopped[0]);
    });
  }
  /**
   * The drop-in's message-level entry: what the reference's graph does with ONE message of the browser
   * (src/app/page.tsx:183-259 -> agent/game_agent_v2.py:198-349, agent/tools/utils.py:310-358; POLICY.md 3b).
   *   chat ("... in game chat: ..." / "... to Bot k: ...")  -> ChatBotNode: no turn, no state change;
   *   control ("Start game.", "Continue")                    -> one turn;
   *   anything else -> logged verbatim under Player 1 (200 characters, phase 0's name - the reference's own quirk), read as a
   *                    seat's action where it is one (a vote on the newest panel, an input for the statements phase), then one turn.
   * Resolves { state, toolCalls, uiCalls, played, kind }; an action message that is no valid game action is still logged and
   * still plays the turn, as in the reference.
   */
  handleMessage(threadId, text, items) {
    const room = this.rooms.get(threadId);
    if (!room) return Promise.reject(new Error(`unknown thread ${threadId}`));
    return this._serial(room, async () => {
      const kind = M.classify(text);
      if (kind === M.CHAT) return { state: this.agentState(room), toolCalls: [], uiCalls: [], played: false, kind };
      if (kind === M.ACTION) {
        room.log.personMessage(text);
        const st = room.state, info = room.table.info;
        const phase = info.phases.find((x) => x.id === st.current_phase_id);
        const alive = st.slots.map((v) => (st.pack === 1 ? !!v[2] : true));
        for (const [seat, choice] of M.resolve(text, room.panel, phase ? phase.act : 0, st.pack, room.names, alive, room.humanSeats)) {
          try { room.batch.injectAction(0, seat, choice); break; } catch (e) {
            if (e.code !== 'GE-1') throw e;            // GE_ERR_ARG: not a living pending target of this phase - logged, no game effect
          }
        }
      }
      const out = await this._continue(room, items);
      return Object.assign(out, { played: true, kind });
    });
  }
  async _continue(room, items) {
    // `before` is the state BEFORE any injected action of this message: the person's record writes then show up among the
    // turn's update_player_state calls, where the reference's Referee issues them
    const before = room.state;
    let event;
    if (room.playoutMask) {                            // playout bots: advise's keys and seed, so a bot's values are its advice
      const { events } = room.batch.stepRoomsPlayout([0], [room.key], [room.turn], [room.playoutMask], [forecastKey(room.key)],
                                                     this.playoutRollouts, this.playoutMaxTurns, forecastSeed(this.seed), this.playoutFull,
                                                     this.playoutHalving);
      room.batch.setTurn(room.turn + 1);
      event = events[0];
    } else {
      await room.batch.step(1);
      event = room.batch.readEvents(0, 1)[0][0];
    }
    room.turn += 1;
    return this._finish(room, room.batch.readRoom(0), event, items);
  }
  /** Fold one played turn - its event and the state after it - into the thread: the turn's tool calls, log, state and UI. */
  _finish(room, after, event, items) {
    const before = room.state;
    const toolCalls = turnToolCalls(room.table, before, after, event);
    // fold the calls into the log-shaped parts of AgentState the packed state does not carry
    // (playerActions / game_notes / phase_history, as backend_tools.py:163-202, 285-344 would)
    room.log.fold(toolCalls, after);
    room.state = after;
    const state = this.agentState(room);
    const deaths = toolCalls.filter((c) => c.name === 'update_player_state' && c.args.state_name === 'is_alive' && c.args.state_value === false).map((c) => c.args.player_id);
    const uiCalls = uiToolCalls(room.table.dsl, state, { table: room.table, turn: event.turn, deaths, items });
    room.panel = M.newestPanel(uiCalls);               // what a person's next vote message can answer
    return { state, toolCalls, uiCalls };
  }
  serve(port = 8124) {
    const server = http.createServer((req, res) => {
      let body = '';
      req.on('data', (d) => { body += d; });
      req.on('end', async () => {
        try {
          const msg = body ? JSON.parse(body) : {};
          let out;
          if (req.method === 'POST' && req.url === '/rooms') out = this.createRoom(msg);
          else if (req.method === 'POST' && req.url === '/continue') out = await this.continueRoom(msg.threadId, msg.items);
          else if (req.method === 'POST' && req.url === '/run') out = await this.runRoom(msg.threadId, msg.maxTurns, msg.until, msg.items, Object.assign({ playout: !!msg.playout }, msg.forecast && typeof msg.forecast === 'object' ? Object.assign({ forecast: true }, msg.forecast) : { forecast: !!msg.forecast }));
          else if (req.method === 'POST' && req.url === '/forecast') out = await this.forecast(msg.threadId, msg.rollouts, msg.maxTurns, msg.seat, msg.beliefs);
          else if (req.method === 'POST' && req.url === '/advise') out = await this.advise(msg.threadId, msg.playerId, msg.rollouts, msg.maxTurns, msg.view, msg.compare, msg.beliefs);
          else if (req.method === 'POST' && req.url === '/message') out = await this.handleMessage(msg.threadId, msg.text, msg.items);
          else if (req.method === 'POST' && req.url === '/action') out = await this.humanAction(msg.threadId, msg.playerId, msg.choice);
          else if (req.method === 'POST' && req.url === '/close') out = { closed: await this.close(msg.threadId) };
          else { res.writeHead(404); res.end(); return; }
          res.writeHead(200, { 'content-type': 'application/json' });
          res.end(JSON.stringify(out));
        } catch (e) { res.writeHead(400); res.end(JSON.stringify({ error: String(e.message || e) })); }
      });
    });
    return new Promise((resolve) => server.listen(port, '127.0.0.1', () => resolve(server)));
  }
}

module.exports = { RoomService, seatsMask, playoutMaskOf, checkPlayoutOptions, PLAYOUT_CAP, playoutMaxCands, roomIndexOf, prepareAdoption, adoptedOutput, checkForecastArgs, forecastKey, forecastSeed, forecastOutput,
                   adviseCandidates, adviseSeat, runRollouts, adviseOutput, runHints, hintOutput, seatForecastOutput, beliefBytes, neutralBeliefs, checkForecastSeat, checkView, checkRunArgs, checkRunThread, runTurn, runOutput,
                   checkRunForecast, runForecastPerCall, runForecasts };

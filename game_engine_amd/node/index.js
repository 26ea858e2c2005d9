'use strict';
/**
 * TypeScript/Node host of the MI355X batch stepper (types: index.d.ts).
 *
 * Drop-in point in the reference: src/app/api/copilotkit/route.ts:22-47 hands a room's
 * AgentState to the Python LangGraph server (graph "sample_agent" = agent/game_agent_v2.py).
 * This module offers the same step — "advance this room by one turn" — for whole batches of
 * rooms, on the GPU, and returns state in the AgentState shape the frontend already syncs
 * (src/lib/canvas/types.ts:338-360): current_phase_id, current_phase_name,
 * player_states {"1": {<declared fields>}}.  YAML is parsed here with js-yaml, exactly as the
 * reference's TS side does (src/app/api/games/initialize-players/route.ts); everything else is
 * the C ABI behind ge_addon.node.
 */
const fs = require('fs');
const path = require('path');
const addon = require('./ge_addon.node');

function loadYaml() {
  try { return require('js-yaml'); } catch (e) { /* fall through */ }
  try { return require('/usr/share/nodejs/js-yaml'); } catch (e) { /* fall through */ }
  throw new Error('js-yaml is required to read games/*.yaml (the reference ships it: package.json)');
}

/** Same contract as the reference's load_dsl_by_gamename (agent/tools/utils.py:557-581). */
function loadDslByGamename(gamename, gamesDir) {
  if (!gamename) return {};
  const dir = gamesDir || process.env.GE_GAMES_DIR || 'games';
  const y = path.join(dir, `${gamename}.yaml`);
  const j = path.join(dir, `${gamename}.json`);
  if (fs.existsSync(y)) return loadYaml().load(fs.readFileSync(y, 'utf8')) || {};
  if (fs.existsSync(j)) return JSON.parse(fs.readFileSync(j, 'utf8'));
  return {};
}

/** Game name -> file in the games directory, as the reference's TS routes match it
 * (src/app/api/games/initialize-players/route.ts:62-70): case-insensitive, every character outside
 * [a-z0-9] equals '-'.  Returns the file name or null. */
function findGameFile(gameName, gamesDir) {
  const dir = gamesDir || process.env.GE_GAMES_DIR || 'games';
  const norm = (x) => String(x).toLowerCase().replace(/[^a-z0-9]/g, '-');
  const want = norm(gameName);
  for (const f of fs.readdirSync(dir)) {
    if (norm(f.toLowerCase().replace('.yaml', '')) === want) return f;
  }
  return null;
}

/** player_states for the real players of a room, as POST /api/games/initialize-players builds them
 * (route.ts:83-166): template = declaration.player_states_template.player_states['1'], else its first
 * entry, else defaults generated from the declaration.player_states schema (string '' / num 0 /
 * boolean true / list [] / dict {}, or the field's `example`), else {player_states: {}, fallback_mode: true}.
 * Every player gets a copy of the template plus name, id, isHost; keys are gamePlayerId or the
 * 1-based position.  (The Python host's initialize_player_states_from_dsl is the agent-side twin,
 * agent/tools/utils.py:584-653.) */
function initializePlayers(dsl, roomPlayers) {
  const decl = (dsl && dsl.declaration) || {};
  let template;
  const tpl = decl.player_states_template && decl.player_states_template.player_states;
  if (tpl) {
    template = tpl['1'];
    if (!template) {
      const ids = Object.keys(tpl);
      if (ids.length) template = tpl[ids[0]];
    }
  }
  if (!template && decl.player_states) {
    template = {};
    for (const [field, def] of Object.entries(decl.player_states)) {
      const type = (def && def.type) || 'string';
      const ex = def ? def.example : undefined;
      if (type === 'string') template[field] = ex || '';
      else if (type === 'num' || type === 'number') template[field] = ex || 0;
      else if (type === 'boolean') template[field] = ex !== undefined ? ex : true;
      else if (type === 'array' || type === 'list') template[field] = ex || [];
      else if (type === 'object' || type === 'dict') template[field] = ex || {};
      else template[field] = ex || null;
    }
  }
  if (!template || !Object.keys(template).length) {
    return { player_states: {}, fallback_mode: true, message: 'No template found, agent will generate player_states' };
  }
  const out = {};
  roomPlayers.forEach((pl, k) => {
    const pid = pl.gamePlayerId || String(k + 1);
    out[pid] = Object.assign(JSON.parse(JSON.stringify(template)), { name: pl.name, id: pl.id || pid, isHost: pl.isHost || false });
  });
  return { player_states: out };
}

const TEAMS = ['', 'villagers', 'werewolves'];
const VIEW = { size: addon.roomViewSize(), players: 20, det: 20 + 16 * 12 };

class GameTable {
  constructor(dsl, rounds = 1) {
    if (!dsl || typeof dsl !== 'object' || !Object.keys(dsl).length) throw new Error('empty DSL');
    this.dsl = dsl;
    this.handle = addon.compileTable(JSON.stringify(dsl), rounds);
    this.info = addon.tableInfo(this.handle);
    // declared fields the rule packs do not model: constants from the template (nobody writes them under the fixed policy)
    const tps = ((dsl.declaration || {}).player_states_template || {}).player_states || {};
    const tmpl = tps['1'] || tps[Object.keys(tps)[0]] || {};
    // info.fieldNames: slot (include/ge_step.h GE_WW_* / GE_TT_*) -> the DSL's own field name, '' = not declared
    const modelled = new Set(['name', ...this.info.fieldNames.filter((x) => x)]);
    this.extraFields = {};
    for (const [k, v] of Object.entries(tmpl)) if (!modelled.has(k) && ['boolean', 'number', 'string'].includes(typeof v)) this.extraFields[k] = v;
  }
  static fromGamename(gamename, gamesDir, rounds = 1) {
    return new GameTable(loadDslByGamename(gamename, gamesDir), rounds);
  }
  phaseName(id) {
    const p = this.info.phases.find((x) => x.id === id);
    return p ? p.name : `Phase ${id}`;            // utils.py:30 fallback
  }
}

function decodeRoom(table, buf, off) {
  const dv = new DataView(buf, off, VIEW.size);
  const u8 = new Uint8Array(buf, off, VIEW.size);
  const n = u8[17];
  const pack = u8[18];
  const playerStates = {};
  const det = Array.from(u8.slice(VIEW.det, VIEW.det + n));
  const names = table.info.fieldNames;
  const slots = [];              // per player: one value per slot of the pack, declared by the DSL or not
  for (let i = 0; i < n; i++) {
    const f = u8.slice(VIEW.players + 12 * i, VIEW.players + 12 * i + 12);
    let vals;
    if (pack === 1) {
      const mem = {};
      if (f[0] === 4) det.forEach((d, k) => { if (d) mem[String(k + 1)] = TEAMS[d]; });
      vals = [table.info.roleNames[f[0]], TEAMS[f[1]], !!f[2], !!f[3], !!f[4], !!f[5], !!f[6], !!f[7], f[8], mem, f[1] === 2];
    } else {
      vals = [!!f[0], !!f[1], f[2], !!f[3], !!f[4], f[5], !!f[6], f[7], f[8]];
    }
    slots.push(vals);
    const rec = {};                // player_states hold exactly what the DSL declares, under its own names
    vals.forEach((v, s) => { if (names[s]) rec[names[s]] = v; });
    playerStates[String(i + 1)] = Object.assign(rec, table.extraFields || {});
  }
  const phaseId = dv.getInt32(0, true);
  return {
    current_phase_id: phaseId, current_phase_name: table.phaseName(phaseId),
    previous_phase_id: dv.getInt32(4, true), end_turn: dv.getInt32(8, true), games: dv.getInt32(12, true),
    player_states: playerStates, pack, slots,
    acted: Array.from({ length: n }, (_, i) => u8[VIEW.players + 12 * i + 9]),
    choice: Array.from({ length: n }, (_, i) => u8[VIEW.players + 12 * i + 10]),
  };
}

// ---- AgentState -> room view: the inverse of decodeRoom / RoomLog.agentState (twin of stepper.agent_state_to_view)
const ACTION_TAG = /^\[t=(\d+)\|c=(\d+)\]/;
const WW_INTS = { 8: null };                       // integer slots and the largest value the record holds (null: the player count)
const TT_INTS = { 2: 3, 5: 3, 7: 255, 8: 15 };
const ACT_NIGHT = [1, 2, 3];                       // GE_ACT_WOLF_TARGET, GE_ACT_DOCTOR_PROTECT, GE_ACT_DETECTIVE
const EFF_NIGHT_BEGIN = 2;
const GE_MAX_PLAYERS = 12;
const BELIEF_SLOTS = 16;                           // GE_BELIEF_SLOTS
const isInt = (x) => typeof x === 'number' && Number.isInteger(x);
const isDict = (x) => x !== null && typeof x === 'object' && !Array.isArray(x);
const sameValue = (a, b) => JSON.stringify(a) === JSON.stringify(b);

function taggedActions(pa, n, keep) {               // [pid, turn, choice, phase] of every "[t=..|c=..]" entry keep() accepts
  const out = [];
  for (const [key, rec] of Object.entries(pa)) {
    const pid = Number(key);
    if (!Number.isInteger(pid) || pid < 1 || pid > n || !isDict(rec)) continue;
    const acts = rec.actions || {};
    for (const a of (Array.isArray(acts) ? acts : Object.values(acts))) {
      if (!isDict(a)) continue;
      const m = ACTION_TAG.exec(String(a.action === undefined ? '' : a.action));
      if (m && keep(a.phase)) out.push([pid, Number(m[1]), Number(m[2])]);
    }
  }
  return out;
}

/**
 * The room view of a reference AgentState (current_phase_id, player_states, playerActions, phase_history) under the DSL's own
 * field names: the exact inverse of decodeRoom / RoomLog.agentState, with the rules of the Python host's
 * stepper.agent_state_to_view (INTEGRATION.md "Handing a running thread to the stepper").  Returns { view: ArrayBuffer of one
 * ge_room_view, hostSide: { names, statements, extra } }.  A value of the wrong type throws TypeError; one that does not fit the
 * record or the table (unknown role, team typo, out of range, missing player, a derived slot that disagrees) throws RangeError.
 */
function agentStateToView(table, state, { nPlayers, visitActions } = {}) {
  if (!isDict(state)) throw new TypeError('state must be an object');
  const info = table.info, names = info.fieldNames, ww = info.pack === 1;
  const ps = state.player_states;
  if (!isDict(ps) || !Object.keys(ps).length) throw new TypeError("state.player_states must be a non-empty object");
  const n = nPlayers === undefined || nPlayers === null ? Object.keys(ps).length : Number(nPlayers);
  if (!(n >= 1 && n <= GE_MAX_PLAYERS)) throw new RangeError(`${n} players: a room holds 1..${GE_MAX_PLAYERS}`);
  const byId = new Map();
  for (const [key, rec] of Object.entries(ps)) {
    const pid = Number(key);
    if (!Number.isInteger(pid)) throw new RangeError(`player_states key ${JSON.stringify(key)} is not a player id`);
    if (!isDict(rec)) throw new TypeError(`player ${key}: not an object`);
    byId.set(pid, rec);
  }
  const ids = [...byId.keys()].sort((a, b) => a - b);
  if (ids.length !== n || ids.some((x, i) => x !== i + 1)) throw new RangeError(`player_states must name players 1..${n} exactly, got ${JSON.stringify(ids)}`);
  const phases = info.phases, phaseIds = phases.map((p) => p.id);
  const cur = state.current_phase_id;
  if (!isInt(cur)) throw new TypeError(`current_phase_id ${JSON.stringify(cur)} is not an integer`);
  if (!phaseIds.includes(cur)) throw new RangeError(`current_phase_id ${cur} is not a phase of the table`);
  const hist = state.phase_history === undefined || state.phase_history === null ? [] : state.phase_history;
  if (!Array.isArray(hist)) throw new TypeError('phase_history must be an array');
  const histIds = hist.map((e) => {
    if (!isDict(e) || !isInt(e.phase_id)) throw new TypeError(`phase_history entries need an integer phase_id, got ${JSON.stringify(e)}`);
    return e.phase_id;
  });
  let s = histIds.length;                                   // the trailing run of the current phase: hist[s..]
  while (s > 0 && histIds[s - 1] === cur) s--;

  const buf = new ArrayBuffer(VIEW.size);
  const dv = new DataView(buf), u8 = new Uint8Array(buf);
  u8[17] = n; u8[18] = info.pack;
  dv.setInt32(0, cur, true);
  let prev = state.previous_phase_id;
  if (prev === undefined || prev === null) prev = s > 0 ? histIds[s - 1] : 0;   // a fresh room holds phase 0 as its previous phase
  if (!isInt(prev)) throw new TypeError(`previous_phase_id ${JSON.stringify(prev)} is not an integer`);
  if (!phaseIds.includes(prev)) throw new RangeError(`previous_phase_id ${prev} is not a phase of the table`);
  dv.setInt32(4, prev, true);
  u8[16] = histIds.includes(0) ? 1 : 0;
  let end = state.end_turn;
  if (end === undefined || end === null) end = phases[phaseIds.indexOf(cur)].nBranches === 0 ? Math.min(s, 0xFFFE) : -1;
  if (!isInt(end)) throw new TypeError(`end_turn ${JSON.stringify(end)} is not an integer`);
  if (end < -1 || end > 0xFFFE) throw new RangeError(`end_turn ${end} is out of range (-1 .. 65534)`);
  dv.setInt32(8, end, true);
  const games = state.games === undefined || state.games === null ? 0 : state.games;
  if (!isInt(games)) throw new TypeError(`games ${JSON.stringify(games)} is not an integer`);
  if (games < 0 || games > 0xFFFF) throw new RangeError(`games ${games} is out of range (0 .. 65535)`);
  dv.setInt32(12, games, true);

  const roles = info.roleNames, ints = ww ? WW_INTS : TT_INTS;
  const modelled = new Set(['name', ...names.filter((x) => x)]);
  const host = { names: {}, statements: {}, extra: {} };
  const row = (i) => VIEW.players + 12 * i;
  for (let pid = 1; pid <= n; pid++) {
    const rec = byId.get(pid), where = `player ${pid}`;
    const f = info.initFields.slice(0, 12);
    f[9] = f[10] = f[11] = 0;
    for (let k = 0; k < 9; k++) {
      const name = names[k];
      if (!name || !(name in rec)) continue;
      const val = rec[name];
      if (ww && k === 0) {
        if (typeof val !== 'string') throw new TypeError(`${where}: field '${name}': ${JSON.stringify(val)} is not a string`);
        if (!roles.includes(val)) throw new RangeError(`${where}: field '${name}': unknown role ${JSON.stringify(val)} (the DSL declares ${JSON.stringify(roles.slice(1))})`);
        f[k] = roles.indexOf(val);
      } else if (ww && k === 1) {
        if (typeof val !== 'string') throw new TypeError(`${where}: field '${name}': ${JSON.stringify(val)} is not a string`);
        if (!TEAMS.includes(val)) throw new RangeError(`${where}: field '${name}': team ${JSON.stringify(val)} is not one of ${JSON.stringify(TEAMS)}`);
        f[k] = TEAMS.indexOf(val);
      } else if (k in ints) {
        const hi = ints[k] === null ? n : ints[k];
        if (!isInt(val)) throw new TypeError(`${where}: field '${name}': ${JSON.stringify(val)} is not an integer`);
        if (val < 0 || val > hi) throw new RangeError(`${where}: field '${name}': ${val} is not an integer in 0..${hi}`);
        f[k] = val;
      } else {
        if (typeof val !== 'boolean') throw new TypeError(`${where}: field '${name}': ${JSON.stringify(val)} is not a boolean`);
        f[k] = val ? 1 : 0;
      }
    }
    u8.set(f, row(pid - 1));
    if (ww && names[9] && names[9] in rec) {
      const field = names[9], mem = rec[field];
      if (!isDict(mem)) throw new TypeError(`${where}: field '${field}' must be an object`);
      if (Object.keys(mem).length && f[0] !== 4) throw new RangeError(`${where}: field '${field}': only the ${roles[4]} holds investigation results`);
      for (const [q, team] of Object.entries(mem)) {
        const qi = Number(q);
        if (!(Number.isInteger(qi) && qi >= 1 && qi <= n) || (team !== 'villagers' && team !== 'werewolves'))
          throw new RangeError(`${where}: field '${field}': entry ${JSON.stringify(q)}: ${JSON.stringify(team)} must name a player 1..${n} and a team`);
        u8[VIEW.det + qi - 1] = TEAMS.indexOf(team);
      }
    }
    host.names[String(pid)] = rec.name === undefined ? `Player ${pid}` : rec.name;
    if (!ww && names[9]) {
      const st = rec[names[9]] === undefined ? {} : rec[names[9]];
      if (!isDict(st)) throw new TypeError(`${where}: field '${names[9]}' must be an object`);
      host.statements[String(pid)] = Object.assign({}, st);
    }
    const extra = {};
    for (const [k, v] of Object.entries(rec)) if (!modelled.has(k)) extra[k] = v;
    if (Object.keys(extra).length) host.extra[String(pid)] = extra;
  }

  // acted / choice: this visit's latest tagged action per player (turns past the one that entered the phase)
  const pa = state.playerActions === undefined || state.playerActions === null ? {} : state.playerActions;
  if (!isDict(pa)) throw new TypeError('playerActions must be an object');
  const curName = table.phaseName(cur);
  const first = s === 0 && cur === 0 ? 0 : s + 1;
  const latest = new Map();
  for (const [pid, t, c] of taggedActions(pa, n, (ph) => ph === curName))
    if (first <= t && t < histIds.length && t >= (latest.has(pid) ? latest.get(pid)[0] : -1)) latest.set(pid, [t, c]);
  const acted = new Map([...latest].map(([pid, [, c]]) => [pid, c]));
  const visit = new Map(Object.entries(visitActions || {}).map(([k, c]) => [Number(k), c]));
  for (const [pid, c] of visit) acted.set(pid, c);
  const top = ww ? n : 3;
  for (const [pid, c] of acted) {
    if (!isInt(c)) throw new TypeError(`player ${pid}: visit action ${JSON.stringify(c)} is not an integer`);
    if (!(pid >= 1 && pid <= n) || c < 1 || c > top) throw new RangeError(`player ${pid}: visit action ${c} is not a choice in 1..${top}`);
    u8[row(pid - 1) + 9] = 1; u8[row(pid - 1) + 10] = c;
  }
  if (ww && !(names[5] && names[7] && names[8])) {
    // slots the DSL leaves undeclared still drive the rules: derived from the role and this night's logged actions
    let since = -1;
    histIds.forEach((pid, t) => {
      const p = phases.find((x) => x.id === pid);
      if (p && p.effect === EFF_NIGHT_BEGIN && (t === 0 || histIds[t - 1] !== pid)) since = t;
    });
    const actOf = new Map(phases.map((p) => [p.name, p.act]));
    const night = new Map();
    for (const [pid, t, c] of taggedActions(pa, n, (ph) => ACT_NIGHT.includes(actOf.get(ph))))
      if (since < t && t < histIds.length && t >= (night.has(pid) ? night.get(pid)[0] : -1)) night.set(pid, [t, c]);
    if (ACT_NIGHT.includes(phases[phaseIds.indexOf(cur)].act)) for (const [pid, c] of visit) night.set(pid, [histIds.length, c]);
    for (let i = 0; i < n; i++) {
      const o = row(i);
      if (!names[5] && u8[o] >= 2) u8[o + 5] = 1;
      if (night.has(i + 1)) {
        if (!names[7]) u8[o + 7] = 1;
        if (!names[8]) u8[o + 8] = night.get(i + 1)[1];
      }
    }
  }

  // self-check: every modelled field reads back as given
  const back = decodeRoom(table, buf, 0).player_states;
  for (let pid = 1; pid <= n; pid++) {
    const rec = byId.get(pid), got = back[String(pid)];
    names.forEach((name, k) => {
      if (!name || !(name in rec) || !(name in got)) return;
      let want = rec[name];
      if (ww && k === 9) { const w = {}; for (const [q, t] of Object.entries(want)) w[String(q)] = t; want = w; }
      const g = got[name];
      const eq = isDict(want) ? (isDict(g) && sameValue(Object.entries(g).sort(), Object.entries(want).sort())) : g === want;
      if (!eq) throw new RangeError(`player ${pid}: field '${name}' = ${JSON.stringify(want)} does not fit the record (it reads back as ${JSON.stringify(g)})`);
    });
  }
  return { view: buf, hostSide: host };
}

const EVENT_SIZE = 32;

function actionText(act, player, c) {
  if (act === 1 || act === 4) return `voted to eliminate Player ${c}`;
  if (act === 2) return `chose to protect Player ${c}`;
  if (act === 3) return `investigated Player ${c}`;
  if (act === 5) return 'shared three statements: ' + [1, 2, 3].map((s) => `'Statement ${s} of Player ${player}'`).join(', ');
  if (act === 6) return `chose statement ${c} as the lie`;
  return `voted that statement ${c} is the lie`;
}

// add_game_note's categories and their marks (agent/tools/backend_tools.py:175-187; unknown type -> the EVENT mark)
const NOTE_EMOJI = { CRITICAL: '\u{1F534}', VOTING_STATUS: '⚠️', DECISION: '\u{1F3AF}', BOT_REMINDER: '\u{1F916}', UI_FILTER: '\u{1F6AB}',
                     PHASE_STATUS: '⏳', NEXT_PHASE: '\u{1F52E}', GAME_STATUS: '\u{1F3C6}', PHASE_SUGGESTION: '\u{1F4A1}',
                     BRANCH_RECOMMENDATION: '\u{1F500}', EVENT: '\u{1F4DD}' };
/** What _execute_add_game_note appends (bt:188-198). */
function formatNote(noteType, content) {
  const prefix = `${NOTE_EMOJI[noteType] || NOTE_EMOJI.EVENT} ${noteType}:`;
  return content.startsWith(prefix) ? content : `${prefix} ${content}`;
}

function plurality(votes, n) {
  let best = 0, bestC = 0;
  for (let k = 1; k <= n; k++) {
    const c = votes.filter((v) => v === k).length;
    if (c > bestC) { best = k; bestC = c; }
  }
  return best;
}

/**
 * One stepped turn of one room as the reference's backend tool calls
 * (agent/tools/backend_tools.py:10-157), in node order: update_player_actions* ->
 * set_next_phase -> update_player_state* -> add_game_note*.  Same rendering as the Python host
 * (game_engine_amd/toolcalls.py); applying the calls to the reference's dict state reproduces
 * the GPU state, and the notes are the fixed policy's (pinned by tests/golden/strings_*.json).
 * `before`/`after`: RoomState; `event`: from RoomBatch.readEvents().
 */
function turnToolCalls(table, before, after, event) {
  const calls = [];
  const ids = Object.keys(after.player_states).sort((a, b) => Number(a) - Number(b));
  const n = ids.length;
  const from = table.info.phases.find((x) => x.id === event.from_phase_id);
  const to = table.info.phases.find((x) => x.id === event.to_phase_id);
  ids.forEach((pid, i) => {
    if ((event.acted_now >> i) & 1) {
      const c = event.choice[i];
      calls.push({ name: 'update_player_actions', args: { player_id: pid, actions: `[t=${event.turn}|c=${c}] ${actionText(from.act, i + 1, c)}`, phase: from.name } });
    }
  });
  const moved = event.to_phase_id !== event.from_phase_id;
  calls.push({ name: 'set_next_phase', args: { transition: moved, next_phase_id: event.to_phase_id, transition_reason: moved ? 'phase complete' : 'waiting' } });
  const deaths = [];
  const names = table.info.fieldNames;
  const SA = after.slots, SB = before.slots;                      // slot values (WW: 0 role, 2 is_alive, 8 target; TT: 0 speaker, 1 submitted, 7 score)
  const ww = after.pack === 1;
  ids.forEach((pid, i) => {
    const b = before.player_states[pid], a = after.player_states[pid];
    for (const name of Object.keys(a)) {
      if (JSON.stringify(b[name]) !== JSON.stringify(a[name])) calls.push({ name: 'update_player_state', args: { player_id: pid, state_name: name, state_value: a[name] } });
    }
    if (ww && SB[i][2] && !SA[i][2]) deaths.push([pid, SA[i][0]]);
    if (!ww && names[9]) {                                         // `statements`: text the record does not carry
      if (SA[i][1] && !SB[i][1]) {
        const st = {}; [1, 2, 3].forEach((s) => { st[String(s)] = `Statement ${s} of Player ${i + 1}`; });
        calls.push({ name: 'update_player_state', args: { player_id: pid, state_name: names[9], state_value: st } });
      } else if (SB[i][1] && !SA[i][1]) {
        calls.push({ name: 'update_player_state', args: { player_id: pid, state_name: names[9], state_value: {} } });
      }
    }
  });
  if (!moved) return calls;
  const note = (kind, text) => calls.push({ name: 'add_game_note', args: { note_type: kind, content: text } });
  note('PHASE_STATUS', `[t=${event.turn}] phase ${event.from_phase_id} -> ${event.to_phase_id}`);
  if (to.effect === 1) {                                          // GE_EFF_ASSIGN_ROLES
    note('NEXT_PHASE', 'Roles assigned: ' + SA.map((p, i) => `Player${i + 1}=${p[0]}`).join(', '));
  } else if (to.effect === 3 || to.effect === 4) {               // NIGHT_RESOLVE / DAY_RESOLVE
    const how = to.effect === 3 ? 'overnight by the werewolves' : 'by day vote';
    deaths.forEach(([pid, role]) => note('CRITICAL', `Player ${pid} (${role}) eliminated ${how} - marked is_alive=false`));
    if (to.effect === 3 && !deaths.length) {
      const roles = table.info.roleNames;                        // class 2 = Werewolf, 3 = Doctor
      const victim = plurality(SA.filter((p, i) => SB[i][2] && SB[i][0] === roles[2]).map((p) => p[8]), n);
      let protect = 0;
      SA.forEach((p, i) => { if (SB[i][2] && SB[i][0] === roles[3]) protect = p[8]; });
      note('DECISION', `Werewolves targeted Player ${victim}, Doctor protected Player ${protect} - no elimination`);
    }
  } else if (to.effect === 5) {                                   // TT_ROUND_START
    const sp = SA.findIndex((p) => p[0]);
    note('DECISION', `Selected Player ${sp + 1} as next speaker (turn_order)`);
  } else if (to.effect === 7) {                                   // TT_SCORE
    if (SB.some((p) => p[0])) note('SCORE_UPDATE', 'Total scores - ' + SA.map((p, i) => `Player ${i + 1}: ${p[7]}`).join(', '));
  }
  return calls;
}

/**
 * The log-shaped parts of one room's AgentState that the packed state does not carry - playerActions
 * (bt:285-344), game_notes (bt:163-202), phase_history (v2:1207-1215), the Two-Truths `statements` texts
 * and the players' names - kept by folding each turn's tool calls as the reference's `_execute_*` would.
 */
class RoomLog {
  constructor(table, names, gameName = '') {
    this.table = table; this.names = names.slice(); this.gameName = gameName;
    this.playerActions = {}; this.gameNotes = []; this.phaseHistory = []; this.statements = {};
    this.extra = {};               // per player: fields the record does not model (an adopted thread's)
  }
  /** Seed the log of a thread handed over mid-game: its playerActions, game_notes and phase_history, and the host-side fields
   * agentStateToView returned (names, statements, fields the record does not model). */
  adopt(state, hostSide) {
    const copy = (x) => JSON.parse(JSON.stringify(x === undefined || x === null ? null : x));
    this.playerActions = copy(state.playerActions) || {};
    this.gameNotes = copy(state.game_notes) || [];
    this.phaseHistory = copy(state.phase_history) || [];
    this.names = this.names.map((nm, i) => (hostSide.names[String(i + 1)] !== undefined ? hostSide.names[String(i + 1)] : nm));
    this.statements = copy(hostSide.statements) || {};
    this.extra = copy(hostSide.extra) || {};
  }
  /** Apply one turn's calls; `after`: the RoomState after the turn. */
  fold(calls, after, now = Date.now()) {
    for (const c of calls) {
      const a = c.args;
      if (c.name === 'update_player_actions') {
        const pid = a.player_id;
        const rec = this.playerActions[pid] || (this.playerActions[pid] = { name: this.names[Number(pid) - 1], actions: {} });
        const id = String(Object.values(rec.actions).reduce((m, x) => Math.max(m, Number(x.id)), 0) + 1);   // per-player sequence, bt:323-332
        rec.name = this.names[Number(pid) - 1];
        rec.actions[id] = { action: a.actions, timestamp: now, phase: a.phase, id };
      } else if (c.name === 'add_game_note') {
        this.gameNotes.push(formatNote(a.note_type, a.content));
      } else if (c.name === 'update_player_state' && this.table.info.pack === 2 && a.state_name === this.table.info.fieldNames[9]) {
        this.statements[a.player_id] = Object.assign({}, a.state_value);
      }
    }
    this.phaseHistory.push({ phase_id: after.current_phase_id, phase_name: after.current_phase_name, timestamp: new Date(now).toISOString() });   // every turn, v2:1207-1215
  }
  /** File a person's game message as process_human_action_if_needed does (agent/tools/utils.py:343-350): under Player 1,
   * the first 200 characters, and under PHASE 0's NAME whatever the current phase is (InitialRouterNode passes state keys that
   * do not exist, agent/game_agent_v2.py:324-331) - mirrored, not corrected (POLICY.md 3b). */
  personMessage(text, now = Date.now()) {
    const rec = this.playerActions['1'] || (this.playerActions['1'] = { name: this.names[0], actions: {} });
    const id = String(Object.values(rec.actions).reduce((m, x) => Math.max(m, Number(x.id)), 0) + 1);
    rec.name = this.names[0];
    rec.actions[id] = { action: Array.from(String(text)).slice(0, 200).join(''), timestamp: now, phase: this.table.phaseName(0), id };
  }
  /** AgentState of the room (v2:97-117), player_states in the reference's key order. */
  agentState(room) {
    const ps = {};
    Object.keys(room.player_states).forEach((pid, i) => {
      const out = { name: this.names[i] };
      for (const [k, v] of Object.entries(room.player_states[pid])) {
        out[k] = v;
        const fn = this.table.info.fieldNames;
        if (this.table.info.pack === 2 && k === fn[0] && fn[9]) out[fn[9]] = Object.assign({}, this.statements[pid] || {});
      }
      Object.assign(out, this.extra[pid] || {});
      ps[pid] = out;
    });
    return { gameName: this.gameName, current_phase_id: room.current_phase_id, current_phase_name: room.current_phase_name,
             player_states: ps, playerActions: this.playerActions, phase_history: this.phaseHistory, game_notes: this.gameNotes };
  }
}

// include/ge_step.h GE_RUN_UNTIL_*
const RUN_UNTIL = { person: 1, end: 2, phase: 4 };
// an array of names of `names`, one of them, or the bits themselves, as the ABI's bit set
function namedBits(value, names, what) {
  if (typeof value === 'number') return value;
  let bits = 0;
  for (const name of typeof value === 'string' ? [value] : value) {
    if (!Object.prototype.hasOwnProperty.call(names, name)) throw new RangeError(`${what} ${JSON.stringify(name)}`);
    bits |= names[name];
  }
  return bits;
}
/** `until` of runRooms / runRoom as the ABI's bit set: an array of "person" / "end" / "phase", one of them, or the bits. */
function runUntilBits(until) { return namedBits(until, RUN_UNTIL, 'until: unknown stop condition'); }
function runUntilNames(bits) { return Object.keys(RUN_UNTIL).filter((name) => bits & RUN_UNTIL[name]); }

// include/ge_step.h GE_FIND_*
const FIND_WANT = { person: 1, end: 2, phase: 4 };
const ADVICE_SIZE = 224;                                     // sizeof(ge_advice): 16 B header, policy, option[12] (16 B each)
/** n ge_advice records as adviseSeats returns them. */
function decodeAdvice(buf) {
  const dv = new DataView(buf), out = [];
  const option = (at) => ({ finished: dv.getUint32(at, true), wins: dv.getUint32(at + 4, true), score: Number(dv.getBigUint64(at + 8, true)) });
  for (let k = 0; k * ADVICE_SIZE < buf.byteLength; k++) {
    const at = k * ADVICE_SIZE, bits = dv.getUint32(at + 4, true), legal = [], options = [];
    for (let c = 1; c <= 12; c++) {
      if (!((bits >>> (c - 1)) & 1)) continue;
      legal.push(c);
      options.push({ choice: c, ...option(at + 32 + 16 * (c - 1)) });
    }
    out.push({ status: dv.getInt32(at, true), legal, best: dv.getUint32(at + 8, true), phaseId: dv.getUint32(at + 12, true), policy: option(at + 16), options });
  }
  return out;
}
/** `want` of findRooms as the ABI's bit set: an array of "person" / "end" / "phase", one of them, or the bits. */
function findWantBits(want) { return namedBits(want, FIND_WANT, 'want: unknown condition'); }
function findWantNames(bits) { return Object.keys(FIND_WANT).filter((name) => bits & FIND_WANT[name]); }

function decodeEvent(buffer, off) {
  const dv = new DataView(buffer, off, EVENT_SIZE);
  return { turn: dv.getUint32(0, true), from_phase_id: dv.getInt32(4, true), to_phase_id: dv.getInt32(8, true),
           acted_now: dv.getUint16(12, true), restarted: dv.getUint8(14), choice: Array.from(new Uint8Array(buffer, off + 16, 16)) };
}

class RoomBatch {
  /** segments: [{table: GameTable, nPlayers, nRooms}] */
  constructor({ segments, seed = 0n, firstRoom = 0n, device = 0, maxFuse = 0, restart = false, trace = false }) {
    this.segments = segments;
    this.seed = BigInt(seed);
    this.handle = addon.createBatch({
      seed, firstRoom, device, maxFuse, restart, trace,
      segments: segments.map((s) => ({ table: s.table.handle, nPlayers: s.nPlayers, nRooms: s.nRooms, humanMask: s.humanMask || 0 })),
    });
    this.nRooms = segments.reduce((a, s) => a + s.nRooms, 0);
    this._tail = Promise.resolve();     // async steps of one handle run strictly one after the other
  }
  /** Advance every room by nTurns turns; resolves with the batch's turn counter.  The C handle is not
   * thread-safe: async steps of one batch are chained, and any synchronous call (readRoom, injectAction,
   * summary ...) made while one is in flight throws GE_BUSY instead of racing with the worker thread —
   * `await` the step, or queue the call with `whenIdle`. */
  step(nTurns = 1) {
    const p = this._tail.then(() => addon.step(this.handle, nTurns));
    this._tail = p.catch(() => {});
    return p;
  }
  /** Runs fn() once every step queued so far has finished (and before any queued later). */
  whenIdle(fn) {
    const p = this._tail.then(fn);
    this._tail = p.catch(() => {});
    return p;
  }
  stepSync(nTurns = 1) { return addon.stepSync(this.handle, nTurns); }
  reset() { addon.reset(this.handle); }
  /** Restore a checkpoint: room records (readRoomsRaw's ArrayBuffer) and the turn they were taken at. */
  writeRoomsRaw(first, buffer) { addon.writeRooms(this.handle, first, buffer); }
  readRoomsRaw(first, count) { return addon.readRooms(this.handle, first, count); }
  setTurn(turn) { addon.setTurn(this.handle, turn); }
  /** Releases the device memory now (otherwise at garbage collection). */
  close() { if (this.handle) { addon.destroyBatch(this.handle); this.handle = null; } }
  /** Log an action of a host-driven (human) player in the room's current phase (segment.humanMask). */
  injectAction(room, playerId, choice) { addon.injectAction(this.handle, room, playerId, choice); }
  /** Many at once (one kernel): rooms[], playerIds[], choices[] -> Int32Array of per-action status (0 = applied). */
  injectActions(rooms, playerIds, choices) {
    return addon.injectActions(this.handle, BigUint64Array.from(rooms, (r) => BigInt(r)), Uint32Array.from(playerIds), Uint32Array.from(choices));
  }
  tableOf(room) {
    let base = 0;
    for (const s of this.segments) { if (room < base + s.nRooms) return s.table; base += s.nRooms; }
    throw new RangeError(`room ${room}`);
  }
  /** AgentState-shaped view of one room (agent/game_agent_v2.py:97-117). */
  readRoom(room) { return decodeRoom(this.tableOf(room), addon.readRooms(this.handle, room, 1), 0); }
  readRooms(first, count) {
    const buf = addon.readRooms(this.handle, first, count);
    const out = [];
    for (let i = 0; i < count; i++) out.push(decodeRoom(this.tableOf(first + i), buf, i * VIEW.size));
    return out;
  }
  /** [room][turn] events of the most recent step() (batch created with trace: true). */
  readEvents(first, count) {
    const { nTurns, buffer } = addon.readEvents(this.handle, first, count);
    const out = [];
    for (let r = 0; r < count; r++) {
      const row = [];
      for (let t = 0; t < nTurns; t++) row.push(decodeEvent(buffer, (r * nTurns + t) * EVENT_SIZE));
      out.push(row);
    }
    return out;
  }
  /** One turn of each listed room (local indices, pairwise distinct), room k keyed as global room keys[k] at turn turns[k]
   * (what a lone batch with firstRoom = keys[k] and turn counter turns[k] does to it in one step); the batch's turn counter,
   * its trace and every unlisted room are untouched.  Returns event k of room k (readEvents' event shape).  Synchronous. */
  stepRooms(rooms, keys, turns) {
    const { buffer } = addon.stepRooms(this.handle, BigUint64Array.from(rooms, (r) => BigInt(r)), BigUint64Array.from(keys, (k) => BigInt(k)),
                                       Uint32Array.from(turns));
    const out = [];
    for (let k = 0; k < rooms.length; k++) out.push(decodeEvent(buffer, k * EVENT_SIZE));
    return out;
  }
  /** stepRooms with playout seats (twin of the Python RoomBatch.step_rooms_playout, POLICY.md §3d): bit i of masks[k] makes seat
   * i+1 of room k a playout bot, which - when the policy has it act with at least 2 candidates - takes the candidate whose
   * rolloutSeats entry (room k as it stands, playoutKeys[k], turns[k], the seat or 0 with fullView, that one action, nRollouts,
   * maxTurns, seed) has the most seat_wins of the seat; ties go to the policy's own pick among the tied.  Returns
   * { events, decided }: stepRooms's events (the decided seats listed as acted) and decided[k] (bit i = seat i+1 chose by
   * playouts).  halving (GE_PLAYOUT_HALVING, POLICY.md §3h): a seat's candidates are valued in ceil(log2 c) rounds of growing
   * replica ranges, the worse half leaving after each - fewer playouts, more launches per turn, and slower at every shape measured on an MI355X (x 0.38 .. 0.71 of the unflagged call's speed).
   * All-or-nothing.  Synchronous. */
  stepRoomsPlayout(rooms, keys, turns, masks, playoutKeys, nRollouts, maxTurns = 256, seed, fullView = false, halving = false) {
    const { buffer, decided } = addon.stepRoomsPlayout(this.handle, BigUint64Array.from(rooms, (r) => BigInt(r)),
      BigUint64Array.from(keys, (k) => BigInt.asUintN(64, BigInt(k))), Uint32Array.from(turns), Uint32Array.from(masks),
      BigUint64Array.from(playoutKeys, (k) => BigInt.asUintN(64, BigInt(k))), nRollouts, maxTurns,
      seed === undefined ? this.seed : BigInt.asUintN(64, BigInt(seed)), (fullView ? 1 : 0) | (halving ? 4 : 0));
    const events = [];
    for (let k = 0; k < rooms.length; k++) events.push(decodeEvent(buffer, k * EVENT_SIZE));
    return { events, decided };
  }
  /** Play each listed room on until a person is needed (twin of the Python RoomBatch.run_rooms, POLICY.md §3f): room k takes
   * stepRooms's entries (rooms[k], keys[k], turns[k] + t), t = 0, 1, ..., and stops after the first turn that leaves it in a state
   * named in `until` - "person": a host-driven seat of its segment is a pending target (an injectAction of it would be accepted);
   * "end": a terminal phase; "phase": the turn moved the phase - or after maxTurns turns; the first turn is always played.  `until`
   * is an array of those names or the ABI's bit set.  Returns { played, stopped, events, views }: played[k] turns were played,
   * stopped[k] has the RUN_UNTIL bits that held after the last one (0: the limit), events[k] / views[k] hold one stepRooms event
   * and one readRoomsAt state per played turn (views: false -> null).  All-or-nothing like stepRooms; maxTurns outside 1 .. 4096,
   * rooms.length * maxTurns above 2^20 or turns[k] + maxTurns above 0xFFFFFFFF throw and run nothing.  Synchronous; GE_BUSY while
   * an async step() is in flight. */
  runRooms(rooms, keys, turns, maxTurns = 64, until = ['person', 'end'], views = true) {
    const bits = runUntilBits(until);
    const r = addon.runRooms(this.handle, BigUint64Array.from(rooms, (x) => BigInt(x)), BigUint64Array.from(keys, (k) => BigInt.asUintN(64, BigInt(k))),
                             Uint32Array.from(turns), maxTurns, bits, !!views);
    const events = [], states = views ? [] : null;
    for (let k = 0; k < rooms.length; k++) {
      const ev = [], vw = [];
      for (let t = 0; t < r.played[k]; t++) {
        ev.push(decodeEvent(r.events, (k * maxTurns + t) * EVENT_SIZE));
        if (views) vw.push(decodeRoom(this.tableOf(Number(rooms[k])), r.views, (k * maxTurns + t) * VIEW.size));
      }
      events.push(ev);
      if (views) states.push(vw);
    }
    return { played: r.played, stopped: r.stopped, events, views: states };
  }
  /** The rooms of first .. first + count - 1 that need attention, as they stand (twin of the Python RoomBatch.find_rooms, POLICY.md
   * §3k; the batch is only read).  want: an array of "person" (a host-driven seat of the room's segment is a pending target:
   * runRooms's test), "end" (a terminal phase) and "phase" (the room's phase id is in `phases`), or the ABI's bit set.  phases: an
   * array of phase ids for every segment, or an object segment -> array; it requires "phase" in want.  Returns { hits, matched }:
   * hits are the first min(matched, cap) matches in ascending room order, each { room, why: [names], pending: [seats that could act
   * now], phaseId, segment }; matched counts every match of the range.  count undefined: to the end of the batch; cap undefined:
   * count; cap 0 counts only.  A truncated scan goes on from first = last hit's room + 1.  Synchronous; GE_BUSY while an async
   * step() is in flight. */
  findRooms({ want = ['person', 'end'], phases = null, first = 0, count, cap } = {}) {
    const bits = findWantBits(want);
    let masks = null;
    if (phases !== null && phases !== undefined) {
      if (!(bits & FIND_WANT.phase)) throw new RangeError('findRooms: phases requires "phase" in want');
      masks = new Uint32Array(4);                              // GE_MAX_SEGMENTS
      for (let g = 0; g < this.segments.length; g++) {
        for (const pid of Array.isArray(phases) ? phases : (phases[g] || [])) {
          if (!Number.isInteger(pid) || pid < 0 || pid >= 32) throw new RangeError(`findRooms: phase id ${pid}`);
          masks[g] = (masks[g] | (1 << pid)) >>> 0;
        }
      }
    }
    const n = count === undefined ? this.nRooms - first : count;
    const r = addon.findRooms(this.handle, first, n, bits, masks, cap === undefined ? n : cap);
    const dv = new DataView(r.hits), hits = [];
    for (let k = 0; k < r.nHits; k++) {
      const pending = dv.getUint16(16 * k + 12, true), seats = [];
      for (let i = 0; i < 12; i++) if ((pending >> i) & 1) seats.push(i + 1);
      hits.push({ room: Number(dv.getBigUint64(16 * k, true)), why: findWantNames(dv.getUint32(16 * k + 8, true)), pending: seats,
                  phaseId: dv.getUint8(16 * k + 14), segment: dv.getUint8(16 * k + 15) });
    }
    return { hits, matched: r.matched };
  }
  /** Advice for listed seats, found, played and ranked on the device (twin of the Python RoomBatch.advise_seats, POLICY.md §3m).
   * Entry k is seat seats[k] (1-based, any seat: no human mask is consulted) of room rooms[k].  Returns one object per entry:
   * { status, legal: [choices injectAction would accept now], best, phaseId, policy: { finished, wins, score }, options: [{ choice,
   * finished, wins, score }] } - an option's three numbers are summary.finished, seat_wins[seat-1] and seat_score[seat-1] of
   * rolloutSeats's entry (rooms[k], keys[k], turns[k], the seat or 0 with fullView, [[seat, choice]]; nRollouts, maxTurns, seed),
   * policy the same of that entry without actions, best the legal choice with the most wins (Werewolf) or the highest score
   * (Two-Truths), the lowest on a tie.  A seat that could not act now has status -1 (GE_ERR_ARG), no options and zeros: an answer,
   * not an error.  Throws only for a structural error, before anything runs.  The batch is only read.  Synchronous; GE_BUSY while
   * an async step() is in flight. */
  adviseSeats(rooms, keys, turns, seats, nRollouts, maxTurns = 1024, seed, fullView = false) {
    if (rooms.length !== keys.length || rooms.length !== turns.length || rooms.length !== seats.length) throw new RangeError('adviseSeats: arrays differ in length');
    const buf = addon.adviseSeats(this.handle, BigUint64Array.from(rooms, (r) => BigInt(r)), BigUint64Array.from(keys, (k) => BigInt.asUintN(64, BigInt(k))),
                                  Uint32Array.from(turns), Uint32Array.from(seats), nRollouts, maxTurns,
                                  seed === undefined ? this.seed : BigInt.asUintN(64, BigInt(seed)), fullView ? 1 : 0);
    return decodeAdvice(buf);
  }
  /** Per-room host-driven seats (twin of the Python RoomBatch.set_seats, POLICY.md §3l): masks[k] (bit i = seat i + 1 is host-driven)
   * becomes the seat mask of room rooms[k] (local indices, pairwise distinct).  From then on step, stepRooms, the run-ons, findRooms
   * and the playout-seat check honour the room's own mask instead of its segment's.  All-or-nothing: a room outside the batch, a
   * repeated room or a mask bit at or above the room's player count throws and changes nothing.  The mask is configuration: reset,
   * record writes and restarts leave it; a change takes effect with the next turn played.  Synchronous; GE_BUSY while an async
   * step() is in flight. */
  setSeats(rooms, masks) {
    if (rooms.length !== masks.length) throw new RangeError('setSeats: rooms and masks differ in length');
    addon.setSeats(this.handle, BigUint64Array.from(rooms, (r) => BigInt(r)), Uint32Array.from(masks));
  }
  /** The seat masks of rooms first .. first + count - 1 as a Uint32Array (the segment's mask where none was ever set); count
   * undefined: to the end of the batch.  Synchronous; GE_BUSY while an async step() is in flight. */
  seats(first = 0, count) {
    return addon.seats(this.handle, first, count === undefined ? this.nRooms - first : count);
  }
  /** Every room back to its segment's mask; the seat plane is freed.  Synchronous; GE_BUSY while an async step() is in flight. */
  clearSeats() {
    addon.clearSeats(this.handle);
  }
  /** runRooms with playout seats (twin of the Python RoomBatch.run_rooms_playout, POLICY.md §3g): room k takes stepRoomsPlayout's
   * entries (rooms[k], keys[k], turns[k] + t, masks[k], playoutKeys[k]; nRollouts, playoutMaxTurns, seed, fullView), t = 0, 1, ...,
   * and stops as runRooms stops it; between the turns of the call the host does not wait for the device.  Returns { played, stopped,
   * events, views, decided }: the first four as runRooms returns them, events being stepRoomsPlayout's (the decided seats listed as
   * acted); decided[k][t] is turn t's decided mask.  All-or-nothing: runRooms's checks, then stepRoomsPlayout's, with the cost cap
   * per turn and turns[k] + maxTurns - 1 + playoutMaxTurns within 0xFFFFFFFF.  halving: every turn's decisions as
   * stepRoomsPlayout's under it.  Synchronous; GE_BUSY while an async step() is in flight. */
  runRoomsPlayout(rooms, keys, turns, masks, playoutKeys, nRollouts, playoutMaxTurns = 256, seed, fullView = false, maxTurns = 64,
                  until = ['person', 'end'], views = true, halving = false) {
    const bits = runUntilBits(until);
    const r = addon.runRoomsPlayout(this.handle, BigUint64Array.from(rooms, (x) => BigInt(x)), BigUint64Array.from(keys, (k) => BigInt.asUintN(64, BigInt(k))),
                                    Uint32Array.from(turns), Uint32Array.from(masks), BigUint64Array.from(playoutKeys, (k) => BigInt.asUintN(64, BigInt(k))),
                                    nRollouts, playoutMaxTurns, seed === undefined ? this.seed : BigInt.asUintN(64, BigInt(seed)),
                                    (fullView ? 1 : 0) | (halving ? 4 : 0), maxTurns, bits, !!views);
    const events = [], states = views ? [] : null, decided = [];
    for (let k = 0; k < rooms.length; k++) {
      const ev = [], vw = [];
      for (let t = 0; t < r.played[k]; t++) {
        ev.push(decodeEvent(r.events, (k * maxTurns + t) * EVENT_SIZE));
        if (views) vw.push(decodeRoom(this.tableOf(Number(rooms[k])), r.views, (k * maxTurns + t) * VIEW.size));
      }
      events.push(ev);
      if (views) states.push(vw);
      decided.push(Array.from(r.decided.subarray(k * maxTurns, k * maxTurns + r.played[k])));
    }
    return { played: r.played, stopped: r.stopped, events, views: states, decided };
  }
  /** runRooms with a forecast of every turn it played (twin of the Python RoomBatch.run_rooms_forecast, POLICY.md §3i): played,
   * stopped, events and views are runRooms's for the same (rooms, keys, turns, maxTurns, until), and stats[k][p], p = 0 ..
   * played[k], is a BigUint64Array of the 77 rolloutSeats words of room k as it stood at point p - point 0 before the call, point p
   * after its turn p - 1 - under (forecastKeys[k], turns[k] + p, seats[k], no actions; nRollouts, playoutMaxTurns, seed).  seats
   * null: the full view for every entry; seed undefined: the batch's.  All-or-nothing: runRooms's checks, then 1 <= nRollouts <=
   * 2^20, playoutMaxTurns <= 4096, n * (maxTurns + 1) <= 2^16, n * (maxTurns + 1) * nRollouts <= 2^26, seats within their rooms'
   * player counts, turns[k] + maxTurns + playoutMaxTurns within 0xFFFFFFFF.  Synchronous; GE_BUSY while an async step() is in flight. */
  runRoomsForecast(rooms, keys, turns, forecastKeys, nRollouts, playoutMaxTurns = 1024, seats = null, seed, maxTurns = 64, until = ['person', 'end']) {
    const bits = runUntilBits(until);
    const r = addon.runRoomsForecast(this.handle, BigUint64Array.from(rooms, (x) => BigInt(x)), BigUint64Array.from(keys, (k) => BigInt.asUintN(64, BigInt(k))),
                                     Uint32Array.from(turns), BigUint64Array.from(forecastKeys, (k) => BigInt.asUintN(64, BigInt(k))),
                                     seats == null ? new Uint32Array(rooms.length) : Uint32Array.from(seats), nRollouts, playoutMaxTurns,
                                     seed === undefined ? this.seed : BigInt.asUintN(64, BigInt(seed)), maxTurns, bits);
    const events = [], states = [], stats = [];
    for (let k = 0; k < rooms.length; k++) {
      const ev = [], vw = [], fc = [];
      for (let t = 0; t < r.played[k]; t++) {
        ev.push(decodeEvent(r.events, (k * maxTurns + t) * EVENT_SIZE));
        vw.push(decodeRoom(this.tableOf(Number(rooms[k])), r.views, (k * maxTurns + t) * VIEW.size));
      }
      for (let p = 0; p <= r.played[k]; p++) fc.push(r.stats.subarray(77 * (k * (maxTurns + 1) + p), 77 * (k * (maxTurns + 1) + p + 1)));
      events.push(ev); states.push(vw); stats.push(fc);
    }
    return { played: r.played, stopped: r.stopped, events, views: states, stats };
  }
  /** Playouts (twin of the Python RoomBatch.rollout_rooms): entry k is played nRollouts times from room rooms[k] as it stands,
   * replica r as global room keys[k] + r (mod 2^64) under `seed` (default: the batch's) at turns turns[k] .. turns[k] + maxTurns - 1,
   * every seat played by the policy and a finished game left finished.  Returns a BigUint64Array of rooms.length x 77 words
   * (ge_rollout_stats: the 41 summary words, then seat_alive, seat_wins, seat_score x 12).  The batch is only read.  Synchronous. */
  rolloutRooms(rooms, keys, turns, nRollouts, maxTurns = 1024, seed) {
    return this._rollout(rooms, keys, turns, null, null, nRollouts, maxTurns, seed).words;
  }
  /** Playouts after given actions (twin of the Python RoomBatch.rollout_actions): entry k is rolloutRooms's entry (rooms[k], keys[k],
   * turns[k]) with actions[k], an array of [playerId, choice] pairs, logged in every replica, in that order, before its first turn.
   * Legality is decided per entry on the device.  Returns { words: BigUint64Array of rooms.length x 77, status: Int32Array }:
   * status[k] = 0 and entry k's ge_rollout_stats, or the refused action's status (< 0) and 77 zero words.  Throws only for a
   * structural error (rolloutRooms's caps, more than 12 actions in one entry).  The batch is only read.  Synchronous. */
  rolloutActions(rooms, keys, turns, actions, nRollouts, maxTurns = 1024, seed) {
    return this._rollout(rooms, keys, turns, null, Array.from(actions), nRollouts, maxTurns, seed);
  }
  /** Playouts from a seat's view (twin of the Python RoomBatch.rollout_seats, POLICY.md §3c): rolloutActions's entry k with every
   * replica's copy re-dealt, after the actions, over what seat seats[k] (1-based) cannot see; seats[k] = 0: the full view,
   * rolloutActions's entry word for word.  actions may be omitted (null: no actions).  Returns { words, status } as
   * rolloutActions.  Throws only for a structural error (rolloutActions's, or a seat above its room's player count).  The batch
   * is only read.  Synchronous. */
  rolloutSeats(rooms, keys, turns, seats, actions, nRollouts, maxTurns = 1024, seed) {
    return this._rollout(rooms, keys, turns, Uint32Array.from(seats), actions == null ? null : Array.from(actions), nRollouts, maxTurns, seed);
  }
  /** rolloutSeats with every entry also compared, playout by playout, against its baseline entry (twin of the Python
   * RoomBatch.rollout_compare, POLICY.md §3e): baseline[k] is an index into this call (the same room), subjects[k] the seat
   * (1-based) whose outcome is compared.  Returns { words, status, cmp }: words and status as rolloutSeats for the same entries,
   * cmp a BigUint64Array of 6 words per entry (compared, better, worse, gain, loss, diff_sq of ge_compare_stats; all zero when the
   * entry or its baseline was refused).  At most 65 536 entries.  The batch is only read.  Synchronous. */
  rolloutCompare(rooms, keys, turns, seats, actions, baseline, subjects, nRollouts = 4096, maxTurns = 1024, seed) {
    return this._rollout(rooms, keys, turns, Uint32Array.from(seats), actions == null ? null : Array.from(actions), nRollouts, maxTurns, seed,
                         Uint32Array.from(baseline), Uint32Array.from(subjects));
  }
  /** rolloutSeats - with baseline and subjects, rolloutCompare - under the caller's beliefs (twin of the Python
   * RoomBatch.rollout_beliefs, POLICY.md §3j): beliefs is rooms.length x 16 bytes (a Uint8Array, or an array of 16-byte rows), byte c
   * of entry k how much its caller suspects seat c + 1 of being a werewolf (Werewolf) or statement c + 1 of being the lie
   * (Two-Truths), as prior odds 0 .. 255.  Equal weights give rolloutSeats's entry word for word; nothing in the engine derives
   * the weights.  Returns { words, status }, with baseline and subjects { words, status, cmp }.  Throws only for a structural
   * error (theirs, a non-zero byte at a slot the room does not have, baseline without subjects).  The batch is only read.  Synchronous. */
  rolloutBeliefs(rooms, keys, turns, seats, actions, beliefs, nRollouts = 4096, maxTurns = 1024, seed, baseline = null, subjects = null) {
    const n = Array.from(rooms).length;
    let bel = beliefs;
    if (!(bel instanceof Uint8Array)) {
      const rows = Array.from(beliefs, (r) => Array.from(r));
      if (rows.some((r) => r.length !== BELIEF_SLOTS || r.some((v) => !Number.isInteger(v) || v < 0 || v > 255))) {
        throw new RangeError(`rolloutBeliefs: beliefs must be rows of ${BELIEF_SLOTS} bytes`);
      }
      bel = Uint8Array.from(rows.flat());
    }
    if (bel.length !== n * BELIEF_SLOTS) throw new RangeError(`rolloutBeliefs: beliefs must be ${BELIEF_SLOTS} bytes per entry`);
    if ((baseline == null) !== (subjects == null)) throw new RangeError('rolloutBeliefs: baseline and subjects go together');
    return this._rollout(rooms, keys, turns, Uint32Array.from(seats), actions == null ? null : Array.from(actions), nRollouts, maxTurns, seed,
                         baseline == null ? null : Uint32Array.from(baseline), subjects == null ? null : Uint32Array.from(subjects), bel);
  }
  /** The rollout* methods: one native call (ge_batch_rollout_seats with seats, else ge_batch_rollout_actions with actions -
   * [playerId, choice] pairs per entry, flattened to CSR - else ge_batch_rollout_rooms).  Returns { words, status }. */
  _rollout(rooms, keys, turns, seats, actions, nRollouts, maxTurns, seed, baseline = null, subjects = null, beliefs = null) {
    let first = null, players = null, choices = null;
    if (actions) {
      const acts = actions.map((a) => Array.from(a));
      first = new Uint32Array(acts.length + 1);
      acts.forEach((a, k) => { first[k + 1] = first[k] + a.length; });
      const flat = acts.flat();
      players = Uint32Array.from(flat, (pc) => pc[0]);
      choices = Uint32Array.from(flat, (pc) => pc[1]);
    }
    return addon.rollout(this.handle, BigUint64Array.from(rooms, (r) => BigInt(r)), BigUint64Array.from(keys, (k) => BigInt.asUintN(64, BigInt(k))),
                         Uint32Array.from(turns), seats, first, players, choices, nRollouts, maxTurns, seed === undefined ? this.seed : BigInt(seed),
                         baseline, subjects, beliefs);
  }
  /** The listed rooms' states, out[k] = room rooms[k] (any order, repeats allowed). */
  readRoomsAt(rooms) {
    const buf = this.readRoomsAtRaw(rooms);
    return Array.from(rooms, (r, k) => decodeRoom(this.tableOf(Number(r)), buf, k * VIEW.size));
  }
  readRoomsAtRaw(rooms) { return addon.readRoomsAt(this.handle, BigUint64Array.from(rooms, (r) => BigInt(r))); }
  /** Store views[k] (ArrayBuffers of one room view each, or one ArrayBuffer of rooms.length views) into room rooms[k] (pairwise
   * distinct): one copy and one device scatter, each record exactly as writeRoomsRaw stores it.  All or nothing. */
  writeRoomsAt(rooms, views) {
    let buf = views;
    if (Array.isArray(views)) {
      const u8 = new Uint8Array(VIEW.size * views.length);
      views.forEach((v, k) => u8.set(new Uint8Array(v), k * VIEW.size));
      buf = u8.buffer;
    }
    addon.writeRoomsAt(this.handle, BigUint64Array.from(rooms, (r) => BigInt(r)), buf);
  }
  segmentOf(room) {
    let base = 0;
    for (const s of this.segments) { if (room < base + s.nRooms) return s; base += s.nRooms; }
    throw new RangeError(`room ${room}`);
  }
  /** Adopt a reference AgentState into one room (agentStateToView); returns its host-side fields. */
  writeAgentState(room, state, visitActions) { return this.writeAgentStates([room], [state], visitActions ? [visitActions] : undefined)[0]; }
  /** Many at once: every state is converted (and refused) before one writeRoomsAt. */
  writeAgentStates(rooms, states, visitActions) {
    if (rooms.length !== states.length || (visitActions && visitActions.length !== states.length)) throw new RangeError('rooms, states and visitActions differ in length');
    const conv = states.map((st, k) => {
      const seg = this.segmentOf(Number(rooms[k]));
      return agentStateToView(seg.table, st, { nPlayers: seg.nPlayers, visitActions: visitActions ? visitActions[k] : undefined });
    });
    this.writeRoomsAt(rooms, conv.map((c) => c.view));
    return conv.map((c) => c.hostSide);
  }
  summary() { return decodeSummary(addon.summary(this.handle)); }
}

/**
 * The same rooms spread over several GPUs of one node, from ONE Node process (SURVEY §8e): device d
 * owns the global rooms [firstRoom + d*R, firstRoom + (d+1)*R) with R = rooms per device, so per-room
 * results equal those of a single batch or of any other device count (the RNG is keyed by the global
 * index).  Rooms never interact: step() just runs every shard's launches concurrently (one async
 * work item per shard, each on its own device); the only cross-GPU step is summary(), a host-side
 * sum of the fixed-size per-device summaries (the multi-process Python host does the same sum after
 * one RCCL all-gather, game_engine_amd/dist.py).
 */
class ShardedBatch {
  /** segments: per-device segments (every device gets the same mix); devices: HIP device indices */
  constructor({ segments, devices, seed = 0n, firstRoom = 0n, maxFuse = 0, restart = false, trace = false }) {
    if (!devices || !devices.length) throw new RangeError('devices');
    this.roomsPerDevice = segments.reduce((a, s) => a + s.nRooms, 0);
    this.shards = devices.map((device, d) => new RoomBatch({
      segments, seed, device, maxFuse, restart, trace,
      firstRoom: BigInt(firstRoom) + BigInt(d) * BigInt(this.roomsPerDevice),
    }));
    this.nRooms = this.roomsPerDevice * devices.length;
  }
  async step(nTurns = 1) { return (await Promise.all(this.shards.map((b) => b.step(nTurns))))[0]; }
  reset() { this.shards.forEach((b) => b.reset()); }
  close() { this.shards.forEach((b) => b.close()); }
  shardOf(room) {
    if (!(room >= 0 && room < this.nRooms)) throw new RangeError(`room ${room}`);
    return [this.shards[Math.floor(room / this.roomsPerDevice)], room % this.roomsPerDevice];
  }
  readRoom(room) { const [b, r] = this.shardOf(room); return b.readRoom(r); }
  injectAction(room, playerId, choice) { const [b, r] = this.shardOf(room); b.injectAction(r, playerId, choice); }
  /** whole-job summary: every field is a sum over rooms (checksum: mod 2^64), `turn` is common */
  summary() {
    const parts = this.shards.map((b) => b.summary());
    const add = (f) => BigInt.asUintN(64, parts.reduce((a, p) => a + p[f], 0n));
    const addHist = (f) => parts[0][f].map((_, i) => BigInt.asUintN(64, parts.reduce((a, p) => a + p[f][i], 0n)));
    return {
      rooms: add('rooms'), finished: add('finished'), village_wins: add('village_wins'), wolf_wins: add('wolf_wins'),
      alive_players: add('alive_players'), sum_end_turn: add('sum_end_turn'), end_turn_hist: addHist('end_turn_hist'),
      score_hist: addHist('score_hist'), checksum: add('checksum'), turn: parts[0].turn, games_recycled: add('games_recycled'),
    };
  }
}

function decodeSummary(buffer) {
  const w = new BigUint64Array(buffer);
  return {
    rooms: w[0], finished: w[1], village_wins: w[2], wolf_wins: w[3], alive_players: w[4],
    sum_end_turn: w[5], end_turn_hist: Array.from(w.slice(6, 22)), score_hist: Array.from(w.slice(22, 38)),
    checksum: w[38], turn: w[39], games_recycled: w[40],
  };
}

/**
 * The native device group (ge_group_*, include/ge_step.h; SURVEY §8e process model): ONE Node process drives N
 * distinct GPUs of a node.  `segments` describe the WHOLE job; device i of n owns the i-th of n contiguous parts of
 * every segment, and every room keeps the global index it has in one RoomBatch of the same arguments - results are
 * identical to that batch's for any device count.  step() runs all devices concurrently on the libuv pool; summary()
 * is the per-device reductions + ONE RCCL all-gather over xGMI + the sum, all inside libge_step.so (RCCL is loaded at
 * run time; there is none in the host).  ShardedBatch above is the host-side form of the same thing (its summary is a
 * host sum): it also runs with several shards on ONE device, which RCCL refuses, and serves as the cross-check.
 */
/**
 * Where a room of the WHOLE job lives after the device group's sharding (ge_group_partition, csrc/ge_host.h group_partition:
 * part i of n holds rooms [floor(R i / n), floor(R (i + 1) / n)) of every segment of R rooms, segment by segment):
 * [part, index inside that part's batch, segment] for `room` counted segment-major as in one RoomBatch.
 */
function locateInShards(segmentRooms, n, room) {
  let base = 0;
  for (let k = 0; k < segmentRooms.length; k++) {
    const R = segmentRooms[k];
    if (room < base + R) {
      const r = room - base;
      const part = (j, Rj) => Number(BigInt(Rj) * BigInt(j) / BigInt(n));     // exact floor, whatever the room count
      let i = Math.min(n - 1, Math.floor((r + 1) * n / R));
      while (i > 0 && part(i, R) > r) i--;
      while (part(i + 1, R) <= r) i++;
      let local = r - part(i, R);                          // rooms of the earlier segments on this part come first
      for (let j = 0; j < k; j++) local += part(i + 1, segmentRooms[j]) - part(i, segmentRooms[j]);
      return [i, local, k];
    }
    base += R;
  }
  throw new RangeError(`room ${room}`);
}

class DeviceGroup {
  constructor({ segments, devices, seed = 0n, firstRoom = 0n, maxFuse = 0, restart = false, trace = false }) {
    if (!devices || !devices.length) throw new RangeError('devices');
    this.segments = segments;
    this.devices = devices.slice();
    this.handle = addon.createGroup({
      seed, firstRoom, maxFuse, restart, trace, devices,
      segments: segments.map((s) => ({ table: s.table.handle, nPlayers: s.nPlayers, nRooms: s.nRooms, humanMask: s.humanMask || 0 })),
    });
    this.nRooms = segments.reduce((a, s) => a + s.nRooms, 0);
    this._tail = Promise.resolve();
  }
  /** Advance every room of every device by nTurns turns (async steps of one group are chained, as for RoomBatch). */
  step(nTurns = 1) {
    const p = this._tail.then(() => addon.groupStep(this.handle, nTurns));
    this._tail = p.catch(() => {});
    return p;
  }
  whenIdle(fn) {
    const p = this._tail.then(fn);
    this._tail = p.catch(() => {});
    return p;
  }
  /** whole-job summary: per-device reductions, one ncclAllGather of the ge_summary records, the sum */
  summary() { return decodeSummary(addon.groupSummary(this.handle)); }
  /** [shard, local index, table] of a room given by its index in segment-major order (the order of one RoomBatch) */
  locate(room) {
    const [i, local, k] = locateInShards(this.segments.map((s) => s.nRooms), this.devices.length, room);
    return [i, local, this.segments[k].table];
  }
  readRoom(room) {
    const [shard, local, table] = this.locate(room);
    return decodeRoom(table, addon.groupReadRooms(this.handle, shard, local, 1), 0);
  }
  close() { if (this.handle) { addon.destroyGroup(this.handle); this.handle = null; } }
}

const { compileCriteria, audienceGroups, uiToolCalls } = require('./ui_script.js');

module.exports = { GameTable, RoomBatch, decodeAdvice, runUntilBits, runUntilNames, findWantBits, findWantNames, decodeRoom, agentStateToView, ShardedBatch, DeviceGroup, locateInShards, RoomLog, formatNote, loadDslByGamename, findGameFile, initializePlayers, turnToolCalls, compileCriteria, audienceGroups, uiToolCalls,
                   deviceCount: addon.deviceCount, addon };

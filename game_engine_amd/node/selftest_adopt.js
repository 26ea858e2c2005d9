'use strict';
// node selftest_adopt.js --views            CPU: stdin [{dsl: <path>, state, nPlayers?, visitActions?}] -> stdout, per case, the hex of
//                                           agentStateToView's view or {error: 'TypeError' | 'RangeError'} (tests/test_adopt_state.py)
// node selftest_adopt.js <dsl.json> <strings_golden.json>
//                                           GPU: adopt the thread at every turn of every case through RoomService.adoptRoom and, all at
//                                           once, through RoomPoolService.adoptRooms; every later turn must equal the golden's
const fs = require('fs');
const { GameTable, agentStateToView } = require('./index.js');

const strip = (x) => {
  if (Array.isArray(x)) return x.map(strip);
  if (x && typeof x === 'object') { const o = {}; for (const [k, v] of Object.entries(x)) if (k !== 'timestamp') o[k] = strip(v); return o; }
  return x;
};
const same = (a, b) => JSON.stringify(a) === JSON.stringify(b);

function views() {
  const cases = JSON.parse(fs.readFileSync(0, 'utf8'));
  const tables = new Map();
  const out = cases.map((c) => {
    if (!tables.has(c.dsl)) tables.set(c.dsl, new GameTable(JSON.parse(fs.readFileSync(c.dsl, 'utf8'))));
    try {
      const { view } = agentStateToView(tables.get(c.dsl), c.state, { nPlayers: c.nPlayers, visitActions: c.visitActions });
      return Buffer.from(view).toString('hex');
    } catch (e) {
      if (e instanceof TypeError || e instanceof RangeError) return { error: e.constructor.name, message: e.message };
      throw e;
    }
  });
  fs.writeSync(1, JSON.stringify(out) + '\n');
  process.exit(0);                  // as selftest.js: no device work is pending, nothing is left to tear down
}

/** (k, the thread's AgentState after turn k) rebuilt from a strings golden case (as tests/test_adopt_state.py golden_states) */
function goldenStates(c) {
  const pa = {}, hist = [], notes = [], out = [];
  c.turns.forEach((t, k) => {
    for (const a of t.actions_added) {
      const rec = pa[a.player_id] || (pa[a.player_id] = { name: a.name, actions: {} });
      rec.actions[a.id] = { action: a.action, phase: a.phase, id: a.id };
    }
    hist.push(...t.history_added); notes.push(...t.notes_added);
    out.push(JSON.parse(JSON.stringify({ current_phase_id: t.current_phase_id, current_phase_name: t.current_phase_name,
                                         player_states: t.player_states, playerActions: pa, phase_history: hist, game_notes: notes })));
  });
  return out;
}

function check(state, sizes, want, where) {
  if (state.current_phase_id !== want.current_phase_id || state.current_phase_name !== want.current_phase_name) throw new Error(`phase, ${where}`);
  const acts = [];
  for (const pid of Object.keys(state.playerActions).sort((a, b) => a - b)) {
    const rec = state.playerActions[pid];
    for (const id of Object.keys(rec.actions).sort((a, b) => a - b)) acts.push({ player_id: pid, name: rec.name, id: rec.actions[id].id, action: rec.actions[id].action, phase: rec.actions[id].phase });
  }
  if (acts.length !== sizes[0] + want.actions_added.length || !want.actions_added.every((a) => acts.some((x) => same(x, a)))) throw new Error(`playerActions, ${where}`);
  if (!same(state.game_notes.slice(sizes[1]), want.notes_added)) throw new Error(`game_notes, ${where}`);
  if (!same(strip(state.phase_history.slice(sizes[2])), want.history_added)) throw new Error(`phase_history, ${where}`);
  if (!same(strip(state.player_states), want.player_states)) throw new Error(`player_states, ${where}: ${JSON.stringify(state.player_states['1'])}`);
  return [acts.length, state.game_notes.length, state.phase_history.length];
}
const sizesOf = (s) => [Object.values(s.playerActions).reduce((m, r) => m + Object.keys(r.actions).length, 0), s.game_notes.length, s.phase_history.length];

async function goldens() {
  const { RoomService } = require('./room_service.js');
  const { RoomPoolService } = require('./room_pool.js');
  const dsl = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
  const gold = JSON.parse(fs.readFileSync(process.argv[3], 'utf8'));
  let adoptions = 0, turns = 0;
  for (const c of gold.cases) {
    const states = goldenStates(c), T = c.turns.length;
    const svc = new RoomService({ seed: BigInt(c.seed) });
    for (let k = 0; k < T; k++) {
      const out = svc.adoptRoom({ threadId: 't', gameName: gold.game, state: states[k], dsl, roomIndex: c.room });
      if (out.toolCalls.length || out.state.current_phase_id !== states[k].current_phase_id) throw new Error(`adoptRoom at ${k}`);
      let sizes = sizesOf(states[k]);
      for (let t = k + 1; t < T; t++) { sizes = check((await svc.continueRoom('t')).state, sizes, c.turns[t], `service, adopted at ${k}, turn ${t}`); turns++; }
      adoptions++;
    }
    await svc.close('t');
    const pool = new RoomPoolService({ seed: BigInt(c.seed), chunkRooms: 32 });
    const outs = await pool.adoptRooms(states.map((s, k) => ({ threadId: `t${k}`, gameName: gold.game, state: s, dsl, roomIndex: c.room })));
    const sizes = states.map(sizesOf);
    outs.forEach((o, k) => { if (o.state.current_phase_id !== states[k].current_phase_id) throw new Error(`adoptRooms entry ${k}`); });
    for (let step = 1; step < T; step++) {
      const live = states.map((_, k) => k).filter((k) => k + step < T);
      const res = await pool.handleMessages(live.map((k) => [`t${k}`, 'Continue']));
      live.forEach((k, j) => { sizes[k] = check(res[j].state, sizes[k], c.turns[k + step], `pool, adopted at ${k}, turn ${k + step}`); turns++; });
    }
    adoptions += T;
    await pool.close();
  }
  fs.writeSync(1, JSON.stringify({ ok: true, adoptions, turns }) + '\n');
}

if (process.argv[2] === '--views') views();
else goldens().then(() => process.exit(0), (e) => { console.error(e); process.exit(1); });

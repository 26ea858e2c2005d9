'use strict';
// node selftest_run_playout.js <script.json> <out.json> - GPU: runRoom / runRooms with { playout: true }.  A script of creates (some
// threads with playout seats), runs, answers and messages goes through RoomPoolService (runRooms), RoomService (runRoom) and a twin
// RoomService that plays the same turns with one continueRoom each; every run must give the twin's outputs turn for turn (log
// timestamps aside), and played / stopped must agree.  Also: without the option a thread with playout seats is still refused, by a
// message that names the option, and runRoomsPlayout is refused with GE_BUSY while an async step() is in flight.  Writes the pool's
// outputs to <out.json> for the Python side to compare with its own (tests/test_gpu_run_playout_service.py).
const fs = require('fs');
const { GameTable, RoomBatch, addon } = require('./index.js');
const { RoomPoolService } = require('./room_pool.js');
const { RoomService } = require('./room_service.js');
const script = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const dsls = {};
for (const [game, path] of Object.entries(script.dsls)) dsls[game] = JSON.parse(fs.readFileSync(path, 'utf8'));

const strip = (x) => {
  if (Array.isArray(x)) return x.map(strip);
  if (x && typeof x === 'object') { const o = {}; for (const [k, v] of Object.entries(x)) if (k !== 'timestamp') o[k] = strip(v); return o; }
  return x;
};
const same = (a, b) => JSON.stringify(strip(a)) === JSON.stringify(strip(b));
const refusedNamingTheOption = async (p, name) => {
  try { await p; } catch (e) { if (e instanceof RangeError && /playout: true/.test(e.message)) return; throw e; }
  throw new Error(`${name}: not refused`);
};

// the first (human seat, choice) the thread accepts, seats and choices ascending; a refusal is GE_ERR_ARG, anything else is an error
async function answer(svc, threadId, seats, n) {
  for (const seat of seats) {
    for (let c = 1; c <= Math.max(n, 3); c++) {
      try { await svc.humanAction(threadId, seat, c); return [seat, c]; } catch (e) { if (e.code !== 'GE-1') throw e; }
    }
  }
  return null;
}

(async () => {
  const opts = { seed: BigInt(script.seed), playoutRollouts: script.playoutRollouts, playoutMaxTurns: script.playoutMaxTurns };
  const pool = new RoomPoolService(Object.assign({ chunkRooms: script.chunkRooms }, opts));
  const one = new RoomService(opts), twin = new RoomService(opts);
  const info = {}, outputs = [];
  let turns = 0;
  for (const op of script.ops) {
    if (op[0] === 'create') {
      const [, threadId, gameName, players, playoutSeats] = op;
      for (const s of [pool, one, twin]) s.createRoom({ threadId, gameName, players, dsl: dsls[gameName], playoutSeats: playoutSeats || [] });
      info[threadId] = { n: players.length, seats: players.map((p, i) => (p.isBot === false ? i + 1 : 0)).filter((x) => x) };
      outputs.push(null);
    } else if (op[0] === 'run') {
      const [, threadIds, maxTurns, until, items] = op;
      const got = await pool.runRooms(threadIds, maxTurns, until, threadIds.map(() => items), { playout: true });
      for (let j = 0; j < threadIds.length; j++) {
        const t = threadIds[j];
        const single = await one.runRoom(t, maxTurns, until, items, { playout: true });
        const want = [];
        for (let k = 0; k < single.played; k++) want.push(strip(await twin.continueRoom(t, items)));   // as its caller sees each then
        for (const o of [single, got[j]]) {
          if (o.played !== want.length || o.turns.length !== o.played || !same(o.turns, want)) throw new Error(`run ${t}: not the twin's continueRoom outputs`);
          if (JSON.stringify(o.stopped) !== JSON.stringify(single.stopped) || o.stopped.some((x) => !until.includes(x))) throw new Error(`run ${t}: stopped`);
        }
        if (!single.stopped.length && single.played !== maxTurns) throw new Error(`run ${t}: stopped for no reason before the limit`);
        turns += single.played;
      }
      outputs.push(strip(got));
    } else if (op[0] === 'answer') {
      const t = op[1];
      const a = await answer(pool, t, info[t].seats, info[t].n);
      for (const s of [one, twin]) if (JSON.stringify(await answer(s, t, info[t].seats, info[t].n)) !== JSON.stringify(a)) throw new Error(`answer ${t}: the services differ`);
      outputs.push(a);
    } else if (op[0] === 'message') {
      const [, t, text] = op;
      const a = await pool.handleMessage(t, text), b = await one.handleMessage(t, text), c = await twin.handleMessage(t, text);
      if (!same(a, c) || !same(b, c)) throw new Error(`message ${t}: the thread is not where continueRoom calls would have left it`);
      outputs.push(strip(a));
    } else if (op[0] === 'refused') {                          // without the option the refusal stands, and names the option
      const t = op[1];
      await refusedNamingTheOption(pool.runRooms([script.plain, t]), 'pool playout thread');
      await refusedNamingTheOption(pool.runRoom(t, 8, ['end'], undefined, { playout: false }), 'pool playout thread, playout: false');
      await refusedNamingTheOption(one.runRoom(t), 'service playout thread');
      outputs.push(null);
    }
  }
  await pool.close();
  // the binding: GE_BUSY while an async step() is in flight, and a plain call afterwards
  const b = new RoomBatch({ segments: [{ table: new GameTable(dsls[Object.keys(dsls)[0]]), nPlayers: 8, nRooms: 10000 }], seed: 3n, maxFuse: 1 });
  const stepping = addon.step(b.handle, 64);                   // the raw binding: RoomBatch.step() would queue instead
  let busy = false;
  try { b.runRoomsPlayout([0], [0], [0], [3], [1], 8, 16, 1n, false, 4, ['end']); } catch (e) { busy = e.code === 'GE_BUSY'; }
  await stepping;
  if (!busy) throw new Error('runRoomsPlayout during an async step was not refused with GE_BUSY');
  const r = b.runRoomsPlayout([3, 1], [7, 9], [0, 0], [0xFF, 0], [70, 90], 8, 16, 5n, false, 6, [], false);
  if (r.played[0] !== 6 || r.played[1] !== 6 || r.stopped[0] !== 0 || r.views !== null || r.events[1].length !== 6 || r.decided[0].length !== 6 ||
      r.decided[1].some((d) => d !== 0)) throw new Error('runRoomsPlayout: binding result');
  const twinBatch = new RoomBatch({ segments: [{ table: new GameTable(dsls[Object.keys(dsls)[0]]), nPlayers: 8, nRooms: 10000 }], seed: 3n, maxFuse: 1 });
  await twinBatch.step(64);
  for (let t = 0; t < 6; t++) {                                // the composition it replaces, on a twin batch
    const s = twinBatch.stepRoomsPlayout([3, 1], [7, 9], [t, t], [0xFF, 0], [70, 90], 8, 16, 5n, false);
    for (let k = 0; k < 2; k++) {
      if (JSON.stringify(s.events[k]) !== JSON.stringify(r.events[k][t]) || s.decided[k] !== r.decided[k][t]) throw new Error(`runRoomsPlayout: turn ${t} of entry ${k} is not stepRoomsPlayout's`);
    }
  }
  b.close(); twinBatch.close();
  fs.writeFileSync(process.argv[3], JSON.stringify(outputs));
  console.log(JSON.stringify({ ok: true, turns }));
})().catch((e) => { console.error(e); process.exit(1); });

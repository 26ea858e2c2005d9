'use strict';
// node selftest_find.js <spec.json> - GPU: findRooms and the pool's waiting() / finished().  spec.script: a list of findRooms
// options, run on a batch of 300 Werewolf x 8 + 200 Two-Truths x 4 rooms stepped 37 turns (what tests/test_gpu_find_rooms.py builds
// in the Python host); spec.pool: { seed, chunkRooms, threads, closed, rounds } - threads opened, played on, some closed (their
// slots stay as they were left), then rounds of runRooms / waiting / finished / answers.  Prints one JSON line: { finds, pool } for
// the Python side to compare with its own.  Also: findRooms is refused with GE_BUSY while an async step() is in flight, and phases
// without "phase" in want is refused.
const fs = require('fs');
const { GameTable, RoomBatch, addon } = require('./index.js');
const { RoomPoolService } = require('./room_pool.js');
const spec = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));

async function answer(svc, threadId, seat, n) {
  for (let c = 1; c <= n; c++) {
    try { await svc.humanAction(threadId, seat, c); return c; } catch (e) { if (e.code !== 'GE-1') throw e; }
  }
  return null;
}

(async () => {
  const out = { finds: null, pool: null };
  if (spec.script) {
    const b = new RoomBatch({ segments: [{ table: new GameTable(spec.ww), nPlayers: 8, nRooms: 300, humanMask: 0b1001 },
                                         { table: new GameTable(spec.tt), nPlayers: 4, nRooms: 200, humanMask: 0b10 }],
                              seed: 11n, firstRoom: 5n, restart: true });
    const stepping = addon.step(b.handle, 37);                 // the raw binding: RoomBatch.step() would queue instead
    let busy = false;
    try { b.findRooms({ want: ['end'] }); } catch (e) { busy = e.code === 'GE_BUSY'; }
    await stepping;
    if (!busy) throw new Error('findRooms during an async step was not refused with GE_BUSY');
    let refused = false;
    try { b.findRooms({ want: ['person'], phases: [1] }); } catch (e) { refused = e instanceof RangeError; }
    if (!refused) throw new Error('phases without "phase" in want was not refused');
    out.finds = spec.script.map((call) => b.findRooms(call));
    b.close();
  }
  if (spec.pool) {
    const p = spec.pool;
    const pool = new RoomPoolService({ seed: BigInt(p.seed), chunkRooms: p.chunkRooms });
    const players = Array.from({ length: 8 }, (_, i) => ({ name: `P${i + 1}`, gamePlayerId: i + 1, isBot: !p.humans.includes(i + 1) }));
    const ids = Array.from({ length: p.threads }, (_, k) => `t${k}`);
    for (const threadId of ids) pool.createRoom({ threadId, gameName: 'werewolf-(mafia)', players, dsl: spec.ww });
    await pool.runRooms(ids, 64, ['person', 'end']);
    for (const t of p.closed) await pool.close(t);
    const live = ids.filter((t) => !p.closed.includes(t));
    const rounds = [];
    for (let r = 0; r < p.rounds; r++) {
      const sub = live.filter((_, k) => (r + k) % 3 !== 0);
      await pool.runRooms(sub, 1 + (r % 3), ['person', 'end']);
      const waiting = await pool.waiting(), finished = (await pool.finished()).sort();
      for (const t of [...Object.keys(waiting), ...finished]) if (!live.includes(t)) throw new Error(`a free slot was reported as thread ${t}`);
      const answers = [];
      for (const t of Object.keys(waiting).sort()) for (const seat of waiting[t]) answers.push([t, seat, await answer(pool, t, seat, 8)]);
      rounds.push({ waiting, finished, answers });
    }
    await pool.close();
    out.pool = rounds;
  }
  console.log(JSON.stringify(out));
})().catch((e) => { console.error(e); process.exit(1); });

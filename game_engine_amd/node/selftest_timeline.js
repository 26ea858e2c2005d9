'use strict';
// node selftest_timeline.js <script.json> <out.json> - GPU: runRoom / runRooms with { forecast: true } (POLICY.md §3i).  A script of
// creates and runs goes through RoomPoolService (runRooms) and RoomService (runRoom); of every run, element 0 of a thread's forecasts
// must be forecast() before the run and the last element forecast() after it, the pool and the lone service must agree, and without
// the option the result has no forecasts.  A thread with playout seats and bad options are refused.  Writes the pool's forecasts to
// <out.json> for the Python side to compare with its own (tests/test_gpu_timeline_service.py).
const fs = require('fs');
const { RoomPoolService } = require('./room_pool.js');
const { RoomService } = require('./room_service.js');
const script = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const dsls = {};
for (const [game, path] of Object.entries(script.dsls)) dsls[game] = JSON.parse(fs.readFileSync(path, 'utf8'));
const same = (a, b) => JSON.stringify(a) === JSON.stringify(b);
const rejects = async (f, name) => { try { await f(); } catch (e) { if (e instanceof RangeError) return; throw e; } throw new Error(`${name}: not refused`); };

(async () => {
  const opts = { seed: BigInt(script.seed), playoutRollouts: 8, playoutMaxTurns: 16 };
  const pool = new RoomPoolService(Object.assign({ chunkRooms: script.chunkRooms }, opts));
  const one = new RoomService(opts);
  const outputs = [];
  let points = 0;
  for (const op of script.ops) {
    if (op[0] === 'create') {
      const [, threadId, gameName, players, playoutSeats] = op;
      for (const s of [pool, one]) s.createRoom({ threadId, gameName, players, dsl: dsls[gameName], playoutSeats: playoutSeats || [] });
      outputs.push(null);
    } else if (op[0] === 'run') {
      const [, threadIds, maxTurns, until, rollouts, fMaxTurns, seats] = op;
      const fseats = seats.map((s) => (s === null ? undefined : s));
      const before = [];
      for (let j = 0; j < threadIds.length; j++) before.push(await pool.forecast(threadIds[j], rollouts, fMaxTurns, fseats[j]));
      const got = await pool.runRooms(threadIds, maxTurns, until, undefined, { forecast: true, rollouts, maxTurns: fMaxTurns, seats: fseats });
      for (let j = 0; j < threadIds.length; j++) {
        const t = threadIds[j], f = got[j].forecasts;
        const single = await one.runRoom(t, maxTurns, until, undefined, { forecast: true, rollouts, maxTurns: fMaxTurns, seat: fseats[j] });
        if (!f || f.length !== got[j].played + 1 || !same(single.forecasts, f) || single.played !== got[j].played) throw new Error(`run ${t}: forecasts of the pool and the service differ`);
        if (!same(f[0], before[j])) throw new Error(`run ${t}: element 0 is not forecast() before the run`);
        if (!same(f[f.length - 1], await pool.forecast(t, rollouts, fMaxTurns, fseats[j]))) throw new Error(`run ${t}: the last element is not forecast() after the run`);
        if (!same(f[f.length - 1], await one.forecast(t, rollouts, fMaxTurns, fseats[j]))) throw new Error(`run ${t}: the service's forecast() after the run`);
        points += f.length;
      }
      outputs.push(got.map((o) => ({ played: o.played, stopped: o.stopped, forecasts: o.forecasts })));
    } else if (op[0] === 'plain') {
      const [, threadIds, maxTurns, until] = op;
      const got = await pool.runRooms(threadIds, maxTurns, until);
      for (let j = 0; j < threadIds.length; j++) {
        const single = await one.runRoom(threadIds[j], maxTurns, until, undefined, { forecast: false, rollouts: 0 });
        if ('forecasts' in got[j] || 'forecasts' in single || single.played !== got[j].played) throw new Error('a run without the option has forecasts');
      }
      outputs.push(null);
    } else if (op[0] === 'refused') {
      const [, plain, bot] = op;
      const f = { forecast: true, rollouts: 8, maxTurns: 16 };
      await rejects(() => one.runRoom(bot, 4, ['end'], undefined, f), 'service playout thread');
      await rejects(() => one.runRoom(bot, 4, ['end'], undefined, Object.assign({ playout: true }, f)), 'service playout thread with playout');
      await rejects(() => pool.runRooms([plain, bot], 4, ['end'], undefined, Object.assign({ playout: true }, f)), 'pool playout thread');
      for (const bad of [{ rollouts: 0 }, { rollouts: 65537 }, { maxTurns: 4097 }, { seat: 0 }, { seat: 99 }]) {
        await rejects(() => one.runRoom(plain, 4, ['end'], undefined, Object.assign({}, f, bad)), `service ${JSON.stringify(bad)}`);
        await rejects(() => pool.runRoom(plain, 4, ['end'], undefined, Object.assign({}, f, bad)), `pool ${JSON.stringify(bad)}`);
      }
      await rejects(() => one.runRoom(plain, 4096, ['end'], undefined, { forecast: true, rollouts: 65536 }), 'points x rollouts above the cap');
      outputs.push(null);
    }
  }
  await pool.close();
  await one.close();
  fs.writeFileSync(process.argv[3], JSON.stringify(outputs));
  console.log(JSON.stringify({ ok: true, points }));
})().catch((e) => { console.error(e); process.exit(1); });

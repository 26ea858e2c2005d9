'use strict';
// node selftest_advise_seats.js <spec.json> - GPU: RoomBatch.adviseSeats and the services' hint / hints beside advise / advises, for
// the Python side (tests/test_gpu_advise_seats_hosts.py) to compare with its own.  spec.calls: a list of { rooms, keys, turns, seats,
// nRollouts, maxTurns, seed, fullView } run on a batch of 40 Werewolf x 8 + 24 Two-Truths x 4 rooms stepped spec.steps turns;
// spec.service / spec.pool: threads opened and played on until a person is needed, then hinted and advised.  Prints one JSON line
// { calls, service, pool }.  Also: adviseSeats is refused with GE_BUSY while an async step() is in flight.
// node selftest_advise_seats.js --output <spec.json> - no GPU: spec { pack, names, hex, meta: [{ threadId, turn, seat, phaseId,
// rollouts, maxTurns, seatView }] } - the ge_advice records of `hex` decoded and printed as hint's JSON, one array.
const fs = require('fs');
const { GameTable, RoomBatch, addon, decodeAdvice } = require('./index.js');
const { RoomService, hintOutput } = require('./room_service.js');
const { RoomPoolService } = require('./room_pool.js');

if (process.argv[2] === '--output') {
  const spec = JSON.parse(fs.readFileSync(process.argv[3], 'utf8'));
  const bytes = Uint8Array.from(spec.hex.match(/../g) || [], (h) => parseInt(h, 16));
  const adv = decodeAdvice(bytes.buffer);
  const st = (m) => ({ pack: spec.pack, current_phase_id: m.phaseId });
  console.log(JSON.stringify(spec.meta.map((m, k) => hintOutput(null, spec.names, m.threadId, m.turn, m.seat, st(m), m.rollouts, m.maxTurns, adv[k], m.seatView))));
  process.exit(0);
}
const spec = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const players = (n, humans) => Array.from({ length: n }, (_, i) => ({ name: `P${i + 1}`, gamePlayerId: i + 1, isBot: !humans.includes(i + 1) }));

(async () => {
  const out = { calls: null, service: null, pool: null };
  if (spec.calls) {
    const b = new RoomBatch({ segments: [{ table: new GameTable(spec.ww), nPlayers: 8, nRooms: 40, humanMask: 0b1 },
                                         { table: new GameTable(spec.tt), nPlayers: 4, nRooms: 24, humanMask: 0b10 }],
                              seed: 11n, firstRoom: 5n });
    const stepping = addon.step(b.handle, spec.steps);         // the raw binding: RoomBatch.step() would queue instead
    let busy = false;
    try { b.adviseSeats([0], [0], [0], [1], 4, 4); } catch (e) { busy = e.code === 'GE_BUSY'; }
    await stepping;
    if (!busy) throw new Error('adviseSeats during an async step was not refused with GE_BUSY');
    let refused = false;
    try { b.adviseSeats([0], [0], [0], [9], 4, 4); } catch (e) { refused = e.code === 'GE-1'; }
    if (!refused) throw new Error('a seat above the player count was not refused with GE_ERR_ARG');
    out.calls = spec.calls.map((c) => b.adviseSeats(c.rooms, c.keys.map((k) => BigInt(k)), c.turns, c.seats, c.nRollouts, c.maxTurns,
                                                    c.seed === null ? undefined : BigInt(c.seed), c.fullView));
    b.close();
  }
  if (spec.service) {
    const s = spec.service;
    const svc = new RoomService({ seed: BigInt(s.seed) });
    const res = [];
    for (const t of s.threads) {
      svc.createRoom({ threadId: t.id, gameName: t.game, players: players(t.n, t.humans), dsl: spec[t.dsl] });
      await svc.runRoom(t.id, 64, ['person', 'end']);
      res.push({ seat: await svc.hint(t.id, undefined, s.rollouts, s.maxTurns), full: await svc.hint(t.id, t.humans[0], s.rollouts, s.maxTurns, 'full'),
                 other: await svc.hint(t.id, t.other, s.rollouts, s.maxTurns),
                 adviseSeat: await svc.advise(t.id, undefined, s.rollouts, s.maxTurns, 'seat'), adviseFull: await svc.advise(t.id, undefined, s.rollouts, s.maxTurns) });
      await svc.close(t.id);
    }
    out.service = res;
  }
  if (spec.pool) {
    const p = spec.pool;
    const pool = new RoomPoolService({ seed: BigInt(p.seed), chunkRooms: p.chunkRooms });
    const ids = [];
    for (const t of p.threads) {
      pool.createRoom({ threadId: t.id, gameName: t.game, players: players(t.n, t.humans), dsl: spec[t.dsl] });
      ids.push(t.id);
    }
    await pool.runRooms(ids, 64, ['person', 'end']);
    const waiting = await pool.waiting();
    const all = await pool.hints(undefined, undefined, p.rollouts, p.maxTurns);
    const listed = await pool.hints(ids, undefined, p.rollouts, p.maxTurns, 'full');
    const one = (await pool.hints([ids[0]], [5], p.rollouts, p.maxTurns))[0];
    const advises = await pool.advises(ids, undefined, p.rollouts, p.maxTurns, 'seat');
    await pool.close();
    out.pool = { waiting, all, listed, one, advises };
  }
  console.log(JSON.stringify(out));
})().catch((e) => { console.error(e); process.exit(1); });

'use strict';
// node selftest_room_seats.js <spec.json> - GPU: per-room host-driven seats (POLICY.md §3l) in the Node host.  spec.batch: { rooms,
// masks, listed, keys, turns } on a batch of 130 Werewolf x 8 (human mask 0b1) + 70 Two-Truths x 4 (0b10) rooms stepped 23 turns
// (what tests/test_gpu_room_seats.py builds in the Python host): seats() before, after setSeats and after clearSeats, then under the
// masks one stepRooms, one findRooms and three whole-batch steps.  spec.service: { seed, humans, seats, before, after } - a pooled
// thread and a RoomService thread with the same room index, `before` Continue messages, setHumanSeats, `after` more, a person
// answering wherever a seat waits.  Prints one JSON line for the Python side to compare with its own.  Also: the three calls are
// refused with GE_BUSY while an async step() is in flight, and setHumanSeats rejects an unknown thread and a seat outside 1 .. n.
const fs = require('fs');
const { GameTable, RoomBatch, addon } = require('./index.js');
const { RoomService } = require('./room_service.js');
const { RoomPoolService } = require('./room_pool.js');
const spec = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));

function busy(fn) {
  try { fn(); } catch (e) { return e.code === 'GE_BUSY'; }
  return false;
}
const noTime = (k, v) => (k === 'timestamp' ? undefined : v);   // phase_history entries carry the wall clock
async function rejects(p) {
  try { await p; } catch (e) { return true; }
  return false;
}
async function answer(services, threadId, seats, n) {
  for (const seat of seats) {
    for (let c = 1; c <= Math.max(n, 3); c++) {
      const ok = [];
      for (const s of services) {
        try { await s.humanAction(threadId, seat, c); ok.push(true); } catch (e) { if (e.code !== 'GE-1') throw e; ok.push(false); }
      }
      if (ok[0] !== ok[1]) throw new Error(`the services differ on seat ${seat} choice ${c}`);
      if (ok[0]) return [seat, c];
    }
  }
  return null;
}

(async () => {
  const out = { batch: null, service: null };
  if (spec.batch) {
    const s = spec.batch;
    const b = new RoomBatch({ segments: [{ table: new GameTable(spec.ww), nPlayers: 8, nRooms: 130, humanMask: 0b1 },
                                         { table: new GameTable(spec.tt), nPlayers: 4, nRooms: 70, humanMask: 0b10 }],
                              seed: 11n, firstRoom: 5n, restart: true });
    const stepping = addon.step(b.handle, 23);                 // the raw binding: RoomBatch.step() would queue instead
    const refused = [busy(() => b.setSeats([0], [1])), busy(() => b.seats()), busy(() => b.clearSeats())];
    await stepping;
    if (!refused.every((x) => x)) throw new Error(`a seats call during an async step was not refused with GE_BUSY: ${refused}`);
    const r = { before: Array.from(b.seats()) };
    b.setSeats(s.rooms, s.masks);
    r.set = Array.from(b.seats());
    r.window = Array.from(b.seats(128, 5));
    b.clearSeats();
    r.cleared = Array.from(b.seats());
    b.setSeats(s.rooms, s.masks);
    r.events = b.stepRooms(s.listed, s.keys, s.turns);
    r.find = b.findRooms({ want: ['person'] });
    await b.step(3);
    const sum = await b.whenIdle(() => b.summary());           // the checksum covers every record
    r.checksum = String(sum.checksum);
    r.turn = Number(sum.turn);
    b.close();
    out.batch = r;
  }
  if (spec.service) {
    const p = spec.service;
    const one = new RoomService({ seed: BigInt(p.seed) }), pool = new RoomPoolService({ seed: BigInt(p.seed), chunkRooms: 4 });
    const players = Array.from({ length: 8 }, (_, i) => ({ name: `P${i + 1}`, gamePlayerId: i + 1, isBot: !p.humans.includes(i + 1) }));
    for (const svc of [one, pool]) svc.createRoom({ threadId: 't', gameName: 'werewolf-(mafia)', players, dsl: spec.ww, roomIndex: 41 });
    const log = [];
    let seats = p.humans;
    for (let k = 0; k < p.before + p.after; k++) {
      if (k === p.before) {
        for (const svc of [one, pool]) {
          if (!(await rejects(svc.setHumanSeats('nobody', [1]))) || !(await rejects(svc.setHumanSeats('t', [0]))) || !(await rejects(svc.setHumanSeats('t', [9]))))
            throw new Error('setHumanSeats accepted an unknown thread or a seat outside 1..8');
          const got = await svc.setHumanSeats('t', p.seats);
          if (JSON.stringify(got) !== JSON.stringify(p.seats)) throw new Error(`setHumanSeats resolved with ${got}`);
        }
        seats = p.seats;
      }
      const a = await one.handleMessage('t', 'Continue'), b = await pool.handleMessage('t', 'Continue');
      if (JSON.stringify(a.state, noTime) !== JSON.stringify(b.state, noTime)) throw new Error(`message ${k}: the pooled thread and the RoomService thread differ`);
      const waiting = (await pool.waiting()).t || [];            // after the turn, before the person answers
      log.push({ waiting, phase: a.state.current_phase_id, answer: await answer([one, pool], 't', seats, 8) });
    }
    await one.close('t');
    await pool.close();
    out.service = log;
  }
  console.log(JSON.stringify(out));
})().catch((e) => { console.error(e); process.exit(1); });

'use strict';
// node selftest_halving.js <script.json> - GPU: one stepRoomsPlayout and one runRoomsPlayout with halving (POLICY.md §3h) on a
// Werewolf x 8 batch, then a thread with playout seats driven through RoomService and RoomPoolService with playoutHalving; prints
// one line of JSON for the Python side to compare with its own calls (tests/test_gpu_halving.py).
const fs = require('fs');
const { GameTable, RoomBatch } = require('./index.js');
const { RoomService } = require('./room_service.js');
const { RoomPoolService } = require('./room_pool.js');

const script = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const dsl = JSON.parse(fs.readFileSync(script.dsl, 'utf8'));

(async () => {
  const out = {};
  const b = new RoomBatch({ segments: [{ table: new GameTable(dsl), nPlayers: 8, nRooms: script.nRooms }], seed: BigInt(script.seed), maxFuse: 1 });
  b.stepSync(script.warm);
  const { rooms, keys, masks, playoutKeys } = script;
  const turns = rooms.map(() => script.warm);
  const step = b.stepRoomsPlayout(rooms, keys, turns, masks, playoutKeys, script.rollouts, script.maxTurns, script.pseed, false, true);
  out.stepEvents = step.events; out.stepDecided = Array.from(step.decided);
  const run = b.runRoomsPlayout(rooms, keys, turns.map((t) => t + 1), masks, playoutKeys, script.rollouts, script.maxTurns, script.pseed, false,
                                script.runTurns, ['phase'], false, true);
  out.runPlayed = Array.from(run.played); out.runStopped = Array.from(run.stopped); out.runEvents = run.events; out.runDecided = run.decided;
  out.records = Buffer.from(b.readRoomsRaw(0, script.nRooms)).toString('hex');
  b.close();
  out.threads = [];
  const opts = { seed: BigInt(script.seed), playoutRollouts: script.rollouts, playoutMaxTurns: script.maxTurns, playoutHalving: true };
  for (const svc of [new RoomService(opts), new RoomPoolService(Object.assign({ chunkRooms: 2 }, opts))]) {
    const players = script.names.map((name, i) => ({ name, gamePlayerId: i + 1, isBot: true }));
    svc.createRoom({ threadId: 't', gameName: script.game, players, dsl, roomIndex: script.room, playoutSeats: script.seats });
    const lines = [];
    for (let t = 0; t < script.turns; t++) {
      const r = await svc.handleMessage('t', 'Continue');
      lines.push(JSON.stringify({ toolCalls: r.toolCalls, uiCalls: r.uiCalls }));
    }
    out.threads.push(lines);
    await svc.close();
  }
  console.log(JSON.stringify(out));
})().catch((e) => { console.error(e); process.exit(1); });

'use strict';
// node selftest_compare.js <script.json> - GPU: one thread driven message by message through RoomService and then through
// RoomPoolService, with an advise(compare) in both views for the lowest human seat before every message; prints each as one line
// of compact JSON, for the Python side to compare byte for byte with its own (tests/test_gpu_compare_service.py).
const fs = require('fs');
const { RoomService } = require('./room_service.js');
const { RoomPoolService } = require('./room_pool.js');

const script = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const dsl = JSON.parse(fs.readFileSync(script.dsl, 'utf8'));
const players = script.names.map((name, i) => ({ name, gamePlayerId: i + 1, isBot: !script.humans.includes(i + 1) }));

(async () => {
  for (const svc of [new RoomService({ seed: BigInt(script.seed) }), new RoomPoolService({ seed: BigInt(script.seed), chunkRooms: 8 })]) {
    svc.createRoom({ threadId: 't', gameName: script.game, players, dsl, roomIndex: script.room });
    for (const text of script.messages) {
      for (const view of ['full', 'seat']) console.log(JSON.stringify(await svc.advise('t', undefined, script.rollouts, script.maxTurns, view, true)));
      await svc.handleMessage('t', text);
    }
    await svc.close();
  }
})().catch((e) => { console.error(e); process.exit(1); });

'use strict';
// node selftest_beliefs.js <script.json> - GPU: one thread driven message by message through RoomService and then through
// RoomPoolService, with a seat-view advise (plain and comparing) and a seat-view forecast under the script's beliefs for the lowest
// human seat before every message; prints each as one line of compact JSON, for the Python side to compare byte for byte with its
// own (tests/test_gpu_beliefs_service.py).
const fs = require('fs');
const { RoomService } = require('./room_service.js');
const { RoomPoolService } = require('./room_pool.js');

const script = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const dsl = JSON.parse(fs.readFileSync(script.dsl, 'utf8'));
const players = script.names.map((name, i) => ({ name, gamePlayerId: i + 1, isBot: !script.humans.includes(i + 1) }));
const seat = Math.min(...script.humans);

(async () => {
  for (const svc of [new RoomService({ seed: BigInt(script.seed) }), new RoomPoolService({ seed: BigInt(script.seed), chunkRooms: 8 })]) {
    svc.createRoom({ threadId: 't', gameName: script.game, players, dsl, roomIndex: script.room });
    for (const text of script.messages) {
      console.log(JSON.stringify(await svc.advise('t', undefined, script.rollouts, script.maxTurns, 'seat', false, script.beliefs)));
      console.log(JSON.stringify(await svc.advise('t', undefined, script.rollouts, script.maxTurns, 'seat', true, script.beliefs)));
      console.log(JSON.stringify(await svc.forecast('t', script.rollouts, script.maxTurns, seat, script.beliefs)));
      await svc.handleMessage('t', text);
    }
    for (const bad of [() => svc.forecast('t', 4, 4, undefined, script.beliefs), () => svc.advise('t', undefined, 4, 4, 'full', false, script.beliefs),
                       () => svc.forecast('t', 4, 4, seat, { 99: 1 }), () => svc.forecast('t', 4, 4, seat, { 1: 256 })]) {
      let refused = false;
      try { await bad(); } catch (e) { refused = e instanceof RangeError; }
      if (!refused) throw new Error('a bad beliefs argument was not refused with a RangeError');
    }
    await svc.close();
  }
})().catch((e) => { console.error(e); process.exit(1); });

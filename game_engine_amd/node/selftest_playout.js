'use strict';
// node selftest_playout.js <script.json> - GPU: threads with playout seats (and one without) driven message by message through
// RoomService and then through RoomPoolService; prints every turn's output as one line of compact JSON, for the Python side to
// compare byte for byte with its own (tests/test_gpu_playout_service.py).
const fs = require('fs');
const { RoomService } = require('./room_service.js');
const { RoomPoolService } = require('./room_pool.js');

const script = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const opts = { seed: BigInt(script.seed), playoutRollouts: script.rollouts, playoutMaxTurns: script.maxTurns, playoutView: script.view };

(async () => {
  for (const svc of [new RoomService(opts), new RoomPoolService(Object.assign({ chunkRooms: 2 }, opts))]) {
    for (const th of script.threads) {
      const dsl = JSON.parse(fs.readFileSync(th.dsl, 'utf8'));
      const players = th.names.map((name, i) => ({ name, gamePlayerId: i + 1, isBot: true }));
      svc.createRoom({ threadId: th.id, gameName: th.game, players, dsl, roomIndex: th.room, playoutSeats: th.seats });
    }
    for (let t = 0; t < script.turns; t++)
      for (const th of script.threads) {
        const out = await svc.handleMessage(th.id, 'Continue');
        console.log(JSON.stringify({ toolCalls: out.toolCalls, uiCalls: out.uiCalls }));
      }
    await svc.close();
  }
})().catch((e) => { console.error(e); process.exit(1); });

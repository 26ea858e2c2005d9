'use strict';
// node selftest_pool.js <script.json> <out.json> - GPU: a script of creates / ticks / closes through RoomPoolService and, thread by
// thread, through RoomService; every output must be the same (log timestamps aside).  Writes the pool's outputs to <out.json> for
// the Python side to compare with its own (tests/test_gpu_room_pool.py).
const fs = require('fs');
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

(async () => {
  const pool = new RoomPoolService({ seed: BigInt(script.seed), chunkRooms: script.chunkRooms });
  const ref = new RoomService({ seed: BigInt(script.seed) });
  const outputs = [];
  let compared = 0;
  for (const op of script.ops) {
    if (op[0] === 'create') {
      const [, threadId, gameName, players] = op;
      const a = pool.createRoom({ threadId, gameName, players, dsl: dsls[gameName] });
      const b = ref.createRoom({ threadId, gameName, players, dsl: dsls[gameName] });
      if (JSON.stringify(strip(a)) !== JSON.stringify(strip(b))) throw new Error(`create ${threadId}: pool and service differ`);
      outputs.push(strip(a));
    } else if (op[0] === 'tick') {
      const got = await pool.handleMessages(op[1].map(([t, text]) => [t, text]));
      for (let k = 0; k < got.length; k++) {
        const [t, text] = op[1][k];
        const want = await ref.handleMessage(t, text);
        if (JSON.stringify(strip(got[k])) !== JSON.stringify(strip(want))) throw new Error(`tick: thread ${t} message ${JSON.stringify(text)}: pool and service differ`);
        compared++;
      }
      outputs.push(strip(got));
    } else {
      await pool.close(op[1]);
      await ref.close(op[1]);
      outputs.push(null);
    }
  }
  await pool.close();
  fs.writeFileSync(process.argv[3], JSON.stringify(outputs));
  console.log(JSON.stringify({ ok: true, compared }));
})().catch((e) => { console.error(e); process.exit(1); });

'use strict';
/**
 * RoomPoolService — many game threads hosted in a few resident batches (twin of game_engine_amd/room_pool.py).
 *
 * RoomService gives every thread its own N = 1 batch and pays about three synchronising calls per message.  Here threads of
 * the same (game, player count, human seats) share a pool of fixed-capacity batch chunks, a thread owning one slot.  Its RNG
 * stream is keyed by roomIndexOf(threadId) (or the roomIndex it was created with) and its turn counter is its own, so a thread
 * plays exactly the game it plays on a RoomService: RoomBatch.stepRooms moves a slot by one turn keyed as that global room at
 * that turn.  handleMessages is one tick for many threads: per chunk touched, one injection round per candidate seat, one
 * stepRooms and one readRoomsAt.  The chunks are shared, so every call of the service runs strictly one after the other.
 */
const { GameTable, RoomBatch, RoomLog, decodeRoom, turnToolCalls, uiToolCalls } = require('./index.js');
const { roomIndexOf, prepareAdoption, adoptedOutput, checkForecastArgs, adviseCandidates, adviseSeat, runRollouts, adviseOutput, runHints, hintOutput,
        seatForecastOutput, beliefBytes, neutralBeliefs, checkForecastSeat, checkView, seatsMask, playoutMaskOf, checkPlayoutOptions, PLAYOUT_CAP, playoutMaxCands, forecastKey, forecastSeed, checkRunArgs, checkRunThread, runTurn, runOutput,
        checkRunForecast, runForecastPerCall, runForecasts } = require('./room_service.js');
const popcount = (m) => { let c = 0; for (let x = m; x; x &= x - 1) c++; return c; };
const M = require('./messages.js');

const GE_ERR_ARG = -1;

class RoomPoolService {
  /** playoutRollouts / playoutMaxTurns / playoutView / playoutHalving: as RoomService's. */
  constructor({ gamesDir = 'games', seed = 0n, device = 0, chunkRooms = 1024, playoutRollouts = 256, playoutMaxTurns = 256, playoutView = 'seat',
                playoutHalving = false } = {}) {
    this.playoutFull = checkPlayoutOptions(playoutRollouts, playoutMaxTurns, playoutView, playoutHalving);
    this.playoutHalving = playoutHalving;
    this.playoutRollouts = playoutRollouts; this.playoutMaxTurns = playoutMaxTurns;
    if (!(chunkRooms >= 1)) throw new RangeError('chunkRooms must be >= 1');
    this.gamesDir = gamesDir; this.seed = BigInt(seed); this.device = device; this.chunkRooms = chunkRooms;
    this.tables = new Map();       // gameName -> GameTable
    this.pools = new Map();        // `${gameName}/${nPlayers}/${humanMask}` -> { table, nPlayers, humanMask, chunks, free, used, seated, templateRaw }
    this.rooms = new Map();        // threadId -> { pool, chunk, ci, slot, key, turn, table, gameName, names, humanSeats, panel, state, log }
    this.queue = Promise.resolve();
  }
  table(gameName, dsl) {
    if (!this.tables.has(gameName)) this.tables.set(gameName, dsl ? new GameTable(dsl) : GameTable.fromGamename(gameName, this.gamesDir));
    return this.tables.get(gameName);
  }
  _serial(fn) {
    const p = this.queue.then(fn);
    this.queue = p.catch(() => {});
    return p;
  }
  _acquire(pool, template = true) {
    if (pool.free.length === 0) {
      const ci = pool.chunks.length;
      const chunk = new RoomBatch({ segments: [{ table: pool.table, nPlayers: pool.nPlayers, nRooms: this.chunkRooms, humanMask: pool.humanMask }],
                                    seed: this.seed, firstRoom: 0n, device: this.device, maxFuse: 1 });
      pool.chunks.push(chunk);
      if (!pool.templateRaw) pool.templateRaw = chunk.readRoomsAtRaw([0]);
      for (let s = this.chunkRooms - 1; s >= 0; s--) pool.free.push([ci, s]);
    }
    const [ci, slot] = pool.free.pop();
    const chunk = pool.chunks[ci];
    const id = `${ci}/${slot}`;
    if (template && pool.used.has(id)) chunk.writeRoomsRaw(slot, pool.templateRaw);   // a reused slot starts from the template (no prepared deal)
    if (pool.seated.has(id)) {     // ... and with the pool's own seating (setHumanSeats changed the slot's mask)
      chunk.setSeats([slot], [pool.humanMask]);
      pool.seated.delete(id);
    }
    pool.used.add(id);
    return { chunk, ci, slot };
  }
  /** As RoomService.createRoom: players[i].isBot === false marks a human seat; roomIndex = the global room index the RNG is keyed by. */
  createRoom({ threadId, gameName, players, dsl, roomIndex, playoutSeats }) {
    const table = this.table(gameName, dsl);
    const humanMask = players.reduce((m, p, i) => (p.isBot === false ? m | (1 << i) : m), 0);
    const playoutMask = playoutMaskOf(players.length, humanMask, playoutSeats);
    if (this.rooms.has(threadId)) this._release(threadId);
    const pk = `${gameName}/${players.length}/${humanMask}`;
    if (!this.pools.has(pk)) this.pools.set(pk, { table, nPlayers: players.length, humanMask, chunks: [], free: [], used: new Set(), seated: new Set(), templateRaw: null });
    const pool = this.pools.get(pk);
    const { chunk, ci, slot } = this._acquire(pool);
    const names = players.map((p, i) => p.name || `Player ${i + 1}`);
    const humanSeats = players.map((p, i) => (p.isBot === false ? i + 1 : 0)).filter((x) => x);
    const room = { pool, chunk, ci, slot, key: roomIndex === undefined ? roomIndexOf(threadId) : BigInt(roomIndex), turn: 0,
                   table, gameName, names, humanSeats, playoutMask, panel: null, state: decodeRoom(table, pool.templateRaw, 0), log: new RoomLog(table, names, gameName) };
    this.rooms.set(threadId, room);
    return this.agentState(room);
  }
  /**
   * Take over many threads that are already mid-game (twin of the Python RoomPoolService.adopt_rooms): entries
   * [{ threadId, gameName, state, players?, humanSeats?, dsl?, roomIndex?, turn?, visitActions? }].  Every state is converted
   * first and the slots taken next; a refusal leaves the service as it was.  Then one writeRoomsAt per chunk touched (a reused
   * slot is written over directly).  Resolves, in order, what RoomService.adoptRoom returns for each.
   */
  adoptRooms(entries) {
    return this._serial(() => {
      const seen = new Set();
      const prep = entries.map((e) => {
        if (seen.has(e.threadId)) throw new Error(`thread ${e.threadId} is named twice`);
        seen.add(e.threadId);
        const table = this.table(e.gameName, e.dsl);
        const a = prepareAdoption(table, e);
        return Object.assign({ e, table, playoutMask: playoutMaskOf(a.n, a.humanMask, e.playoutSeats) }, a);
      });
      const taken = [];
      try {
        for (const p of prep) {
          const pk = `${p.e.gameName}/${p.n}/${p.humanMask}`;
          if (!this.pools.has(pk)) this.pools.set(pk, { table: p.table, nPlayers: p.n, humanMask: p.humanMask, chunks: [], free: [], used: new Set(), seated: new Set(), templateRaw: null });
          const pool = this.pools.get(pk);
          taken.push(Object.assign({ pool }, this._acquire(pool, false)));
        }
        const byChunk = new Map();
        taken.forEach((t, k) => {
          if (!byChunk.has(t.chunk)) byChunk.set(t.chunk, []);
          byChunk.get(t.chunk).push(k);
        });
        for (const [chunk, ks] of byChunk) chunk.writeRoomsAt(ks.map((k) => taken[k].slot), ks.map((k) => prep[k].view));
        const states = new Array(prep.length);
        for (const [chunk, ks] of byChunk) chunk.readRoomsAt(ks.map((k) => taken[k].slot)).forEach((st, j) => { states[ks[j]] = st; });
        return prep.map((p, k) => {
          const { pool, chunk, ci, slot } = taken[k];
          if (this.rooms.has(p.e.threadId)) this._release(p.e.threadId);
          const room = { pool, chunk, ci, slot, key: p.e.roomIndex === undefined ? roomIndexOf(p.e.threadId) : BigInt(p.e.roomIndex), turn: p.turn,
                         table: p.table, gameName: p.e.gameName, names: p.names, humanSeats: p.humanSeats, playoutMask: p.playoutMask, panel: null, state: states[k],
                         log: new RoomLog(p.table, p.names, p.e.gameName) };
          room.log.adopt(p.e.state, Object.assign({}, p.hostSide, { names: Object.fromEntries(p.names.map((nm, i) => [String(i + 1), nm])) }));
          this.rooms.set(p.e.threadId, room);
          return adoptedOutput(room, p.turn);
        });
      } catch (err) {
        for (const t of taken) if (![...this.rooms.values()].some((r) => r.chunk === t.chunk && r.slot === t.slot)) t.pool.free.push([t.ci, t.slot]);
        throw err;
      }
    });
  }
  agentState(room) { return room.log.agentState(room.state); }
  _room(threadId) {
    const room = this.rooms.get(threadId);
    if (!room) throw new Error(`unknown thread ${threadId}`);
    return room;
  }
  humanAction(threadId, playerId, choice) {
    return this._serial(() => {
      const room = this._room(threadId);
      const st = room.chunk.injectActions([room.slot], [playerId], [choice]);
      if (st[0] !== 0) { const e = new Error(`injectAction: status ${st[0]}`); e.code = `GE${st[0]}`; throw e; }
      room.state = room.chunk.readRoomsAt([room.slot])[0];
      return this.agentState(room);
    });
  }
  /** As RoomService.setHumanSeats (POLICY.md §3l): from the next turn on exactly `seats` (player ids) of the thread are played by
   * people.  The thread stays in its slot and its pool; the slot's seat mask goes back to the pool's when the slot is reused.
   * Rejects for an unknown thread or a seat outside 1..n, before anything changes; resolves with the seats. */
  setHumanSeats(threadId, seats) {
    return this._serial(() => {
      const room = this._room(threadId);
      const mask = seatsMask(threadId, room.pool.nPlayers, seats);
      room.chunk.setSeats([room.slot], [mask]);
      room.pool.seated.add(`${room.ci}/${room.slot}`);
      room.humanSeats = room.names.map((_, i) => i + 1).filter((i) => (mask >> (i - 1)) & 1);
      room.playoutMask &= ~mask;
      return room.humanSeats.slice();
    });
  }
  continueRoom(threadId, items) {
    return this._serial(() => this._turns([this._room(threadId)], [items])[0]);
  }
  handleMessage(threadId, text, items) {
    return this.handleMessages([[threadId, text, items]]).then((o) => o[0]);
  }
  /** One tick: [[threadId, text, items?], ...] -> [output, ...] in the same order, each what handleMessage resolves for it.
   * A thread may appear once per tick (rejected before anything runs otherwise). */
  handleMessages(msgs) {
    return this._serial(() => {
      const seen = new Set();
      const entries = msgs.map(([tid, text, items]) => {
        if (seen.has(tid)) throw new Error(`thread ${tid} is named twice in one tick`);
        seen.add(tid);
        return { room: this._room(tid), text, items };
      });
      const out = new Array(entries.length).fill(null);
      const play = [];
      let pending = [];
      entries.forEach((e, i) => {
        const kind = M.classify(e.text);
        if (kind === M.CHAT) { out[i] = { state: this.agentState(e.room), toolCalls: [], uiCalls: [], played: false, kind }; return; }
        play.push([i, kind]);
        if (kind === M.ACTION) {
          const room = e.room;
          room.log.personMessage(e.text);
          const st = room.state, info = room.table.info;
          const phase = info.phases.find((x) => x.id === st.current_phase_id);
          const alive = st.slots.map((v) => (st.pack === 1 ? !!v[2] : true));
          const cands = M.resolve(e.text, room.panel, phase ? phase.act : 0, st.pack, room.names, alive, room.humanSeats);
          if (cands.length) pending.push([i, cands]);
        }
      });
      // injection rounds: a thread's next candidate seat only where the previous one was refused with GE_ERR_ARG (RoomService's loop)
      for (let r = 0; pending.length; r++) {
        const byChunk = new Map();
        for (const p of pending) {
          const c = entries[p[0]].room.chunk;
          if (!byChunk.has(c)) byChunk.set(c, []);
          byChunk.get(c).push(p);
        }
        const next = [];
        for (const [chunk, group] of byChunk) {
          const st = chunk.injectActions(group.map(([i]) => entries[i].room.slot), group.map(([, c]) => c[r][0]), group.map(([, c]) => c[r][1]));
          group.forEach((p, k) => {
            if (st[k] === 0) return;
            if (st[k] !== GE_ERR_ARG) { const e = new Error(`injectActions: status ${st[k]}`); e.code = `GE${st[k]}`; throw e; }
            if (r + 1 < p[1].length) next.push(p);
          });
        }
        pending = next;
      }
      const res = this._turns(play.map(([i]) => entries[i].room), play.map(([i]) => entries[i].items));
      play.forEach(([i, kind], k) => { out[i] = Object.assign(res[k], { played: true, kind }); });
      return out;
    });
  }
  /** As RoomService.runRoom (same turns and output), from the thread's pool slot. */
  runRoom(threadId, maxTurns = 64, until = ['person', 'end'], items, options) {
    return this.runRooms([threadId], maxTurns, until, items === undefined || items === null ? undefined : [items], options).then((o) => o[0]);
  }
  /** Play many threads on, each until a person is needed in it (RoomService.runRoom's conditions and output, in order): one
   * RoomBatch.runRooms call per chunk touched, every thread under its own key and from its own turn.  items[j]: thread j's canvas
   * items.  A thread named twice, an unknown thread, a thread with playout seats and bad arguments are refused before anything
   * runs.  options { playout: true }: threads with playout seats are run too - a chunk holding one takes one RoomBatch.runRoomsPlayout
   * call (POLICY.md §3g; mask 0 for its other threads; more calls only where the playouts of one turn would pass the call's cap).
   * Every chunk's call is made before any turn is folded: if one of them fails (a device error), the threads of the chunks
   * already run have moved on the device while no thread's turn or log has - such a service is to be closed, not continued.
   * options { forecast: true, rollouts, maxTurns, seat | seats }: every thread's result gains forecasts (RoomService.runRoom's;
   * seats[j]: the seat thread j's are seen from, seat: one seat for all), from one RoomBatch.runRoomsForecast call per chunk touched
   * (POLICY.md §3i; more calls only where one call's points would pass its caps); threads with playout seats are refused. */
  runRooms(threadIds, maxTurns = 64, until = ['person', 'end'], items, options) {
    return this._serial(() => {
      const bits = checkRunArgs(maxTurns, until);
      const playout = !!(options && options.playout);
      if (new Set(threadIds).size !== threadIds.length) throw new RangeError('runRooms: a thread is named twice');
      const rooms = Array.from(threadIds, (t) => this._room(t));
      const its = items || [];
      if (items && its.length !== rooms.length) throw new RangeError('runRooms: threadIds and items differ in length');
      const seats = options && options.forecast && Array.isArray(options.seats) ? options.seats : null;   // per thread; else options.seat for all
      if (seats && seats.length !== rooms.length) throw new RangeError('runRooms: threadIds and seats differ in length');
      const fcs = rooms.map((room, j) => checkRunForecast(threadIds[j], room, maxTurns, seats ? Object.assign({}, options, { seat: seats[j] }) : options));
      const fc = fcs[0] || null;
      rooms.forEach((room, j) => {
        checkRunThread(threadIds[j], room, playout);
        if (room.turn + maxTurns + (room.playoutMask ? this.playoutMaxTurns - 1 : 0) > 0xFFFFFFFF) throw new RangeError(`thread ${threadIds[j]}: the turn counter would overflow`);
      });
      const byChunk = new Map();
      rooms.forEach((room, j) => {
        if (!byChunk.has(room.chunk)) byChunk.set(room.chunk, []);
        byChunk.get(room.chunk).push(j);
      });
      const perCall = fc ? runForecastPerCall(maxTurns, fc.rollouts) : Math.max(1, Math.floor((1 << 20) / maxTurns));   // the call's cap on n x maxTurns
      const got = new Array(rooms.length);
      for (const [chunk, all] of byChunk) {
        const withBots = all.some((j) => rooms[j].playoutMask);
        const parts = [];
        if (withBots) parts.push(...this._playoutParts(all.map((j) => rooms[j]), perCall));
        else for (let lo = 0; lo < all.length; lo += perCall) parts.push([lo, Math.min(lo + perCall, all.length)]);
        for (const [a, b] of parts) {
          const js = all.slice(a, b);
          const slots = js.map((j) => rooms[j].slot), keys = js.map((j) => rooms[j].key), turns = js.map((j) => rooms[j].turn);
          const r = fc
            ? chunk.runRoomsForecast(slots, keys, turns, keys.map((k) => forecastKey(k)), fc.rollouts, fc.maxTurns, js.map((j) => fcs[j].seat || 0),
                                     forecastSeed(this.seed), maxTurns, bits)
            : withBots
            ? chunk.runRoomsPlayout(slots, keys, turns, js.map((j) => rooms[j].playoutMask), keys.map((k) => forecastKey(k)), this.playoutRollouts,
                                    this.playoutMaxTurns, forecastSeed(this.seed), this.playoutFull, maxTurns, bits, true, this.playoutHalving)
            : chunk.runRooms(slots, keys, turns, maxTurns, bits);
          js.forEach((j, k) => { got[j] = { events: r.events[k], views: r.views[k], stopped: r.stopped[k], stats: fc ? r.stats[k] : null }; });
        }
      }
      return rooms.map((room, j) => {
        const forecasts = fc ? runForecasts(room.table, room.names, threadIds[j], room.turn, fcs[j], got[j].stats) : undefined;
        room.turn += got[j].events.length;
        return runOutput(got[j].events.map((ev, t) => runTurn(this._finish(room, got[j].views[t], ev, its[j]))), got[j].stopped, forecasts);
      });
    });
  }
  /** As RoomService.forecast (same keys, seed, seat view, beliefs and output), from the thread's pool slot. */
  forecast(threadId, nRollouts = 4096, maxTurns = 1024, seat, beliefs) {
    return this.forecasts([threadId], nRollouts, maxTurns, seat === undefined || seat === null ? undefined : [seat],
                          beliefs === undefined || beliefs === null ? undefined : [beliefs]).then((o) => o[0]);
  }
  /** As RoomService.advise (same candidates, keys, seed, views, compare, beliefs and output), from the thread's pool slot. */
  advise(threadId, playerId, nRollouts = 4096, maxTurns = 1024, view = 'full', compare = false, beliefs) {
    return this.advises([threadId], [playerId], nRollouts, maxTurns, view, compare,
                        beliefs === undefined || beliefs === null ? undefined : [beliefs]).then((o) => o[0]);
  }
  /** Advice for many threads, in order (playerIds[j] undefined / null or no playerIds: thread j's lowest human seat): one
   * rolloutActions call per chunk touched (rolloutSeats in the "seat" view; with compare one rolloutCompare, and every option
   * gains "versus" as RoomService.advise's).  beliefs[j] (view "seat" only): thread j's advised seat's suspicions, as
   * RoomService.advise's; a chunk any of whose threads has some gets one rolloutBeliefs call instead, its other threads under
   * equal weights.  No thread changes. */
  advises(threadIds, playerIds, nRollouts = 4096, maxTurns = 1024, view = 'full', compare = false, beliefs) {
    checkForecastArgs(nRollouts, maxTurns);
    const seatView = checkView(view);
    return this._serial(() => {
      const rooms = threadIds.map((t) => this._room(t));
      const pids = playerIds || [];
      const seats = rooms.map((room, j) => adviseSeat(threadIds[j], room.humanSeats, pids[j]));
      const cands = rooms.map((room) => adviseCandidates(room.table, room.state));
      const bel = rooms.map((room, j) => beliefBytes(threadIds[j], room.table.info.pack, room.names.length, (beliefs || [])[j], seatView));
      const res = runRollouts(rooms.map((room, j) => ({ batch: room.chunk, slot: room.slot, key: room.key, turn: room.turn, seat: seats[j], cands: cands[j],
                                                        beliefs: bel[j], neutral: neutralBeliefs(room.table.info.pack, room.names.length) })),
                              seatView, nRollouts, maxTurns, this.seed, !!compare);
      return rooms.map((room, j) => adviseOutput(room.table, room.names, threadIds[j], room.turn, seats[j], room.state, cands[j], nRollouts, maxTurns,
                                                 res[j], 0, seatView, bel[j]));
    });
  }
  /** Hints for many (thread, seat) pairs, each as RoomService.hint's (twin of the Python RoomPoolService.hints): one adviseSeats
   * call per chunk touched (POLICY.md §3m).  threadIds undefined / null: every thread waiting() reports, in the order the threads
   * were created, and each of its pending seats ascending.  With threadIds: playerIds[j] (undefined / null or no playerIds: thread
   * j's lowest human seat).  No thread changes. */
  hints(threadIds, playerIds, nRollouts = 4096, maxTurns = 1024, view = 'seat') {
    checkForecastArgs(nRollouts, maxTurns);
    const seatView = checkView(view);
    return this._serial(() => {
      let pairs;
      if (threadIds === undefined || threadIds === null) {
        if (playerIds !== undefined && playerIds !== null) throw new RangeError('hints: playerIds need threadIds');
        const wait = new Map(this._scan(['person']).map(([t, h]) => [t, h.pending]));
        pairs = [];
        for (const t of this.rooms.keys()) for (const seat of wait.get(t) || []) pairs.push([t, seat]);
      } else {
        const pids = playerIds || [];
        pairs = threadIds.map((t, j) => [t, adviseSeat(t, this._room(t).humanSeats, pids[j])]);
      }
      const rooms = pairs.map(([t]) => this._room(t));
      const advs = runHints(rooms.map((room, j) => ({ batch: room.chunk, slot: room.slot, key: room.key, turn: room.turn, seat: pairs[j][1],
                                                      cost: playoutMaxCands(room.table.info.pack, room.names.length) + 1 })),
                            seatView, nRollouts, maxTurns, this.seed);
      return rooms.map((room, j) => hintOutput(room.table, room.names, pairs[j][0], room.turn, pairs[j][1], room.state, nRollouts, maxTurns, advs[j], seatView));
    });
  }
  /** Forecasts of many threads, in order: one rolloutRooms per chunk touched; with seats (seats[j] 1 .. n: thread j from that
   * seat's view, undefined / null: the full view), one rolloutSeats per chunk touched.  beliefs[j] (for a thread with a seat): as
   * RoomService.forecast's; a chunk any of whose threads has some gets one rolloutBeliefs call instead.  No thread changes. */
  forecasts(threadIds, nRollouts = 4096, maxTurns = 1024, seats, beliefs) {
    checkForecastArgs(nRollouts, maxTurns);
    return this._serial(() => {
      const rooms = threadIds.map((t) => this._room(t));
      const sv = seats || [];
      rooms.forEach((room, j) => checkForecastSeat(threadIds[j], room.names.length, sv[j]));
      const bel = rooms.map((room, j) => beliefBytes(threadIds[j], room.table.info.pack, room.names.length, (beliefs || [])[j],
                                                     sv[j] !== undefined && sv[j] !== null));
      const res = runRollouts(rooms.map((room, j) => ({ batch: room.chunk, slot: room.slot, key: room.key, turn: room.turn, seat: sv[j],
                                                        beliefs: bel[j], neutral: neutralBeliefs(room.table.info.pack, room.names.length) })),
                              !!seats, nRollouts, maxTurns, this.seed);
      return rooms.map((room, j) => seatForecastOutput(room.table, room.names, threadIds[j], room.turn, nRollouts, maxTurns, sv[j], res[j].words, 0, bel[j]));
    });
  }
  /** One turn of each room (distinct threads): one stepRooms and one readRoomsAt per chunk touched; a chunk holding a thread
   * with playout seats is stepped by stepRoomsPlayout instead (mask 0 for its other threads; more calls only when the
   * playouts would pass the call's cap). */
  _turns(rooms, items) {
    const byChunk = new Map();
    rooms.forEach((room, j) => {
      if (!byChunk.has(room.chunk)) byChunk.set(room.chunk, []);
      byChunk.get(room.chunk).push(j);
    });
    const events = new Array(rooms.length), afters = new Array(rooms.length);
    for (const [chunk, js] of byChunk) {
      const slots = js.map((j) => rooms[j].slot);
      const ev = js.some((j) => rooms[j].playoutMask) ? this._stepPlayout(chunk, js.map((j) => rooms[j]))
        : chunk.stepRooms(slots, js.map((j) => rooms[j].key), js.map((j) => rooms[j].turn));
      const views = chunk.readRoomsAt(slots);
      js.forEach((j, k) => { events[j] = ev[k]; afters[j] = views[k]; rooms[j].turn += 1; });
    }
    return rooms.map((room, j) => this._finish(room, afters[j], events[j], items[j]));
  }
  /** Runs [a, b) of one chunk's rooms whose playouts of one turn stay under the call's cap (and of at most `most` rooms). */
  _playoutParts(rooms, most) {
    const cost = rooms.map((r) => popcount(r.playoutMask) * playoutMaxCands(r.table.info.pack, r.pool.nPlayers) * this.playoutRollouts);
    const parts = [];
    let lo = 0, acc = 0;
    cost.forEach((c, k) => {
      if ((acc + c > PLAYOUT_CAP || (most !== undefined && k - lo >= most)) && k > lo) { parts.push([lo, k]); lo = k; acc = 0; }
      acc += c;
    });
    parts.push([lo, rooms.length]);
    return parts;
  }
  /** stepRoomsPlayout of one chunk's rooms under advise's keys and seed, in runs under the call's cap. */
  _stepPlayout(chunk, rooms) {
    const parts = this._playoutParts(rooms);
    const out = [];
    for (const [a, b] of parts) {
      const rs = rooms.slice(a, b);
      out.push(...chunk.stepRoomsPlayout(rs.map((r) => r.slot), rs.map((r) => r.key), rs.map((r) => r.turn), rs.map((r) => r.playoutMask),
                                         rs.map((r) => forecastKey(r.key)), this.playoutRollouts, this.playoutMaxTurns, forecastSeed(this.seed),
                                         this.playoutFull, this.playoutHalving).events);
    }
    return out;
  }
  _finish(room, after, event, items) {
    // as RoomService._continue: `before` is the state before any action injected with this message
    const before = room.state;
    const toolCalls = turnToolCalls(room.table, before, after, event);
    room.log.fold(toolCalls, after);
    room.state = after;
    const state = this.agentState(room);
    const deaths = toolCalls.filter((c) => c.name === 'update_player_state' && c.args.state_name === 'is_alive' && c.args.state_value === false).map((c) => c.args.player_id);
    const uiCalls = uiToolCalls(room.table.dsl, state, { table: room.table, turn: event.turn, deaths, items });
    room.panel = M.newestPanel(uiCalls);
    return { state, toolCalls, uiCalls };
  }
  // one findRooms per chunk that holds a thread; [threadId, hit] of the slots a thread owns (a free slot holds a template room or
  // what its last thread left: never reported)
  _scan(want) {
    const owner = new Map();                                   // chunk -> Map(slot -> threadId)
    for (const [threadId, room] of this.rooms) {
      if (!owner.has(room.chunk)) owner.set(room.chunk, new Map());
      owner.get(room.chunk).set(room.slot, threadId);
    }
    const out = [];
    for (const [chunk, slots] of owner) {
      for (const h of chunk.findRooms({ want }).hits) if (slots.has(h.room)) out.push([slots.get(h.room), h]);
    }
    return out;
  }
  /** The threads that wait for a person, and for whom: { threadId: [seats that could act now] } (twin of the Python
   * RoomPoolService.waiting) - one findRooms per chunk instead of a walk over the threads' states. */
  waiting() { return this._serial(() => Object.fromEntries(this._scan(['person']).map(([t, h]) => [t, h.pending]))); }
  /** The threads whose game stands in a terminal phase: [threadId] (twin of the Python RoomPoolService.finished). */
  finished() { return this._serial(() => this._scan(['end']).map(([t]) => t)); }
  _release(threadId) {
    const room = this.rooms.get(threadId);
    if (!room) return false;
    this.rooms.delete(threadId);
    room.pool.free.push([room.ci, room.slot]);
    return true;
  }
  /** Forget a thread (its slot goes back to the pool); without an id, every thread and every chunk's device memory. */
  close(threadId) {
    return this._serial(() => {
      if (threadId !== undefined) return this._release(threadId);
      this.rooms.clear();
      for (const pool of this.pools.values()) for (const c of pool.chunks) c.close();
      this.pools.clear();
      return true;
    });
  }
}

module.exports = { RoomPoolService, roomIndexOf };

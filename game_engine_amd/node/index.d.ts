// Type declarations for the Node/TypeScript host of the MI355X batch stepper.
// The state shapes mirror the reference's TS AgentState (src/lib/canvas/types.ts:338-360).

export interface WerewolfPlayerState {
  role: string; team: '' | 'villagers' | 'werewolves'; is_alive: boolean; role_revealed: boolean;
  can_vote: boolean; has_secret_role: boolean; night_action_eligible: boolean;
  night_action_submitted: boolean; selected_target_id: number;
  investigated_alignments: Record<string, string>;
}
export interface TwoTruthsPlayerState {
  is_speaker: boolean; statements_submitted: boolean; lie_index: number; lie_revealed: boolean;
  can_vote: boolean; vote_choice: number; has_voted: boolean; total_score: number; rounds_as_speaker: number;
}
export interface RoomState {
  current_phase_id: number;
  current_phase_name: string;
  previous_phase_id: number;
  end_turn: number;                 // -1 while the game runs
  games: number;
  /** exactly the fields the DSL declares, under the DSL's own names (GameTable.info.fieldNames) */
  player_states: Record<string, WerewolfPlayerState | TwoTruthsPlayerState | Record<string, unknown>>;
  pack: number;                     // 1 werewolf, 2 two-truths
  slots: unknown[][];               // per player: one value per slot of the pack (GE_WW_* / GE_TT_* order), declared or not
  acted: number[];                  // this visit's action log, per player
  choice: number[];
}
export interface Summary {
  rooms: bigint; finished: bigint; village_wins: bigint; wolf_wins: bigint; alive_players: bigint;
  sum_end_turn: bigint; end_turn_hist: bigint[]; score_hist: bigint[]; checksum: bigint; turn: bigint;
  games_recycled: bigint;
}
export interface TurnEvent {
  turn: number; from_phase_id: number; to_phase_id: number; acted_now: number; restarted: number; choice: number[];
}
export type RunUntil = 'person' | 'end' | 'phase';
export function runUntilBits(until: RunUntil[] | RunUntil | number): number;
export function runUntilNames(bits: number): RunUntil[];
export type FindWant = 'person' | 'end' | 'phase';
export function findWantBits(want: FindWant[] | FindWant | number): number;
export function findWantNames(bits: number): FindWant[];
/** A room findRooms matched: why = the conditions of `want` that hold, pending = the host-driven seats that could act now. */
export interface RoomHit { room: number; why: FindWant[]; pending: number[]; phaseId: number; segment: number; }
/** What adviseSeats says of one choice (or of the policy playing the seat): finished playouts, those the seat's side won, the seat's summed score. */
export interface AdviceOption { finished: number; wins: number; score: number; }
/** adviseSeats's answer for one (room, seat): status 0, or -1 when no choice of the seat would be accepted now (then no options). */
export interface SeatAdvice { status: number; legal: number[]; best: number; phaseId: number; policy: AdviceOption; options: (AdviceOption & { choice: number })[]; }
export interface ToolCall { name: 'update_player_actions' | 'set_next_phase' | 'update_player_state' | 'add_game_note'; args: Record<string, unknown>; }
export interface PhaseInfo { id: number; name: string; completion: number; act: number; effect: number; nBranches: number; }

export class GameTable {
  constructor(dsl: object, rounds?: number);
  static fromGamename(gamename: string, gamesDir?: string, rounds?: number): GameTable;
  /** fieldNames: slot (include/ge_step.h GE_WW_* / GE_TT_*) -> the DSL's own field name, "" = not declared */
  readonly info: { pack: number; rounds: number; minPlayers: number; roleNames: string[]; fieldNames: string[]; phases: PhaseInfo[] };
  phaseName(id: number): string;
}
export interface Segment { table: GameTable; nPlayers: number; nRooms: number; /** bit i: player i+1 is driven by the host (a human) */ humanMask?: number; }
export interface BatchOptions {
  segments: Segment[]; seed?: bigint | number; firstRoom?: bigint | number; device?: number;
  maxFuse?: number; restart?: boolean; trace?: boolean;
}
export class RoomBatch {
  constructor(opts: BatchOptions);
  readonly nRooms: number;
  /** Async steps of one batch are chained; a synchronous call made while one is in flight throws GE_BUSY. */
  step(nTurns?: number): Promise<number>;
  whenIdle<T>(fn: () => T): Promise<T>;
  stepSync(nTurns?: number): number;
  reset(): void;
  /** Checkpoint = readRoomsRaw + the turn; restore = writeRoomsRaw + setTurn into a fresh batch. */
  readRoomsRaw(first: number, count: number): ArrayBuffer;
  writeRoomsRaw(first: number, buffer: ArrayBuffer): void;
  setTurn(turn: number | bigint): void;
  close(): void;
  injectAction(room: number, playerId: number, choice: number): void;
  /** One kernel for many host-driven players' actions; per-action status, 0 = applied. */
  injectActions(rooms: ArrayLike<number | bigint>, playerIds: ArrayLike<number>, choices: ArrayLike<number>): Int32Array;
  readRoom(room: number): RoomState;
  readRooms(first: number, count: number): RoomState[];
  readEvents(first: number, count: number): TurnEvent[][];
  /** One turn of each listed room (local, pairwise distinct), room k keyed as global room keys[k] at turn turns[k]; event k of room k. */
  stepRooms(rooms: ArrayLike<number | bigint>, keys: ArrayLike<number | bigint>, turns: ArrayLike<number>): TurnEvent[];
  stepRoomsPlayout(rooms: ArrayLike<number | bigint>, keys: ArrayLike<number | bigint>, turns: ArrayLike<number>, masks: ArrayLike<number>,
                   playoutKeys: ArrayLike<number | bigint>, nRollouts: number, maxTurns?: number, seed?: number | bigint,
                   fullView?: boolean, /** sequential halving of each decision's playouts (POLICY.md §3h) */ halving?: boolean):
    { events: TurnEvent[]; decided: Uint32Array };
  /** Play each listed room on until a person is needed (POLICY.md §3f): stepRooms's entries (rooms[k], keys[k], turns[k] + t) until the
   *  turn leaves a state named in `until` ("person" | "end" | "phase", or the ABI's bits) or maxTurns turns are played.  events[k] /
   *  views[k] hold one entry per played turn (views: false -> null); stopped[k] = the bits that held after the last turn (0: the limit).
   *  Synchronous; GE_BUSY while an async step() is in flight. */
  runRooms(rooms: ArrayLike<number | bigint>, keys: ArrayLike<number | bigint>, turns: ArrayLike<number>, maxTurns?: number,
           until?: RunUntil[] | RunUntil | number, views?: boolean):
    { played: Uint32Array; stopped: Uint32Array; events: TurnEvent[][]; views: RoomState[][] | null };
  /** The rooms of a range that need attention, as they stand (POLICY.md §3k; the batch is only read): "person" = runRooms's test,
   *  "end" = a terminal phase, "phase" = the room's phase id is in `phases` (ids for every segment, or segment -> ids).  hits: the
   *  first min(matched, cap) matches in ascending room order; cap 0 counts only.  Synchronous; GE_BUSY while an async step() is in flight. */
  findRooms(options?: { want?: FindWant[] | FindWant | number; phases?: number[] | Record<number, number[]> | null; first?: number;
                        count?: number; cap?: number }): { hits: RoomHit[]; matched: number };
  /** Advice for listed seats on the device (POLICY.md §3m): per (rooms[k], seats[k]) the choices injectAction would accept now, each
   *  played as rolloutSeats's entry (keys[k], turns[k], the seat's view or the full view, that one action), and the best of them.
   *  Throws only for a structural error; a seat that cannot act now answers with status -1.  The batch is only read.  Synchronous;
   *  GE_BUSY while an async step() is in flight. */
  adviseSeats(rooms: ArrayLike<number | bigint>, keys: ArrayLike<number | bigint>, turns: ArrayLike<number>, seats: ArrayLike<number>,
              nRollouts: number, maxTurns?: number, seed?: number | bigint, fullView?: boolean): SeatAdvice[];
  /** Per-room host-driven seats (POLICY.md §3l): masks[k] (bit i = seat i + 1 is host-driven) becomes the seat mask of room rooms[k];
   *  step, stepRooms, the run-ons, findRooms and the playout-seat check then honour the room's own mask.  All-or-nothing.
   *  Synchronous; GE_BUSY while an async step() is in flight. */
  setSeats(rooms: ArrayLike<number | bigint>, masks: ArrayLike<number>): void;
  /** The seat masks of rooms first .. first + count - 1 (the segment's mask where none was ever set).  Synchronous; GE_BUSY while an
   *  async step() is in flight. */
  seats(first?: number, count?: number): Uint32Array;
  /** Every room back to its segment's mask.  Synchronous; GE_BUSY while an async step() is in flight. */
  clearSeats(): void;
  /** runRooms with playout seats (POLICY.md §3g): stepRoomsPlayout's entries (rooms[k], keys[k], turns[k] + t, masks[k], playoutKeys[k])
   *  turn after turn, stopped as runRooms stops them, without a host wait between the turns.  decided[k][t]: turn t's decided mask.
   *  Synchronous; GE_BUSY while an async step() is in flight. */
  runRoomsPlayout(rooms: ArrayLike<number | bigint>, keys: ArrayLike<number | bigint>, turns: ArrayLike<number>, masks: ArrayLike<number>,
                  playoutKeys: ArrayLike<number | bigint>, nRollouts: number, playoutMaxTurns?: number, seed?: bigint | number,
                  fullView?: boolean, maxTurns?: number, until?: RunUntil[] | RunUntil | number, views?: boolean, halving?: boolean):
    { played: Uint32Array; stopped: Uint32Array; events: TurnEvent[][]; views: RoomState[][] | null; decided: number[][] };
  /** runRooms with a forecast of every turn it played (POLICY.md §3i): runRooms's result (with views) and stats[k][p], p = 0 ..
   *  played[k]: the 77 rolloutSeats words of room k as it stood at point p (0: before the call; p: after its turn p - 1) under
   *  (forecastKeys[k], turns[k] + p, seats[k], no actions; nRollouts, playoutMaxTurns, seed).  seats null: the full view.
   *  Synchronous; GE_BUSY while an async step() is in flight. */
  runRoomsForecast(rooms: ArrayLike<number | bigint>, keys: ArrayLike<number | bigint>, turns: ArrayLike<number>,
                   forecastKeys: ArrayLike<number | bigint>, nRollouts: number, playoutMaxTurns?: number, seats?: ArrayLike<number> | null,
                   seed?: bigint | number, maxTurns?: number, until?: RunUntil[] | RunUntil | number):
    { played: Uint32Array; stopped: Uint32Array; events: TurnEvent[][]; views: RoomState[][]; stats: BigUint64Array[][] };
  /** Playouts of each listed room (replica r of entry k = global room keys[k] + r under seed, default the batch's): rooms.length x 77
   *  words of ge_rollout_stats (41 summary words, then seat_alive, seat_wins, seat_score x 12).  The batch is only read. */
  rolloutRooms(rooms: ArrayLike<number | bigint>, keys: ArrayLike<number | bigint>, turns: ArrayLike<number>, nRollouts: number,
               maxTurns?: number, seed?: bigint | number): BigUint64Array;
  /** Playouts after given actions: entry k is rolloutRooms's entry with actions[k] ([playerId, choice] pairs) logged in every replica
   *  before its first turn.  status[k] = 0 and entry k's 77 words, or the refused action's status (< 0) and 77 zero words.  Throws only
   *  for a structural error.  The batch is only read. */
  rolloutActions(rooms: ArrayLike<number | bigint>, keys: ArrayLike<number | bigint>, turns: ArrayLike<number>,
                 actions: ArrayLike<ArrayLike<[number, number]>>, nRollouts: number, maxTurns?: number,
                 seed?: bigint | number): { words: BigUint64Array; status: Int32Array };
  /** Playouts from a seat's view (POLICY.md §3c): rolloutActions's entry k with every replica re-dealt, after the actions, over
   *  what seat seats[k] cannot see; seats[k] = 0 is rolloutActions's entry word for word.  actions null: none.  The batch is only read. */
  rolloutSeats(rooms: ArrayLike<number | bigint>, keys: ArrayLike<number | bigint>, turns: ArrayLike<number>, seats: ArrayLike<number>,
               actions: ArrayLike<ArrayLike<[number, number]>> | null, nRollouts: number, maxTurns?: number,
               seed?: bigint | number): { words: BigUint64Array; status: Int32Array };
  /** rolloutSeats with every entry also compared, playout by playout, against entry baseline[k] of the same call (the same room) for
   *  seat subjects[k] (POLICY.md §3e): cmp holds 6 words per entry (compared, better, worse, gain, loss, diff_sq), all zero when the
   *  entry or its baseline was refused.  At most 65 536 entries.  The batch is only read. */
  rolloutCompare(rooms: ArrayLike<number | bigint>, keys: ArrayLike<number | bigint>, turns: ArrayLike<number>, seats: ArrayLike<number>,
                 actions: ArrayLike<ArrayLike<[number, number]>> | null, baseline: ArrayLike<number>, subjects: ArrayLike<number>,
                 nRollouts?: number, maxTurns?: number, seed?: bigint | number): { words: BigUint64Array; status: Int32Array; cmp: BigUint64Array };
  /** rolloutSeats - with baseline and subjects, rolloutCompare - under the caller's beliefs (POLICY.md §3j): 16 bytes per entry, byte c
   *  how much the caller suspects seat c + 1 (Werewolf) or statement c + 1 (Two-Truths), as prior odds 0..255.  Equal weights are
   *  rolloutSeats's entry word for word; nothing in the engine derives the weights.  The batch is only read. */
  rolloutBeliefs(rooms: ArrayLike<number | bigint>, keys: ArrayLike<number | bigint>, turns: ArrayLike<number>, seats: ArrayLike<number>,
                 actions: ArrayLike<ArrayLike<[number, number]>> | null, beliefs: Uint8Array | ArrayLike<ArrayLike<number>>,
                 nRollouts?: number, maxTurns?: number, seed?: bigint | number, baseline?: ArrayLike<number> | null,
                 subjects?: ArrayLike<number> | null): { words: BigUint64Array; status: Int32Array; cmp?: BigUint64Array };
  /** out[k] = room rooms[k] (any order, repeats allowed). */
  readRoomsAt(rooms: ArrayLike<number | bigint>): RoomState[];
  readRoomsAtRaw(rooms: ArrayLike<number | bigint>): ArrayBuffer;
  /** views[k] -> room rooms[k] (pairwise distinct): one copy and one device scatter; all or nothing. */
  writeRoomsAt(rooms: ArrayLike<number | bigint>, views: ArrayBuffer | ArrayBuffer[]): void;
  /** Adopt a reference AgentState into one room (agentStateToView); returns its host-side fields. */
  writeAgentState(room: number, state: AgentStateInput, visitActions?: Record<string, number>): HostSide;
  writeAgentStates(rooms: ArrayLike<number>, states: AgentStateInput[], visitActions?: (Record<string, number> | undefined)[]): HostSide[];
  summary(): Summary;
}
/** One Node process, several GPUs: device d owns the global rooms [firstRoom + d*R, firstRoom + (d+1)*R). */
export class ShardedBatch {
  constructor(opts: { segments: Segment[]; devices: number[]; seed?: bigint; firstRoom?: bigint; maxFuse?: number; restart?: boolean; trace?: boolean });
  readonly nRooms: number;
  readonly roomsPerDevice: number;
  readonly shards: RoomBatch[];
  step(nTurns?: number): Promise<bigint | number>;
  reset(): void;
  close(): void;
  readRoom(room: number): RoomState;
  injectAction(room: number, playerId: number, choice: number): void;
  summary(): Summary;
}
/** The native device group (ge_group_*): ONE Node process, N distinct GPUs.  `segments` = the WHOLE job, split per segment
 * over the devices with the global room indices of one RoomBatch; summary() = per-device reductions + ONE RCCL all-gather
 * inside libge_step.so.  (ShardedBatch is the host-side form: host-summed, also runs several shards on one device.) */
export class DeviceGroup {
  constructor(opts: { segments: Segment[]; devices: number[]; seed?: bigint; firstRoom?: bigint; maxFuse?: number; restart?: boolean; trace?: boolean });
  readonly nRooms: number;
  readonly devices: number[];
  step(nTurns?: number): Promise<void>;
  whenIdle<T>(fn: () => T): Promise<T>;
  summary(): Summary;
  /** room = index in segment-major order, as in one RoomBatch of the same segments */
  readRoom(room: number): RoomState;
  locate(room: number): [number, number, GameTable];   // via locateInShards
  close(): void;
}
export function turnToolCalls(table: GameTable, before: RoomState, after: RoomState, event: TurnEvent): ToolCall[];
/** What _execute_add_game_note appends: '<mark> <TYPE>: <content>' (backend_tools.py:175-198). */
export function formatNote(noteType: string, content: string): string;
/** playerActions / game_notes / phase_history / statements of one room, folded from each turn's tool calls as the reference's _execute_* would. */
export class RoomLog {
  constructor(table: GameTable, names: string[], gameName?: string);
  fold(calls: ToolCall[], after: RoomState, now?: number): void;
  agentState(room: RoomState): Record<string, unknown>;
}
export function loadDslByGamename(gamename: string, gamesDir?: string): object;
export function deviceCount(): number;
/** route.ts:62-70 file matching (case-insensitive, non-alphanumerics equal '-') */
export function findGameFile(gameName: string, gamesDir?: string): string | null;
export interface RoomPlayer { id?: string; name: string; isHost?: boolean; gamePlayerId?: string; }
/** POST /api/games/initialize-players (route.ts:83-166) without the HTTP layer */
export function initializePlayers(dsl: object, roomPlayers: RoomPlayer[]): { player_states: Record<string, Record<string, unknown>>; fallback_mode?: boolean; message?: string };
export function compileCriteria(expr: string): (player: Record<string, unknown>) => boolean;
export function audienceGroups(dsl: object, playerStates: Record<string, Record<string, unknown>>): Record<string, string[]>;
export interface FrontendToolCall { name: string; args: { audience_type?: boolean; audience_ids?: string[]; [k: string]: unknown }; }
/** Frontend tool calls of the room's current phase (ActionExecutor / UIUpdateNode without an LLM): every parameter the
 * handler requires (frontend_tools.json), nothing it does not declare. */
export function uiToolCalls(dsl: object, room: RoomState, opts?: { table?: GameTable; act?: number; turn?: number; deaths?: string[];
  items?: { id: string; type: string }[] }): FrontendToolCall[];
export function validateCall(call: FrontendToolCall): string[];
/** [part, index inside the part's batch, segment] of a room of the whole job after the group's sharding (ge_group_partition). */
export function locateInShards(segmentRooms: number[], nParts: number, room: number): [number, number, number];

/** A reference AgentState as a LangGraph thread holds it (agent/game_agent_v2.py:97-117). */
export interface AgentStateInput {
  current_phase_id: number;
  player_states: Record<string, Record<string, unknown>>;
  playerActions?: Record<string, { name?: string; actions: Record<string, { action: string; phase: string; id?: string }> }>;
  phase_history?: { phase_id: number; phase_name?: string }[];
  game_notes?: string[];
  previous_phase_id?: number;
  end_turn?: number;
  games?: number;
}
/** What the record does not carry: names, Two-Truths statements, and keys the record does not model, per player id. */
export interface HostSide {
  names: Record<string, string>;
  statements: Record<string, Record<string, string>>;
  extra: Record<string, Record<string, unknown>>;
}
/** The room view of an AgentState (one ge_room_view); TypeError for a wrong type, RangeError for a value that does not fit. */
export function agentStateToView(table: GameTable, state: AgentStateInput,
                                 opts?: { nPlayers?: number; visitActions?: Record<string, number> }): { view: ArrayBuffer; hostSide: HostSide };

// Types for room_pool.js — many game threads hosted in a few resident batches.
import { AdoptOptions, Advice, AgentStateView, Forecast, Hint, PlayoutOptions, RoomPlayer, RunOptions, RunResult, RunUntil, TurnResult } from './room_service';

export type MessageResult = TurnResult & { played: boolean; kind: 'chat' | 'control' | 'action' };
export class RoomPoolService {
  /** chunkRooms: slots per batch chunk of a pool (one pool per game, player count and human seats) */
  constructor(opts?: { gamesDir?: string; seed?: bigint | number; device?: number; chunkRooms?: number } & PlayoutOptions);
  /** As RoomService.createRoom: the thread's RNG is keyed by roomIndex (default: hash of the thread id), its turn counter starts at 0. */
  createRoom(opts: { threadId: string; gameName: string; players: RoomPlayer[]; dsl?: object; roomIndex?: number | bigint; playoutSeats?: number[] }): AgentStateView;
  /** As RoomService.adoptRoom for many threads: every state is converted before a slot is taken, then one writeRoomsAt per chunk. */
  adoptRooms(entries: AdoptOptions[]): Promise<TurnResult[]>;
  humanAction(threadId: string, playerId: number, choice: number): Promise<AgentStateView>;
  /** A seat changes hands mid-game (POLICY.md §3l): from the next turn on exactly `seats` (player ids) are played by people.  Rejects
   *  for an unknown thread or a seat outside 1..n, before anything changes; resolves with the seats. */
  setHumanSeats(threadId: string, seats: number[]): Promise<number[]>;
  continueRoom(threadId: string, items?: { id: string; type: string }[]): Promise<TurnResult>;
  /** As RoomService.runRoom, from the thread's pool slot. */
  runRoom(threadId: string, maxTurns?: number, until?: RunUntil[], items?: { id: string; type: string }[], options?: RunOptions): Promise<RunResult>;
  /** The threads that wait for a person, and the seats that could act now in each: one findRooms per chunk (POLICY.md §3k). */
  waiting(): Promise<Record<string, number[]>>;
  /** The threads whose game stands in a terminal phase. */
  finished(): Promise<string[]>;
  /** runRoom for many threads, in order: one runRooms call per chunk touched; a thread may be named once.  items[j]: thread j's items.
   *  options.forecast: one runRoomsForecast call per chunk touched instead, and every result gains forecasts (options.seats[j]: thread j's seat). */
  runRooms(threadIds: string[], maxTurns?: number, until?: RunUntil[], items?: ({ id: string; type: string }[] | undefined)[],
           options?: RunOptions): Promise<RunResult[]>;
  handleMessage(threadId: string, text: string, items?: { id: string; type: string }[]): Promise<MessageResult>;
  /** One tick for many threads (each at most once): per chunk touched one stepRooms and one readRoomsAt; outputs in input order. */
  handleMessages(msgs: [string, string, { id: string; type: string }[]?][]): Promise<MessageResult[]>;
  /** As RoomService.forecast (same keys, seed and output), from the thread's slot. */
  forecast(threadId: string, nRollouts?: number, maxTurns?: number, seat?: number, beliefs?: Record<number, number>): Promise<Forecast>;
  /** Forecasts of many threads in order: one rolloutRooms per chunk touched. */
  forecasts(threadIds: string[], nRollouts?: number, maxTurns?: number, seats?: (number | undefined)[],
            beliefs?: (Record<number, number> | undefined)[]): Promise<Forecast[]>;
  /** As RoomService.advise (same candidates, keys, seed and output), from the thread's slot. */
  advise(threadId: string, playerId?: number, nRollouts?: number, maxTurns?: number, view?: 'full' | 'seat', compare?: boolean,
         beliefs?: Record<number, number>): Promise<Advice>;
  /** Advice for many threads in order (playerIds[j] absent: thread j's lowest human seat): one rolloutActions per chunk touched
   *  (with compare one rolloutCompare, and every option gains "versus"). */
  advises(threadIds: string[], playerIds?: (number | undefined)[], nRollouts?: number, maxTurns?: number,
          view?: 'full' | 'seat', compare?: boolean, beliefs?: (Record<number, number> | undefined)[]): Promise<Advice[]>;
  /** Hints for many (thread, seat) pairs: one adviseSeats per chunk touched.  Without threadIds: every thread waiting() reports, each
   *  of its pending seats; with them, playerIds[j] (absent: thread j's lowest human seat). */
  hints(threadIds?: string[] | null, playerIds?: (number | undefined)[] | null, nRollouts?: number, maxTurns?: number,
        view?: 'full' | 'seat'): Promise<Hint[]>;
  /** Forget a thread (its slot is reused); without an id, every thread and every chunk's device memory. */
  close(threadId?: string): Promise<boolean>;
}
export function roomIndexOf(threadId: string): bigint;

// Types for room_service.js — the single-room (one LangGraph thread) drop-in.
import { RoomState, ToolCall, FrontendToolCall, AgentStateInput } from './index';

export interface RoomPlayer { name?: string; gamePlayerId?: number; /** false marks a human seat (host-driven) */ isBot?: boolean; }
/** AgentState as the frontend syncs it (src/lib/canvas/types.ts:338-360), log-shaped parts included. */
export interface AgentStateView {
  gameName: string; current_phase_id: number; current_phase_name: string;
  player_states: Record<string, Record<string, unknown>>;
  playerActions: Record<string, { name: string; actions: Record<string, { action: string; timestamp: number; phase: string; id: string }> }>;
  phase_history: { phase_id: number; phase_name: string }[];
  game_notes: string[];
}
export interface AdoptOptions {
  threadId: string; gameName: string; state: AgentStateInput; players?: RoomPlayer[]; /** player ids of human seats */ humanSeats?: number[];
  dsl?: object; roomIndex?: number | bigint; /** the thread's next turn (default phase_history.length) */ turn?: number;
  /** a human seat's action already logged in this visit: {playerId: choice} */ visitActions?: Record<string, number>;
  /** bot seats that choose each action by playouts (POLICY.md §3d) */ playoutSeats?: number[];
}
/** How the playout bots of threads created with playoutSeats choose (POLICY.md §3d): nRollouts (default 256) and maxTurns (256)
 * of each candidate's playouts, from the bot's own view ("seat", the default) or the true record ("full": a cheating bot).
 * playoutHalving (default false): sequential halving of each decision's playouts (POLICY.md §3h) - fewer playouts, more launches
 * per turn, and slower at every shape measured (DESIGN.md §4); a bot's candidate values are then advise's option forecasts for the finalists only. */
export interface PlayoutOptions { playoutRollouts?: number; playoutMaxTurns?: number; playoutView?: 'seat' | 'full'; playoutHalving?: boolean; }
export interface TurnResult { state: AgentStateView; toolCalls: ToolCall[]; uiCalls: FrontendToolCall[]; }
/** runRoom: one TurnResult per played turn; stopped: the conditions that held after the last one ([]: the limit). */
export type RunUntil = 'person' | 'end' | 'phase';
/** runRoom / runRooms options.  playout: run threads with playout seats too, by one runRoomsPlayout call (POLICY.md §3g); without
 *  it such a thread is refused. */
export interface RunOptions {
  playout?: boolean;
  /** a win-odds timeline of the run (POLICY.md §3i): the result gains forecasts, one Forecast per point 0 .. played, each what
   *  forecast(threadId, rollouts, maxTurns, seat) would have resolved at that moment; a thread with playout seats is refused */
  forecast?: boolean;
  /** forecast's nRollouts (default 4096), maxTurns (default 1024) and seat (default: the full view) */
  rollouts?: number; maxTurns?: number; seat?: number;
  /** RoomPoolService.runRooms: the seat of each thread's forecasts (instead of one seat for all) */
  seats?: (number | undefined)[];
}
export interface RunResult { turns: TurnResult[]; played: number; stopped: RunUntil[]; forecasts?: Forecast[]; }
/** How a thread ends from where it stands, over `rollouts` playouts (JSON integers: divide by rollouts for odds). */
export interface Forecast {
  threadId: string; turn: number; rollouts: number; maxTurns: number;
  /** playouts that reached a terminal phase; the sum of their end turns; those with an end turn */
  finished: number; endTurnSum: number; ended: number;
  /** present when the forecast is from a seat's view */
  seat?: number;
  /** Werewolf: finished playouts won by each side */
  sides?: { villagers: number; werewolves: number };
  /** Werewolf: {name, alive, wins}; Two-Truths: {name, scoreSum, topScore} */
  players: Record<string, { name: string; alive?: number; wins?: number; scoreSum?: number; topScore?: number }>;
}
/** The forecast for each choice a seat can make now, beside the policy's (INTEGRATION.md "Advising a seat"). */
export interface Advice {
  threadId: string; turn: number; playerId: number; phaseId: number; rollouts: number; maxTurns: number;
  /** the thread's forecast: the policy's own choice */
  policy: Forecast;
  /** the accepted candidates in ascending order; label = the seat's name (Werewolf) or the statement number (Two-Truths) */
  options: { choice: number; label: string; forecast: Forecast;
             /** with compare: the option against the policy's entry, playout by playout, for the advised seat (POLICY.md §3e) */
             versus?: { compared: number; better: number; worse: number; gain: number; loss: number; diffSq: number } }[];
  /** "seat" when every playout started from what the advised seat knows */
  view?: 'seat';
  /** true when the options carry "versus" */
  compare?: true;
}
/** advise in a few numbers per choice, ranked on the device (INTEGRATION.md "Hints for everyone who waits"). */
export interface Hint {
  threadId: string; turn: number; playerId: number; phaseId: number; rollouts: number; maxTurns: number;
  /** the choice with the most wins (Two-Truths: the highest score), the lowest on a tie; null when the seat has nothing to do now */
  best: number | null;
  /** the policy plays the seat; null when the seat has nothing to do now */
  policy: { finished: number; wins: number; score: number } | null;
  /** the choices the seat can make now, ascending: the advised seat's own wins / topScore, scoreSum and the finished playouts of advise's option forecast */
  options: { choice: number; label: string; wins: number; score: number; finished: number }[];
  view?: 'seat';
}
export class RoomService {
  constructor(opts?: { gamesDir?: string; seed?: bigint | number; device?: number } & PlayoutOptions);
  createRoom(opts: { threadId: string; gameName: string; players: RoomPlayer[]; dsl?: object; /** global room index the RNG is keyed by (default: hash of the thread id) */ roomIndex?: number | bigint;
                     /** bot seats that choose each action by playouts (POLICY.md §3d; RangeError for a human seat or an id outside 1..n) */ playoutSeats?: number[] }): AgentStateView;
  /** Take over a thread that is already mid-game (INTEGRATION.md "Handing a running thread to the stepper"): toolCalls is empty,
   *  uiCalls the UI of the phase now showing.  Throws TypeError / RangeError for a state that does not fit, before anything changes. */
  adoptRoom(opts: AdoptOptions): TurnResult;
  /** Requests of one thread are served strictly one after the other. */
  humanAction(threadId: string, playerId: number, choice: number): Promise<AgentStateView>;
  /** A seat changes hands mid-game (POLICY.md §3l): from the next turn on exactly `seats` (player ids) are played by people.  Rejects
   *  for an unknown thread or a seat outside 1..n, before anything changes; resolves with the seats. */
  setHumanSeats(threadId: string, seats: number[]): Promise<number[]>;
  /** One message of the browser, as the reference's graph reads it (page.tsx:272-275, 302-305, 341-349, 2774, 2843, 2962;
   *  POLICY.md 3b): chat plays no turn; anything else plays one, after a game message was logged under Player 1 and - where it
   *  is a valid action of a host-driven seat - applied. */
  handleMessage(threadId: string, text: string, items?: { id: string; type: string }[]): Promise<TurnResult & { played: boolean; kind: 'chat' | 'control' | 'action' }>;
  /** items: the frontend's canvas items (AgentState.items), for clearCanvas's exemptList */
  continueRoom(threadId: string, items?: { id: string; type: string }[]): Promise<TurnResult>;
  /** The thread played on until a person is needed (POLICY.md §3f): turns[t] is what continueRoom would have resolved for that turn.
   *  Rejects with a RangeError, before anything runs, for a thread with playout seats, maxTurns outside 1 .. 4096 or an unknown condition. */
  runRoom(threadId: string, maxTurns?: number, until?: RunUntil[], items?: { id: string; type: string }[], options?: RunOptions): Promise<RunResult>;
  /** nRollouts playouts (<= 65 536) of the thread's room, every seat played by the policy, keyed (threadKey << 16) + r under seed
   *  (service seed ^ 0x9E3779B97F4A7C15); the thread is not changed (INTEGRATION.md "Forecasting a thread").  seat: from what that
   *  seat knows (hidden roles / the lie dealt again per replica); the JSON gains "seat".  beliefs (with seat): what it suspects,
   *  { seat or statement number: 0..255 }, unnamed ones 16 (INTEGRATION.md "Advising a seat from what it suspects"); the JSON gains "beliefs". */
  forecast(threadId: string, nRollouts?: number, maxTurns?: number, seat?: number, beliefs?: Record<number, number>): Promise<Forecast>;
  /** For every choice playerId (default: the lowest human seat; RangeError if there is none) can make now, the forecast given
   *  that choice, under forecast's keys and seed; the thread is not changed (INTEGRATION.md "Advising a seat").  view "seat": from
   *  what that seat knows, the form to show a player (INTEGRATION.md "Advising a seat from what it knows"); the JSON gains "view".
   *  compare: every option gains "versus" and the JSON "compare": true (INTEGRATION.md "Is this choice really better?"); the rest is unchanged.
   *  beliefs (view "seat" only): as forecast's; the JSON gains "beliefs", the 16 bytes used. */
  advise(threadId: string, playerId?: number, nRollouts?: number, maxTurns?: number, view?: 'full' | 'seat', compare?: boolean,
         beliefs?: Record<number, number>): Promise<Advice>;
  /** advise's numbers for playerId (default: the lowest human seat) without the per-option forecasts: the legal choices found, played
   *  and ranked on the device (RoomBatch.adviseSeats) under advise's keys and seed.  view defaults to "seat".  The thread is not changed. */
  hint(threadId: string, playerId?: number, nRollouts?: number, maxTurns?: number, view?: 'full' | 'seat'): Promise<Hint>;
  /** Forget a thread and free its device memory; resolves false for an unknown thread. */
  close(threadId: string): Promise<boolean>;
  serve(port?: number): Promise<import('http').Server>;
}
export function roomIndexOf(threadId: string): bigint;
export type { RoomState };

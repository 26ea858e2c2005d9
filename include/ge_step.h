/* ge_step.h — C ABI of the MI355X batch room-phase stepper (libge_step.so).
 *
 * Drop-in boundary for ONE path of liruihan000/game_engine: the per-turn loop
 *   InitialRouterNode -> BotBehaviorNode -> PhaseNode -> RefereeNode -> ActionExecutor
 *   (reference agent/game_agent_v2.py:198/468/987/619/1243, graph :1571-1587;
 *    newer fused form agent/game_agent_v3.py:205/448/540)
 * which the reference runs one room per LangGraph thread (src/app/api/copilotkit/route.ts:22-47)
 * with an LLM call per node.  Here the same turn is applied to a BATCH of independent rooms
 * on the GPU with the LLM replaced by the fixed policy of POLICY.md.
 *
 * Conventions:
 *   - plain C, no torch / STL types; every function returns 0 or a negative ge_status;
 *     nothing throws or aborts across this boundary; HIP errors map to GE_ERR_HIP.
 *   - the caller owns every host buffer it passes; the library owns device memory behind
 *     the opaque ge_batch handle.
 *   - a handle is not thread-safe: one handle per host thread / GPU.  Every call leaves the
 *     calling thread's current HIP device as it found it.
 *   - ge_batch_step is asynchronous on the given stream; read / summary / sync synchronise.
 *     Consecutive ge_batch_step calls may name different streams: the library orders each call
 *     behind the previous one with an event, and every synchronising call waits for the stream
 *     of the most recent step (which, by that ordering, is behind all earlier ones).
 *   - there is NO CPU fallback: without a HIP device ge_batch_create fails with GE_ERR_NO_DEVICE.
 */
#ifndef GE_STEP_H
#define GE_STEP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI history (a host checks ge_abi_version() == GE_ABI_VERSION; a ge_game_table carries the version it was compiled by):
 *   2  stream ordering, device-side reset, batched injection     3  ge_game_table.field_names (schema binding)
 *   4  device group (ge_group_*, GE_ERR_COMM); ge_batch_write_rooms became all-or-nothing and REFUSES (GE_ERR_ARG) a view whose
 *      `pack` / player count is not the segment's or whose phase ids name no row of its table (until then unknown ids were
 *      silently stored as row 0) - a caller that zero-initialises views must set `pack`
 *   5  ge_group_partition + ge_batch_create_shard (the group's sharding arithmetic for hosts that place shards themselves); ge_last_rejected_room;
 *      mixed and generic batches get single-turn kernel builds; the Werewolf x 12 deal side plane is allocated on first use;
 *      later additions, new symbols only (the version stays 5): ge_batch_step_rooms + ge_batch_read_rooms_at (many game threads
 *      in one resident batch, each room stepped under its own key and turn); ge_batch_write_rooms_at (the indexed write);
 *      ge_batch_rollout_rooms + ge_rollout_stats (on-device playouts of listed rooms: win odds per side and per seat);
 *      ge_batch_rollout_actions (playouts that start from given actions: win odds per choice a seat can make now);
 *      ge_batch_rollout_seats (the same playouts from what one seat knows: hidden roles / the lie dealt again per replica);
 *      ge_batch_step_rooms_playout + GE_PLAYOUT_FULL_VIEW (playout seats: bots that choose each action by their own playouts);
 *      ge_batch_rollout_compare + ge_compare_stats (an entry against a baseline entry, playout by playout: the paired counts);
 *      ge_batch_run_rooms + GE_RUN_UNTIL_* (listed rooms played on until a person is needed: many turns per call, every turn traced);
 *      ge_batch_run_rooms_playout (the same with playout seats: the playouts of every turn enqueued without the host in between);
 *      ge_batch_run_rooms_forecast (ge_batch_run_rooms with the ge_batch_rollout_seats forecast of every turn it played: a win-odds timeline);
 *      GE_PLAYOUT_HALVING (a new flag of both playout-seat calls, no new symbol: sequential halving of each decision's playout
 *      budget; a library from before it refuses the bit with GE_ERR_ARG);
 *      ge_batch_rollout_beliefs + GE_BELIEF_SLOTS (seat-view playouts and comparisons whose re-deal is weighted by the caller's suspicions);
 *      ge_batch_find_rooms + ge_room_hit + GE_FIND_* (a device scan of a range: the rooms that wait for a person, have ended or stand in given phases);
 *      ge_batch_advise_seats + ge_advice + GE_ADVISE_FULL_VIEW (listed seats advised on the device: their legal choices found, played and ranked);
 *      ge_batch_observe_seats + ge_batch_act_seats + ge_seat_obs (a seat of every room observed into, and played from, device memory the caller owns);
 *      ge_batch_teach_seats (ge_batch_advise_seats for a seat list of every room of a range, into device memory the caller owns);
 *      ge_batch_run_seats + GE_RUN_UNTIL_SEAT (every room of a range played on until a listed seat must act, turn counts and stop bits in device memory);
 *      ge_batch_gather_seats + ge_batch_act_listed + GE_GATHER_* (decision lists: the due (room, seat) entries of a range compacted in order with their observations, and played from such a list) */
#define GE_ABI_VERSION 5
#define GE_MAX_PHASES 32
#define GE_MAX_PLAYERS 12
#define GE_MAX_SEGMENTS 4
#define GE_MAX_TERMS 4
#define GE_MAX_CLAUSES 4
#define GE_MAX_BRANCHES 4
#define GE_NAME_LEN 64
#define GE_MAX_SLOTS 12

typedef enum ge_status {
    GE_OK = 0,
    GE_ERR_ARG = -1,        /* null pointer, bad size, out-of-range value */
    GE_ERR_DSL = -2,        /* the DSL cannot be compiled (message in the err buffer) */
    GE_ERR_NO_DEVICE = -3,  /* no usable HIP device: the product has no CPU path */
    GE_ERR_HIP = -4,        /* a HIP runtime call failed (ge_last_hip_error) */
    GE_ERR_NOMEM = -5,
    GE_ERR_RANGE = -6,      /* room range outside the batch / turn counter would overflow */
    GE_ERR_UNSUPPORTED = -7,/* valid DSL feature the kernels do not implement yet; no RCCL to load for a device group */
    GE_ERR_COMM = -9        /* an RCCL call failed (ge_last_comm_error); -8 is the N-API host's GE_BUSY */
} ge_status;

/* rule packs: which declared player_states schema the game uses
 * (reference games/werewolf-(mafia).yaml:21-72, games/two-truths-and-a-lie.yaml declaration) */
enum { GE_PACK_WEREWOLF = 1, GE_PACK_TWO_TRUTHS = 2 };
/* State slots of the packs, in ge_room_view.players[] column order (0..8), then the slots that are not columns.
 * A generated DSL names its fields itself: each slot binds to the name the declaration uses for it
 * (ge_game_table.field_names; e.g. the reference's earlier Werewolf draft, game_draft/werewolf-(mafia).yaml:30-75,
 * says has_night_action / known_alignments / wolf_chat_enabled and declares no selected_target_id).  A slot the
 * DSL does not declare still exists in the record; it is just not part of the room's player_states. */
enum { GE_WW_ROLE = 0, GE_WW_TEAM, GE_WW_IS_ALIVE, GE_WW_ROLE_REVEALED, GE_WW_CAN_VOTE, GE_WW_HAS_SECRET_ROLE,
       GE_WW_NIGHT_ELIGIBLE,      /* night_action_eligible | has_night_action */
       GE_WW_NIGHT_SUBMITTED, GE_WW_SELECTED_TARGET,
       GE_WW_DET_MEMORY,          /* investigated_alignments | known_alignments (ge_room_view.det) */
       GE_WW_WOLF_CHAT,           /* wolf_chat_enabled: derived, = (team == werewolves) (POLICY.md 3a) */
       GE_WW_SLOTS };
enum { GE_TT_IS_SPEAKER = 0, GE_TT_STATEMENTS_SUBMITTED, GE_TT_LIE_INDEX, GE_TT_LIE_REVEALED, GE_TT_CAN_VOTE,
       GE_TT_VOTE_CHOICE, GE_TT_HAS_VOTED, GE_TT_TOTAL_SCORE, GE_TT_ROUNDS_AS_SPEAKER,
       GE_TT_STATEMENTS,          /* text the record does not carry; follows statements_submitted */
       GE_TT_SLOTS };
/* completion_criteria.type (dsl_phases_generation_prompt.txt:106-150) */
enum { GE_COMP_UI = 0, GE_COMP_TIMER = 1, GE_COMP_ACTION = 2 };
/* what a bot action in a player_action phase means (bot_behavior_system_prompt.txt:21-56) */
enum { GE_ACT_NONE = 0, GE_ACT_WOLF_TARGET, GE_ACT_DOCTOR_PROTECT, GE_ACT_DETECTIVE, GE_ACT_DAY_VOTE,
       GE_ACT_TT_STATEMENTS, GE_ACT_TT_LIE, GE_ACT_TT_VOTE };
/* what the Referee applies when a phase is entered (referee_system_prompt_2.txt:1-8,19-22,75-82) */
enum { GE_EFF_NONE = 0, GE_EFF_ASSIGN_ROLES, GE_EFF_NIGHT_BEGIN, GE_EFF_NIGHT_RESOLVE, GE_EFF_DAY_RESOLVE,
       GE_EFF_TT_ROUND_START, GE_EFF_TT_REVEAL, GE_EFF_TT_SCORE };
/* resolver bound to a natural-language next_phase key (ww:435-447, tt "Check Round Progress") */
enum { GE_RES_ALWAYS = 0, GE_RES_WOLVES_ZERO, GE_RES_WOLVES_GE_VILLAGERS, GE_RES_FOLLOWS_DAY,
       GE_RES_FOLLOWS_NIGHT, GE_RES_ALL_ROUNDS_DONE, GE_RES_OTHERWISE };

/* numeric player fields a target condition may compare (declared `num` fields of the rule packs:
 * werewolf selected_target_id; two-truths lie_index, vote_choice, total_score, rounds_as_speaker) */
enum { GE_NUM_SELECTED_TARGET = 0, GE_NUM_LIE_INDEX = 1, GE_NUM_VOTE_CHOICE = 2, GE_NUM_TOTAL_SCORE = 3,
       GE_NUM_ROUNDS_AS_SPEAKER = 4 };
enum { GE_LIT_NONE = 0, GE_LIT_BASE = 1, GE_LIT_NUM = 2 };

/* One literal of a target condition in clause form (OR of AND-clauses).  The grammar is the one the
 * reference's DSL generator is told to write (agent/prompt/dsl_phases_generation_prompt.txt:120-132):
 *   player.<field> ==|!=|<|<=|>|>= <value>,  player.<field> in [..] / not in [..],  joined by and / or.
 * GE_LIT_BASE: the player has ANY of the base predicates in the bit set `bases` (== / != / in over booleans
 * and enums, POLICY.md §3 numbering); GE_LIT_NUM: lo <= player.<num_field> <= hi (lo > hi: never true).
 * `neg` inverts the literal. */
typedef struct ge_literal {
    uint8_t kind;                         /* GE_LIT_* */
    uint8_t neg;
    uint8_t num_field;                    /* GE_NUM_* (GE_LIT_NUM) */
    uint8_t pad;
    uint16_t bases;                       /* GE_LIT_BASE: bit b = base predicate b */
    uint8_t lo, hi;                       /* GE_LIT_NUM */
} ge_literal;

/* One DSL phase, compiled.  Replaces what the LLM reads out of dsl['phases'][id] each turn
 * (v2:1057, 1087-1103). */
typedef struct ge_phase_row {
    int32_t phase_id;                     /* DSL id (0..16, 99, ...) */
    uint8_t completion;                   /* GE_COMP_* */
    uint8_t act;                          /* GE_ACT_*  (GE_COMP_ACTION phases) */
    uint8_t effect;                       /* GE_EFF_*  applied when this phase is entered */
    uint8_t n_terms;                      /* target_players.condition: AND of terms */
    uint8_t term_base[GE_MAX_TERMS];      /* base predicate index inside the pack (POLICY.md) */
    uint8_t term_neg[GE_MAX_TERMS];       /* 1: the term is "== false" / "!=" */
    uint8_t n_branches;                   /* 0: terminal phase (next_phase: null) */
    uint8_t br_res[GE_MAX_BRANCHES];      /* GE_RES_*, evaluated in DSL order, first match wins */
    uint8_t br_target[GE_MAX_BRANCHES];   /* dense row index of the successor */
    uint8_t pad[3];
    char name[GE_NAME_LEN];               /* phases.<id>.name, UTF-8, truncated */
    /* target_players.condition in clause form: always filled.  `generic` = 0: the condition is the plain
     * conjunction term_base / term_neg above (what both shipped games use; the kernels' fast path);
     * 1: only the clause form describes it (or / in [..] with several values / numeric comparisons). */
    uint8_t generic;
    uint8_t n_clauses;                    /* 0: no condition (every living player) */
    uint8_t clause_len[GE_MAX_CLAUSES];
    uint8_t pad2[2];
    ge_literal clause[GE_MAX_CLAUSES][GE_MAX_TERMS];
} ge_phase_row;

/* A compiled game (one YAML file).  Host-visible so callers may inspect or build one by hand. */
typedef struct ge_game_table {
    int32_t abi_version;
    int32_t pack;                         /* GE_PACK_* */
    int32_t n_phases;
    int32_t rounds;                       /* two-truths: agreed speaking turns per player */
    int32_t min_players;                  /* declaration.min_players */
    uint8_t init_fields[12];              /* player_states_template, canonical field order */
    char role_names[5][GE_NAME_LEN];      /* werewolf: "", Villager, Werewolf, Doctor, Detective as declared */
    char field_names[GE_MAX_SLOTS][GE_NAME_LEN];  /* slot (GE_WW_* / GE_TT_*) -> declared field name, "" = not declared */
    ge_phase_row rows[GE_MAX_PHASES];
} ge_game_table;

/* Compiles a game DSL given as JSON text (the host parses YAML with its own loader, as the
 * reference does: yaml.safe_load in agent/tools/utils.py:572, js-yaml in
 * src/app/api/games/initialize-players/route.ts).  Replaces the LLM's reading of the DSL.
 * `err` (may be NULL) receives a NUL-terminated message on GE_ERR_DSL. */
int ge_table_compile_json(const char *dsl_json, size_t len, int rounds, ge_game_table *out,
                          char *err, size_t err_cap);

/* Row `row` of the device phase table (8 words, csrc/ge_layout.h DevRow) as a batch segment of `n_players` players of this
 * table gets it.  Host arithmetic only, no GPU: for inspection and tests of the image the kernels read. */
int ge_table_dev_row(const ge_game_table *tb, uint32_t n_players, uint32_t row, uint32_t *out8);

/* Canonical, layout-independent view of one room: the integer projection of the reference's
 * AgentState (v2:97-117): current_phase_id, phase history tail, player_states fields.
 * players[i] = player id i+1; field order per pack:
 *   werewolf : role team is_alive role_revealed can_vote has_secret_role night_action_eligible
 *              night_action_submitted selected_target_id acted choice
 *   two-truths: is_speaker statements_submitted lie_index lie_revealed can_vote vote_choice
 *              has_voted total_score rounds_as_speaker acted choice
 * (acted/choice = this visit's latest logged action per player, i.e. the playerActions log
 *  of bt:285-344 reduced to what later turns read.)
 * det[i]: the Detective's investigated_alignments for player i+1: 0 unknown, 1 villagers, 2 werewolves. */
typedef struct ge_room_view {
    int32_t phase_id;
    int32_t prev_phase_id;
    int32_t end_turn;                     /* turn in which a terminal phase was entered (saturates at 65534), else -1 */
    int32_t games;                        /* GE_FLAG_RESTART: games this slot completed before the current one */
    uint8_t phase0_done;                  /* phase-0 guard of v2:1025-1052 already taken */
    uint8_t n_players;
    uint8_t pack;
    uint8_t pad;
    uint8_t players[16][12];
    uint8_t det[16];
} ge_room_view;

/* What one turn of one room logged and decided (GE_FLAG_TRACE). */
typedef struct ge_turn_event {
    uint32_t turn;
    int32_t from_phase_id;                /* current_phase_id when the turn started */
    int32_t to_phase_id;                  /* ... when it ended (== from: no transition) */
    uint16_t acted_now;                   /* bit i: player i+1 logged an action this turn (BotBehaviorNode) */
    uint8_t restarted;                    /* GE_FLAG_RESTART: the slot was re-initialised at the start of this turn */
    uint8_t pad;
    uint8_t choice[16];                   /* the choice each of those players logged (player id / statement no.) */
} ge_turn_event;

typedef struct ge_segment_desc {
    const ge_game_table *table;           /* copied at create; need not outlive the call */
    uint32_t n_players;                   /* werewolf 4..12, two-truths 3..12 */
    uint32_t human_mask;                  /* bit i: player i+1 is driven by the host (a human), not by the bot
                                             policy: BotBehaviorNode never acts for it (the reference excludes
                                             player 1, bot_behavior_system_prompt.txt:3) and a phase waits for its
                                             action (ge_batch_inject_action).  0 = all bots. */
    uint64_t n_rooms;
} ge_segment_desc;

/* ge_batch_desc.flags */
#define GE_FLAG_NONE 0u
/* steady state: a room that starts a turn in a terminal phase is first re-initialised to the
 * DSL template (a new game on the same slot; the turn counter and hence the RNG stream keep
 * running).  Off: terminal phases are absorbing, as in the reference. */
#define GE_FLAG_RESTART 1u
/* keep, for every room, one ge_turn_event per turn of the most recent ge_batch_step call (which
 * must then not exceed max_fuse turns): what the turn logged and decided, so that a host can
 * surface it as the reference's backend tool calls (update_player_actions / set_next_phase /
 * update_player_state, agent/tools/backend_tools.py:10-157).  Costs 16 B of HBM writes per room-turn. */
#define GE_FLAG_TRACE 2u

typedef struct ge_batch_desc {
    uint64_t seed;
    uint64_t first_room;                  /* global index of this batch's room 0 (sharding: the RNG is
                                             keyed by GLOBAL room index, so results do not depend on
                                             how rooms are split over GPUs) */
    uint32_t n_segments;                  /* rooms are grouped by game: one segment per (table, N) */
    uint32_t flags;
    int32_t device;                       /* HIP device ordinal */
    uint32_t max_fuse;                    /* turns fused into one launch (state stays in registers);
                                             0 = library default, 1 = one launch per turn */
    ge_segment_desc seg[GE_MAX_SEGMENTS];
} ge_batch_desc;

typedef struct ge_batch ge_batch;

/* Aggregate over the rooms of a batch (what the cross-shard all-gather exchanges).
 * Every field is a sum over rooms, so shard summaries add up to the whole-job summary. */
typedef struct ge_summary {
    uint64_t rooms;
    uint64_t finished;                    /* rooms in a terminal phase */
    uint64_t village_wins, wolf_wins;     /* werewolf rooms finished with no / some wolves alive */
    uint64_t alive_players;               /* werewolf: alive seats; two-truths: every seat (n_players per room) */
    uint64_t sum_end_turn;                /* over finished rooms whose end_turn is set: a room written in a terminal
                                             phase with end_turn -1 counts as finished but adds nothing here or below */
    uint64_t end_turn_hist[16];           /* finished rooms by end_turn / 8 (last bucket open) */
    uint64_t score_hist[16];              /* two-truths: players by total_score (last bucket open) */
    uint64_t checksum;                    /* sum over rooms of hash(global room index, packed state) */
    uint64_t turn;                        /* turns stepped so far */
    uint64_t games_recycled;              /* GE_FLAG_RESTART: finished games whose slot was re-initialised */
} ge_summary;

/* Creates the batch with every room in the DSL's initial state (player_states_template,
 * phase 0): the batched InitialRouterNode init of v2:255-289 + utils.py:584-653. */
int ge_batch_create(const ge_batch_desc *desc, ge_batch **out);

/* Advances EVERY room by n_turns turns (one turn = one graph run of the reference, §3.1).
 * `hip_stream` is a hipStream_t (NULL = the default stream).  Asynchronous. */
int ge_batch_step(ge_batch *b, uint32_t n_turns, void *hip_stream);

/* Back to the initial state and turn 0 (same seed, same rooms): a device-side fill of every room
 * record with the DSL's template state.  Synchronises. */
int ge_batch_reset(ge_batch *b);

/* Sets the turn counter (0 .. 2^32-1).  The RNG is keyed by (global room, turn) and end_turn and
 * the event trace are turn-based, so a checkpoint is (room records, turn): restore = create the
 * batch, ge_batch_write_rooms (or a copy into ge_batch_state), ge_batch_set_turn.  What the
 * reference's LangGraph checkpointer keeps per thread besides the state (the run counter).  Synchronises. */
int ge_batch_set_turn(ge_batch *b, uint64_t turn);     /* (also drops the records' prepared-deal caches: a raw restore may come from another seed) */

int ge_batch_sync(ge_batch *b);
int ge_batch_turn(const ge_batch *b, uint64_t *turn);
int ge_batch_n_rooms(const ge_batch *b, uint64_t *n_rooms);

/* Copies `count` rooms starting at local index `first` into dst (cap_bytes >= count*sizeof(ge_room_view)).
 * Synchronises.  Room order: segment 0's rooms, then segment 1's, ...
 * Only the packed records (32 - 48 B per room) cross PCIe, through a pinned staging buffer the batch keeps; the views are built
 * from them by the host cores - from 16 384 rooms on by several threads (at most 16, fewer if the process's CPU affinity or the
 * environment variable GE_IO_THREADS says so).  1 048 576 Werewolf x 8 rooms: 5.7 ms (profiles/r03_host_io.txt). */
int ge_batch_read_rooms(ge_batch *b, uint64_t first, uint64_t count, ge_room_view *dst, size_t cap_bytes);

/* Overwrites rooms from canonical views (checkpoint restore, tests of hand-built states).  All views are checked first
 * (n_players and pack of the segment the room lies in, phase_id / prev_phase_id naming phases of that segment's table - the
 * reference never stores an id outside dsl['phases'] either, v2:1173-1191 - werewolf role classes 0 .. 4): GE_ERR_ARG leaves
 * every room as it was.  Threads as above. */
int ge_batch_write_rooms(ge_batch *b, uint64_t first, uint64_t count, const ge_room_view *src);

/* Logs an action of a host-driven player between turns, exactly as if the player had acted in the
 * room's current phase: the action joins this visit's log (acted / choice) and the Referee's record
 * effect is applied (POLICY.md §3 "record").  What the reference does with a human's message at the
 * start of the next graph run (agent/tools/utils.py:310-358 -> bt:285-344).  `choice` is a player id
 * (werewolf) or a statement number (two-truths); GE_ERR_ARG if the player is not a target of the
 * current phase, has already acted, or the choice is out of range.  Synchronises. */
int ge_batch_inject_action(ge_batch *b, uint64_t room, uint32_t player_id, uint32_t choice);

/* The same for n actions at once (a batch of rooms with human seats): one kernel, one thread per
 * distinct room, which applies that room's actions in input order.  rooms[k] / player_ids[k] /
 * choices[k] describe action k; status[k] (status may be NULL) receives GE_OK or the reason it was
 * refused (GE_ERR_ARG as for ge_batch_inject_action, GE_ERR_RANGE for a room outside the batch).  A refused
 * action changes nothing; the others are applied.  Returns GE_OK if every action was applied, else the
 * status of the first refused one.  Synchronises. */
int ge_batch_inject_actions(ge_batch *b, uint64_t n, const uint64_t *rooms, const uint32_t *player_ids,
                            const uint32_t *choices, int32_t *status);

/* One turn of each listed room, room k keyed as global room keys[k] at turn turns[k] (what a lone batch with
 * first_room = keys[k] and turn counter turns[k] would do to that room in one ge_batch_step(b, 1)).  rooms[] are local
 * indices, pairwise distinct.  Unlisted rooms, the batch's turn counter and its GE_FLAG_TRACE buffer are untouched.
 * events (may be NULL) receives event k of room k.  All-or-nothing: GE_ERR_RANGE for a room outside the batch or
 * turns[k] == 0xFFFFFFFF, GE_ERR_ARG for a repeated room; nothing is stepped then.  n == 0: GE_OK.  Synchronises.
 * The batch's segment flags apply (human mask, GE_FLAG_RESTART, generic conditions).  A stepped record is stored without a
 * prepared role deal (as ge_batch_write_rooms stores one), so ordinary ge_batch_step calls before and after stay exact. */
int ge_batch_step_rooms(ge_batch *b, uint64_t n, const uint64_t *rooms, const uint64_t *keys, const uint32_t *turns,
                        ge_turn_event *events);
/* Canonical views of the listed rooms, dst[k] = room rooms[k] (any order, repeats allowed): a device gather of the packed
 * records into the staging buffer, one copy, host-side unpacking as in ge_batch_read_rooms.  GE_ERR_RANGE for a room
 * outside the batch.  cap_bytes >= n * sizeof(ge_room_view).  Synchronises. */
int ge_batch_read_rooms_at(ge_batch *b, uint64_t n, const uint64_t *rooms, ge_room_view *dst, size_t cap_bytes);
/* The scatter twin: src[k] is stored into batch room rooms[k] (a thread adopted mid-game into a slot of a resident batch).
 * The record stored is exactly what ge_batch_write_rooms stores for the same view (no prepared role deal).  All-or-nothing:
 * GE_ERR_RANGE for a room outside the batch, GE_ERR_ARG for a repeated room or for a view that does not fit the segment its
 * room lies in (as ge_batch_write_rooms checks it; ge_last_rejected_room() then names that entry's batch room); nothing is
 * written then.  n == 0: GE_OK.  One copy through the staging buffer, one device scatter.  Synchronises. */
int ge_batch_write_rooms_at(ge_batch *b, uint64_t n, const uint64_t *rooms, const ge_room_view *src);

/* Outcome of n_rollouts playouts of one room (ge_batch_rollout_rooms): 77 x u64 = 616 B. */
typedef struct ge_rollout_stats {
    ge_summary summary;                   /* ge_batch_summary of the composition below, word for word (rooms = n_rollouts) */
    uint64_t seat_alive[12];              /* werewolf: playouts in which seat i+1 is alive at the end, finished or not */
    uint64_t seat_wins[12];               /* werewolf: finished playouts won by seat i+1's team (no wolf alive: villagers, else
                                             werewolves); two-truths: finished playouts in which seat i+1's total_score is the
                                             highest (every tied seat counts) */
    uint64_t seat_score[12];              /* two-truths: sum of seat i+1's total_score over the playouts */
} ge_rollout_stats;                       /* seats at or above n_players read 0 */

/* Playouts: entry k (rooms[k], keys[k], turns[k]) is played n_rollouts times from batch room rooms[k] as it stands, replica r
 * as global room keys[k] + r (mod 2^64) under `seed`, at turns turns[k] .. turns[k] + max_turns - 1, every seat played by the
 * policy (human mask 0) and without GE_FLAG_RESTART (a finished game stays finished); the segment's table and generic conditions
 * apply.  Definition: create B' (seed, first_room = keys[k], flags 0, one segment: the same table and n_players, human mask 0,
 * n_rollouts rooms), ge_batch_write_rooms(B', 0, n_rollouts, copies of room rooms[k]), ge_batch_set_turn(B', turns[k]),
 * ge_batch_step(B', max_turns); out[k].summary = ge_batch_summary(B').  Prepared role deals of the source are ignored.
 * No state of a replica is kept in device memory: each plays in registers and only its outcome is reduced.
 * Every entry is checked before anything runs, and on an error *out is untouched: GE_ERR_ARG for a NULL pointer with n > 0,
 * n_rollouts == 0 or > 2^20, n * n_rollouts > 2^26 or max_turns > 4096; GE_ERR_RANGE for a room outside the batch or
 * turns[k] + max_turns > 0xFFFFFFFF.  Repeated rooms are allowed.  n == 0: GE_OK.  The batch is only read (records, deal
 * caches, turn counter, GE_FLAG_TRACE buffer).  Ordered behind the previous step; synchronises. */
int ge_batch_rollout_rooms(ge_batch *b, uint64_t n, const uint64_t *rooms, const uint64_t *keys, const uint32_t *turns,
                           uint32_t n_rollouts, uint32_t max_turns, uint64_t seed, ge_rollout_stats *out);

/* Playouts after given actions.  Entry k is ge_batch_rollout_rooms's entry (rooms[k], keys[k], turns[k]) with the actions
 * first_action[k] .. first_action[k+1]-1 (player_ids[a], choices[a]) logged in every replica, in that order, before its first
 * turn.  Definition: the ge_batch_rollout_rooms composition with ge_batch_inject_actions(B', every replica x those actions)
 * between write_rooms and set_turn.  An entry with no actions is ge_batch_rollout_rooms's entry, word for word.
 * Structural errors are all-or-nothing, checked before anything runs, and leave *out and entry_status untouched: every cap and
 * range check of ge_batch_rollout_rooms; GE_ERR_ARG for a NULL array with n > 0 (entry_status may be NULL), first_action[0] != 0,
 * decreasing offsets, or more than GE_MAX_PLAYERS actions in one entry.
 * Legality is decided per entry on the device, by the code of ge_batch_inject_actions (a living target of the current phase's
 * condition, not yet acted this visit, a choice in range).  If an action of entry k is refused, entry_status[k] gets that
 * action's status, the entry is not played and out[k] is untouched; every other entry is played and its entry_status[k] is
 * GE_OK.  Returns GE_OK if every entry was played, else the status of the first refused entry.  The batch is only read.
 * Ordered behind the previous step; synchronises. */
int ge_batch_rollout_actions(ge_batch *b, uint64_t n, const uint64_t *rooms, const uint64_t *keys, const uint32_t *turns,
                             const uint32_t *first_action /* n + 1 offsets */, const uint32_t *player_ids, const uint32_t *choices,
                             int32_t *entry_status /* n, may be NULL */, uint32_t n_rollouts, uint32_t max_turns, uint64_t seed,
                             ge_rollout_stats *out);

/* Playouts from a seat's view (POLICY.md §3c).  Entry k is ge_batch_rollout_actions's entry with one more step between the
 * actions and set_turn: replica r's copy has what seat seats[k] (1-based) cannot see dealt again - Werewolf: the hidden tuples
 * of the seats it cannot rule out, uniformly over the deals consistent with its own role, the revealed roles, its wolf
 * partners and (a Detective) its investigations; Two-Truths: the speaker's lie while it is not revealed - from the view key
 * mix32(room_key(seed, keys[k] + r) ^ 0x56494557 ^ turns[k] * 0x9E3779B9).  seats[k] = 0: no re-deal, the entry is
 * ge_batch_rollout_actions's word for word.  first_action may be NULL (no actions; player_ids / choices are then not read).
 * Structural errors as ge_batch_rollout_actions, plus GE_ERR_ARG for seats NULL with n > 0 or seats[k] > the n_players of
 * room rooms[k]'s segment; refusals per entry as there.  The batch is only read.  Ordered behind the previous step; synchronises. */
int ge_batch_rollout_seats(ge_batch *b, uint64_t n, const uint64_t *rooms, const uint64_t *keys, const uint32_t *turns,
                           const uint32_t *seats /* n */, const uint32_t *first_action /* n + 1, may be NULL: no actions */,
                           const uint32_t *player_ids, const uint32_t *choices, int32_t *entry_status /* may be NULL */,
                           uint32_t n_rollouts, uint32_t max_turns, uint64_t seed, ge_rollout_stats *out);

/* Paired comparison of playout entries (POLICY.md §3e).  For an entry k of a call and a subject seat s, the outcome X_k(r) of
 * replica r is - Werewolf: 1 if the replica is finished and seat s's team has won, else 0 (the bit seat_wins[s-1] counts);
 * Two-Truths: seat s's total_score at the end of the playout, finished or not (the value seat_score[s-1] sums).  For entry k
 * with baseline entry b = baseline[k], over r = 0 .. n_rollouts-1: */
typedef struct ge_compare_stats {         /* 6 x u64 = 48 B; all zero when entry k or its baseline was refused */
    uint64_t compared;                    /* playouts compared: n_rollouts, or 0 */
    uint64_t better, worse;               /* playouts with X_k(r) > X_b(r), with X_k(r) < X_b(r) */
    uint64_t gain, loss;                  /* sum of max(X_k - X_b, 0), sum of max(X_b - X_k, 0) */
    uint64_t diff_sq;                     /* sum of (X_k - X_b)^2 */
} ge_compare_stats;
/* So gain - loss = seat_wins[s-1] (Werewolf) / seat_score[s-1] (Two-Truths) of entry k minus that of entry b; in Werewolf
 * gain == better, loss == worse and diff_sq == better + worse; baseline[k] == k gives compared = n_rollouts and zeros elsewhere.
 *
 * ge_batch_rollout_compare is ge_batch_rollout_seats, arguments and meaning unchanged - out[k] and entry_status[k] are what it
 * gives for the same entries, word for word - plus, per entry, baseline[k] (an index into the same call), subjects[k] (the
 * subject seat, 1-based) and cmp[k].  Replica r of an entry is compared with replica r of its baseline.  Keys, turns and seats
 * of an entry and its baseline need not be equal - the counts are defined either way - but only equal keys, turns and seats
 * make it a comparison on common random numbers: replica r of both then draws the same stream and the same re-deal, and the
 * two differ only by what their actions change.  Structural errors, all before anything runs and with nothing touched, in this
 * order: ge_batch_rollout_seats's own; then GE_ERR_ARG for baseline, subjects or cmp NULL with n > 0, n > 65 536 (an entry and
 * its baseline are staged together), a baseline[k] >= n, rooms[baseline[k]] != rooms[k] (the same room, hence the same seat
 * numbering), subjects[k] == 0 or above the n_players of room rooms[k]'s segment, subjects[baseline[k]] != subjects[k] (a
 * playout keeps its outcome for one seat: an entry and its baseline are compared for the same one).  Refusals per entry as
 * ge_batch_rollout_seats; cmp[k] is all zero when entry k or its baseline was refused.  Each playout's outcome takes one byte
 * of device memory and none crosses to the host.  The batch is only read.  Ordered behind the previous step; synchronises. */
int ge_batch_rollout_compare(ge_batch *b, uint64_t n, const uint64_t *rooms, const uint64_t *keys, const uint32_t *turns,
                             const uint32_t *seats /* n */, const uint32_t *first_action /* n + 1, may be NULL: no actions */,
                             const uint32_t *player_ids, const uint32_t *choices, int32_t *entry_status /* may be NULL */,
                             uint32_t n_rollouts, uint32_t max_turns, uint64_t seed, ge_rollout_stats *out,
                             const uint32_t *baseline /* n */, const uint32_t *subjects /* n, 1-based */, ge_compare_stats *cmp /* n */);

/* Seat-view playouts weighted by the caller's beliefs (POLICY.md §3j).  Entry k carries GE_BELIEF_SLOTS bytes
 * beliefs[16 k .. 16 k + 15]: byte c is how much the caller suspects seat c + 1 of being a werewolf (Werewolf) or statement c + 1
 * of being the lie (Two-Truths), as prior odds 0 .. 255.  The re-deal of ge_batch_rollout_seats differs at two draws only: the
 * wolf seats among the seats the viewing seat cannot rule out are taken by successive weighted draws without replacement
 * (a pick whose remaining weights sum to 0 is uniform, so the call stays total), and a redrawn lie is one weighted draw over
 * bytes 0 .. 2 (all zero: uniform).  What the seat knows - its partners, a Detective's results, revealed roles - is never
 * overridden.  This is successive sampling by prior odds, not an exact posterior, and nothing in the library derives the
 * weights.  Equal weights (any common value 1 .. 255) give ge_batch_rollout_seats's entry word for word; seats[k] = 0 means no
 * re-deal and the entry's beliefs are not read by the device.
 * baseline, subjects and cmp all NULL: the call is ge_batch_rollout_seats under these draws.  All three given: it is
 * ge_batch_rollout_compare under them - out, entry_status and cmp exactly as there - and a comparison is on common random
 * numbers only for equal keys, turns, seats and beliefs.  Structural errors, all before anything runs and with nothing
 * touched, in this order: ge_batch_rollout_seats's own; GE_ERR_ARG for beliefs NULL with n > 0; GE_ERR_ARG for a non-zero byte
 * at a slot >= the n_players of room rooms[k]'s segment (Werewolf) or >= 3 (Two-Truths) - a wrong stride; GE_ERR_ARG when some
 * but not all of baseline / subjects / cmp are NULL; then, when comparing, ge_batch_rollout_compare's own.  Refusals per entry
 * as ge_batch_rollout_seats.  The beliefs travel in the call's one upload, 16 B per entry.  Cost of the weighted draws against
 * ge_batch_rollout_seats on the same entries, measured on an MI355X (profiles/beliefs_probe.txt): 65 536 playouts x 1 024 turns
 * per layout 0.96 .. 1.02 x the unweighted call (within run-to-run spread), one advise call of 8 entries x 4 096 playouts
 * x 1.03 .. 1.04.  The batch is only read.  Ordered behind the previous step; synchronises. */
#define GE_BELIEF_SLOTS 16
int ge_batch_rollout_beliefs(ge_batch *b, uint64_t n, const uint64_t *rooms, const uint64_t *keys, const uint32_t *turns,
                             const uint32_t *seats, const uint32_t *first_action, const uint32_t *player_ids, const uint32_t *choices,
                             int32_t *entry_status, const uint8_t *beliefs /* n x GE_BELIEF_SLOTS */,
                             uint32_t n_rollouts, uint32_t max_turns, uint64_t seed, ge_rollout_stats *out,
                             const uint32_t *baseline, const uint32_t *subjects, ge_compare_stats *cmp /* all three NULL: no comparison */);

/* Playout seats (POLICY.md §3d): ge_batch_step_rooms with some bot seats choosing their action by playouts.  Room k is stepped
 * as ge_batch_step_rooms's entry (rooms[k], keys[k], turns[k]), except that every seat s of playout_masks[k] (bit i = seat
 * i+1) that the policy would make act in this turn, with at least 2 candidates, takes the candidate with the highest
 * seat_wins[s-1] of ge_batch_rollout_seats's entry (room k at node entry, playout_keys[k], turns[k], seat s - or 0 under
 * GE_PLAYOUT_FULL_VIEW -, actions [(s, c)], n_rollouts, max_turns, seed); a tie goes to the pick(d, m)-th of the m tied
 * candidates, d being the seat's own draw, so a full tie is the policy's own choice.  The chosen actions are logged as
 * ge_batch_inject_actions logs them, then the turn is played; events[k] lists them as acted in the turn.  No decision is made
 * in a turn that starts from a terminal phase under GE_FLAG_RESTART, takes the phase-0 guard, or whose phase's completion is not
 * player_action.  decided[k] (may be NULL): bit i = seat i+1's action was chosen by playouts.  Unlisted rooms, the turn
 * counter and the GE_FLAG_TRACE buffer are untouched.  All-or-nothing, nothing runs on an error: ge_batch_step_rooms's checks;
 * GE_ERR_ARG for NULL masks / playout keys with n > 0, unknown flags, n_rollouts == 0 or > 2^20, max_turns > 4096, a mask bit
 * at or above the room's player count or on a host-driven seat of its segment, or sum_k popcount(mask_k) * c_k * n_rollouts >
 * 2^26, c_k = the most candidates a seat of room k can have (Werewolf: n_players, Two-Truths: max(n_players, 3)); GE_ERR_RANGE for turns[k] + max_turns > 0xFFFFFFFF.  Ordered behind the previous step; synchronises. */
/* Under GE_PLAYOUT_HALVING (POLICY.md §3h) a deciding seat with c candidates does not play n = n_rollouts playouts for each of them
 * but R = ceil(log2 c) rounds: with o_j = floor(n * (2^j - 1) / (2^R - 1)), round j plays replicas o_j .. o_{j+1} - 1 of the entry
 * above (key playout_keys[k] + o_j, n_rollouts o_{j+1} - o_j; nothing when that is 0) for every candidate still in, adds its
 * seat_wins[s-1] to the candidate's running value V, and - except after the last round - keeps the candidates whose V is at
 * least the ceil(c / 2^(j+1))-th largest (a tie at the cut keeps every tied candidate).  The choice is the highest V among the
 * candidates of the last round, ties to the pick(d, m)-th as above.  All survivors have played the same replicas, on common
 * random numbers; a finalist has played replicas 0 .. n - 1, so its V is the value it has without the flag; no candidate plays
 * more than n playouts, so the cost cap and the turn range are checked unchanged, as upper bounds.  c = 2, or an n so small that
 * o_{R-1} = 0 (n = 1), is the call without the flag; mask 0 and max_turns = 0 are ge_batch_step_rooms word for word with the
 * flag as without it.  The flag adds launches per turn (R rounds of playouts and R - 1 cuts instead of one launch), and on an
 * MI355X the flagged call was SLOWER at every shape measured, x 0.38 .. 0.71 of the unflagged call's speed while playing 1.3 .. 2.5 x fewer
 * playouts (profiles/halving_probe.txt): the flag saves playouts, not time.  It is off unless asked for.
 * Its value is 4u, not 2u: flags = 2 has been refused with GE_ERR_ARG since the call exists, hosts' tests pin that, and it stays
 * refused, as does every bit from 8u up. */
#define GE_PLAYOUT_FULL_VIEW 1u   /* value candidates from the true record (seat 0) instead of the seat's view */
#define GE_PLAYOUT_HALVING   4u   /* sequential halving of each decision's playout budget (POLICY.md §3h); 2u stays refused */
int ge_batch_step_rooms_playout(ge_batch *b, uint64_t n, const uint64_t *rooms, const uint64_t *keys, const uint32_t *turns,
                                const uint32_t *playout_masks /* n: bit i = seat i+1 */, const uint64_t *playout_keys /* n */,
                                uint32_t n_rollouts, uint32_t max_turns, uint64_t seed, uint32_t flags,
                                ge_turn_event *events /* n, may be NULL */, uint32_t *decided /* n, may be NULL */);

/* Listed rooms played on until a person is needed (POLICY.md §3f).  Room k is stepped by ge_batch_step_rooms's entries (rooms[k],
 * keys[k], turns[k] + t) for t = 0, 1, ...  The first turn is always played (a "Continue" plays a turn whatever the state); after
 * each played turn the conditions named in `until` are tested on the record it left, and the room stops after the first turn for
 * which one holds, or after max_turns turns:
 *   GE_RUN_UNTIL_PERSON  the phase's completion is player_action and some seat of the segment's human_mask is a pending target:
 *                        ge_batch_inject_action(room, seat, c) would be accepted for at least one choice c
 *   GE_RUN_UNTIL_END     the phase is terminal (with or without GE_FLAG_RESTART; under restart the next call's first turn recycles
 *                        the room, as ge_batch_step_rooms does)
 *   GE_RUN_UNTIL_PHASE   the turn's event has to_phase_id != from_phase_id
 * played[k] = turns played; stopped[k] (may be NULL) = the bits of the named conditions that held after the last played turn (0: the
 * limit was hit).  events[k * max_turns + t] and views[k * max_turns + t] (either may be NULL), t < played[k], are exactly that
 * turn's ge_batch_step_rooms event and the ge_batch_read_rooms_at view taken after it; slots at t >= played[k] are untouched.  The
 * stored record is the one after the last played turn, without a prepared deal; unlisted rooms, the turn counter and the
 * GE_FLAG_TRACE buffer are untouched.  So max_turns = 1 is ge_batch_step_rooms word for word, and until = 0 is max_turns calls of it.
 * All-or-nothing, nothing runs on an error, in this order: ge_batch_step_rooms's checks; GE_ERR_ARG for played NULL with n > 0,
 * max_turns == 0 or > 4096, n * max_turns > 2^20, unknown `until` bits, or views with views_cap_bytes < n * max_turns *
 * sizeof(ge_room_view); GE_ERR_RANGE for turns[k] + max_turns > 0xFFFFFFFF.  n == 0: GE_OK.  One launch per segment present; each
 * turn's event and packed record go to a device trace plane (64 B per room-turn), and only the turns somebody played cross to the
 * host.  With ge_batch_set_timing on, ge_batch_kernel_time includes the call's launches.  Ordered behind the previous step;
 * synchronises. */
#define GE_RUN_UNTIL_PERSON 1u   /* stop after a turn that leaves the room waiting for a host-driven seat */
#define GE_RUN_UNTIL_END    2u   /* ... in a terminal phase */
#define GE_RUN_UNTIL_PHASE  4u   /* ... after a turn whose event has to_phase_id != from_phase_id */
int ge_batch_run_rooms(ge_batch *b, uint64_t n, const uint64_t *rooms, const uint64_t *keys, const uint32_t *turns,
                       uint32_t max_turns, uint32_t until,
                       uint32_t *played /* n */, uint32_t *stopped /* n, may be NULL */,
                       ge_turn_event *events /* n * max_turns, may be NULL */,
                       ge_room_view *views /* n * max_turns, may be NULL */, size_t views_cap_bytes);

/* Listed rooms with playout seats played on until a person is needed (POLICY.md §3g): ge_batch_run_rooms_playout is to
 * ge_batch_step_rooms_playout what ge_batch_run_rooms is to ge_batch_step_rooms.  Room k is stepped by ge_batch_step_rooms_playout's
 * entries (rooms[k], keys[k], turns[k] + t, playout_masks[k], playout_keys[k]; the call's n_rollouts, playout_max_turns, seed and
 * flags) for t = 0, 1, ...; the first turn is always played, after each played turn `until` is tested as ge_batch_run_rooms tests it,
 * and the room stops after the first turn for which a named condition holds, or after max_turns turns.  played / stopped as
 * ge_batch_run_rooms; for t < played[k], events[k * max_turns + t] is that turn's ge_batch_step_rooms_playout event (the decided
 * seats listed as acted), views[k * max_turns + t] the ge_batch_read_rooms_at view after it and decided[k * max_turns + t] its
 * decided mask; slots at t >= played[k] are untouched.  The stored record is the one after the last played turn, without a prepared
 * deal; unlisted rooms, the turn counter and the GE_FLAG_TRACE buffer are untouched.  So all masks 0, or playout_max_turns = 0, is
 * ge_batch_run_rooms word for word (the latter with decisions made: a full tie is the policy's own choice), and max_turns = 1 is
 * ge_batch_step_rooms_playout followed by ge_batch_read_rooms_at.
 * All-or-nothing, nothing runs on an error, in this order: with n > 0 ge_batch_run_rooms's checks in its order (ge_batch_step_rooms's,
 * played, max_turns, n * max_turns <= 2^20, `until`, the views' capacity, turns[k] + max_turns <= 0xFFFFFFFF); then
 * ge_batch_step_rooms_playout's playout checks in its order, where the turn range (GE_ERR_RANGE) is turns[k] + (max_turns - 1) +
 * playout_max_turns <= 0xFFFFFFFF - the last turn's playouts must fit - and the cost cap sum_k popcount(mask_k) * c_k * n_rollouts <=
 * 2^26 is per turn, because only one turn's playouts exist at a time; then n == 0: GE_OK.
 * Between the turns of a call the host does not wait for the device: per turn the plan, the playouts (their number read from device
 * memory), the decision and the turn are enqueued for the rooms still live, in groups of turns with one 4-byte read of the live
 * count between groups; only the rows of the turns enqueued cross to the host.  With ge_batch_set_timing on, ge_batch_kernel_time
 * includes the call's launches.  Under GE_PLAYOUT_HALVING (above; POLICY.md §3h) every turn's decisions are
 * ge_batch_step_rooms_playout's under that flag: per turn the rounds of playouts and the cuts between them are enqueued like the
 * rest, with no host wait added.  Ordered behind the previous step; synchronises. */
int ge_batch_run_rooms_playout(ge_batch *b, uint64_t n, const uint64_t *rooms, const uint64_t *keys, const uint32_t *turns,
                               const uint32_t *playout_masks /* n: bit i = seat i+1 */, const uint64_t *playout_keys /* n */,
                               uint32_t n_rollouts, uint32_t playout_max_turns, uint64_t seed, uint32_t flags /* GE_PLAYOUT_FULL_VIEW | GE_PLAYOUT_HALVING */,
                               uint32_t max_turns, uint32_t until,
                               uint32_t *played /* n */, uint32_t *stopped /* n, may be NULL */,
                               uint32_t *decided /* n * max_turns, may be NULL */,
                               ge_turn_event *events /* n * max_turns, may be NULL */,
                               ge_room_view *views /* n * max_turns, may be NULL */, size_t views_cap_bytes);

/* A run-on with a forecast of every turn: a win-odds timeline in one call (POLICY.md §3i).  ge_batch_run_rooms_forecast is
 * ge_batch_run_rooms with the same (rooms, keys, turns, max_turns, until): played, stopped, events and views are ge_batch_run_rooms's
 * word for word, and so are the stored records, the unlisted rooms, the batch's turn counter and the GE_FLAG_TRACE buffer.  In
 * addition, for entry k and point p = 0 .. played[k], stats[k * (max_turns + 1) + p] is out[0] of the ge_batch_rollout_seats entry
 * (room rooms[k] as it stood at point p, forecast_keys[k], turns[k] + p, seats[k], no actions; the call's n_rollouts,
 * playout_max_turns and seed), word for word.  Point 0 is the room before the call, point p >= 1 the room after the call's turn
 * p - 1 (views[k * max_turns + p - 1]).  Slots at p > played[k] are untouched.  seats NULL: the full view (seat 0) for every entry.
 * The key is the same at every point, so replica r of two points draws the same stream at the same absolute turns (common random
 * numbers: a swing between two points is the turn's effect, not resampling noise); point played[k] of one call equals point 0 of
 * the next call on the room with turns[k] + played[k]; playouts play every seat by the policy without GE_FLAG_RESTART, so a point
 * taken in a terminal phase is a finished game, even in a restart batch.
 * All-or-nothing, nothing runs and nothing is touched on an error, in this order: with n > 0 ge_batch_run_rooms's checks in its
 * order; then GE_ERR_ARG for forecast_keys or stats NULL, stats_cap_bytes < n * (max_turns + 1) * sizeof(ge_rollout_stats),
 * n_rollouts == 0 or > 2^20, playout_max_turns > 4096, n * (max_turns + 1) > 2^16 (the accumulators are 640 B per point),
 * n * (max_turns + 1) * n_rollouts > 2^26, or a seats[k] above the player count of room k's segment; then GE_ERR_RANGE for
 * turns[k] + max_turns + playout_max_turns > 0xFFFFFFFF; then n == 0: GE_OK.
 * The points are played from records the device already holds: point 0 from the batch records in front of the run, the others
 * from the run's trace plane (64 B per room-turn) behind it on the same stream, with no host wait in between - a block of a turn
 * its room did not play reads the run's turn count and leaves - and only the rows of the turns somebody played cross to the host.
 * One launch per segment present for point 0, for the run and for the traced points.  With ge_batch_set_timing on,
 * ge_batch_kernel_time includes the call's launches.  Ordered behind the previous step; synchronises.
 * Not measured: tools/timeline_probe.py times the call against the composition it replaces (ge_batch_run_rooms, then per played
 * turn a ge_batch_write_rooms_at into scratch rooms and a ge_batch_rollout_seats) but has not been run on an MI355X; the grid of
 * the traced points is sized by max_turns, so a short run under a high limit pays for blocks that leave at their first test. */
int ge_batch_run_rooms_forecast(ge_batch *b, uint64_t n, const uint64_t *rooms, const uint64_t *keys, const uint32_t *turns,
                                uint32_t max_turns, uint32_t until,
                                const uint64_t *forecast_keys /* n */, const uint32_t *seats /* n, may be NULL: full view */,
                                uint32_t n_rollouts, uint32_t playout_max_turns, uint64_t seed,
                                uint32_t *played /* n */, uint32_t *stopped /* n, may be NULL */,
                                ge_turn_event *events /* n * max_turns, may be NULL */,
                                ge_room_view *views /* n * max_turns, may be NULL */, size_t views_cap_bytes,
                                ge_rollout_stats *stats /* n * (max_turns + 1) */, size_t stats_cap_bytes);

/* The rooms of a range that need attention: a device scan of a resident batch (POLICY.md §3k).  Over the rooms first .. first +
 * count - 1 as they stand (local indices, as ge_batch_read_rooms counts), a room matches when some condition named in `want` holds:
 *   GE_FIND_PERSON  some seat of the segment's human_mask is a pending target - word for word the PERSON test of ge_batch_run_rooms.
 *                   `pending` says which: bit i is set exactly when seat i+1 is in the segment's human_mask and
 *                   ge_batch_inject_action(room, i+1, c) would be accepted for at least one c (0 without GE_FIND_PERSON in `want`)
 *   GE_FIND_END     the room's phase is terminal, with or without GE_FLAG_RESTART: the record is judged as stored
 *   GE_FIND_PHASE   bit phase_id of phase_masks[segment of the room] is set (n_segments words, read only with this bit)
 * `why` holds the bits of `want` that hold for the room (never 0).  *n_match = the matches in the range; *n_hits = min(n_match,
 * cap); hits[0 .. n_hits) are the first matches in ascending room order, slots from n_hits on are untouched.  cap == 0 counts only
 * (hits may be NULL).  A truncated scan is resumed with first = hits[n_hits - 1].room + 1.
 * The batch is only read: records, prepared deals (in the record and in the Werewolf x 12 side plane), the turn counter and the
 * GE_FLAG_TRACE buffer stay as they are.  All errors before anything runs, every output untouched, in this order: GE_ERR_ARG for
 * want == 0 or unknown bits; for n_hits or n_match NULL; for hits NULL with cap > 0; for GE_FIND_PHASE with phase_masks NULL; for a
 * mask bit at or above the phase count of its segment's table (a wrong stride); GE_ERR_RANGE for first + count beyond the batch;
 * then count == 0: GE_OK, both counters 0.
 * One test launch per segment of the range (lane = room, records loaded as the step kernels load them: one result word per room,
 * one match count per wavefront), one launch that scans the wavefront counts, one that re-reads the result words and stores the
 * hits at their wavefronts' offsets: no block waits for another, and the order of the output does not depend on scheduling.  Only
 * n_hits * 16 bytes and two counters cross to the host.  With ge_batch_set_timing on, ge_batch_kernel_time includes the call's
 * launches.  Ordered behind the previous step; synchronises.
 * Measured on an MI355X (tools/find_probe.py, profiles/find_probe.txt: Werewolf x 8, human_mask = 1, 40 turns stepped and nobody
 * answering, so that 99 % of the rooms match and every hit is copied back - the call's worst case; medians of 20 calls): against
 * ge_batch_read_rooms of the range into a reused array plus the host's END test, the call is 21 x faster at 65 536 rooms (124 us
 * against 2.66 ms) and 8.8 x at 1 048 576 (1.50 ms against 13.2 ms); its three launches take 11 us and 40 us of that, the rest is
 * the copy of the hits (16 B each) and their conversion.
 * A phase id of 32 or more has no bit in a mask word (the shipped tables' terminal phases, 98 and 99): GE_FIND_END finds those. */
#define GE_FIND_PERSON 1u   /* == GE_RUN_UNTIL_PERSON: some seat of the segment's human_mask is a pending target */
#define GE_FIND_END    2u   /* == GE_RUN_UNTIL_END: the room's phase is terminal */
#define GE_FIND_PHASE  4u   /* bit phase_id of phase_masks[segment of the room] is set */
typedef struct ge_room_hit {          /* 16 B */
    uint64_t room;                    /* local index, as ge_batch_read_rooms counts */
    uint32_t why;                     /* the bits of `want` that hold for the room (never 0) */
    uint16_t pending;                 /* want & GE_FIND_PERSON: bit i = host-driven seat i+1 could act now; else 0 */
    uint8_t  phase_id;
    uint8_t  segment;
} ge_room_hit;
int ge_batch_find_rooms(ge_batch *b, uint64_t first, uint64_t count, uint32_t want,
                        const uint32_t *phase_masks /* n_segments words; read only with GE_FIND_PHASE */,
                        ge_room_hit *hits, uint64_t cap, uint64_t *n_hits, uint64_t *n_match);

/* Per-room host-driven seats: a seat plane beside the records (POLICY.md §3l).  Every room has a seat mask (bit i = seat i + 1 is
 * host-driven).  Until the first ge_batch_set_seats a room's seat mask is its segment's human_mask and no memory is spent; a batch
 * that never sets a seat behaves exactly as before.
 *   ge_batch_set_seats    rooms[] are local indices, pairwise distinct; masks[k] becomes room rooms[k]'s seat mask.  All-or-nothing,
 *                         every entry checked before anything changes, in this order: GE_ERR_ARG for b NULL, or rooms / masks NULL
 *                         with n > 0; GE_ERR_RANGE for a room outside the batch; GE_ERR_ARG for a repeated room; GE_ERR_ARG for a
 *                         mask bit at or above the n_players of the room's segment.  n == 0: GE_OK, nothing allocated.  The first
 *                         successful call allocates the plane - 2 B per room on the device plus a host mirror, filled with the
 *                         segments' masks; a failed allocation returns GE_ERR_NOMEM and leaves the batch without a plane, usable
 *                         as before.  Ordered behind the previous step; synchronises.
 *   ge_batch_get_seats    dst[i] = seat mask of room first + i (the segment's human_mask where none was ever set), served from the
 *                         host mirror: no device synchronisation.  GE_ERR_ARG for dst NULL with count > 0, GE_ERR_RANGE for a range
 *                         beyond the batch.
 *   ge_batch_clear_seats  every room back to its segment's human_mask; the plane is freed (without a plane: GE_OK).  Synchronises.
 * Once a plane exists, "the segment's human_mask" reads "the room's seat mask" in every definition above, and nothing else about
 * those calls changes: the turn itself (the policy acts for no seat of the mask: ge_batch_step, ge_batch_step_rooms,
 * ge_batch_step_rooms_playout and the three run-ons), the PERSON test of ge_batch_run_rooms / _playout / _forecast, GE_FIND_PERSON
 * and `pending` of ge_batch_find_rooms, and the refusal of a playout-mask bit on a host-driven seat in ge_batch_step_rooms_playout and
 * ge_batch_run_rooms_playout (the host mirror decides it: a seat of the segment's mask that the room has handed back to the policy
 * is accepted).  Unchanged: the rollouts (human mask 0 by definition: the same result word for word with or without a plane),
 * ge_batch_inject_action(s) (never consulted the mask), ge_batch_summary and its checksum, ge_batch_state, ge_room_view,
 * ge_batch_read_rooms(_at) and ge_batch_write_rooms(_at).
 * The mask is configuration, not game state: it survives ge_batch_reset, ge_batch_set_turn, every write of records and a
 * GE_FLAG_RESTART recycle; a checkpoint is (records, turn, seats).  A change takes effect with the next turn played: a seat handed to
 * the policy acts on the next turn if it is a pending target that has not acted this visit, with the ordinary draw of (room, turn,
 * player); a seat handed to a person that has already acted this visit stays acted.  ge_group_shard lends the shard's batch, so the
 * three calls work per shard; there is no group-level call.
 * ge_batch_step on a batch with a plane: room r takes, for t = 0 .. n_turns - 1, exactly ge_batch_step_rooms's entry (r, global
 * index of r, turn + t) under its seat mask.  The turn counter advances by n_turns, the same range checks apply, and under
 * GE_FLAG_TRACE the buffer holds these turns' events as ge_batch_read_events defines them.  Records are stored without a prepared
 * deal and the Werewolf x 12 deal side plane is neither read nor written; so with all seat masks equal to the segment's mask the
 * records (as views), events, summary and checksum equal those of the same batch without a plane.  It keeps the stream-ordered
 * contract of ge_batch_step, uses plain launches (one per segment and per max_fuse turns) and never a captured graph; the graphs
 * cached for the no-plane path stay valid and are used again after ge_batch_clear_seats.  With ge_batch_set_timing on its launches
 * count in ge_batch_kernel_time.
 * Measured on an MI355X (tools/seats_probe.py, profiles/seats_probe.txt; wall time, medians of 20 calls).  (a) A batch without a
 * plane, this library against the one before the change, whose indexed kernels had no plane pointer to test: ge_batch_step_rooms of
 * 1 024 entries x 0.998, ge_batch_run_rooms of 1 024 entries x 16 turns x 0.997, ge_batch_find_rooms over 65 536 / 1 048 576
 * Werewolf x 8 rooms x 1.017 / x 1.008 - each inside the spread of the older library against itself in the same run (5 - 18 %), so
 * "has a plane" stays a run-time test of a kernel argument.  (b) ge_batch_step with a plane against the same batch with the equal
 * segment mask and no plane (the flagship kernels), time per turn, single-turn launches / fused launches of 64 turns: Werewolf x 8
 * at 65 536 rooms x 1.00 / x 1.06, at 1 048 576 rooms x 1.26 / x 3.37; Werewolf x 12 at 2 097 152 rooms x 1.44 / x 4.52; Two-Truths
 * x 4 at 1 048 576 rooms x 0.92 / x 1.19.  The step with a plane is the lone-wavefront single-turn lane (tables read from global
 * memory, deals on the spot), a form DESIGN.md §4 measured slower than the large-batch builds: where seating is uniform over many
 * rooms, a batch per seating steps faster. */
int ge_batch_set_seats(ge_batch *b, uint64_t n, const uint64_t *rooms, const uint32_t *masks);
int ge_batch_get_seats(ge_batch *b, uint64_t first, uint64_t count, uint32_t *dst);
int ge_batch_clear_seats(ge_batch *b);

/* Advice for listed seats, on the device (POLICY.md §3m): which choices seat seats[k] (1-based) of batch room rooms[k] can make
 * now, what ge_batch_rollout_seats says about each of them, and which is best.  Definition, by composition: the choices are
 * c = 1 .. C, C = the n_players of the room's segment (Werewolf) or 3 (Two-Truths).  Bit c-1 of `legal` is set exactly when
 * ge_batch_inject_action(room, seats[k], c) on a copy of the room returns GE_OK - the human mask and the seat plane play no part:
 * any seat may be advised.  For every legal c, option[c-1] = (summary.finished, seat_wins[s-1], seat_score[s-1]) of
 * ge_batch_rollout_seats's entry (rooms[k], keys[k], turns[k], seat s = seats[k] - seat 0 under GE_ADVISE_FULL_VIEW -, actions
 * [(s, c)], n_rollouts, max_turns, seed); `policy` is the same three words of that entry without actions (the policy plays the
 * seat).  `best` is the legal choice with the highest value, the lowest such choice on a tie; the value is `wins` in Werewolf and
 * `score` in Two-Truths - the outcome ge_batch_rollout_compare compares.  A Two-Truths statements phase has the single legal
 * choice 1 and is played like any other.  legal == 0 (the seat is no pending target: the phase takes no action, the seat is dead,
 * has acted, or the game is over): status = GE_ERR_ARG, nothing is played and every other word of the record is 0.
 * A structurally valid call returns GE_OK whatever the per-entry statuses are - unlike ge_batch_rollout_actions, which returns
 * the first refused entry's status: a seat that is not pending is an expected answer to a host that lists seats it has not
 * tested, not a failed call.  Read out[k].status.
 * All checks run before anything runs, and on a failure *out is untouched: GE_ERR_ARG for a NULL array with n > 0, unknown flag
 * bits, n_rollouts == 0 or > 2^20, max_turns > 4096; GE_ERR_RANGE for a room outside the batch or turns[k] + max_turns >
 * 0xFFFFFFFF; then GE_ERR_ARG for seats[k] == 0 or above the n_players of room k's segment, or sum_k (c_k + 1) * n_rollouts >
 * 2^26, c_k = the most candidates a seat of room k can have (Werewolf: n_players, Two-Truths: max(n_players, 3): an upper bound
 * of what is played, as in ge_batch_step_rooms_playout).  n == 0: GE_OK.  Repeated rooms and repeated (room, seat) pairs are
 * allowed.  The batch is only read: records, prepared deals, the seat plane, the turn counter and the GE_FLAG_TRACE buffer stay
 * as they are.  Ordered behind the previous step; synchronises.
 * On the device: a plan kernel (lane = listed entry) finds `legal` with the code of ge_batch_inject_action on copies of the
 * record and writes popcount(legal) + 1 entries of ge_batch_rollout_seats; that call's playout kernel plays them where they
 * lie; a reduce kernel stores the 224 bytes.  Only the entry list goes up, and the advice records and 8 bytes per launch unit
 * come back (a pass of the call holds at most 65 536 playout entries).
 * Measured on an MI355X (tools/advise_seats_probe.py, profiles/advise_seats_probe.txt: Werewolf x 8, human_mask = 1, 40 turns stepped,
 * seat 1 of every waiting room advised at 64 playouts per choice; medians of 9 ticks, the call against itself in the same run x 1.02):
 * ge_batch_find_rooms + this call against ge_batch_find_rooms + ge_batch_read_rooms_at + the host listing every seat id +
 * ge_batch_rollout_seats + the host's maximum (the same playouts, the same `best` in every room): 1.10 ms against 3.35 ms at 4 096
 * rooms (3 556 waiting), 15.4 ms against 77.5 ms at 65 536 (56 688 waiting); 13.6 MB come back instead of 330 MB.  No other shape
 * has been measured. */
typedef struct ge_advice_option { uint32_t finished, wins; uint64_t score; } ge_advice_option;   /* 16 B */
typedef struct ge_advice {                 /* 224 B */
    int32_t  status;     /* GE_OK, or GE_ERR_ARG: no choice of this seat would be accepted now; everything below is then 0 */
    uint32_t legal;      /* bit c-1: choice c is accepted by ge_batch_inject_action for this seat now, and was played */
    uint32_t best;       /* the legal choice with the highest value, the lowest such choice on a tie */
    uint32_t phase_id;   /* the room's current phase id (DSL id, as ge_room_hit.phase_id) */
    ge_advice_option policy;       /* the entry without an action: the policy plays the seat */
    ge_advice_option option[12];   /* option[c-1], zero where bit c-1 of legal is clear */
} ge_advice;
#define GE_ADVISE_FULL_VIEW 1u   /* play from the true record (seat 0) instead of the seat's view */
int ge_batch_advise_seats(ge_batch *b, uint64_t n, const uint64_t *rooms, const uint64_t *keys, const uint32_t *turns,
                          const uint32_t *seats /* n, 1-based */, uint32_t n_rollouts, uint32_t max_turns, uint64_t seed,
                          uint32_t flags, ge_advice *out /* n */);

/* Seat observations and actions in device memory: a decision maker that lives on the GPU and sits in a seat of every room
 * (POLICY.md §3n).  Both calls take a range of rooms (local indices, as ge_batch_read_rooms counts) and a short list of seats
 * (host memory, 1-based, pairwise distinct, at most 12), and device memory the caller owns, with count * n_seats entries:
 * entry (r - first) * n_seats + j belongs to batch room r and seat seats[j].
 *   ge_batch_observe_seats  obs_dev[entry] = what seat seats[j] is shown of room r, 192 bytes: the canonical view's columns with
 *                           every field hidden that ge_batch_rollout_seats's re-deal from that seat may change (§3n restates the
 *                           rule field by field; `unknown` is the mask of the seats it hides), the seat's legal choices
 *                           (`legal` = ge_advice.legal: bit c-1 is set exactly when ge_batch_inject_action(r, seat, c) on a copy
 *                           of the room returns GE_OK), and two outcome words that are not part of the observation proper: `done`
 *                           (the stored phase is terminal, judged as GE_FIND_END judges it, with or without GE_FLAG_RESTART) and
 *                           `won` (done, and the seat counts in ge_rollout_stats.seat_wins's rule for this finished room: its
 *                           true team won / its total_score is the highest, ties count; 0 until done).  The batch is only read.
 *   ge_batch_act_seats      by composition: ge_batch_inject_actions over the entries (r, seats[j], choices_dev[entry]) with a
 *                           non-zero choice, in ascending (r, j) order.  status_dev[entry] (may be NULL) = GE_OK for a zero or an
 *                           applied choice, GE_ERR_ARG for a refused one - a choice below 0 or above 15 is refused -, and a
 *                           refused action changes nothing.  Records are written as ge_batch_inject_actions writes them; a room
 *                           whose choices are all zero is not written.
 * Neither the segment's human mask nor the seat plane plays a part, as for ge_batch_inject_action and ge_batch_advise_seats.
 * The stream contract is ge_batch_step's, not the indexed calls': the launches go on hip_stream, ordered behind the batch's
 * earlier work; every later call on the batch is ordered behind them; no byte crosses to the host and the host waits for
 * nothing.  With ge_batch_set_timing on, the launches count in ge_batch_kernel_time.
 * All checks run before anything is launched, in this order: GE_ERR_ARG for b NULL; for seats, obs_dev or choices_dev NULL with
 * count * n_seats > 0; for n_seats > 12; for a repeated seat; GE_ERR_RANGE for a range beyond the batch; GE_ERR_ARG for a seat
 * of 0 or above the n_players of a segment the range touches; for cap_bytes < count * n_seats * sizeof(ge_seat_obs); for a
 * device pointer whose first or last byte hipPointerGetAttributes does not report as memory of the batch's device, managed
 * memory or pinned host memory (memory of a peer device is refused) - the library launches on no pointer it has not vetted;
 * then count == 0 or n_seats == 0: GE_OK.
 * On the device: lane = room, the record loaded as ge_batch_find_rooms loads it, one launch per segment of the range, the seat
 * list in the launch's arguments.  The knowledge sets are computed by the code the re-deal uses and `legal` by the loop of
 * ge_batch_advise_seats's plan kernel; the bitboards are unpacked into the byte columns in registers; a wavefront's records go
 * through LDS so that every 16-byte store instruction writes 1 KiB of consecutive bytes.  ge_batch_act_seats is the injection
 * kernel's body with its inputs read from choices_dev.
 * Measured on an MI355X (tools/env_probe.py, profiles/env_probe.txt: Werewolf x 8, human_mask = 1, restart on, 40 turns stepped
 * first, seat 1 played by a uniform legal choice computed in torch on the device; medians of 15).  (a) The loop act_seats, step,
 * observe_seats and the choice against the way there was before - ge_batch_read_rooms, a host-side choice in numpy (cheaper than
 * the legality and redaction a real host must restate: a lower bound), ge_batch_inject_actions, ge_batch_step: 0.218 ms against
 * 8.41 ms per turn at 65 536 rooms (x 39), 0.434 ms against 104 ms at 1 048 576 (x 240).  (b) ge_batch_observe_seats alone, launch
 * interval: 11.9 us at 65 536 rooms x 1 seat, 60.3 us at 1 048 576 x 1 seat (235 MB of records read and observations written:
 * 3.90 TB/s, 49 % of 8 TB/s), 266.8 us x 4 seats (839 MB, 3.14 TB/s); the layouts measured beside the LDS round trip and dropped:
 * each lane storing its own record 13.7, 83.9 and 340.4 us, the same with streaming stores 452.6 us at 1 048 576 x 1.  No other
 * shape has been measured. */
typedef struct ge_seat_obs {            /* 192 B = 12 x 16 B */
    uint8_t  seat, n_players, pack, act;          /* act: GE_ACT_* of the current phase's row */
    uint8_t  phase_row, done, won, pad0;          /* phase_row: dense row in the segment's table (an embedding index) */
    uint16_t legal, unknown;
    int32_t  phase_id, prev_phase_id, end_turn, games;   /* as ge_room_view */
    uint32_t pad1;                                 /* 0 */
    uint8_t  players[12][12];                      /* redacted view columns; rows >= n_players are 0 */
    uint8_t  det[12];
    uint8_t  pad2[4];                              /* 0 */
} ge_seat_obs;
int ge_batch_observe_seats(ge_batch *b, uint64_t first, uint64_t count, uint32_t n_seats, const uint32_t *seats /* host, 1-based */,
                           ge_seat_obs *obs_dev /* DEVICE: count * n_seats */, size_t cap_bytes, void *hip_stream);
int ge_batch_act_seats(ge_batch *b, uint64_t first, uint64_t count, uint32_t n_seats, const uint32_t *seats /* host */,
                       const int32_t *choices_dev /* DEVICE: count * n_seats, 0 = no action */,
                       int32_t *status_dev /* DEVICE, may be NULL */, void *hip_stream);

/* A teacher beside the two calls above: the seat-view playout advice of ge_batch_advise_seats for a seat list of every room of a
 * range, into device memory the caller owns (POLICY.md §3o).  Result, by composition: entry (r - first) * n_seats + j of out_dev
 * is, byte for byte, the ge_advice that ge_batch_advise_seats returns for the listed entry (rooms = r, keys = key(r), turns = turn,
 * seats = seats[j]) under the same n_rollouts, max_turns, seed and flags - `legal`, the refusal record (status = GE_ERR_ARG, every
 * other word 0), `policy`, option[] and `best` exactly as there, phase_id the phase's id.  key(r) = keys_dev[r - first] where
 * keys_dev is given, else key0 + (r << 20) mod 2^64, r the batch room index as ge_batch_read_rooms counts it: n_rollouts <= 2^20,
 * so the replica key ranges of two rooms never overlap; all listed seats of a room share the room's key.  The batch is only read;
 * neither the human mask nor the seat plane plays a part.  GE_PLAYOUT_HALVING and beliefs are not offered.
 * The stream contract is ge_batch_observe_seats's: every launch and memset goes on hip_stream, ordered behind the batch's earlier
 * work; later calls on the batch are ordered behind it; no byte crosses to the host and the host waits for nothing - with one
 * exception: a call that needs more scratch than the batch holds grows it, and hipFree / hipMalloc may wait for the device; a later
 * call of no larger shape allocates nothing and waits for nothing.  With ge_batch_set_timing on, the call counts as one interval in
 * ge_batch_kernel_time.
 * All checks run before anything is launched, and a failure leaves out_dev untouched, in this order: GE_ERR_ARG for b NULL; for a
 * flag bit other than GE_ADVISE_FULL_VIEW; for n_rollouts 0 or above 2^20, or max_turns above 4096; then the checks of
 * ge_batch_observe_seats in their order - GE_ERR_ARG for seats or out_dev NULL with count * n_seats > 0, for n_seats > 12, for a
 * repeated seat; GE_ERR_RANGE for a range beyond the batch; GE_ERR_ARG for a seat of 0 or above the n_players of a segment the
 * range touches, for cap_bytes < count * n_seats * sizeof(ge_advice), for an out_dev the batch's device does not reach, a non-NULL
 * keys_dev (count x 8 bytes) vetted the same way -; GE_ERR_RANGE for turn + max_turns > 0xFFFFFFFF; GE_ERR_ARG when the sum over
 * the touched segments of pairs x (c + 1) x n_rollouts exceeds 2^26, c as in ge_batch_advise_seats, whose cap and reservation this
 * is; then count == 0 or n_seats == 0: GE_OK.
 * On the device: no counter comes back, so the entry layout is fixed by shape - a pair (room, seat) owns c + 1 consecutive entry
 * slots of ge_batch_rollout_seats, slot k - 1 for choice k and the last for the entry without an action.  A plan kernel (lane =
 * pair, `legal` as ge_batch_observe_seats finds it) gives a live slot the replica range [0, n_rollouts) and a dead one - an illegal
 * choice, any slot of a pair with legal == 0 - an empty range; the playout kernel is the replica-range form of the playout-seat
 * calls, unchanged, launched on the grid of every slot: the wavefronts of a dead slot return before they load anything.  A reduce
 * kernel (lane = pair) stores the 224 bytes.  Slots are played in passes of at most 65 536, enqueued back to back.
 * Measured on an MI355X (tools/teach_probe.py, profiles/teach_probe.txt: Werewolf x 8, human_mask = 1, restart on, 40 turns stepped
 * first, seat 1 of every room at 64 playouts per choice played to the end; medians of 15).  (a) The advice of every room as a device
 * tensor, end to end with a final synchronise, against the way there was before - ge_batch_observe_seats, `legal` copied to the
 * host, the due pairs listed in numpy, ge_batch_advise_seats, the records uploaded; the same bytes: 1.04 ms against 1.99 ms at
 * 4 096 rooms (3 863 due), 15.6 ms against 29.2 ms at 65 536 (62 147 due).  (b) Of the call's kernel time the playouts are 97.4 % and
 * 98.3 %, the plan 1.1 % and 0.6 %, the memset 0.8 % and 0.7 %, the reduce 0.7 % and 0.4 %.  (c) The dead slots - the same call
 * where no pair is due: plan, memset, the grid of every slot with each wavefront leaving at its first test, reduce - cost 0.037 ms
 * and 0.302 ms, 3.5 % and 1.9 % of (a): what a device-side count of the live slots could save at most.  (d) The reduce with its
 * records staged through LDS 6.6 and 7.5 us per launch, with each lane storing its own record 7.6 and 8.4 us.  No other shape has
 * been measured. */
int ge_batch_teach_seats(ge_batch *b, uint64_t first, uint64_t count, uint32_t n_seats, const uint32_t *seats /* host, 1-based */,
                         const uint64_t *keys_dev /* DEVICE: count, or NULL */, uint64_t key0, uint32_t turn,
                         uint32_t n_rollouts, uint32_t max_turns, uint64_t seed, uint32_t flags /* GE_ADVISE_FULL_VIEW */,
                         ge_advice *out_dev /* DEVICE: count * n_seats */, size_t cap_bytes, void *hip_stream);

/* Every room of a range played on until a listed seat must act, in device memory (POLICY.md §3p): the step between
 * ge_batch_act_seats and ge_batch_observe_seats that loses no game end.  Under GE_FLAG_RESTART a fused ge_batch_step recycles a
 * finished room on the very next turn, so the observation behind it never shows `done`; here a room stops where the learner has
 * to look at it.  Result, by composition: with T the batch's turn counter at the call, every room r of first .. first + count - 1
 * (local indices, as ge_batch_read_rooms counts) takes exactly ge_batch_run_rooms's entry (rooms = r, keys = the global index of r,
 * turns = T) under max_turns and until & 7, with one more stop test:
 *   GE_RUN_UNTIL_SEAT    on the record the turn left, some listed seat is a pending target: ge_batch_inject_action(r, seat, c)
 *                        would be accepted for at least one c - ge_seat_obs.legal != 0 for that seat.  It is GE_RUN_UNTIL_PERSON's
 *                        test word for word with the listed seats in place of the room's seat mask.
 * The turn itself is ge_batch_step_rooms's: the room's seat mask (the segment's human_mask, or the seat plane) decides whom the
 * policy plays, and the seat list plays no part in the turn, as for ge_batch_observe_seats - a caller that plays a seat makes it
 * host-driven.  The first turn is always played.  played_dev[r - first] = turns played; stopped_dev[r - first] (may be NULL) = the
 * named bits that held after the last played turn (0: the limit was hit).  The stored record is the one after the last played
 * turn, without a prepared deal; the Werewolf x 12 side plane is neither read nor written, so ge_batch_step before or after stays
 * exact.  The turn counter advances by max_turns whatever the rooms played: rooms that stopped early, and rooms outside the
 * range, simply took no turn at the later indices - the RNG is keyed by (room, turn), so any turn is a valid next turn.  The
 * GE_FLAG_TRACE buffer and what ge_batch_read_events reports are untouched.  A room that stopped in a terminal phase is recycled by
 * the first turn of the next call under GE_FLAG_RESTART, as ge_batch_step_rooms does it: every end is there to be observed once.
 * So max_turns = 1, until = 0 is ge_batch_step_rooms over the range word for word, and until = 0 leaves the records that
 * ge_batch_step(max_turns) leaves on the same batch with a seat plane.
 * The stream contract is ge_batch_observe_seats's: the launches go on hip_stream, behind the batch's earlier work; later calls on
 * the batch are ordered behind them; no byte crosses to the host and the host waits for nothing.  With ge_batch_set_timing on, the
 * call is one interval of ge_batch_kernel_time.
 * All checks run before anything is launched, and a failure touches nothing, in this order: GE_ERR_ARG for b NULL; for max_turns
 * 0 or above 4096; for `until` bits above 15, or GE_RUN_UNTIL_SEAT with n_seats == 0; for played_dev NULL with count > 0; for
 * seats NULL with n_seats > 0, n_seats > 12 or a repeated seat; GE_ERR_RANGE for a range beyond the batch; GE_ERR_ARG for a seat
 * of 0 or above the n_players of a segment the range touches; for played_dev / stopped_dev (count x 4 bytes each) that the
 * batch's device does not reach, vetted as ge_batch_observe_seats vets obs_dev; GE_ERR_RANGE for T + max_turns > 0xFFFFFFFF; then
 * count == 0: GE_OK, nothing launched, the turn counter unchanged.  ge_batch_run_rooms and its siblings go on refusing bit 8.
 * On the device: lane = room, one wavefront per block, one launch per segment of the range; ge_batch_step's ranged turn loop under
 * a seat plane with ge_batch_run_rooms's stop tests, no trace plane and no staging.  The action queue is a wave-wide collective,
 * so a room that has stopped stores its record, its turn count and its stop bits and its lane stays on as a shadow that never
 * acts: a wavefront leaves with its last room, which is the call's inherent cost.
 * Measured on an MI355X (tools/run_seats_probe.py, profiles/run_seats_probe.txt: Werewolf x 8, human_mask = 1, restart on, 40 turns
 * stepped first, seat 1 played by a uniform legal choice computed in torch on the device, max_turns = 16; medians of 15).  (a) Wall
 * time per decision point delivered - an observation entry with legal != 0 or done - through act_seats, run_seats, observe_seats
 * against the one way without the call that loses no game end under restart, act_seats, ge_batch_step(1), observe_seats per turn:
 * 4.61 ns against 36.0 ns at 65 536 rooms (x 7.8), 0.96 ns against 5.22 ns at 1 048 576 (x 5.5); the baseline timed against itself
 * in the same run: x 0.99 and x 1.00.  (b) The call alone, launch interval: 30.8 us (+- 11.6) and 269.6 us (+- 11.4) at a mean
 * `played` of 8.1 turns; 49.4 % of the wavefront-turns are spent by shadow lanes (1 - mean played / mean over wavefronts of the
 * most any of its rooms played): what compacting live rooms across wavefronts could shed at most.  No other shape has been measured. */
#define GE_RUN_UNTIL_SEAT 8u   /* accepted by ge_batch_run_seats only: stop after a turn that leaves a listed seat a pending target */
int ge_batch_run_seats(ge_batch *b, uint64_t first, uint64_t count, uint32_t n_seats,
                       const uint32_t *seats /* host, 1-based, may be NULL with n_seats == 0 */, uint32_t max_turns, uint32_t until,
                       uint32_t *played_dev /* DEVICE: count */, uint32_t *stopped_dev /* DEVICE: count, may be NULL */,
                       void *hip_stream);

/* Decision lists: observe and play only the seats that must act (POLICY.md §3q).  Where the learner sits in every seat - self-play,
 * multi-agent training - the dense [rooms, listed seats] grid of the calls above is mostly entries that are no decision point:
 * at night only a few seats may act, dead seats never act.  These two calls work on a compact list of entries in device memory
 * instead; an entry index is ge_batch_observe_seats's, e = (r - first) * n_seats + j.  Both are compositions of the calls above.
 *   ge_batch_gather_seats  Let O be what ge_batch_observe_seats(first, count, seats) would store.  Entry e is due when
 *                          (want & GE_GATHER_SEAT and O[e].legal != 0) or (want & GE_GATHER_END and O[e].done != 0).  With
 *                          e_0 < e_1 < ... < e_(M-1) the due entries in ascending order: for i < min(M, cap), obs_dev[i] = O[e_i]
 *                          byte for byte and entries_dev[i] = e_i; n_dev[0] = min(M, cap), n_dev[1] = M.  Nothing at or beyond
 *                          index n_dev[0] of obs_dev / entries_dev is written.  cap = 0 counts only (obs_dev and entries_dev may
 *                          then be NULL).  The batch is only read; neither the human mask nor the seat plane plays a part.  A
 *                          finished room under GE_GATHER_END emits every listed seat, each with its own `won`.
 *   ge_batch_act_listed    Let n = min(*n_dev, cap), read on the device, and D the dense array of count * n_seats choices that is 0
 *                          except D[entries_dev[i]] = choices_dev[i] for i < n with entries_dev[i] < count * n_seats.  The call is
 *                          ge_batch_act_seats(first, count, seats, D), and status_dev[i] (may be NULL) that call's status at
 *                          entries_dev[i]; an entry at or above count * n_seats gets GE_ERR_ARG and touches nothing;
 *                          status_dev[i] for i >= n is not written.  The list may be in any order - a room's actions are applied in
 *                          ascending seat-list position, as ge_batch_act_seats applies them.  Of an entry named twice one choice
 *                          is applied, which one is unspecified, and every copy reports the applied one's status.  Whatever the
 *                          list holds, a record is written by one lane only, and nothing is written but records of the range
 *                          and status_dev[0 .. n).
 * ge_batch_teach_seats over a list is not offered: a caller indexes the dense advice with entries_dev.
 * The stream contract is ge_batch_observe_seats's: every launch and memset goes on hip_stream, behind the batch's earlier work;
 * later calls on the batch are ordered behind it; no byte crosses to the host and the host waits for nothing - with the exception
 * of ge_batch_teach_seats: a call of a larger shape than any before grows the batch's scratch, and hipFree / hipMalloc may wait
 * for the device.  With ge_batch_set_timing on, each call is one interval of ge_batch_kernel_time.
 * All checks run before anything is launched, and a failure leaves the outputs untouched.  ge_batch_gather_seats, in this order:
 * GE_ERR_ARG for b NULL; for want 0 or with bits above 3; for n_dev NULL; for obs_dev or entries_dev NULL with cap > 0 and
 * count * n_seats > 0; then ge_batch_observe_seats's checks in their order - GE_ERR_ARG for seats NULL with count * n_seats > 0,
 * for n_seats > 12, for a repeated seat; GE_ERR_RANGE for a range beyond the batch; GE_ERR_ARG for a seat of 0 or above the
 * n_players of a segment the range touches; for obs_dev (cap x 192 bytes) or entries_dev (cap x 4 bytes), with cap > 0 and
 * count * n_seats > 0, or n_dev (8 bytes) that the batch's device does not reach, vetted as ge_batch_observe_seats vets obs_dev -;
 * GE_ERR_ARG for count * n_seats >= 2^32.  An empty range or an empty seat list is not an error and is not silent either: GE_OK,
 * and n_dev = {0, 0} is stored on hip_stream (so n_dev is vetted even then).  ge_batch_act_listed: ge_batch_act_seats's checks in
 * their order with n_dev beside seats - GE_ERR_ARG for b NULL; for seats or n_dev NULL, or entries_dev or choices_dev NULL with
 * cap > 0, where count * n_seats > 0; for n_seats > 12; for a repeated seat; GE_ERR_RANGE for a range beyond the batch; GE_ERR_ARG
 * for a seat of 0 or above the n_players of a segment the range touches; for count * n_seats >= 2^32; then count * n_seats == 0:
 * GE_OK; GE_ERR_ARG for n_dev (4 bytes), entries_dev, choices_dev or a non-NULL status_dev (cap x 4 bytes each) that the batch's
 * device does not reach; then cap == 0: GE_OK, nothing launched.
 * On the device, ge_batch_gather_seats has ge_batch_find_rooms's shape - no block waits for another: no flag to spin on, no
 * look-back, no cooperative launch.  Test launches (one per segment of the range, lane = room): the due seats of the room as one
 * word - GE_GATHER_SEAT is GE_RUN_UNTIL_SEAT's test, the pending targets among the listed seats, far cheaper than `legal`'s
 * n_players injections per seat - and one due-entry count per wavefront.  One scan launch (ge_batch_find_rooms's scan block) turns
 * the counts into offsets and stores n_dev.  Emit launches (one per segment, lane = room): a wavefront without a due entry or
 * wholly beyond cap leaves before it loads a record; a listed seat none of the wavefront's rooms has due is skipped; a due entry's
 * record is built by ge_batch_observe_seats's own code and stored at the wavefront's offset + the due entries of the wavefront's
 * earlier rooms + the seat's rank among the room's due seats.  So the list's order is entry order whatever order the blocks ran in,
 * and a record is three whole 64-byte lines at any list position.  ge_batch_act_listed: a zeroed dense choice plane and a dense
 * status plane in the batch's scratch, a scatter (lane = list position), ge_batch_act_seats's kernel unchanged, a status gather.
 * Measured on an MI355X (tools/decisions_probe.py, profiles/decisions_probe.txt: Werewolf x 8, all eight seats listed and
 * host-driven, restart on, 40 turns stepped first, the seats played by a uniform legal choice computed in torch on the device,
 * max_turns = 16; medians of 15; decision points counted outside the timed windows).  (a) A decision point delivered - a list row,
 * an entry with legal != 0 or done - through act_listed, run_seats, gather_seats and the choice over all cap rows costs 1.38 ns of
 * wall time at 65 536 rooms and 0.86 ns at 1 048 576 (0.26 ms and 2.61 ms per call), against 1.28 ns and 0.89 ns through the dense
 * way on the same build - act_seats, run_seats, observe_seats over eight seats, the choice over [rooms, 8] (0.24 ms and 2.72 ms per
 * call): at 65 536 rooms the list loop is the slower one, x 0.93, at 1 048 576 the list loop is the faster one, x 1.04; the dense
 * way timed against itself x 1.03 and x 1.00.  The list does not pay here: of a call, the library's kernels are 91.4 us and 520.5
 * us in the list loop and 74.7 us and 626.2 us in the dense loop (kernel trace), and the rest is the choice over rooms x 8 rows in
 * either loop, which the list does not shorten because its length stays on the device.  (b) The call alone, gather_seats against
 * observe_seats on the same records, launch interval: 59.6 us (+- 9.9) against 54.2 us at 65 536 rooms - the list call is the
 * slower one there, x 0.91 - and 344.0 us (+- 73.5) against 491.2 us at 1 048 576 (x 1.43); 35.5 % and 35.6 % of the entries were
 * due; 41 MB against 103 MB and 661 MB against 1644 MB moved; of the call, by kernel trace, the test launch 4.2 and 10.1 us, the
 * scan 2.2 and 16.6 us, the emit launch 50.3 and 302.2 us: per record the emit costs 1.8 times what the dense kernel does at 1 048
 * 576 rooms, because a wavefront works through every seat that any of its rooms has due while the lanes of its other rooms idle.
 * (c) The emit launch with each lane storing its own record 49.1 and 297.3 us, with a wavefront's records staged through LDS 51.6
 * and 369.9 us (profiles/decisions_probe_stores.txt, measured once on a build that held both) - the opposite of
 * ge_batch_observe_seats, whose staged records leave as consecutive kilobytes while a list's destinations are scattered; the staged
 * layout was deleted.  (d) The loop at the one-seat shape of ge_batch_run_seats's measurement (human_mask = 1, seat 1 listed, 85 %
 * of the entries due): 3.02 ns against 2.59 ns per point at 65 536 rooms - the list loop is the slower one, x 0.86 -, 0.75 ns
 * against 0.69 ns at 1 048 576 - the list loop is the slower one, x 0.92: where almost every entry is due the list is extra work.
 * No other shape has been measured. */
#define GE_GATHER_SEAT 1u   /* the entry's ge_seat_obs.legal != 0 */
#define GE_GATHER_END  2u   /* the entry's ge_seat_obs.done  != 0 */
int ge_batch_gather_seats(ge_batch *b, uint64_t first, uint64_t count, uint32_t n_seats,
                          const uint32_t *seats /* host, 1-based */, uint32_t want,
                          ge_seat_obs *obs_dev /* DEVICE: cap */, uint32_t *entries_dev /* DEVICE: cap */,
                          uint64_t cap /* entries */, uint32_t *n_dev /* DEVICE: 2 words */, void *hip_stream);
int ge_batch_act_listed(ge_batch *b, uint64_t first, uint64_t count, uint32_t n_seats, const uint32_t *seats /* host */,
                        const uint32_t *n_dev /* DEVICE: 1 word */, uint64_t cap,
                        const uint32_t *entries_dev /* DEVICE: cap */, const int32_t *choices_dev /* DEVICE: cap */,
                        int32_t *status_dev /* DEVICE: cap, may be NULL */, void *hip_stream);

/* GE_FLAG_TRACE: events of the most recent ge_batch_step call, dst[(room - first) * *n_turns + t].
 * cap_bytes >= count * n_turns * sizeof(ge_turn_event).  Synchronises. */
int ge_batch_read_events(ge_batch *b, uint64_t first, uint64_t count, uint32_t *n_turns,
                         ge_turn_event *dst, size_t cap_bytes);

/* Device-side reduction of the whole batch.  Synchronises. */
int ge_batch_summary(ge_batch *b, ge_summary *out);

/* Raw packed state of one segment in HBM (for checkpoint = plain D2H copy, or zero-copy wrapping
 * by the host framework).  bytes_per_room is the algorithmic record size. */
int ge_batch_state(ge_batch *b, uint32_t segment, void **dev_ptr, size_t *bytes, uint32_t *bytes_per_room);

/* Timing of the kernels launched by the most recent ge_batch_step calls since the last reset,
 * measured with hipEvents on the stream they were launched on. */
int ge_batch_set_timing(ge_batch *b, int on);     /* off by default: no events are recorded */
int ge_batch_kernel_time(ge_batch *b, int reset, double *total_ms, uint64_t *launches);

void ge_batch_destroy(ge_batch *b);

/* ---- device group: ONE host process, N GPUs of a node (SURVEY.md 8(e) process model; what a Node addon needs).
 * Rooms never interact - the reference runs one LangGraph thread per room (src/app/api/copilotkit/route.ts:24-37) and has
 * no collective at all (agent/requirements.txt:1-11) - so the group shards rooms and steps the devices concurrently with no
 * exchange; the single collective of the whole job is ONE ncclAllGather (RCCL over xGMI) of the per-device ge_summary.
 *
 * `desc` describes the WHOLE job (desc->device is ignored): device i of n gets the i-th of n contiguous parts of every
 * segment, and every room keeps the global index it has in a single batch of the same desc - results are identical to
 * that batch's, whatever n is.  `devices` are distinct HIP ordinals (duplicates: GE_ERR_ARG); every segment needs at
 * least n rooms.  The group owns one stream per device.  RCCL is loaded at run time (librccl.so.1) when the first group
 * is created - GE_ERR_UNSUPPORTED if there is none; hosts that never create a group never load it.
 * Not thread-safe, like a ge_batch.  The multi-PROCESS form (one rank per GPU, torch.distributed) is game_engine_amd/dist.py. */
typedef struct ge_group ge_group;
/* The group's sharding, for a host that places the shards itself (several per device, or devices of its own choosing without RCCL)
 * - and what ge_group_create does internally: part `part` of `n_parts` takes the part-th of n_parts contiguous parts of every
 * segment of `desc` (the whole job; every segment needs >= n_parts rooms).  *shard = desc with those room counts;
 * seg_first[0 .. GE_MAX_SEGMENTS) = the global index of the part's first room of each segment (what the RNG is keyed by).
 * Pure host arithmetic: no device is touched.  ge_batch_create_shard(shard, seg_first, &b) then creates that part as an ordinary
 * batch (shard->device says where); n such batches hold, room for room, what ONE batch of `desc` holds, and their summaries add up
 * to its summary (checksums and histograms are sums over rooms). */
int ge_group_partition(const ge_batch_desc *desc, int n_parts, int part, ge_batch_desc *shard, uint64_t *seg_first);
int ge_batch_create_shard(const ge_batch_desc *shard, const uint64_t *seg_first, ge_batch **out);
int ge_group_create(const ge_batch_desc *desc, const int *devices, int n_devices, ge_group **out);
int ge_group_size(const ge_group *g);                           /* number of devices, or GE_ERR_ARG */
int ge_group_shard(ge_group *g, int i, ge_batch **out);         /* borrow device i's batch (read_rooms, inject, events ...); owned by the group */
int ge_group_step(ge_group *g, uint32_t n_turns);               /* every shard, asynchronous, each on its device's stream */
int ge_group_sync(ge_group *g);
/* Per-device reductions, one ncclAllGather of the n ge_summary records on the devices' streams, then the sum (every
 * field is a sum over rooms; `turn` is common).  Synchronises. */
int ge_group_summary(ge_group *g, ge_summary *out);
void ge_group_destroy(ge_group *g);
int ge_last_comm_error(void);             /* ncclResult_t of the last GE_ERR_COMM on this thread */

const char *ge_strerror(int status);
int ge_last_hip_error(void);              /* hipError_t of the last GE_ERR_HIP on this thread */
uint64_t ge_last_rejected_room(void);     /* ge_batch_write_rooms(_at) returned GE_ERR_ARG for a view that does not fit its segment: the index (in the batch) of
                                             the first such room, on this thread; ~0 if none yet (ABI 5) */
int ge_abi_version(void);
int ge_device_count(void);                /* number of HIP devices, 0 if none; never fails */

#ifdef __cplusplus
}
#endif
#endif /* GE_STEP_H */

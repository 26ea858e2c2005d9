// ge_rollout.inl — on-device playouts (ge_batch_rollout_rooms): from where a room stands, R replicas of it are played to the end
// (or for M turns) and only their outcome is reduced (included at the end of ge_step.hip, behind ge_pool.inl: the existing kernels
// keep their code-object offsets).  Each chunk's entries are grouped, staged and launched by ge_pool.inl's PoolEntries and by_kind;
// what this file adds is the replica lane, the action and view prologues, the reduction and the chunked staging of a call.
//
// Replica r of entry k is what a lone batch B' (seed, first_room = keys[k], flags 0, one segment of R rooms with human mask 0)
// does to a copy of batch room rooms[k] under set_turn(turns[k]) + step(M): global room keys[k] + r at turns turns[k] ..
// turns[k] + M - 1, every seat played by the policy, a terminal phase absorbing (no GE_FLAG_RESTART).  The result of entry k is
// ge_batch_summary(B') word for word plus per-seat counts (ge_rollout_stats).
//
// One wavefront per (entry, 64 replicas); the lane is the replica.  Nothing of a replica lives in HBM: the source record is loaded
// once (the same address in every lane), unpacked into registers and stepped there with the single-turn ww_turn / tt_turn of the
// lone-wavefront build through ge_pool.inl's indexed lane (lane_ww_ctx / lane_cond_ctx, lane_ww_turn / lane_tt_turn).  Lanes past R stay in the wavefront
// (the action queue is a wave-wide collective): they play replica 0's game again, acting as it does, so that they settle when it
// does, and add nothing.  Prepared role deals are never used (Deal
// {0}: an assignment deals on the spot), so neither the record's deal cache nor the Werewolf x 12 side plane is read.
//
// Early exit.  A turn taken from a terminal phase with restart off moves nowhere (no branch) and applies no effect, but it is not
// always a no-op: bots still act where the terminal row's completion is "action" (orc_room_step / ww_turn / tt_turn log them), and
// the phase-0 guard sets its flag.  A replica is settled when its phase is terminal, that row's completion is not "action" (the
// host's settle mask) and the guard is behind it (not phase 0, or its flag set): then no bot is due, nothing is drawn, and every
// further turn leaves the record bit-identical.  A wavefront leaves the turn loop once __ballot shows every lane settled.
//
// Reduction.  Per wavefront: ballot + popc for the booleans, wave_sum (ge_kernels.inl) for the sums, LDS atomics for the two
// histograms (as ge_summary_kernel); then one lane per field adds the wavefront's non-zero fields to the entry's 75 accumulator
// words with u64 global atomics.  Chosen over per-wave partials + a reduce kernel because partials would need a buffer of
// n * R / 64 records (up to 600 B x 2^20 wavefronts at the caps) and a second launch, while the atomics are at most 75 per
// wavefront after tens to hundreds of turns of work each.  Every field is an integer sum, so the result does not depend on the
// order the wavefronts arrive in.
//
// Playouts after actions (ge_batch_rollout_actions, ACT = 1).  Entry e also carries actions first_action[e] ..
// first_action[e + 1] - 1: the prologue logs them in the loaded source record with the inject_ww / inject_tt of
// ge_batch_inject_actions (row and condition read in place, as inject_group_* does) before the record goes into registers.
// The record and the actions are the same in every lane, so the verdict is wave-uniform; it is kept in a scalar register.
// A refused action refuses the entry: lane 0 of the entry's first wavefront writes its status to status[e], and every
// wavefront of the entry returns before the turn loop and adds nothing.  ge_batch_rollout_rooms launches ACT = 0, whose
// code is the kernel's code before this form existed.
//
// Playouts from a seat's view (ge_batch_rollout_seats, ACT = 2; POLICY.md §3c).  After the actions, each lane re-deals what
// seat seats[e] cannot see in its own copy of the record, from the view key of its replica, before the record goes into
// registers.  The record is the same in every lane at that point, so it is taken into scalar registers (readfirstlane) and
// everything that does not depend on the draws - the unknown seats, the known teams, the hidden tuples sorted by a
// compare-exchange network, the wolf count still to place - is wave-uniform.  Per lane: at most 2 x NB picks (n-th set bit of
// a shrinking mask, every count uniform) and, per tuple, its bits shifted from its uniform source seat to the lane's
// destination seat in a few 64-bit bundles of bit-planes (no array indexed by seat: no scratch).  seats[e] = 0 skips it.
//
// Playouts over a replica range (playout seats under GE_PLAYOUT_HALVING, ACT = 4; POLICY.md §3h; launched by ge_playout.inl and
// ge_run_playout.inl).  Everything ACT = 2 does, for the replicas [lo, hi) of the entry's range instead of [0, R): the lane is
// replica lo + r_in, a lane past hi plays replica lo's game again and adds nothing, and a wavefront whose first lane is past hi
// returns before it loads, writes a status or reduces anything.  The accumulators are not zeroed between rounds: an entry's
// words are the sums over every replica it has played.
//
// Playouts from a traced turn (ge_batch_run_rooms_forecast, ACT = 5; POLICY.md §3i; launched by ge_timeline.inl behind the run
// kernel).  Everything ACT = 2 does without actions, for a block that is (turn t, entry i) of the run in front of it: the source
// record is words 4.. of trace slot t * n_all + first + i instead of a batch room, the first turn is turns[i] + t + 1 and the
// accumulator row is t * n_all + i (turn-major, as the trace plane).  A block whose t is not below the run's played[i] - read
// from device memory, wave-uniform - returns before it loads or reduces anything.
//
// Playouts from a seat's view weighted by the caller's beliefs (ge_batch_rollout_beliefs, ACT = 6, and ACT = 7 with the outcome
// plane of ACT = 3; POLICY.md §3j).  Everything ACT = 2 / ACT = 3 does, except that the two draws of the re-deal that decide
// what the seat cannot see - which seats of Uq are wolves, which statement is the lie - are successive weighted draws by the
// entry's 16 belief bytes.  The bytes are the same in every lane and are taken into four scalar registers; the pick is a
// per-lane running sum over the statically indexed seats of the lane's shrinking `rem` mask (no array indexed by a seat: no
// scratch), so only the draw and `rem` are per lane.  Cost against ACT = 2 on the same entries, measured
// (profiles/beliefs_probe.txt): 65 536 playouts x 1 024 turns per layout 0.96 .. 1.02 x the unweighted call, within the run-to-run
// spread; the single advise call (8 entries x 4 096) x 1.03 .. 1.04 (0.169 / 0.170 against 0.163 ms).
//
// Playouts that keep their outcome (ge_batch_rollout_compare, ACT = 3; ge_compare.inl).  Everything ACT = 2 does; then each lane
// stores the outcome X of its replica for seat subjects[e] - Werewolf: the seat's team has won, Two-Truths: the seat's
// total_score - as one byte of the entry's row of the outcome plane (waves * 64 bytes per row: a wavefront's lanes write 64
// consecutive bytes; a lane past R writes 0).  A refused entry writes nothing: its row is never read.

namespace {

// accumulator words of one entry: [0] finished [1] village [2] wolves [3] alive [4] sum_end [5..20] end hist [21..36] score hist
// [37] checksum [38] games [39..50] seat_alive [51..62] seat_wins [63..74] seat_score (stride ROLL_STRIDE)
constexpr uint32_t ROLL_FIELDS = 75, ROLL_STRIDE = 80;

struct RolloutArgs {
    const uint64_t *rooms;      // segment-local source room of each entry of this launch
    const uint64_t *keys;       // replica r of entry e is global room keys[e] + r
    const uint32_t *turns;      // its first turn
    unsigned long long *acc;    // [n] x ROLL_STRIDE accumulator words, zeroed by the host
    uint32_t n, seg, seed_key, n_rollouts, max_turns, waves;   // waves: wavefronts per entry (ceil(R / 64))
    uint32_t settle_mask;       // bit p = row p is terminal and its completion is not "action"
};

// the arguments of one form: ACT = 1 adds the entries' actions (CSR over this launch's entries) and their verdicts
template <int ACT> struct RollArgs : RolloutArgs {
    const uint32_t *first_action;   // entry e's actions are players / choices [first_action[e], first_action[e + 1])
    const uint32_t *players, *choices;
    int32_t *status;                // entry e refused: the refused action's status (written once, by the entry's first wavefront)
};
template <> struct RollArgs<0> : RolloutArgs {};
// ACT = 2: the actions, then the view of seat seats[e] (1-based; 0 = the full view)
template <> struct RollArgs<2> : RollArgs<1> {
    const uint32_t *seats;
};
// ACT = 3: the same, and the outcome of every replica for seat subjects[e] (1-based) into row e of the outcome plane
template <> struct RollArgs<3> : RollArgs<2> {
    const uint32_t *subjects;
    unsigned char *plane;           // [n] rows of waves * 64 bytes
};
// ACT = 4: ACT = 2 over a replica range per entry (POLICY.md §3h): entry e plays replicas [range[e].x, range[e].y), lane r_in of
// the entry the replica range[e].x + r_in; x > y marks an entry that plays no more (ge_playout_halve)
template <> struct RollArgs<4> : RollArgs<2> {
    const u32x2 *range;
};

// ACT = 5: ACT = 2 without actions from a turn of the run traced in front of it (POLICY.md §3i): entry e = t * n + i is turn t of
// this launch's entry i (keys, turns, seats and run_out are indexed by i; rooms and the action arrays are not read)
template <> struct RollArgs<5> : RollArgs<2> {
    const u32x4 *trace;             // the run's trace plane (64 B per room-turn, turn-major over n_all entries)
    const u32x2 *run_out;           // [n]: the run's (played, stop bits)
    uint32_t n_all, first;          // this launch's entries are the plane's entries first .. first + n - 1
};

// ACT = 6 / 7: ACT = 2 / 3 under the entry's beliefs (POLICY.md §3j): entry e's 16 bytes are beliefs[e], byte c = seat c + 1
// (Werewolf) or statement c + 1 (Two-Truths)
template <> struct RollArgs<6> : RollArgs<2> {
    const u32x4 *beliefs;
};
template <> struct RollArgs<7> : RollArgs<3> {
    const u32x4 *beliefs;
};
constexpr bool roll_weighted(int act) { return act == 6 || act == 7; }
constexpr bool roll_keeps(int act) { return act == 3 || act == 7; }

struct RollLane {
    RoomStats q;                // (zero on lanes past R)
    uint64_t ck;
    uint32_t alive_mask, win_mask;
};

// a wave-uniform 64-bit value in scalar registers (readfirstlane returns int: each half is taken back as uint32_t before widening)
__device__ __forceinline__ uint64_t uniform_u64(uint64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)v), hi = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint32_t roll_popc(bool b) { return (uint32_t)__popcll(__ballot(b)); }

// the wavefront's contribution -> the entry's accumulator words (lane 0 holds every wave_sum; the block is one wavefront)
template <int NB>
__device__ __forceinline__ void roll_reduce(const RollLane &l, bool valid, const uint32_t *score, unsigned long long *part, uint32_t *h_end,
                                            const uint32_t *h_score, unsigned long long *acc) {
    const uint32_t lane = threadIdx.x;
    const bool ended = valid && l.q.finished && l.q.end_turn != END_NONE;
    if (ended) atomicAdd(&h_end[(l.q.end_turn >> 3) < 15 ? (l.q.end_turn >> 3) : 15], 1u);
    const uint64_t v3 = wave_sum(l.q.alive), v4 = wave_sum(ended ? l.q.end_turn : 0u), v5 = wave_sum(l.ck), v6 = wave_sum(l.q.games);
    uint64_t sc[NB];
#pragma unroll
    for (int i = 0; i < NB; i++) sc[i] = wave_sum(score[i]);
    uint32_t alive_n[NB], win_n[NB];
#pragma unroll
    for (int i = 0; i < NB; i++) {
        alive_n[i] = roll_popc(valid && ((l.alive_mask >> i) & 1u));
        win_n[i] = roll_popc(valid && ((l.win_mask >> i) & 1u));
    }
    const uint32_t fin = roll_popc(valid && l.q.finished), vil = roll_popc(valid && l.q.village), wol = roll_popc(valid && l.q.wolves);
    if (lane == 0) {
        part[0] = fin; part[1] = vil; part[2] = wol; part[3] = v3; part[4] = v4; part[37] = v5; part[38] = v6;
#pragma unroll
        for (int i = 0; i < 12; i++) {
            part[39 + i] = i < NB ? alive_n[i < NB ? i : 0] : 0u;
            part[51 + i] = i < NB ? win_n[i < NB ? i : 0] : 0u;
            part[63 + i] = i < NB ? sc[i < NB ? i : 0] : 0u;
        }
    }
    __syncthreads();
    if (lane < 16) { part[5 + lane] = h_end[lane]; part[21 + lane] = h_score[lane]; }
    __syncthreads();
    for (uint32_t f = lane; f < ROLL_FIELDS; f += 64u) {
        const unsigned long long v = part[f];
        if (v) atomicAdd(&acc[f], v);
    }
}

__device__ __forceinline__ uint64_t roll_ck(uint32_t h_words) {
    return (uint64_t)h_words | ((uint64_t)mix32(h_words ^ 0x5BD1E995u) << 32);
}
__device__ __forceinline__ uint32_t roll_h0(uint64_t g) { return mix32((uint32_t)g ^ mix32((uint32_t)(g >> 32) ^ 0xA5A5A5A5u)); }

// the replica's outcome byte into the entry's row of the outcome plane (ACT = 3): lane r_in of the entry, a plain vector store
__device__ __forceinline__ void roll_keep(const RollArgs<3> &a, uint32_t e, uint32_t r_in, uint32_t x) {
    a.plane[(size_t)e * ((size_t)a.waves * 64u) + r_in] = (unsigned char)x;
}

// the source record of ACT = 5: the packed record of turn t of entry i, as run_trace stored it behind the event's four words
template <int WORDS>
__device__ __forceinline__ void roll_load_trace(const RollArgs<5> &a, uint32_t t, uint32_t i, uint32_t *w) {
    const u32x4 *slot = a.trace + 4u * ((size_t)t * a.n_all + a.first + i);
#pragma unroll
    for (int j = 0; j < (WORDS + 3) / 4; j++) {
        const u32x4 v = slot[1 + j];
        w[4 * j] = v.x; w[4 * j + 1] = v.y;
        if (4 * j + 2 < WORDS) w[4 * j + 2] = v.z;
        if (4 * j + 3 < WORDS) w[4 * j + 3] = v.w;
    }
}

// the entry's actions logged in its source record (ACT = 1 prologue); false (wave-uniform) = refused, status[e] written
__device__ __forceinline__ bool roll_refuse(const RollArgs<1> &a, uint32_t e, uint32_t r_in, int st) {
    st = __builtin_amdgcn_readfirstlane(st);
    if (st == GE_OK) return true;
    if (r_in == 0u) a.status[e] = st;                         // lane 0 of the entry's first wavefront
    return false;
}
template <int NB>
__device__ __forceinline__ bool roll_act_ww(const SegDev &sg, const DevTable *__restrict__ tables, const RollArgs<1> &a, uint32_t e, uint32_t r_in,
                                            uint32_t *w) {
    using L = WWLayout<NB>;
    WW<NB> s;
    L::unpack(w, s);
    const DevRow &row = tables[sg.table_idx].rows[s.phase];
    const DevCond &cond = tables[sg.table_idx].conds[s.phase];   // read in place, as inject_group_ww
    const uint32_t lo = __builtin_amdgcn_readfirstlane(a.first_action[e]), hi = __builtin_amdgcn_readfirstlane(a.first_action[e + 1u]);
    int st = GE_OK;
    for (uint32_t k = lo; k < hi && st == GE_OK; k++) st = inject_ww<NB>(s, row, cond, sg.n_players, a.players[k], a.choices[k]);
    if (!roll_refuse(a, e, r_in, st)) return false;
    L::pack(s, w);
    return true;
}
template <int NB>
__device__ __forceinline__ bool roll_act_tt(const SegDev &sg, const DevTable *__restrict__ tables, const RollArgs<1> &a, uint32_t e, uint32_t r_in,
                                            TT<NB> &s) {
    const DevRow &row = tables[sg.table_idx].rows[s.phase];
    const DevCond &cond = tables[sg.table_idx].conds[s.phase];   // read in place, as inject_group_tt
    const uint32_t lo = __builtin_amdgcn_readfirstlane(a.first_action[e]), hi = __builtin_amdgcn_readfirstlane(a.first_action[e + 1u]);
    int st = GE_OK;
    for (uint32_t k = lo; k < hi && st == GE_OK; k++) st = inject_tt<NB>(s, row, cond, sg.n_players, a.players[k], a.choices[k]);
    return roll_refuse(a, e, r_in, st);
}

// ---- the view re-deal (POLICY.md §3c).  vk = the replica's view key.
__device__ __forceinline__ uint32_t view_key(uint32_t rk, uint32_t turn0) { return mix32(rk ^ 0x56494557u ^ (turn0 * GOLDEN)); }

// an entry's beliefs in scalar registers (the same in every lane); byte c of the 16
struct Beliefs {
    uint32_t w[4];
    __device__ __forceinline__ uint32_t at(int c) const { return (w[c >> 2] >> (8 * (c & 3))) & 255u; }
};
__device__ __forceinline__ Beliefs roll_beliefs(const u32x4 *beliefs, uint32_t e) {
    const u32x4 v = beliefs[e];
    Beliefs b;
    b.w[0] = (uint32_t)__builtin_amdgcn_readfirstlane(v.x); b.w[1] = (uint32_t)__builtin_amdgcn_readfirstlane(v.y);
    b.w[2] = (uint32_t)__builtin_amdgcn_readfirstlane(v.z); b.w[3] = (uint32_t)__builtin_amdgcn_readfirstlane(v.w);
    return b;
}

// the weighted pick of POLICY.md §3j over the first N slots of `rem` (bit c = slot c may be taken; cnt >= 1 of them,
// wave-uniform): the bit of the first slot whose running sum of weights exceeds x = pick(d, W), W the sum over `rem`; W == 0:
// every weight 1.  The running sum grows only at a slot of `rem` with a weight, so the lowest slot at which it exceeds x is
// such a slot.
template <int N> __device__ __forceinline__ uint32_t weighted_pick(const Beliefs &bw, uint32_t rem, uint32_t cnt, uint32_t d) {
    uint32_t W = 0;
#pragma unroll
    for (int c = 0; c < N; c++) W += ((rem >> c) & 1u) ? bw.at(c) : 0u;
    const bool flat = W == 0u;
    const uint32_t x = pick(d, flat ? cnt : W);
    uint32_t acc = 0, over = 0;
#pragma unroll
    for (int c = 0; c < N; c++) {
        acc += ((rem >> c) & 1u) ? (flat ? 1u : bw.at(c)) : 0u;
        over |= (acc > x ? 1u : 0u) << c;
    }
    return over & (0u - over);
}

// Werewolf: what seat `seat` (1-based) of the n players of record `u` knows of the others (POLICY.md §3c), declared in the scope
// that names it: U the seats whose hidden tuple it cannot see, Uw / Uv those of them it knows to be werewolves / not to be - both
// empty where a Detective's memory does not fit the record -, nA / nB the werewolves / the others among U, team_w the record's,
// s_wolf / s_det the seat's own side and role class.  The re-deal below and the seat observation (ge_env.inl, §3n) both take their
// sets from here.  A macro, not a function: through an inlined call the same statements moved the register allocation of the
// playout kernels beyond what tools/asm_baseline.json allows (Werewolf x 12 over a replica range: 64 spilled scalar registers
// for 37); expanded in place, the re-deal compiles to the code it had before the statements had a second user.
#define GE_VIEW_SETS_WW(u, seat, n)                                                                                       \
    const uint32_t all = (1u << (n)) - 1u, me = 1u << ((seat) - 1u);                                                      \
    const uint32_t U = all & ~(u).revealed & ~me;                                                                         \
    const uint32_t team_w = (u).team_w;                                                                                   \
    const bool s_wolf = (team_w & me) != 0u;                                                                              \
    const bool s_det = ((u).rb2 & me) && !((u).rb1 & me) && !((u).rb0 & me);                                              \
    uint32_t Uw = s_wolf ? (U & team_w) : s_det ? (U & (u).det_w) : 0u;                                                   \
    uint32_t Uv = s_wolf ? (U & ~team_w) : s_det ? (U & (u).det_v) : 0u;                                                  \
    const uint32_t nA = popc(U & team_w), nB = popc(U & ~team_w);                                                         \
    {                                                                                                                     \
        const int need = (int)nA - (int)popc(Uw);                                                                         \
        if (need < 0 || need > (int)popc(U & ~Uw & ~Uv)) { Uw = 0u; Uv = 0u; }   /* the Detective's knowledge does not fit */ \
    }

// Werewolf: the hidden tuples of the seats seat s cannot rule out, dealt again over the seats they may sit on.  `u` holds the
// record (wave-uniform on entry); priv = the phase's action log is private (WOLF_TARGET / DOCTOR_PROTECT / DETECTIVE).
// WT: step 1 places the wolves by the beliefs `bw` (POLICY.md §3j) instead of uniformly.
template <int NB, bool WT = false>
__device__ __forceinline__ void view_redeal_ww(WW<NB> &u, uint32_t seat, uint32_t n, bool priv, uint32_t vk, const Beliefs &bw = Beliefs{}) {
    constexpr int S = NB <= 8 ? 8 : 16;                      // bit-plane stride in a bundle
    constexpr uint64_t REP = NB <= 8 ? 0x0101010101010101ull : 0x0001000100010001ull;
    GE_VIEW_SETS_WW(u, seat, n)
    const uint32_t Uq = U & ~Uw & ~Uv, need = nA - popc(Uw);
    // the hidden tuples as sort keys: (team is werewolves, role, team, secret, elig, sub, sel[, acted, choice], seat), so the
    // sorted list is B ascending, then A ascending; seats outside U sort last
    uint32_t key[NB];
#pragma unroll
    for (int c = 0; c < NB; c++) {
        const uint32_t role = ((u.rb0 >> c) & 1u) | ((u.rb1 >> c) & 1u) << 1 | ((u.rb2 >> c) & 1u) << 2;
        const uint32_t team = ((u.team_v >> c) & 1u) | ((team_w >> c) & 1u) << 1;
        const uint32_t sel = (uint32_t)(u.sel >> (4 * c)) & 15u, ch = priv ? (uint32_t)(u.choice >> (4 * c)) & 15u : 0u;
        const uint32_t act = priv ? (u.acted >> c) & 1u : 0u;
        const uint32_t k = ((team_w >> c) & 1u) << 27 | role << 24 | team << 22 | ((u.secret >> c) & 1u) << 21 | ((u.elig >> c) & 1u) << 20 |
                           ((u.sub >> c) & 1u) << 19 | sel << 15 | act << 14 | ch << 10 | (uint32_t)c;
        key[c] = ((U >> c) & 1u) ? k : 0xFFFFFFFFu;
    }
#pragma unroll
    for (int i = 0; i < NB; i++)                             // compare-exchange network (odd-even transposition): static indices
#pragma unroll
        for (int j = i & 1; j + 1 < NB; j += 2) {
            const uint32_t lo = key[j] < key[j + 1] ? key[j] : key[j + 1], hi = key[j] < key[j + 1] ? key[j + 1] : key[j];
            key[j] = lo; key[j + 1] = hi;
        }
    // step 1: the wolf seats.  Every count is uniform, so no lane needs a popcount
    uint32_t sw = Uw, rem = Uq;
    for (uint32_t j = 0; j < need; j++) {
        uint32_t bit;
        if constexpr (WT) bit = weighted_pick<NB>(bw, rem, popc(Uq) - j, draw(vk, 32u + j));
        else bit = 1u << nth_set_bit<NB>(rem, pick(draw(vk, 32u + j), popc(Uq) - j));
        sw |= bit; rem &= ~bit;
    }
    uint32_t remW = sw, remV = U & ~sw;
    // the moved fields as bundles of bit-planes (stride S) and of nibbles
    const uint32_t acted_m = priv ? u.acted : 0u;
    const uint64_t P0 = NB <= 8 ? ((uint64_t)u.rb0 | (uint64_t)u.rb1 << 8 | (uint64_t)u.rb2 << 16 | (uint64_t)u.team_v << 24 | (uint64_t)team_w << 32 |
                                   (uint64_t)u.secret << 40 | (uint64_t)u.elig << 48 | (uint64_t)u.sub << 56)
                                : ((uint64_t)u.rb0 | (uint64_t)u.rb1 << 16 | (uint64_t)u.rb2 << 32 | (uint64_t)u.team_v << 48);
    const uint64_t P1 = NB <= 8 ? (uint64_t)acted_m
                                : ((uint64_t)team_w | (uint64_t)u.secret << 16 | (uint64_t)u.elig << 32 | (uint64_t)u.sub << 48);
    const uint64_t P2 = (uint64_t)acted_m;                   // (NB > 8 only)
    const uint64_t ch_m = priv ? (uint64_t)u.choice : 0ull;
    const uint64_t N0 = NB <= 8 ? ((uint64_t)u.sel | ch_m << 32) : (uint64_t)u.sel;
    const uint64_t N1 = ch_m;                                // (NB > 8 only)
    const uint64_t Urep = (uint64_t)U * REP;
    uint64_t nU = 0;                                         // U as a nibble mask
#pragma unroll
    for (int c = 0; c < NB; c++) nU |= ((U >> c) & 1u) ? 15ull << (4 * c) : 0ull;
    const uint64_t nUrep = NB <= 8 ? (nU | nU << 32) : nU;
    uint64_t q0 = P0 & ~Urep, q1 = P1 & ~Urep, q2 = P2 & ~Urep, m0 = N0 & ~nUrep, m1 = N1 & ~nU;
#pragma unroll
    for (int q = 0; q < NB; q++) {                           // sorted position q: B[q] while q < nB, then A[q - nB]
        if ((uint32_t)q < nA + nB) {
            const bool inA = (uint32_t)q >= nB;
            const uint32_t i = inA ? (uint32_t)q - nB : (uint32_t)q;
            const uint32_t d = pick(draw(vk, (inA ? 48u : 64u) + i), (inA ? nA : nB) - i);
            const uint32_t dst = nth_set_bit<NB>(inA ? remW : remV, d), bit = 1u << dst;
            remW = inA ? remW & ~bit : remW;
            remV = inA ? remV : remV & ~bit;
            const uint32_t src = key[q] & 15u;
            q0 |= ((P0 >> src) & REP) << dst;
            q1 |= ((P1 >> src) & REP) << dst;
            if (NB > 8) q2 |= ((P2 >> src) & 1ull) << dst;
            m0 |= ((N0 >> (4 * src)) & (NB <= 8 ? 0x0000000F0000000Full : 15ull)) << (4 * dst);
            if (NB > 8) m1 |= ((N1 >> (4 * src)) & 15ull) << (4 * dst);
        }
    }
    constexpr uint32_t FM = (1u << NB) - 1u;
    u.rb0 = (uint32_t)q0 & FM; u.rb1 = (uint32_t)(q0 >> S) & FM; u.rb2 = (uint32_t)(q0 >> (2 * S)) & FM; u.team_v = (uint32_t)(q0 >> (3 * S)) & FM;
    if (NB <= 8) {
        u.team_w = (uint32_t)(q0 >> 32) & FM; u.secret = (uint32_t)(q0 >> 40) & FM; u.elig = (uint32_t)(q0 >> 48) & FM; u.sub = (uint32_t)(q0 >> 56) & FM;
        if (priv) { u.acted = (uint32_t)q1 & FM; u.choice = (typename WW<NB>::nib_t)(m0 >> 32); }
        u.sel = (typename WW<NB>::nib_t)(uint32_t)m0;
    } else {
        u.team_w = (uint32_t)q1 & FM; u.secret = (uint32_t)(q1 >> 16) & FM; u.elig = (uint32_t)(q1 >> 32) & FM; u.sub = (uint32_t)(q1 >> 48) & FM;
        if (priv) { u.acted = (uint32_t)q2 & FM; u.choice = (typename WW<NB>::nib_t)m1; }
        u.sel = (typename WW<NB>::nib_t)m0;
    }
    if (!s_det) {                                            // the Detective's memory follows the new deal (2 werewolves, else 1)
        const uint32_t K = U & (u.det_v | u.det_w);
        u.det_w = (u.det_w & ~K) | (K & u.team_w);
        u.det_v = (u.det_v & ~K) | (K & ~u.team_w);
    }
}

// Two-Truths: the lie of speaker `sp` (0-based: the lowest speaker) is no secret to seat `seat` - its own, or revealed (§3c; a
// macro for the reason GE_VIEW_SETS_WW is one)
#define GE_VIEW_SHOWN_TT(sp, revealed, seat) ((sp) == (seat) - 1u || (((revealed) >> (sp)) & 1u))

// Two-Truths: the speaker's lie, drawn again for a seat that is not the speaker, before the reveal (`s` wave-uniform)
// WT: the lie is drawn by the beliefs' first three bytes (POLICY.md §3j)
template <int NB, bool WT = false>
__device__ __forceinline__ void view_redeal_tt(TT<NB> &s, uint32_t seat, uint32_t vk, const Beliefs &bw = Beliefs{}) {
    const uint32_t spk = (uint32_t)__builtin_amdgcn_readfirstlane(s.speaker), lie = (uint32_t)__builtin_amdgcn_readfirstlane(s.lie);
    const uint32_t rev = (uint32_t)__builtin_amdgcn_readfirstlane(s.revealed);
    if (spk == 0u) return;
    const uint32_t sp = ctz(spk);                            // the lowest speaker
    if (GE_VIEW_SHOWN_TT(sp, rev, seat) || ((lie >> (2 * sp)) & 3u) == 0u) return;
    uint32_t fresh;
    if constexpr (WT) fresh = 1u + ctz(weighted_pick<3>(bw, 7u, 3u, draw(vk, 80u)));
    else fresh = 1u + pick(draw(vk, 80u), 3u);
    s.lie = (lie & ~(3u << (2 * sp))) | fresh << (2 * sp);
}

// the ACT = 2 prologue of a Werewolf entry: the record words after the actions, re-dealt for the entry's seat in this lane
template <int NB, bool WT = false>
__device__ __forceinline__ void roll_view_ww(const SegDev &sg, const DevTable *__restrict__ tables, const RollArgs<2> &a, uint32_t e,
                                             uint32_t rk, uint32_t turn0, uint32_t *w, const u32x4 *beliefs = nullptr) {
    using L = WWLayout<NB>;
    const uint32_t seat = (uint32_t)__builtin_amdgcn_readfirstlane(a.seats[e]);
    if (seat == 0u) return;
#pragma unroll
    for (int i = 0; i < L::WORDS; i++) w[i] = (uint32_t)__builtin_amdgcn_readfirstlane(w[i]);   // the same in every lane
    WW<NB> u;
    L::unpack(w, u);
    const uint32_t act = (tables[sg.table_idx].rows[u.phase].r0 >> 2) & 7u;
    const bool priv = act == ACT_WOLF_TARGET || act == ACT_DOCTOR_PROTECT || act == ACT_DETECTIVE;
    if constexpr (WT) view_redeal_ww<NB, true>(u, seat, sg.n_players, priv, view_key(rk, turn0), roll_beliefs(beliefs, e));
    else view_redeal_ww<NB>(u, seat, sg.n_players, priv, view_key(rk, turn0));
    L::pack(u, w);
}

template <int NB, int GENERIC, int ACT>
__device__ __forceinline__ void roll_ww(const SegDev &sg, const DevTable *__restrict__ tables, const RollArgs<ACT> &a, void *lw, uint32_t e,
                                        uint32_t r_in, unsigned long long *part, uint32_t *h_end, uint32_t *h_score) {
    using L = WWLayout<NB>;
    uint32_t r_lo = 0u, r_hi = a.n_rollouts;
    if constexpr (ACT == 4) {                                 // the entry's replica range: wave-uniform
        const u32x2 rg = a.range[e];
        r_lo = (uint32_t)__builtin_amdgcn_readfirstlane(rg.x); r_hi = (uint32_t)__builtin_amdgcn_readfirstlane(rg.y);
        const uint32_t r_first = (uint32_t)__builtin_amdgcn_readfirstlane(r_in);
        if (r_lo > r_hi || r_first >= r_hi - r_lo) return;    // nothing of the range in this wavefront: it touches nothing
    }
    uint32_t row = e, t_src = 0u;                             // the accumulator row; ACT = 5: the traced turn the block starts from
    if constexpr (ACT == 5) {                                 // block = (turn, entry) of the run: wave-uniform
        t_src = e / a.n; e -= t_src * a.n;
        if (t_src >= (uint32_t)__builtin_amdgcn_readfirstlane(a.run_out[e].x)) return;   // a turn nobody played: it touches nothing
        row = t_src * a.n_all + e;
    }
    const bool valid = r_in < r_hi - r_lo;
    const uint32_t r = r_lo + (valid ? r_in : 0u);
    uint64_t room = 0;
    if constexpr (ACT != 5) room = uniform_u64(a.rooms[e]);
    const uint64_t key = uniform_u64(a.keys[e]);
    const uint32_t turn0 = (uint32_t)__builtin_amdgcn_readfirstlane(a.turns[e]) + (ACT == 5 ? t_src + 1u : 0u);
    uint32_t w[L::WORDS];
    if constexpr (ACT == 5) roll_load_trace<L::WORDS>(a, t_src, e, w);
    else load_words<L::WORDS>(sg.base, sg.rooms_padded, room, w);
    if constexpr (ACT != 0 && ACT != 5)
        if (!roll_act_ww<NB>(sg, tables, a, e, r_in, w)) return;
    const uint64_t g = key + r;
    const uint32_t rk = room_key_from(a.seed_key, g);
    if constexpr (roll_weighted(ACT)) roll_view_ww<NB, true>(sg, tables, a, e, rk, turn0, w, a.beliefs);
    else if constexpr (ACT >= 2) roll_view_ww<NB>(sg, tables, a, e, rk, turn0, w);
    const uint32_t phase0 = __builtin_amdgcn_readfirstlane(sg.phase0_idx);
    const WwCtx ctx = lane_ww_ctx<GENERIC>(sg, tables, lw, rk, true, 0u);   // every seat played by the policy
    const DevRow *rows = ctx.rows;
    WWR<NB> s;
    uint32_t cache;                                           // the record's prepared deal: not of these keys, never used
    ww_load_regs<NB>(w, s, cache);
    for (uint32_t t = 0; t < a.max_turns; t++) {
        lane_ww_turn<NB, GENERIC>(s, ctx, turn0 + t, false);
        const bool settled = ((a.settle_mask >> s.phase) & 1u) && (s.phase != phase0 || (s.flags & FLAG_PHASE0_DONE));
        if (__ballot(!settled) == 0ull) break;
    }
    ww_store_regs<NB>(s, 0u, w);                              // the canonical record: no prepared deal
    RollLane l;
    l.q = stats_ww<NB>(w, rows, h_score);
    if (NB == 8) w[7] &= WWLayout<8>::CHECKSUM_MASK7;
    l.ck = roll_ck(fold_words<L::WORDS>(roll_h0(g), w));
    const uint32_t alive = s.template get<F_ALIVE>();
    l.alive_mask = alive;
    l.win_mask = !l.q.finished ? 0u : (l.q.village ? s.template get<F_TEAM_V>() : s.template get<F_TEAM_W>());
    if (!valid) { l.q = RoomStats{0, 0, 0, 0, 0, 0}; l.ck = 0; }
    uint32_t score[NB];
#pragma unroll
    for (int i = 0; i < NB; i++) score[i] = 0u;
    if constexpr (roll_keeps(ACT)) {
        const uint32_t subj = (uint32_t)__builtin_amdgcn_readfirstlane(a.subjects[e]) - 1u;
        roll_keep(a, e, r_in, valid ? (l.win_mask >> subj) & 1u : 0u);
    }
    roll_reduce<NB>(l, valid, score, part, h_end, h_score, a.acc + (size_t)row * ROLL_STRIDE);
}

template <int NB, int GENERIC, int ACT>
__device__ __forceinline__ void roll_tt(const SegDev &sg, const DevTable *__restrict__ tables, const RollArgs<ACT> &a, void *lw, uint32_t e,
                                        uint32_t r_in, unsigned long long *part, uint32_t *h_end, uint32_t *h_score) {
    using L = TTLayout<NB>;
    uint32_t r_lo = 0u, r_hi = a.n_rollouts;
    if constexpr (ACT == 4) {                                 // the entry's replica range: wave-uniform
        const u32x2 rg = a.range[e];
        r_lo = (uint32_t)__builtin_amdgcn_readfirstlane(rg.x); r_hi = (uint32_t)__builtin_amdgcn_readfirstlane(rg.y);
        const uint32_t r_first = (uint32_t)__builtin_amdgcn_readfirstlane(r_in);
        if (r_lo > r_hi || r_first >= r_hi - r_lo) return;    // nothing of the range in this wavefront: it touches nothing
    }
    uint32_t row = e, t_src = 0u;                             // the accumulator row; ACT = 5: the traced turn the block starts from
    if constexpr (ACT == 5) {                                 // block = (turn, entry) of the run: wave-uniform
        t_src = e / a.n; e -= t_src * a.n;
        if (t_src >= (uint32_t)__builtin_amdgcn_readfirstlane(a.run_out[e].x)) return;   // a turn nobody played: it touches nothing
        row = t_src * a.n_all + e;
    }
    const bool valid = r_in < r_hi - r_lo;
    const uint32_t r = r_lo + (valid ? r_in : 0u);
    uint64_t room = 0;
    if constexpr (ACT != 5) room = uniform_u64(a.rooms[e]);
    const uint64_t key = uniform_u64(a.keys[e]);
    const uint32_t turn0 = (uint32_t)__builtin_amdgcn_readfirstlane(a.turns[e]) + (ACT == 5 ? t_src + 1u : 0u);
    uint32_t w[L::WORDS];
    if constexpr (ACT == 5) roll_load_trace<L::WORDS>(a, t_src, e, w);
    else load_words<L::WORDS>(sg.base, sg.rooms_padded, room, w);
    const uint64_t g = key + r;
    const uint32_t rk = room_key_from(a.seed_key, g);
    const unsigned char *img = reinterpret_cast<const unsigned char *>(tables + sg.table_idx);
    const DevRow *rows = reinterpret_cast<const DevRow *>(img);
    const CondCtx cc = lane_cond_ctx<GENERIC>(sg, tables);
    const uint32_t term_mask = __builtin_amdgcn_readfirstlane(sg.term_mask);
    const uint32_t phase0 = __builtin_amdgcn_readfirstlane(sg.phase0_idx);
    TT<NB> s;
    L::unpack(w, s);
    if constexpr (ACT != 0 && ACT != 5)
        if (!roll_act_tt<NB>(sg, tables, a, e, r_in, s)) return;
    if constexpr (ACT >= 2) {
        const uint32_t seat = (uint32_t)__builtin_amdgcn_readfirstlane(a.seats[e]);
        if constexpr (roll_weighted(ACT)) {
            if (seat != 0u) view_redeal_tt<NB, true>(s, seat, view_key(rk, turn0), roll_beliefs(a.beliefs, e));
        } else if (seat != 0u) view_redeal_tt<NB>(s, seat, view_key(rk, turn0));
    }
    uint32_t done = tt_done_mask<NB>(s.rounds, sg.rounds);
    for (uint32_t t = 0; t < a.max_turns; t++) {
        lane_tt_turn<NB, GENERIC>(s, done, sg, tables, cc, lw, true, rk, turn0 + t, false, 0u, term_mask);
        const bool settled = ((a.settle_mask >> s.phase) & 1u) && (s.phase != phase0 || (s.flags & FLAG_PHASE0_DONE));
        if (__ballot(!settled) == 0ull) break;
    }
    L::pack(s, w);
    RollLane l;
    l.q = stats_tt<NB>(w, rows, valid ? sg.n_players : 0u, h_score);   // (0 players: a lane past R adds nothing to the histogram)
    l.ck = roll_ck(fold_words<L::WORDS>(roll_h0(g), w));
    uint32_t score[NB], top = 0;
#pragma unroll
    for (int i = 0; i < NB; i++) {                            // static indices: no scratch
        score[i] = (uint32_t)i < sg.n_players ? (s.score[i / 4] >> (8 * (i % 4))) & 255u : 0u;
        top = score[i] > top ? score[i] : top;
    }
    uint32_t win = 0;
#pragma unroll
    for (int i = 0; i < NB; i++) win |= ((uint32_t)i < sg.n_players && score[i] == top ? 1u : 0u) << i;
    l.alive_mask = 0;
    l.win_mask = l.q.finished ? win : 0u;
    if (!valid) {
        l.q = RoomStats{0, 0, 0, 0, 0, 0}; l.ck = 0;
#pragma unroll
        for (int i = 0; i < NB; i++) score[i] = 0u;
    }
    if constexpr (roll_keeps(ACT)) {
        const uint32_t subj = (uint32_t)__builtin_amdgcn_readfirstlane(a.subjects[e]) - 1u;
        uint32_t x = 0;
#pragma unroll
        for (int i = 0; i < NB; i++) x = (uint32_t)i == subj ? score[i] : x;   // static indices: no scratch
        roll_keep(a, e, r_in, x);
    }
    roll_reduce<NB>(l, valid, score, part, h_end, h_score, a.acc + (size_t)row * ROLL_STRIDE);
}

// one wavefront per block = one entry's 64 replicas; its action queue (WaveLdsLow) is the block's dynamic LDS (none for
// Two-Truths x 4: no queue)
template <int KIND, int GENERIC, int ACT>
__global__ void __launch_bounds__(64) ge_rollout_kernel(const SegDev *__restrict__ segs, const DevTable *__restrict__ tables, const RollArgs<ACT> a) {
    __shared__ unsigned long long part[ROLL_FIELDS];
    __shared__ uint32_t h_end[16], h_score[16];
    const SegDev &sg = segs[a.seg];
    const uint32_t e = blockIdx.x / a.waves, r = (blockIdx.x - e * a.waves) * 64u + threadIdx.x;
    if (threadIdx.x < ROLL_FIELDS) part[threadIdx.x] = 0;
    if (threadIdx.x < 16) { h_end[threadIdx.x] = 0; h_score[threadIdx.x] = 0; }
    __syncthreads();
    void *lw = ge_lds;
    if constexpr (KindOf<KIND>::WW) roll_ww<KindOf<KIND>::NB, GENERIC, ACT>(sg, tables, a, lw, e, r, part, h_end, h_score);
    else roll_tt<KindOf<KIND>::NB, GENERIC, ACT>(sg, tables, a, lw, e, r, part, h_end, h_score);
}

template <int GEN, int ACT> hipError_t rollout_launch(uint32_t kind, dim3 grid, hipStream_t st, const ge_batch *b, const RollArgs<ACT> &a) {
    return by_kind(kind, [&](auto K) { hipLaunchKernelGGL((ge_rollout_kernel<K(), GEN, ACT>), grid, dim3(64), lane_lds(kind), st, b->segs_dev, b->tables, a); });
}

// bit p = row p of the segment's table is terminal and no bot acts in it (see "Early exit" above)
uint32_t rollout_settle_mask(const Segment &sg) {
    uint32_t m = 0;
    for (int p = 0; p < sg.table.n_phases && p < 32; p++)
        if (((sg.dev.term_mask >> p) & 1u) && sg.table.rows[p].completion != GE_COMP_ACTION) m |= 1u << p;
    return m;
}

}  // namespace

// one call of the three entry points.  first_action null: every entry's slice is empty; seats null: the full view.  act is the
// kernel form the call launches: 0 = ge_batch_rollout_rooms, 1 = ge_batch_rollout_actions, 2 = ge_batch_rollout_seats,
// 3 = ge_batch_rollout_compare (ge_compare.inl; baseline / subjects / cmp are its own); `weighted` launches 2 as 6 and 3 as 7
// (ge_batch_rollout_beliefs, ge_compare.inl)
struct RollRequest {
    uint64_t n;
    const uint64_t *rooms, *keys;
    const uint32_t *turns, *seats, *first_action, *players, *choices;
    int32_t *entry_status;
    uint32_t n_rollouts, max_turns;
    uint64_t seed;
    ge_rollout_stats *out;
    int act;
    const uint32_t *baseline = nullptr, *subjects = nullptr;
    ge_compare_stats *cmp = nullptr;
    bool weighted = false;                                    // ge_batch_rollout_beliefs: act 2 or 3 under `beliefs` (POLICY.md §3j)
    const uint8_t *beliefs = nullptr;                         // n x GE_BELIEF_SLOTS
};

// one chunk's staging: the upload [rooms u64 x cn][keys u64 x cn][turns u32 x cn]; with actions [first u32 x (cn + 1)]
// [players u32 x na][choices u32 x na], with seats [seats u32 x cn]; each array from a 16 B boundary.  Then the download:
// [status i32 x cn] (with actions), the accumulators 8 B x ROLL_STRIDE x cn.  A comparing call (act 3) uploads [subjects u32 x cn]
// [baseline u32 x cn] (sorted positions) behind the seats and downloads [ge_compare_stats x cn] behind the accumulators; its
// outcome plane lies behind `total` on the device only (dev_total), so the pinned host buffer does not grow by it.  A weighted call
// uploads [beliefs 16 B x cn] behind those, in front of the status words
struct RollStage {
    size_t keys, turns, first, players, choices, seats, status, acc, total;
    size_t subjects, baseline, cmp, plane, dev_total;
    size_t beliefs;
};

// ge_compare.inl: the paired sums of a comparing call's chunk staged at dev, behind its playouts on stream s
static hipError_t compare_launch(hipStream_t s, char *dev, const RollStage &o, uint32_t cn, uint32_t n_rollouts, uint32_t waves);

// the arguments of form ACT for segment g's entries [lo, lo + cnt) of the chunk staged at dev
template <int ACT> RollArgs<ACT> rollout_form_args(const RolloutArgs &base, char *dev, const RollStage &o, uint32_t lo) {
    RollArgs<ACT> a;
    static_cast<RolloutArgs &>(a) = base;
    if constexpr (ACT >= 1) {
        a.first_action = reinterpret_cast<const uint32_t *>(dev + o.first) + lo;
        a.players = reinterpret_cast<const uint32_t *>(dev + o.players);
        a.choices = reinterpret_cast<const uint32_t *>(dev + o.choices);
        a.status = reinterpret_cast<int32_t *>(dev + o.status) + lo;
    }
    if constexpr (ACT >= 2) a.seats = reinterpret_cast<const uint32_t *>(dev + o.seats) + lo;
    if constexpr (roll_keeps(ACT)) {
        a.subjects = reinterpret_cast<const uint32_t *>(dev + o.subjects) + lo;
        a.plane = reinterpret_cast<unsigned char *>(dev + o.plane) + (size_t)lo * ((size_t)base.waves * 64u);
    }
    if constexpr (roll_weighted(ACT)) a.beliefs = reinterpret_cast<const u32x4 *>(dev + o.beliefs) + lo;
    return a;
}

// a.n entries the host has counted, one block per (entry, 64 replicas)
template <int ACT> hipError_t rollout_launch_counted(const ge_batch *b, hipStream_t s, const RollArgs<ACT> &a) {
    const dim3 grid(a.n * a.waves);                         // <= 2^26 blocks (n * R <= 2^26)
    const uint32_t kind = b->segs[a.seg].dev.kind;
    return b->plan.generic ? rollout_launch<1, ACT>(kind, grid, s, b, a) : rollout_launch<0, ACT>(kind, grid, s, b, a);
}

// segment g's entries [lo, lo + cnt) of the chunk staged at dev, as form ACT
template <int ACT>
hipError_t rollout_launch_form(const ge_batch *b, hipStream_t s, const RolloutArgs &base, char *dev, const RollStage &o, uint32_t lo) {
    return rollout_launch_counted(b, s, rollout_form_args<ACT>(base, dev, o, lo));
}

// an entry's accumulator words as its ge_rollout_stats; turn_end = its first turn + max_turns
static void rollout_stats_from(const unsigned long long *h, uint32_t n_rollouts, uint64_t turn_end, ge_rollout_stats &out) {
    memset(&out, 0, sizeof out);
    out.summary.rooms = n_rollouts;
    out.summary.finished = h[0]; out.summary.village_wins = h[1]; out.summary.wolf_wins = h[2]; out.summary.alive_players = h[3];
    out.summary.sum_end_turn = h[4];
    for (int j = 0; j < 16; j++) { out.summary.end_turn_hist[j] = h[5 + j]; out.summary.score_hist[j] = h[21 + j]; }
    out.summary.checksum = h[37];
    out.summary.turn = turn_end;
    out.summary.games_recycled = h[38];
    for (int j = 0; j < 12; j++) { out.seat_alive[j] = h[39 + j]; out.seat_wins[j] = h[51 + j]; out.seat_score[j] = h[63 + j]; }
}

static int rollout_rooms_impl(ge_batch *b, const RollRequest &r) {
    GE_ON_DEVICE(b);
    int st = sync_impl(b);
    if (st != GE_OK) return st;
    const bool act = r.act >= 1, view = r.act >= 2, cmp = r.act == 3;
    const uint32_t n_seg = (uint32_t)b->segs.size();
    const uint32_t waves = (r.n_rollouts + 63u) / 64u;
    const uint32_t seed_k = seed_key((uint32_t)r.seed, (uint32_t)(r.seed >> 32));
    std::vector<uint32_t> settle(n_seg);
    for (uint32_t g = 0; g < n_seg; g++) settle[g] = rollout_settle_mask(b->segs[g]);
    int first_bad = GE_OK;                                  // with actions: the status of the first refused entry
    // entries in chunks (bounded staging and accumulator memory); within a chunk grouped by segment (PoolEntries), one launch
    // per segment present (a wavefront never mixes layouts)
    const uint64_t CHUNK = 65536;
    for (uint64_t c0 = 0; c0 < r.n; c0 += CHUNK) {
        const uint32_t cn = (uint32_t)std::min<uint64_t>(CHUNK, r.n - c0);
        const PoolEntries en(b, cn, r.rooms + c0);
        const std::vector<uint32_t> &order = en.order;
        const uint32_t na = r.first_action ? r.first_action[c0 + cn] - r.first_action[c0] : 0u;
        RollStage o;
        o.keys = 8 * (size_t)cn; o.turns = 16 * (size_t)cn;
        o.first = up16(o.turns + 4 * (size_t)cn); o.players = up16(o.first + (act ? 4 * ((size_t)cn + 1u) : 0u));
        o.choices = up16(o.players + 4 * (size_t)na); o.seats = up16(o.choices + 4 * (size_t)na);
        o.subjects = up16(o.seats + (view ? 4 * (size_t)cn : 0u));
        o.baseline = up16(o.subjects + (cmp ? 4 * (size_t)cn : 0u));
        o.beliefs = up16(o.baseline + (cmp ? 4 * (size_t)cn : 0u));
        o.status = up16(o.beliefs + (r.weighted ? (size_t)GE_BELIEF_SLOTS * cn : 0u));
        o.acc = act ? up16(o.status + 4 * (size_t)cn) : o.first;
        const size_t acc_bytes = 8 * (size_t)ROLL_STRIDE * cn;
        o.cmp = o.acc + acc_bytes;
        o.total = o.cmp + (cmp ? sizeof(ge_compare_stats) * (size_t)cn : 0u);
        o.plane = (o.total + 255u) & ~(size_t)255u;
        o.dev_total = cmp ? o.plane + (size_t)cn * waves * 64u : o.total;
        uint32_t *host32 = nullptr;
        if ((st = io_stage(b, o.total, &host32)) != GE_OK) return st;
        unsigned char *host = reinterpret_cast<unsigned char *>(host32);
        en.stage(b, r.rooms + c0, r.keys + c0, r.turns + c0, host, o.keys, o.turns);
        if (act) {                                            // the actions in the sorted order, offsets from the chunk's first
            uint32_t *h_first = reinterpret_cast<uint32_t *>(host + o.first), *h_pl = reinterpret_cast<uint32_t *>(host + o.players);
            uint32_t *h_ch = reinterpret_cast<uint32_t *>(host + o.choices);
            uint32_t at = 0;
            for (uint32_t i = 0; i < cn; i++) {
                const uint64_t k = c0 + order[i];
                h_first[i] = at;
                if (!r.first_action) continue;
                for (uint32_t x = r.first_action[k]; x < r.first_action[k + 1]; x++, at++) { h_pl[at] = r.players[x]; h_ch[at] = r.choices[x]; }
            }
            h_first[cn] = at;
            if (view) {
                uint32_t *h_seat = reinterpret_cast<uint32_t *>(host + o.seats);
                for (uint32_t i = 0; i < cn; i++) h_seat[i] = r.seats[c0 + order[i]];
            }
            if (cmp) {                                        // the baselines follow the sort: input index -> sorted position
                uint32_t *h_subj = reinterpret_cast<uint32_t *>(host + o.subjects), *h_base = reinterpret_cast<uint32_t *>(host + o.baseline);
                std::vector<uint32_t> pos(cn);
                for (uint32_t i = 0; i < cn; i++) pos[order[i]] = i;
                for (uint32_t i = 0; i < cn; i++) { h_subj[i] = r.subjects[c0 + order[i]]; h_base[i] = pos[r.baseline[c0 + order[i]]]; }
            }
            if (r.weighted)
                for (uint32_t i = 0; i < cn; i++)
                    memcpy(host + o.beliefs + (size_t)GE_BELIEF_SLOTS * i, r.beliefs + (size_t)GE_BELIEF_SLOTS * (c0 + order[i]), GE_BELIEF_SLOTS);
            memset(host + o.status, 0, 4 * (size_t)cn);         // GE_OK unless the device refuses the entry
        }
        char *dev = nullptr;
        if ((st = pool_scratch(b, o.dev_total, &dev)) != GE_OK) return st;
        hipStream_t s = b->last_stream;
        if ((st = order_after_previous(b, s)) != GE_OK) return st;
        HIP_TRY(hipMemcpyAsync(dev, host, o.acc, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(dev + o.acc, 0, acc_bytes, s));
        for (uint32_t g = 0; g < n_seg; g++) {
            const uint32_t lo = en.begin[g], cnt = en.begin[g + 1u] - lo;
            if (!cnt) continue;
            RolloutArgs a;
            a.rooms = reinterpret_cast<const uint64_t *>(dev) + lo;
            a.keys = reinterpret_cast<const uint64_t *>(dev + o.keys) + lo;
            a.turns = reinterpret_cast<const uint32_t *>(dev + o.turns) + lo;
            a.acc = reinterpret_cast<unsigned long long *>(dev + o.acc) + (size_t)ROLL_STRIDE * lo;
            a.n = cnt; a.seg = g; a.seed_key = seed_k; a.n_rollouts = r.n_rollouts; a.max_turns = r.max_turns; a.waves = waves;
            a.settle_mask = settle[g];
            HIP_TRY((r.act == 0 ? rollout_launch_form<0>(b, s, a, dev, o, lo)
                     : r.weighted ? (cmp ? rollout_launch_form<7>(b, s, a, dev, o, lo) : rollout_launch_form<6>(b, s, a, dev, o, lo))
                     : cmp      ? rollout_launch_form<3>(b, s, a, dev, o, lo)
                     : view     ? rollout_launch_form<2>(b, s, a, dev, o, lo)
                                : rollout_launch_form<1>(b, s, a, dev, o, lo)));
        }
        if (cmp) HIP_TRY(compare_launch(s, dev, o, cn, r.n_rollouts, waves));   // behind every segment's playouts, over the whole chunk
        const size_t off_down = act ? o.status : o.acc;
        const int32_t *h_st = reinterpret_cast<const int32_t *>(host + o.status);
        const unsigned long long *h_acc = reinterpret_cast<const unsigned long long *>(host + o.acc);
        HIP_TRY(hipMemcpyAsync(host + off_down, dev + off_down, o.total - off_down, hipMemcpyDeviceToHost, s));
        if ((st = sync_impl(b)) != GE_OK) return st;
        if (act) {                                            // verdicts in input order: the first refused entry decides the result
            std::vector<int32_t> v(cn);
            for (uint32_t i = 0; i < cn; i++) v[order[i]] = h_st[i];
            for (uint32_t k = 0; k < cn; k++) {
                if (r.entry_status) r.entry_status[c0 + k] = v[k];
                if (v[k] != GE_OK && first_bad == GE_OK) first_bad = v[k];
            }
        }
        for (uint32_t i = 0; i < cn; i++) {                      // scattered back into input order
            const uint64_t k = c0 + order[i];
            if (cmp) memcpy(&r.cmp[k], host + o.cmp + sizeof(ge_compare_stats) * (size_t)i, sizeof(ge_compare_stats));
            if (act && h_st[i] != GE_OK) continue;               // a refused entry's record is left as it is
            rollout_stats_from(h_acc + (size_t)ROLL_STRIDE * i, r.n_rollouts, (uint64_t)r.turns[k] + r.max_turns, r.out[k]);
        }
    }
    return first_bad;
}

// the three entry points: structural checks, all before anything runs (on an error *out and entry_status are untouched), then
// the playouts; legality is the device's.  The order of the checks is part of the ABI's behaviour: pointers, caps and the action
// offsets (GE_ERR_ARG), then rooms and turns (GE_ERR_RANGE), then the seats (GE_ERR_ARG, after the rooms: a seat's bound is its
// room's segment)
static int rollout_call(ge_batch *b, const RollRequest &r) {
    if (!b) return GE_ERR_ARG;
    if (r.n == 0) return GE_OK;
    const uint64_t n = r.n;
    if (!r.rooms || !r.keys || !r.turns || !r.out) return GE_ERR_ARG;
    if ((r.act == 1 && !r.first_action) || (r.act >= 2 && !r.seats) || (r.first_action && (!r.players || !r.choices))) return GE_ERR_ARG;
    if (r.n_rollouts == 0 || r.n_rollouts > (1u << 20) || n > (1ull << 26) || n * (uint64_t)r.n_rollouts > (1ull << 26) || r.max_turns > 4096u)
        return GE_ERR_ARG;
    if (r.first_action) {
        if (r.first_action[0] != 0) return GE_ERR_ARG;
        for (uint64_t k = 0; k < n; k++)
            if (r.first_action[k + 1] < r.first_action[k] || r.first_action[k + 1] - r.first_action[k] > GE_MAX_PLAYERS) return GE_ERR_ARG;
    }
    for (uint64_t k = 0; k < n; k++)
        if (r.rooms[k] >= b->n_rooms || (uint64_t)r.turns[k] + r.max_turns > 0xFFFFFFFFull) return GE_ERR_RANGE;
    if (r.seats)
        for (uint64_t k = 0; k < n; k++)                      // (rooms[k] is in range: its segment is known)
            if (r.seats[k] > b->segs[pool_segment_of(b, r.rooms[k])].dev.n_players) return GE_ERR_ARG;
    if (r.weighted) {                                         // ge_batch_rollout_beliefs's own, behind ge_batch_rollout_seats's
        if (!r.beliefs) return GE_ERR_ARG;
        for (uint64_t k = 0; k < n; k++) {                    // a byte past the room's slots is a wrong stride, not a belief
            const SegDev &sd = b->segs[pool_segment_of(b, r.rooms[k])].dev;
            const uint32_t slots = (sd.kind == K_WW8 || sd.kind == K_WW12) ? sd.n_players : 3u;
            for (uint32_t c = slots; c < GE_BELIEF_SLOTS; c++)
                if (r.beliefs[(size_t)GE_BELIEF_SLOTS * k + c]) return GE_ERR_ARG;
        }
    }
    if (r.act == 3) {                                         // ge_batch_rollout_compare's own, behind ge_batch_rollout_seats's
        if (!r.baseline || !r.subjects || !r.cmp || n > 65536u) return GE_ERR_ARG;   // one staging chunk: an entry and its baseline are resident together
        for (uint64_t k = 0; k < n; k++)
            if (r.baseline[k] >= n) return GE_ERR_ARG;
        for (uint64_t k = 0; k < n; k++)
            if (r.rooms[r.baseline[k]] != r.rooms[k]) return GE_ERR_ARG;
        for (uint64_t k = 0; k < n; k++)
            if (r.subjects[k] == 0u || r.subjects[k] > b->segs[pool_segment_of(b, r.rooms[k])].dev.n_players) return GE_ERR_ARG;
        // a row of the outcome plane holds one byte per replica, the outcome for the row's own subject: an entry is compared with
        // its baseline's row, so both must name the same seat (until this check the sums of such an entry mixed two seats' outcomes)
        for (uint64_t k = 0; k < n; k++)
            if (r.subjects[r.baseline[k]] != r.subjects[k]) return GE_ERR_ARG;
    }
    return guarded([&] { return rollout_rooms_impl(b, r); });
}

extern "C" {

int ge_batch_rollout_rooms(ge_batch *b, uint64_t n, const uint64_t *rooms, const uint64_t *keys, const uint32_t *turns, uint32_t n_rollouts,
                           uint32_t max_turns, uint64_t seed, ge_rollout_stats *out) {
    return rollout_call(b, {n, rooms, keys, turns, nullptr, nullptr, nullptr, nullptr, nullptr, n_rollouts, max_turns, seed, out, 0});
}

int ge_batch_rollout_actions(ge_batch *b, uint64_t n, const uint64_t *rooms, const uint64_t *keys, const uint32_t *turns,
                             const uint32_t *first_action, const uint32_t *player_ids, const uint32_t *choices, int32_t *entry_status,
                             uint32_t n_rollouts, uint32_t max_turns, uint64_t seed, ge_rollout_stats *out) {
    return rollout_call(b, {n, rooms, keys, turns, nullptr, first_action, player_ids, choices, entry_status, n_rollouts, max_turns, seed, out, 1});
}

int ge_batch_rollout_seats(ge_batch *b, uint64_t n, const uint64_t *rooms, const uint64_t *keys, const uint32_t *turns, const uint32_t *seats,
                           const uint32_t *first_action, const uint32_t *player_ids, const uint32_t *choices, int32_t *entry_status,
                           uint32_t n_rollouts, uint32_t max_turns, uint64_t seed, ge_rollout_stats *out) {
    return rollout_call(b, {n, rooms, keys, turns, seats, first_action, player_ids, choices, entry_status, n_rollouts, max_turns, seed, out, 2});
}

}  // extern "C"

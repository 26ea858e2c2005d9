// ge_playout.inl — playout seats (ge_batch_step_rooms_playout, POLICY.md §3d): ge_batch_step_rooms with some bot seats choosing
// their action by their own seat-view playouts (included at the end of ge_step.hip, behind ge_rollout.inl: the existing kernels
// keep their code-object offsets).  The entry checks, the grouping and staging of the listed rooms, the turn launch (step 4) and
// the event decoding are ge_pool.inl's (pool_check_entries, PoolEntries, launch_pool_turn, pool_decode_event); the playouts are
// ge_rollout.inl's.  What this file adds is the plan and decide kernels - one body each over PlayoutGame - and the playout pass:
// the units and passes, the pass's entry block, the arguments of its kernels and the playing of a unit (PassEntries .. play_unit),
// which ge_run_playout.inl uses as they are and ge_advise.inl in part.
//
// Per listed room, on the device, with no room record crossing to the host:
//   1. ge_playout_plan: one lane per room.  It unpacks the record and finds the seats of its playout mask that decide in this
//      turn (a due bot of §1 step 1 with at least 2 candidates; none at all in a restart-terminal or phase-0-guard turn).  A
//      seat is a target exactly when ge_batch_inject_actions would accept an action of it (inject_ww / inject_tt on a copy of
//      the record: the same condition, liveness and "not yet acted" tests).  Each (seat, candidate) becomes one entry of
//      ge_batch_rollout_seats in the form RollArgs<2> reads; a room takes a contiguous run of entries from its unit's atomic
//      counter, seat-major and candidates ascending.
//   2. The host reads the units' entry counts back (4 bytes each) and launches ge_rollout_kernel<.., ACT = 2> on the
//      device-resident entries through rollout_launch_form: the playout kernel is ge_batch_rollout_seats's own, unchanged.
//   3. ge_playout_decide: one lane per room.  Per deciding seat, the argmax of seat_wins over its entries with the tie-break
//      pick(d, m) (d = the seat's draw of this turn); the chosen actions are logged by inject_ww / inject_tt and the record is
//      stored as ge_inject_kernel stores it.
//   4. ge_pool_kernel plays the turn exactly as ge_batch_step_rooms launches it: the injected seats have acted, so the policy
//      skips them; the host ORs them into the turn's events.
// A room's entries depend only on its own record, keys and turn, never on where the atomic counter put them, so the result is
// deterministic.
//
// Under GE_PLAYOUT_HALVING (POLICY.md §3h) step 2 becomes rounds: each entry carries a replica range (8 bytes), the plan writes
// round 0's, ge_rollout_kernel<.., ACT = 4> plays the ranges into accumulators that are zeroed once and add up across the rounds,
// and between two rounds ge_playout_halve cuts each seat's entries to the better half and hands the survivors their next range.
// Steps 1, 3 and 4 are the same code; without the flag the launches are the ones above.

namespace {

struct PlanArgs {
    const uint64_t *rooms, *keys, *pkeys;   // this unit's listed rooms (segment-local), their turn keys and playout keys
    const uint32_t *turns, *masks;
    uint32_t *room_first, *room_cnt;        // per listed room: its entries [first, first + cnt) of the pass
    uint32_t *counter;                      // the unit's entry counter (zeroed by the host)
    uint64_t *e_rooms, *e_keys;             // the pass's entries (RollArgs<2>'s arrays)
    uint32_t *e_turns, *e_seats, *e_first, *e_players, *e_choices;
    int32_t *e_status;
    uint32_t n, seg, seed_key, restart, full_view, e_base;   // e_base: the unit's first entry in the pass
};

struct DecideArgs {
    const uint64_t *rooms, *keys;
    const uint32_t *turns, *room_first, *room_cnt;
    const uint32_t *e_players, *e_choices;
    const unsigned long long *acc;          // the pass's accumulators, ROLL_STRIDE words per entry
    u32x4 *out;                             // per listed room: decided mask, choice nibbles (low, high)
    uint32_t n, seg, seed_key;
};

// ---- sequential halving (POLICY.md §3h): rounds of a seat with c >= 2 candidates, and the replica offset o_j of n playouts
__host__ __device__ inline uint32_t halving_rounds(uint32_t c) { return 32u - (uint32_t)__builtin_clz(c - 1u); }
__host__ __device__ inline uint32_t halving_offset(uint32_t n, uint32_t R, uint32_t j) { return n * ((1u << j) - 1u) / ((1u << R) - 1u); }   // n <= 2^20, factor <= 15

// what the ranged plan and ge_playout_halve add to a pass: the entries' replica ranges
struct HalveArgs {
    const uint32_t *room_first, *room_cnt;  // this unit's listed rooms: their entries of the pass
    const uint32_t *e_players;
    const unsigned long long *acc;
    u32x2 *e_range;                         // per entry [lo, hi) of the coming round; lo > hi: eliminated
    uint32_t n, n_rollouts, round;          // round: the one that has just been played
};

// the policy's candidate set of seat i (0-based) in a Werewolf phase of action kind `act` (POLICY.md §3 table; ww_choose's)
template <int NB> __device__ __forceinline__ uint32_t playout_cand_ww(const WW<NB> &s, uint32_t act, uint32_t i) {
    const uint32_t me = 1u << i, alive = s.alive, team_w = s.team_w;
    const uint32_t others = alive & ~me, non_wolf = alive & ~team_w, fresh = others & ~(s.det_v | s.det_w);
    const uint32_t r_det = s.rb2 & ~s.rb1 & ~s.rb0;          // role class Detective
    const uint32_t kw = s.det_w & alive, lo_kw = kw & (0u - kw);
    uint32_t cand = alive;                                    // ACT_DOCTOR_PROTECT
    if (act == ACT_WOLF_TARGET) cand = non_wolf;
    else if (act == ACT_DETECTIVE) cand = fresh ? fresh : others;
    else if (act == ACT_DAY_VOTE) cand = (team_w & me) ? non_wolf : (((r_det & me) && lo_kw) ? lo_kw : others);
    return cand ? cand : alive;
}

// Two-Truths: statement 1 in a statements phase, else 1..3 (as bits 0..2)
__device__ __forceinline__ uint32_t playout_cand_tt(uint32_t act) { return act == ACT_TT_STATEMENTS ? 1u : 7u; }

// what the two games' rooms differ in here: the record, the candidate set of seat i and the injection
template <int NB, bool WWP> struct PlayoutGame;
template <int NB> struct PlayoutGame<NB, true> {
    using S = WW<NB>;
    using L = WWLayout<NB>;
    static __device__ __forceinline__ uint32_t cand(const S &s, uint32_t act, uint32_t i) { return playout_cand_ww<NB>(s, act, i); }
    static __device__ __forceinline__ int inject(S &s, const DevRow &row, const DevCond &cond, uint32_t n, uint32_t p, uint32_t c) {
        return inject_ww<NB>(s, row, cond, n, p, c);
    }
};
template <int NB> struct PlayoutGame<NB, false> {
    using S = TT<NB>;
    using L = TTLayout<NB>;
    static __device__ __forceinline__ uint32_t cand(const S &, uint32_t act, uint32_t) { return playout_cand_tt(act); }
    static __device__ __forceinline__ int inject(S &s, const DevRow &row, const DevCond &cond, uint32_t n, uint32_t p, uint32_t c) {
        return inject_tt<NB>(s, row, cond, n, p, c);
    }
};

// the seats of `mask` that decide in this turn, and the number of entries they need
template <class G>
__device__ __forceinline__ uint32_t playout_deciders(const typename G::S &s, const DevRow &row, const DevCond &cond, uint32_t n, uint32_t mask, uint32_t tk,
                                                     uint32_t &n_entries) {
    const uint32_t act = (row.r0 >> 2) & 7u;
    uint32_t dec = 0, cnt = 0;
    for (uint32_t m = mask; m; m &= m - 1u) {
        const uint32_t i = ctz(m);
        if ((draw(tk, i) & 3u) == 0u) continue;              // not due in this turn
        const uint32_t cand = G::cand(s, act, i);
        typename G::S t = s;                                  // a target exactly when an injected action would be accepted
        const int st = cand ? G::inject(t, row, cond, n, i + 1u, ctz(cand) + 1u) : GE_ERR_ARG;
        if (st != GE_OK || popc(cand) < 2u) continue;
        dec |= 1u << i;
        cnt += popc(cand);
    }
    n_entries = cnt;
    return dec;
}

// HALVE: each entry also gets round 0's replica range [0, o_1) of its seat's candidate count (§3h)
template <int NB, bool WWP, bool HALVE = false>
__device__ __forceinline__ void playout_plan_room(const SegDev &sg, const DevTable *__restrict__ tables, const PlanArgs &a, uint32_t k,
                                                  u32x2 *e_range = nullptr, uint32_t n_rollouts = 0u) {
    using G = PlayoutGame<NB, WWP>;
    using L = typename G::L;
    const uint64_t room = a.rooms[k];
    const uint32_t turn = a.turns[k];
    const uint32_t tk = turn_key(room_key_from(a.seed_key, a.keys[k]), turn);
    uint32_t dec = 0, cnt = 0;
    uint32_t w[12];
    load_words<L::WORDS>(sg.base, sg.rooms_padded, room, w);
    typename G::S s;
    L::unpack(w, s);
    const DevRow &row = tables[sg.table_idx].rows[s.phase];
    const uint32_t act = (row.r0 >> 2) & 7u;
    const bool skip = (a.restart && ((sg.term_mask >> s.phase) & 1u)) || (s.phase == sg.phase0_idx && !(s.flags & FLAG_PHASE0_DONE));
    if (!skip) dec = playout_deciders<G>(s, row, tables[sg.table_idx].conds[s.phase], sg.n_players, a.masks[k], tk, cnt);
    uint32_t first = cnt ? atomicAdd(a.counter, cnt) + a.e_base : 0u;
    a.room_first[k] = first;
    a.room_cnt[k] = cnt;
    for (uint32_t m = dec; m; m &= m - 1u) {
        const uint32_t i = ctz(m);
        u32x2 rg; rg.x = 0u; rg.y = 0u;
        if constexpr (HALVE) rg.y = halving_offset(n_rollouts, halving_rounds(popc(G::cand(s, act, i))), 1u);
        for (uint32_t c = G::cand(s, act, i); c; c &= c - 1u, first++) {
            if constexpr (HALVE) e_range[first] = rg;
            a.e_rooms[first] = room; a.e_keys[first] = a.pkeys[k]; a.e_turns[first] = turn;
            a.e_seats[first] = a.full_view ? 0u : i + 1u;
            a.e_first[first] = first; a.e_first[first + 1u] = first + 1u;
            a.e_players[first] = i + 1u; a.e_choices[first] = ctz(c) + 1u;
            a.e_status[first] = GE_OK;
        }
    }
}

template <int KIND>
__global__ void __launch_bounds__(64) ge_playout_plan(const SegDev *__restrict__ segs, const DevTable *__restrict__ tables, const PlanArgs a) {
    const uint32_t k = blockIdx.x * 64u + threadIdx.x;
    if (k >= a.n) return;
    const SegDev &sg = segs[a.seg];
    playout_plan_room<KindOf<KIND>::NB, KindOf<KIND>::WW>(sg, tables, a, k);
}

template <int KIND>
__global__ void __launch_bounds__(64) ge_playout_plan_ranged(const SegDev *__restrict__ segs, const DevTable *__restrict__ tables, const PlanArgs a,
                                                             u32x2 *e_range, uint32_t n_rollouts) {
    const uint32_t k = blockIdx.x * 64u + threadIdx.x;
    if (k >= a.n) return;
    const SegDev &sg = segs[a.seg];
    playout_plan_room<KindOf<KIND>::NB, KindOf<KIND>::WW, true>(sg, tables, a, k, e_range, n_rollouts);
}

// Between two rounds of §3h: one lane per listed room, whatever its game - only entry arrays and accumulators are read.  Per seat
// (its entries are consecutive, as playout_choose walks them) with c candidates and R rounds: when round + 1 < R, a live entry
// survives iff fewer than k = ceil(c / 2^(round + 1)) live entries of the seat have a strictly larger V (ties at the cut all
// stay), and the survivors get the next round's range; a seat whose rounds are done gets the empty range [n, n).  An eliminated
// entry gets (0xFFFFFFFF, 0): lo > hi, which no live entry has, even when its round is empty (lo == hi).
__global__ void __launch_bounds__(64) ge_playout_halve(const HalveArgs a) {
    const uint32_t k = blockIdx.x * 64u + threadIdx.x;
    if (k >= a.n) return;
    const uint32_t lo = a.room_first[k], hi = lo + a.room_cnt[k];
    for (uint32_t f = lo; f < hi;) {
        const uint32_t seat = a.e_players[f];
        uint32_t g = f + 1u;
        while (g < hi && a.e_players[g] == seat) g++;
        const uint32_t c = g - f, R = halving_rounds(c), j1 = a.round + 1u;   // c <= 12 entries [f, g) of this seat
        const bool cut = j1 < R;
        const uint32_t keep = cut ? (c + (1u << j1) - 1u) >> j1 : c;
        u32x2 next, out;
        next.x = cut ? halving_offset(a.n_rollouts, R, j1) : a.n_rollouts;
        next.y = cut ? halving_offset(a.n_rollouts, R, j1 + 1u) : a.n_rollouts;
        out.x = 0xFFFFFFFFu; out.y = 0u;
        uint32_t live = 0, stay = 0;                           // bit x - f
        for (uint32_t x = f; x < g; x++) {
            const u32x2 r = a.e_range[x];
            live |= (r.x <= r.y ? 1u : 0u) << (x - f);
        }
        for (uint32_t x = f; x < g; x++) {
            const unsigned long long v = a.acc[(size_t)x * ROLL_STRIDE + 51u + (seat - 1u)];
            uint32_t above = 0;
            for (uint32_t y = f; y < g; y++)
                above += ((live >> (y - f)) & 1u) && a.acc[(size_t)y * ROLL_STRIDE + 51u + (seat - 1u)] > v ? 1u : 0u;
            stay |= (above < keep ? 1u : 0u) << (x - f);
        }
        stay &= live;
        for (uint32_t x = f; x < g; x++) a.e_range[x] = ((stay >> (x - f)) & 1u) ? next : out;
        f = g;
    }
}

// per deciding seat of room k: argmax of seat_wins with the pick(d, m) tie-break, logged in `s` by `inject`
template <class INJ>
__device__ __forceinline__ void playout_choose(const DecideArgs &a, uint32_t k, uint32_t tk, INJ &&inject) {
    const uint32_t lo = a.room_first[k], hi = lo + a.room_cnt[k];
    uint32_t cur = 0, tie = 0, decided = 0;
    uint64_t nib = 0;
    unsigned long long best = 0;
    for (uint32_t j = lo;; j++) {
        const bool end = j == hi;
        const uint32_t seat = end ? 0u : a.e_players[j];
        if (cur != 0u && seat != cur) {                       // seat cur's entries are complete
            const uint32_t c = nth_set_bit<16>(tie, pick(draw(tk, cur - 1u), popc(tie))) + 1u;
            if (inject(cur, c) == GE_OK) {                    // (always: the candidates are the policy's own)
                decided |= 1u << (cur - 1u);
                nib |= (uint64_t)c << (4u * (cur - 1u));
            }
        }
        if (end) break;
        const uint32_t c = a.e_choices[j];
        const unsigned long long v = a.acc[(size_t)j * ROLL_STRIDE + 51u + (seat - 1u)];   // seat_wins[seat - 1]
        if (seat != cur || v > best) { cur = seat; best = v; tie = 1u << (c - 1u); }
        else if (v == best) tie |= 1u << (c - 1u);
    }
    u32x4 o;
    o.x = decided; o.y = (uint32_t)nib; o.z = (uint32_t)(nib >> 32); o.w = 0u;
    a.out[k] = o;
}

template <int NB, bool WWP>
__device__ __forceinline__ void playout_decide_room(const SegDev &sg, const DevTable *__restrict__ tables, const DecideArgs &a, uint32_t k) {
    using G = PlayoutGame<NB, WWP>;
    using L = typename G::L;
    const uint64_t room = a.rooms[k];
    const uint32_t tk = turn_key(room_key_from(a.seed_key, a.keys[k]), a.turns[k]);
    uint32_t w[12];
    load_words<L::WORDS>(sg.base, sg.rooms_padded, room, w);
    typename G::S s;
    L::unpack(w, s);
    const DevRow &row = tables[sg.table_idx].rows[s.phase];
    const DevCond &cond = tables[sg.table_idx].conds[s.phase];   // read in place, as inject_group_ww / inject_group_tt
    playout_choose(a, k, tk, [&](uint32_t p, uint32_t c) { return G::inject(s, row, cond, sg.n_players, p, c); });
    L::pack(s, w);
    store_words<L::WORDS>(sg.base, sg.rooms_padded, room, w);
}

// one lane per listed room of a unit with entries (a room without any stores nothing: its output was zeroed by the host)
template <int KIND>
__global__ void __launch_bounds__(64) ge_playout_decide(const SegDev *__restrict__ segs, const DevTable *__restrict__ tables, const DecideArgs a) {
    const uint32_t k = blockIdx.x * 64u + threadIdx.x;
    if (k >= a.n || a.room_cnt[k] == 0u) return;
    const SegDev &sg = segs[a.seg];
    playout_decide_room<KindOf<KIND>::NB, KindOf<KIND>::WW>(sg, tables, a, k);
}

// most candidates one deciding seat of a segment can have: Werewolf a subset of the n seats, Two-Truths at most statements 1..3
// (a Two-Truths segment may have 2 players).  The entry space and the cost cap reserve this per playout seat.
uint32_t playout_max_cands(const SegDev &d) { return (d.kind == K_WW8 || d.kind == K_WW12) ? d.n_players : std::max(d.n_players, 3u); }

// §3h on the host: the rounds a segment's seats can need, and the wavefronts per entry of round j - the longest range any seat of
// 2 .. max_cands candidates has in that round (0: no seat plays anything in it)
uint32_t halving_max_rounds(const SegDev &d) { return halving_rounds(std::max(playout_max_cands(d), 2u)); }
uint32_t halving_waves(uint32_t n_rollouts, uint32_t max_cands, uint32_t j) {
    uint32_t longest = 0;
    for (uint32_t c = 2; c <= max_cands; c++) {
        const uint32_t R = halving_rounds(c);
        if (j < R) longest = std::max(longest, halving_offset(n_rollouts, R, j + 1u) - halving_offset(n_rollouts, R, j));
    }
    return (longest + 63u) / 64u;
}

hipError_t playout_launch(uint32_t kind, dim3 grid, hipStream_t st, const ge_batch *b, const PlanArgs &a) {
    return by_kind(kind, [&](auto K) { hipLaunchKernelGGL((ge_playout_plan<K()>), grid, dim3(64), 0, st, b->segs_dev, b->tables, a); });
}
hipError_t playout_launch(uint32_t kind, dim3 grid, hipStream_t st, const ge_batch *b, const PlanArgs &a, u32x2 *e_range, uint32_t n_rollouts) {
    return by_kind(kind, [&](auto K) { hipLaunchKernelGGL((ge_playout_plan_ranged<K()>), grid, dim3(64), 0, st, b->segs_dev, b->tables, a, e_range, n_rollouts); });
}
hipError_t playout_launch(dim3 grid, hipStream_t st, const HalveArgs &a) {
    hipLaunchKernelGGL(ge_playout_halve, grid, dim3(64), 0, st, a);
    return hipGetLastError();
}
hipError_t playout_launch(uint32_t kind, dim3 grid, hipStream_t st, const ge_batch *b, const DecideArgs &a) {
    return by_kind(kind, [&](auto K) { hipLaunchKernelGGL((ge_playout_decide<K()>), grid, dim3(64), 0, st, b->segs_dev, b->tables, a); });
}

}  // namespace

// a run of sorted listed rooms of one segment whose entries share one pass's arrays
struct PlayoutUnit {
    uint32_t seg, lo, cnt;          // sorted positions [lo, lo + cnt)
    uint32_t e_base, e_cap;         // its entries within the pass: [e_base, e_base + e_cap) at most
    uint32_t pass;
};

// units: runs of one segment with at most CHUNK entries' room (a room needs popcount(mask) x playout_max_cands at most); passes:
// consecutive units whose room fits in CHUNK entries together.  A pass's entries are planned, played and decided together.
// max_cap: the most entries a pass has room for
static void playout_units(const ge_batch *b, const PoolEntries &en, const uint32_t *masks, std::vector<PlayoutUnit> &units, uint32_t &n_pass,
                          uint32_t &max_cap) {
    const uint32_t n_seg = (uint32_t)b->segs.size();
    const std::vector<uint32_t> &begin = en.begin, &order = en.order;
    const uint32_t CHUNK = 65536;
    uint32_t pass_cap = 0;
    n_pass = 0; max_cap = 0;
    for (uint32_t g = 0; g < n_seg; g++) {
        const uint32_t np = playout_max_cands(b->segs[g].dev);
        for (uint32_t i = begin[g]; i < begin[g + 1u]; i++) {
            const uint32_t cap = (uint32_t)__builtin_popcount(masks[order[i]]) * np;
            if (!cap) continue;                               // no playout seat: only the turn (step 4)
            const bool fresh = units.empty() || units.back().seg != g || units.back().lo + units.back().cnt != i || units.back().e_cap + cap > CHUNK;
            if (fresh) {
                if (units.empty() || pass_cap + cap > CHUNK) { n_pass++; pass_cap = 0; }
                units.push_back(PlayoutUnit{g, i, 0u, pass_cap, 0u, n_pass - 1u});
            }
            units.back().cnt++;
            units.back().e_cap += cap;
            pass_cap += cap;
            max_cap = std::max(max_cap, pass_cap);
        }
    }
}

// ---- the playout pass: what ge_batch_step_rooms_playout, ge_batch_run_rooms_playout (ge_run_playout.inl) and
// ge_batch_advise_seats (ge_advise.inl) share.  Each call lays out its own upload and download arrays; these are the same bytes
// and the same launches in all of them.

// The entries of a pass, device only: C entries from byte `at` of the call's scratch, each array from a 16 B boundary -
// [rooms u64][keys u64][turns u32][seats u32][first u32 (+1)][players u32][choices u32][status i32][acc 8 B x ROLL_STRIDE] and,
// `ranged` (GE_PLAYOUT_HALVING), [replica range 8 B].  o: the arrays rollout_form_args reads (a unit's rooms, keys and turns go
// through its RolloutArgs, so o.keys and o.turns are not used); o.total: the end of the block, the scratch the call needs
struct PassEntries {
    size_t rooms, keys, turns, range;
    RollStage o;
    PassEntries(size_t at, size_t C, bool ranged) : rooms(at), keys(rooms + 8 * C), turns(keys + 8 * C) {
        o.keys = o.turns = 0;
        o.seats = up16(turns + 4 * C);
        o.first = up16(o.seats + 4 * C);
        o.players = up16(o.first + 4 * (C + 1u));
        o.choices = up16(o.players + 4 * C);
        o.status = up16(o.choices + 4 * C);
        o.acc = up16(o.status + 4 * C);
        range = o.acc + 8 * (size_t)ROLL_STRIDE * C;
        o.total = range + (ranged ? 8 * C : 0u);
    }
};

// the e_* members of a plan's arguments (PlanArgs, AdvisePlanArgs): the pass's entries in the block at dev
template <class A> static void bind_entries(A &a, char *dev, const PassEntries &e) {
    a.e_rooms = reinterpret_cast<uint64_t *>(dev + e.rooms); a.e_keys = reinterpret_cast<uint64_t *>(dev + e.keys);
    a.e_turns = reinterpret_cast<uint32_t *>(dev + e.turns); a.e_seats = reinterpret_cast<uint32_t *>(dev + e.o.seats);
    a.e_first = reinterpret_cast<uint32_t *>(dev + e.o.first); a.e_players = reinterpret_cast<uint32_t *>(dev + e.o.players);
    a.e_choices = reinterpret_cast<uint32_t *>(dev + e.o.choices); a.e_status = reinterpret_cast<int32_t *>(dev + e.o.status);
}

// the playouts of unit u's first n entries: `seed` the playouts' own, one wavefront per 64 playouts (a round of §3h sets its own)
static RolloutArgs unit_rollout_args(const ge_batch *b, char *dev, const PassEntries &e, const PlayoutUnit &u, uint32_t n, uint64_t seed,
                                     uint32_t n_rollouts, uint32_t max_turns) {
    RolloutArgs a;
    a.rooms = reinterpret_cast<const uint64_t *>(dev + e.rooms) + u.e_base;
    a.keys = reinterpret_cast<const uint64_t *>(dev + e.keys) + u.e_base;
    a.turns = reinterpret_cast<const uint32_t *>(dev + e.turns) + u.e_base;
    a.acc = reinterpret_cast<unsigned long long *>(dev + e.o.acc) + (size_t)ROLL_STRIDE * u.e_base;
    a.n = n; a.seg = u.seg; a.seed_key = seed_key((uint32_t)seed, (uint32_t)(seed >> 32));
    a.n_rollouts = n_rollouts; a.max_turns = max_turns; a.waves = (n_rollouts + 63u) / 64u;
    a.settle_mask = rollout_settle_mask(b->segs[u.seg]);
    return a;
}

// the listed rooms of a playout-seat call on the device, over the sorted positions (a unit's are these + u.lo), and the scalars
// every unit shares; the offsets are the call's own layout (rooms at 0)
struct PassRooms {
    const uint64_t *rooms, *keys, *pkeys;
    const uint32_t *turns, *masks;
    uint32_t *room_first, *room_cnt;        // per listed room: its entries [first, first + cnt) of the pass
    uint32_t seed_key, restart, full_view;
};
static PassRooms pass_rooms(const ge_batch *b, char *dev, size_t o_keys, size_t o_pkeys, size_t o_turns, size_t o_masks, size_t o_rfirst, size_t o_rcnt,
                            uint32_t flags) {
    PassRooms r;
    r.rooms = reinterpret_cast<const uint64_t *>(dev);
    r.keys = reinterpret_cast<const uint64_t *>(dev + o_keys);
    r.pkeys = reinterpret_cast<const uint64_t *>(dev + o_pkeys);
    r.turns = reinterpret_cast<const uint32_t *>(dev + o_turns);
    r.masks = reinterpret_cast<const uint32_t *>(dev + o_masks);
    r.room_first = reinterpret_cast<uint32_t *>(dev + o_rfirst);
    r.room_cnt = reinterpret_cast<uint32_t *>(dev + o_rcnt);
    r.seed_key = seed_key((uint32_t)b->seed, (uint32_t)(b->seed >> 32));
    r.restart = (b->flags & GE_FLAG_RESTART) ? 1u : 0u;
    r.full_view = (flags & GE_PLAYOUT_FULL_VIEW) ? 1u : 0u;
    return r;
}

static PlanArgs plan_args(const PassRooms &r, const PlayoutUnit &u, uint32_t *counter, char *dev, const PassEntries &e) {
    PlanArgs a;
    a.rooms = r.rooms + u.lo; a.keys = r.keys + u.lo; a.pkeys = r.pkeys + u.lo;
    a.turns = r.turns + u.lo; a.masks = r.masks + u.lo;
    a.room_first = r.room_first + u.lo; a.room_cnt = r.room_cnt + u.lo;
    a.counter = counter;
    bind_entries(a, dev, e);
    a.n = u.cnt; a.seg = u.seg; a.seed_key = r.seed_key; a.restart = r.restart; a.full_view = r.full_view; a.e_base = u.e_base;
    return a;
}

// out: the unit's first room's 16 bytes (decided mask, choice nibbles)
static DecideArgs decide_args(const PassRooms &r, const PlayoutUnit &u, u32x4 *out, char *dev, const PassEntries &e) {
    DecideArgs a;
    a.rooms = r.rooms + u.lo; a.keys = r.keys + u.lo; a.turns = r.turns + u.lo;
    a.room_first = r.room_first + u.lo; a.room_cnt = r.room_cnt + u.lo;
    a.e_players = reinterpret_cast<const uint32_t *>(dev + e.o.players);
    a.e_choices = reinterpret_cast<const uint32_t *>(dev + e.o.choices);
    a.acc = reinterpret_cast<const unsigned long long *>(dev + e.o.acc);
    a.out = out;
    a.n = u.cnt; a.seg = u.seg; a.seed_key = r.seed_key;
    return a;
}

// Step 2 for one unit: its entries (a = unit_rollout_args) played as form 2 in one launch or, `halving`, in the rounds of §3h -
// form 4 over the entries' replica ranges, the accumulators adding up, ge_playout_halve between two rounds and no cut behind the
// last.  launch(RollArgs<2 | 4>) is the caller's: it knows whether the host has the entry count (rollout_launch_counted) or the
// device reads it (ge_run_playout.inl)
template <class LAUNCH>
static hipError_t play_unit(const ge_batch *b, hipStream_t s, char *dev, const PassEntries &e, const PassRooms &r, const PlayoutUnit &u, RolloutArgs a,
                            bool halving, LAUNCH &&launch) {
    if (!halving) return launch(rollout_form_args<2>(a, dev, e.o, u.e_base));
    const SegDev &sd = b->segs[u.seg].dev;
    const uint32_t r_max = halving_max_rounds(sd);
    HalveArgs h;
    h.room_first = r.room_first + u.lo; h.room_cnt = r.room_cnt + u.lo;
    h.e_players = reinterpret_cast<const uint32_t *>(dev + e.o.players);
    h.acc = reinterpret_cast<const unsigned long long *>(dev + e.o.acc);
    h.e_range = reinterpret_cast<u32x2 *>(dev + e.range);
    h.n = u.cnt; h.n_rollouts = a.n_rollouts;
    for (uint32_t j = 0; j < r_max; j++) {
        hipError_t err = hipSuccess;
        a.waves = halving_waves(a.n_rollouts, playout_max_cands(sd), j);
        if (a.waves) {                                        // (no round is longer than n_rollouts: the grid is within the plain form's)
            RollArgs<4> ra = rollout_form_args<4>(a, dev, e.o, u.e_base);
            ra.range = h.e_range + u.e_base;
            if ((err = launch(ra)) != hipSuccess) return err;
        }
        if (j + 1u == r_max) break;
        h.round = j;
        if ((err = playout_launch(dim3((u.cnt + 63u) / 64u), s, h)) != hipSuccess) return err;
    }
    return hipSuccess;
}

static int step_playout_impl(ge_batch *b, uint64_t n, const uint64_t *rooms, const uint64_t *keys, const uint32_t *turns, const uint32_t *masks,
                             const uint64_t *pkeys, uint32_t n_rollouts, uint32_t max_turns, uint64_t seed, uint32_t flags, ge_turn_event *events,
                             uint32_t *decided) {
    GE_ON_DEVICE(b);
    int st = sync_impl(b);
    if (st != GE_OK) return st;
    const PoolEntries en(b, n, rooms);
    const std::vector<uint32_t> &order = en.order;
    std::vector<PlayoutUnit> units;
    uint32_t n_pass = 0, max_cap = 0;
    playout_units(b, en, masks, units, n_pass, max_cap);
    const uint32_t n_units = (uint32_t)units.size();
    // one scratch layout, each array from a 16 B boundary.  Upload: [rooms u64][keys u64][pkeys u64][turns u32][masks u32]
    // [unit counters u32][per-room outputs 16 B, zeroed].  Then [room_first u32][room_cnt u32][events 16 B]: the pinned buffer ends
    // here.  Behind it, on the device only, the pass's entries
    const size_t N = (size_t)n;
    const size_t o_keys = 8 * N, o_pkeys = 16 * N, o_turns = 24 * N, o_masks = up16(o_turns + 4 * N), o_ctr = up16(o_masks + 4 * N);
    const size_t o_out = up16(o_ctr + 4 * (size_t)n_units), o_up_end = o_out + 16 * N;
    const size_t o_rfirst = o_up_end, o_rcnt = up16(o_rfirst + 4 * N), o_ev = up16(o_rcnt + 4 * N), host_total = o_ev + 16 * N;
    const bool halving = (flags & GE_PLAYOUT_HALVING) != 0u;
    const PassEntries pe(host_total, max_cap, halving);
    uint32_t *host32 = nullptr;
    if ((st = io_stage(b, host_total, &host32)) != GE_OK) return st;
    unsigned char *host = reinterpret_cast<unsigned char *>(host32);
    en.stage(b, rooms, keys, turns, host, o_keys, o_turns);
    uint64_t *h_pkeys = reinterpret_cast<uint64_t *>(host + o_pkeys);
    uint32_t *h_masks = reinterpret_cast<uint32_t *>(host + o_masks);
    for (size_t i = 0; i < N; i++) { h_pkeys[i] = pkeys[order[i]]; h_masks[i] = masks[order[i]]; }
    memset(host + o_ctr, 0, o_up_end - o_ctr);
    char *dev = nullptr;
    if ((st = pool_scratch(b, pe.o.total, &dev)) != GE_OK) return st;
    hipStream_t s = b->last_stream;
    if ((st = order_after_previous(b, s)) != GE_OK) return st;
    HIP_TRY(hipMemcpyAsync(dev, host, o_up_end, hipMemcpyHostToDevice, s));
    const PassRooms pr = pass_rooms(b, dev, o_keys, o_pkeys, o_turns, o_masks, o_rfirst, o_rcnt, flags);
    const uint32_t *h_ctr = reinterpret_cast<const uint32_t *>(host + o_ctr);
    for (uint32_t p = 0; p < n_pass; p++) {
        // 1. plan every unit of the pass
        for (const PlayoutUnit &u : units) {
            if (u.pass != p) continue;
            const PlanArgs a = plan_args(pr, u, reinterpret_cast<uint32_t *>(dev + o_ctr) + (&u - units.data()), dev, pe);
            const dim3 grid((u.cnt + 63u) / 64u);
            HIP_TRY(halving ? playout_launch(b->segs[u.seg].dev.kind, grid, s, b, a, reinterpret_cast<u32x2 *>(dev + pe.range), n_rollouts)
                            : playout_launch(b->segs[u.seg].dev.kind, grid, s, b, a));
        }
        // 2. the entry counts (the one host round trip), then the playouts of each unit
        HIP_TRY(hipMemcpyAsync(host + o_ctr, dev + o_ctr, 4 * (size_t)n_units, hipMemcpyDeviceToHost, s));
        if ((st = sync_impl(b)) != GE_OK) return st;
        if ((st = order_after_previous(b, s)) != GE_OK) return st;
        for (const PlayoutUnit &u : units) {
            const uint32_t cnt = h_ctr[&u - units.data()];
            if (u.pass != p || !cnt) continue;
            HIP_TRY(hipMemsetAsync(dev + pe.o.acc + 8 * (size_t)ROLL_STRIDE * u.e_base, 0, 8 * (size_t)ROLL_STRIDE * cnt, s));
            HIP_TRY(play_unit(b, s, dev, pe, pr, u, unit_rollout_args(b, dev, pe, u, cnt, seed, n_rollouts, max_turns), halving,
                              [&](const auto &ra) { return rollout_launch_counted(b, s, ra); }));
        }
        // 3. decide and log
        for (const PlayoutUnit &u : units) {
            if (u.pass != p || !h_ctr[&u - units.data()]) continue;
            const DecideArgs a = decide_args(pr, u, reinterpret_cast<u32x4 *>(dev + o_out) + u.lo, dev, pe);
            HIP_TRY(playout_launch(b->segs[u.seg].dev.kind, dim3((u.cnt + 63u) / 64u), s, b, a));
        }
    }
    // 4. the turn, as step_rooms_impl launches it
    if ((st = launch_pool_turn(b, s, en, dev, o_keys, o_turns, o_ev)) != GE_OK) return st;
    HIP_TRY(hipMemcpyAsync(host + o_out, dev + o_out, 16 * N, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(host + o_ev, dev + o_ev, 16 * N, hipMemcpyDeviceToHost, s));
    if ((st = sync_impl(b)) != GE_OK) return st;
    const uint32_t *h_out = reinterpret_cast<const uint32_t *>(host + o_out), *h_ev = reinterpret_cast<const uint32_t *>(host + o_ev);
    for (size_t i = 0; i < N; i++) {
        const uint32_t k = order[i];
        const uint32_t dmask = h_out[4 * i];
        const uint64_t dnib = (uint64_t)h_out[4 * i + 1] | ((uint64_t)h_out[4 * i + 2] << 32);
        if (decided) decided[k] = dmask;
        if (!events) continue;
        ge_turn_event &e = events[k];                         // as step_rooms_impl decodes it, with the decided seats acted
        pool_decode_event(h_ev + 4 * i, b->segs[en.seg_of[k]].table, e);
        e.acted_now |= (uint16_t)dmask;
        for (int c = 0; c < 16; c++) e.choice[c] |= (uint8_t)((dnib >> (4 * c)) & 15u);
    }
    return GE_OK;
}

// the playout checks of ge_batch_step_rooms_playout, behind ge_batch_step_rooms's (the rooms are in range): ge_batch_rollout_seats's
// caps, the turn range of the playouts, the masks and the cost cap.  more_turns: the turns a room is played on before its last turn's
// playouts (ge_batch_run_rooms_playout: max_turns - 1); the cost cap is per turn, as only one turn's playouts exist at a time
static int playout_check(const ge_batch *b, uint64_t n, const uint64_t *rooms, const uint32_t *turns, const uint32_t *playout_masks,
                         const uint64_t *playout_keys, uint32_t n_rollouts, uint32_t max_turns, uint32_t flags, uint32_t more_turns) {
    if (!playout_masks || !playout_keys || (flags & ~(GE_PLAYOUT_FULL_VIEW | GE_PLAYOUT_HALVING))) return GE_ERR_ARG;
    if (n_rollouts == 0 || n_rollouts > (1u << 20) || max_turns > 4096u) return GE_ERR_ARG;
    for (uint64_t k = 0; k < n; k++)
        if ((uint64_t)turns[k] + more_turns + max_turns > 0xFFFFFFFFull) return GE_ERR_RANGE;
    uint64_t cost = 0;
    for (uint64_t k = 0; k < n; k++) {
        const SegDev &sg = b->segs[pool_segment_of(b, rooms[k])].dev;
        const uint32_t m = playout_masks[k];
        const uint32_t human = b->seats_host.empty() ? sg.human_mask : (uint32_t)b->seats_host[(size_t)rooms[k]];   // the room's own seats (ge_seats.inl): the mirror decides
        if ((m >> sg.n_players) != 0u || (m & human) != 0u) return GE_ERR_ARG;
        cost += (uint64_t)__builtin_popcount(m) * playout_max_cands(sg) * n_rollouts;
        if (cost > (1ull << 26)) return GE_ERR_ARG;
    }
    return GE_OK;
}

extern "C" {

int ge_batch_step_rooms_playout(ge_batch *b, uint64_t n, const uint64_t *rooms, const uint64_t *keys, const uint32_t *turns,
                                const uint32_t *playout_masks, const uint64_t *playout_keys, uint32_t n_rollouts, uint32_t max_turns,
                                uint64_t seed, uint32_t flags, ge_turn_event *events, uint32_t *decided) {
    if (!b) return GE_ERR_ARG;
    if (n == 0) return GE_OK;
    const int st = pool_check_entries(b, n, rooms, keys, turns);   // ge_batch_step_rooms's checks, in its order
    if (st != GE_OK) return st;
    const int pst = playout_check(b, n, rooms, turns, playout_masks, playout_keys, n_rollouts, max_turns, flags, 0u);
    if (pst != GE_OK) return pst;
    return guarded([&] { return step_playout_impl(b, n, rooms, keys, turns, playout_masks, playout_keys, n_rollouts, max_turns, seed, flags,
                                                  events, decided); });
}

}  // extern "C"

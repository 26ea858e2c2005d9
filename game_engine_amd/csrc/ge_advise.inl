// ge_advise.inl — advice for listed seats (ge_batch_advise_seats, POLICY.md §3m): for each listed (room, seat) the choices the
// seat could make now are found, each is played by ge_batch_rollout_seats's own kernel, and the ranking comes back in 224 bytes
// (included at the end of ge_step.hip, behind ge_seats.inl: the existing kernels keep their code-object offsets).  The grouping
// and staging of the listed entries are ge_pool.inl's (PoolEntries, io_stage, pool_scratch), the units and passes follow
// ge_playout.inl's, which also owns the pass's entry block and a unit's playout arguments (PassEntries, bind_entries,
// unit_rollout_args); the playouts are ge_rollout.inl's.  What this file adds is the plan and reduce kernels.
//
// Per listed entry, on the device, with no room record and no ge_rollout_stats crossing to the host:
//   1. ge_advise_plan: one lane per listed entry.  It unpacks the record and tests every choice c = 1 .. C of the seat with
//      inject_ww / inject_tt on a copy of the record - the code of ge_batch_inject_action, so `legal` is its verdict.  An entry
//      with p = popc(legal) > 0 takes a run of p + 1 entries of ge_batch_rollout_seats in the form RollArgs<2> reads: the legal
//      choices ascending, one action (seat, c) each, then the entry without an action (the policy plays the seat).  The entry
//      without an action needs an empty CSR slice, so a run is p + 1 entries but p actions, contiguous in both: one 64-bit
//      atomicAdd on the unit's counter carries both counts (entries in the high word, actions in the low one), so the run
//      behind it in the entry order is also the run behind it in the action order.
//   2. The host reads the units' counters back (8 bytes each: the one round trip) and launches ge_rollout_kernel<.., ACT = 2> on
//      the device-resident entries through rollout_launch_form<2>: the playout kernel is ge_batch_rollout_seats's own, unchanged.
//   3. ge_advise_reduce: one lane per listed entry.  It reads words 0 (finished), 51 + s-1 (seat_wins) and 63 + s-1 (seat_score)
//      of its run's accumulator rows and stores the ge_advice; `best` is the first maximum over the legal choices ascending.
// An entry's words depend only on its own record, key, turn and seat, never on where the atomic counter put its run, so the
// result is deterministic.  Nothing of the batch is written.

namespace {

struct AdvisePlanArgs {
    const uint64_t *rooms, *keys;           // this unit's listed entries (rooms segment-local)
    const uint32_t *turns, *seats;
    u32x4 *plan;                            // per listed entry: first entry of its run in the pass, legal, row of the phase, 0
    unsigned long long *counter;            // the unit's counter (zeroed by the host): entries << 32 | actions
    uint64_t *e_rooms, *e_keys;             // the pass's entries (RollArgs<2>'s arrays)
    uint32_t *e_turns, *e_seats, *e_first, *e_players, *e_choices;
    int32_t *e_status;
    uint32_t n, seg, full_view, e_base;     // e_base: the unit's first entry (and first action) in the pass
};

struct AdviseReduceArgs {
    const u32x4 *plan;
    const uint32_t *seats;
    const unsigned long long *acc;          // the pass's accumulators, ROLL_STRIDE words per entry
    u32x4 *out;                             // per listed entry: a ge_advice as 14 x 16 bytes
    uint32_t n, by_score;                   // by_score: the value of `best` is the score (Two-Truths), else the wins
};

constexpr uint32_t ADVISE_OPTIONS = 12u;    // option[] of ge_advice
constexpr uint32_t ADVISE_VEC = 14u;        // sizeof(ge_advice) / 16

template <int NB, bool WWP>
__device__ __forceinline__ void advise_plan_entry(const SegDev &sg, const DevTable *__restrict__ tables, const AdvisePlanArgs &a, uint32_t k) {
    using G = PlayoutGame<NB, WWP>;
    using L = typename G::L;
    const uint64_t room = a.rooms[k];
    const uint32_t seat = a.seats[k];
    uint32_t w[12];
    load_words<L::WORDS>(sg.base, sg.rooms_padded, room, w);
    typename G::S s;
    L::unpack(w, s);
    const DevRow &row = tables[sg.table_idx].rows[s.phase];
    const DevCond &cond = tables[sg.table_idx].conds[s.phase];   // read in place, as inject_group_ww / inject_group_tt
    const uint32_t C = WWP ? sg.n_players : 3u;
    uint32_t legal = 0;
    for (uint32_t c = 1; c <= C; c++) {                       // legal exactly when the injected action would be accepted
        typename G::S t = s;
        legal |= (G::inject(t, row, cond, sg.n_players, seat, c) == GE_OK ? 1u : 0u) << (c - 1u);
    }
    const uint32_t p = popc(legal);
    uint32_t e = 0, act = 0;
    if (p) {
        const unsigned long long at = atomicAdd(a.counter, ((unsigned long long)(p + 1u) << 32) | p);
        e = a.e_base + (uint32_t)(at >> 32);
        act = a.e_base + (uint32_t)at;
    }
    u32x4 pl;
    pl.x = e; pl.y = legal; pl.z = s.phase; pl.w = 0u;
    a.plan[k] = pl;
    if (!p) return;
    const uint64_t key = a.keys[k];
    const uint32_t turn = a.turns[k], view = a.full_view ? 0u : seat;
    for (uint32_t m = legal;; m &= m - 1u, e++) {             // the options ascending, then the entry without an action
        a.e_rooms[e] = room; a.e_keys[e] = key; a.e_turns[e] = turn; a.e_seats[e] = view;
        a.e_first[e] = act;
        a.e_status[e] = GE_OK;
        if (!m) break;
        a.e_players[act] = seat; a.e_choices[act] = ctz(m) + 1u;
        act++;
    }
    a.e_first[e + 1u] = act;                                  // the empty slice's end: what the run behind this one starts from
}

template <int KIND>
__global__ void __launch_bounds__(64) ge_advise_plan(const SegDev *__restrict__ segs, const DevTable *__restrict__ tables, const AdvisePlanArgs a) {
    const uint32_t k = blockIdx.x * 64u + threadIdx.x;
    if (k >= a.n) return;
    const SegDev &sg = segs[a.seg];
    advise_plan_entry<KindOf<KIND>::NB, KindOf<KIND>::WW>(sg, tables, a, k);
}

// one lane per listed entry of a unit, whatever its game: only the plan, the seats and the accumulators are read
__global__ void __launch_bounds__(64) ge_advise_reduce(const AdviseReduceArgs a) {
    const uint32_t k = blockIdx.x * 64u + threadIdx.x;
    if (k >= a.n) return;
    const u32x4 pl = a.plan[k];
    const uint32_t legal = pl.y, s0 = a.seats[k] - 1u;
    u32x4 *out = a.out + (size_t)ADVISE_VEC * k;
    u32x4 z; z.x = 0u; z.y = 0u; z.z = 0u; z.w = 0u;
    if (!legal) {                                             // refused: GE_ERR_ARG and nothing else
        u32x4 h = z; h.x = (uint32_t)GE_ERR_ARG;
        out[0] = h;
        for (uint32_t j = 1; j < ADVISE_VEC; j++) out[j] = z;
        return;
    }
    const unsigned long long *row = a.acc + (size_t)pl.x * ROLL_STRIDE;
    uint32_t best = 0;
    unsigned long long top = 0;
    for (uint32_t c = 0; c < ADVISE_OPTIONS; c++) {           // the run's rows are the legal choices ascending
        u32x4 o = z;
        if ((legal >> c) & 1u) {
            const unsigned long long wins = row[51u + s0], score = row[63u + s0];
            const unsigned long long v = a.by_score ? score : wins;
            if (best == 0u || v > top) { best = c + 1u; top = v; }
            o.x = (uint32_t)row[0]; o.y = (uint32_t)wins; o.z = (uint32_t)score; o.w = (uint32_t)(score >> 32);
            row += ROLL_STRIDE;
        }
        out[2u + c] = o;
    }
    u32x4 o;                                                  // the entry without an action: the run's last row
    o.x = (uint32_t)row[0]; o.y = (uint32_t)row[51u + s0]; o.z = (uint32_t)row[63u + s0]; o.w = (uint32_t)(row[63u + s0] >> 32);
    out[1] = o;
    u32x4 h;
    h.x = (uint32_t)GE_OK; h.y = legal; h.z = best; h.w = pl.z;   // (the row of the phase: the host puts its phase id)
    out[0] = h;
}

hipError_t advise_launch(uint32_t kind, dim3 grid, hipStream_t st, const ge_batch *b, const AdvisePlanArgs &a) {
    return by_kind(kind, [&](auto K) { hipLaunchKernelGGL((ge_advise_plan<K()>), grid, dim3(64), 0, st, b->segs_dev, b->tables, a); });
}
hipError_t advise_launch(dim3 grid, hipStream_t st, const AdviseReduceArgs &a) {
    hipLaunchKernelGGL(ge_advise_reduce, grid, dim3(64), 0, st, a);
    return hipGetLastError();
}

}  // namespace

static_assert(sizeof(ge_advice_option) == 16 && sizeof(ge_advice) == 16 * ADVISE_VEC, "an advice is 14 16-byte stores");
static_assert(offsetof(ge_advice, policy) == 16 && offsetof(ge_advice, option) == 32, "header, policy, options");

// units: runs of sorted listed entries of one segment with room for at most CHUNK entries of the pass (a listed entry reserves
// playout_max_cands + 1); passes: consecutive units whose room fits in CHUNK entries together.  As playout_units, without masks
static void advise_units(const ge_batch *b, const PoolEntries &en, std::vector<PlayoutUnit> &units, uint32_t &n_pass, uint32_t &max_cap) {
    const uint32_t CHUNK = 65536;
    uint32_t pass_cap = 0;
    n_pass = 0; max_cap = 0;
    for (uint32_t g = 0; g < (uint32_t)b->segs.size(); g++) {
        const uint32_t cap = playout_max_cands(b->segs[g].dev) + 1u;
        for (uint32_t i = en.begin[g]; i < en.begin[g + 1u]; i++) {
            const bool fresh = units.empty() || units.back().seg != g || pass_cap + cap > CHUNK;
            if (fresh) {                                      // one slot more than its entries' room: a unit's last run closes its
                if (units.empty() || pass_cap + cap + 1u > CHUNK) { n_pass++; pass_cap = 0; }   // empty slice in first_action[its end],
                units.push_back(PlayoutUnit{g, i, 0u, pass_cap, 1u, n_pass - 1u});              // which must not be the next unit's first word
                pass_cap += 1u;
            }
            units.back().cnt++;
            units.back().e_cap += cap;
            pass_cap += cap;
            max_cap = std::max(max_cap, pass_cap);
        }
    }
}

static int advise_seats_impl(ge_batch *b, uint64_t n, const uint64_t *rooms, const uint64_t *keys, const uint32_t *turns, const uint32_t *seats,
                             uint32_t n_rollouts, uint32_t max_turns, uint64_t seed, uint32_t flags, ge_advice *out) {
    GE_ON_DEVICE(b);
    int st = sync_impl(b);
    if (st != GE_OK) return st;
    const PoolEntries en(b, n, rooms);
    const std::vector<uint32_t> &order = en.order;
    std::vector<PlayoutUnit> units;
    uint32_t n_pass = 0, max_cap = 0;
    advise_units(b, en, units, n_pass, max_cap);
    const uint32_t n_units = (uint32_t)units.size();
    // one scratch layout, each array from a 16 B boundary.  Upload: [rooms u64][keys u64][turns u32][seats u32][unit counters
    // u64, zeroed].  Then [plan 16 B][advice 224 B] per listed entry and the pass's entries
    const size_t N = (size_t)n;
    const size_t o_keys = 8 * N, o_turns = 16 * N, o_seats = up16(o_turns + 4 * N), o_ctr = up16(o_seats + 4 * N);
    const size_t o_up_end = up16(o_ctr + 8 * (size_t)n_units);
    const size_t o_plan = o_up_end, o_adv = o_plan + 16 * N;
    const PassEntries pe(o_adv + sizeof(ge_advice) * N, max_cap, false);
    // the pinned buffer holds the upload, then the advice records on their way back
    uint32_t *host32 = nullptr;
    if ((st = io_stage(b, std::max(o_up_end, sizeof(ge_advice) * N), &host32)) != GE_OK) return st;
    unsigned char *host = reinterpret_cast<unsigned char *>(host32);
    en.stage(b, rooms, keys, turns, host, o_keys, o_turns);
    uint32_t *h_seats = reinterpret_cast<uint32_t *>(host + o_seats);
    for (size_t i = 0; i < N; i++) h_seats[i] = seats[order[i]];
    memset(host + o_ctr, 0, o_up_end - o_ctr);
    char *dev = nullptr;
    if ((st = pool_scratch(b, pe.o.total, &dev)) != GE_OK) return st;
    hipStream_t s = b->last_stream;
    if ((st = order_after_previous(b, s)) != GE_OK) return st;
    HIP_TRY(hipMemcpyAsync(dev, host, o_up_end, hipMemcpyHostToDevice, s));
    const uint64_t *h_ctr = reinterpret_cast<const uint64_t *>(host + o_ctr);
    for (uint32_t p = 0; p < n_pass; p++) {
        // 1. plan every unit of the pass
        for (const PlayoutUnit &u : units) {
            if (u.pass != p) continue;
            AdvisePlanArgs a;
            a.rooms = reinterpret_cast<const uint64_t *>(dev) + u.lo;
            a.keys = reinterpret_cast<const uint64_t *>(dev + o_keys) + u.lo;
            a.turns = reinterpret_cast<const uint32_t *>(dev + o_turns) + u.lo;
            a.seats = reinterpret_cast<const uint32_t *>(dev + o_seats) + u.lo;
            a.plan = reinterpret_cast<u32x4 *>(dev + o_plan) + u.lo;
            a.counter = reinterpret_cast<unsigned long long *>(dev + o_ctr) + (&u - units.data());
            bind_entries(a, dev, pe);
            a.n = u.cnt; a.seg = u.seg; a.full_view = (flags & GE_ADVISE_FULL_VIEW) ? 1u : 0u; a.e_base = u.e_base;
            HIP_TRY(advise_launch(b->segs[u.seg].dev.kind, dim3((u.cnt + 63u) / 64u), s, b, a));
        }
        // 2. the units' counters (the one host round trip), then the playouts of each unit
        HIP_TRY(hipMemcpyAsync(host + o_ctr, dev + o_ctr, 8 * (size_t)n_units, hipMemcpyDeviceToHost, s));
        if ((st = sync_impl(b)) != GE_OK) return st;
        if ((st = order_after_previous(b, s)) != GE_OK) return st;
        for (const PlayoutUnit &u : units) {
            const uint32_t cnt = (uint32_t)(h_ctr[&u - units.data()] >> 32);
            if (u.pass != p || !cnt) continue;                // (cnt < e_cap: a listed entry reserves its most)
            HIP_TRY(hipMemsetAsync(dev + pe.o.acc + 8 * (size_t)ROLL_STRIDE * u.e_base, 0, 8 * (size_t)ROLL_STRIDE * cnt, s));
            HIP_TRY(rollout_launch_form<2>(b, s, unit_rollout_args(b, dev, pe, u, cnt, seed, n_rollouts, max_turns), dev, pe.o, u.e_base));
        }
        // 3. the advice records (a unit without a run still stores its refusals)
        for (const PlayoutUnit &u : units) {
            if (u.pass != p) continue;
            const uint32_t kind = b->segs[u.seg].dev.kind;
            AdviseReduceArgs a;
            a.plan = reinterpret_cast<const u32x4 *>(dev + o_plan) + u.lo;
            a.seats = reinterpret_cast<const uint32_t *>(dev + o_seats) + u.lo;
            a.acc = reinterpret_cast<const unsigned long long *>(dev + pe.o.acc);
            a.out = reinterpret_cast<u32x4 *>(dev + o_adv) + (size_t)ADVISE_VEC * u.lo;
            a.n = u.cnt; a.by_score = (kind == K_WW8 || kind == K_WW12) ? 0u : 1u;
            HIP_TRY(advise_launch(dim3((u.cnt + 63u) / 64u), s, a));
        }
    }
    HIP_TRY(hipMemcpyAsync(host, dev + o_adv, sizeof(ge_advice) * N, hipMemcpyDeviceToHost, s));
    if ((st = sync_impl(b)) != GE_OK) return st;
    for (size_t i = 0; i < N; i++) {                          // scattered back into input order, the phase's row as its id
        ge_advice &r = out[order[i]];
        memcpy(&r, host + sizeof(ge_advice) * i, sizeof(ge_advice));
        if (r.status == GE_OK) r.phase_id = (uint32_t)b->segs[en.seg_at(i)].table.rows[r.phase_id & 255u].phase_id;
    }
    return GE_OK;
}

extern "C" {

int ge_batch_advise_seats(ge_batch *b, uint64_t n, const uint64_t *rooms, const uint64_t *keys, const uint32_t *turns, const uint32_t *seats,
                          uint32_t n_rollouts, uint32_t max_turns, uint64_t seed, uint32_t flags, ge_advice *out) {
    if (!b) return GE_ERR_ARG;
    if (n == 0) return GE_OK;
    // all before anything runs, in this order (ABI behaviour): pointers, flags and caps (GE_ERR_ARG), rooms and turns
    // (GE_ERR_RANGE), then the seats and the cost cap (GE_ERR_ARG, after the rooms: both are bound to the room's segment)
    if (!rooms || !keys || !turns || !seats || !out) return GE_ERR_ARG;
    if (flags & ~(uint32_t)GE_ADVISE_FULL_VIEW) return GE_ERR_ARG;
    if (n_rollouts == 0 || n_rollouts > (1u << 20) || max_turns > 4096u || n > (1ull << 26)) return GE_ERR_ARG;
    for (uint64_t k = 0; k < n; k++)
        if (rooms[k] >= b->n_rooms || (uint64_t)turns[k] + max_turns > 0xFFFFFFFFull) return GE_ERR_RANGE;
    uint64_t cost = 0;
    for (uint64_t k = 0; k < n; k++) {                        // (rooms[k] is in range: its segment is known)
        const SegDev &sg = b->segs[pool_segment_of(b, rooms[k])].dev;
        if (seats[k] == 0u || seats[k] > sg.n_players) return GE_ERR_ARG;
        cost += (uint64_t)(playout_max_cands(sg) + 1u) * n_rollouts;
        if (cost > (1ull << 26)) return GE_ERR_ARG;
    }
    return guarded([&] { return advise_seats_impl(b, n, rooms, keys, turns, seats, n_rollouts, max_turns, seed, flags, out); });
}

}  // extern "C"

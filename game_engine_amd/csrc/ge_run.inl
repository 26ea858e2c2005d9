// ge_run.inl — listed rooms played on until a person is needed (ge_batch_run_rooms, POLICY.md §3f): ge_batch_step_rooms turn
// after turn inside one launch, each turn's event and record traced (included at the end of ge_step.hip, behind ge_compare.inl:
// the existing kernels keep their code-object offsets).  Checks, grouping, staging and the launch by kind are ge_pool.inl's
// (pool_check_entries, PoolEntries, by_kind), and so is the lane that plays a turn; the timed interval is ge_step.hip's
// timing_begin.  What this file adds is the turn loop in the kernel, its stop tests and the trace plane.
//
// A game thread spends most of its turns in phases where no person has anything to do - timers, UI phases, other roles' night
// phases, "waiting" turns in which a bot acts with probability 3/4.  Played through ge_batch_step_rooms + ge_batch_read_rooms_at
// each of them is two synchronising round trips.  Here entry k is stepped as (rooms[k], keys[k], turns[k] + t), t = 0, 1, ..,
// until the record the turn left meets a condition of `until` or max_turns turns are played; what every turn logged and left
// goes into a device trace plane and crosses to the host once.
//
// ge_run_kernel: one lane per entry, one wavefront per block, the indexed lane of ge_pool.inl (lane_ww_ctx / lane_cond_ctx,
// lane_recycle, lane_ww_turn / lane_tt_turn, lane_event).  The turn loop holds the per-lane restart check, the turn, the trace
// store and the stop test.  The action queue is a wave-wide collective, so a lane whose room has stopped cannot leave the loop:
// it stores its record, its turn count and its stop bits at that moment and stays on as a shadow that never acts and stores
// nothing - what a lane past the end of the list is from the start.  The wavefront leaves when no lane is live.
//
// Stop tests, on the record after the turn:
//   PERSON  a seat of the segment's human mask is a pending target of the (new) phase.  Werewolf: the turn's own ww_targets on the
//           new row, less who has acted.  Two-Truths (whose turn has its target set inline): inject_tt on a copy of the record,
//           choice 1 - the test ge_batch_inject_actions itself makes, as ge_playout_plan uses it.
//   END     the segment's terminal mask.        PHASE   the turn's event moved the phase.
//
// Trace plane: 64 B per room-turn - the event's four words, then the packed record (at most 12 words) - turn-major: slot
// t * n + i for sorted entry i, so a wavefront's stores of one turn are consecutive and the turns anyone played are one
// contiguous block from the start of the plane (the host copies max(played) rows, not max_turns).

namespace {

struct RunArgs {
    const uint64_t *rooms;     // segment-local room of each entry of this launch
    const uint64_t *keys;      // global room index its RNG stream is keyed by
    const uint32_t *turns;     // its first turn
    u32x4 *trace;              // the call's trace plane; this launch's entries start at slot `first`
    u32x2 *out;                // [n]: turns played, stop bits
    const uint16_t *seats;     // the batch's seat plane, or null (ge_pool.inl lane_seat_mask)
    uint32_t n, seg, seed_key, restart;
    uint32_t max_turns, until, n_all, first;
};

// turn t of sorted entry i: event words, then the record's WORDS words (a 16-byte store per started group of four)
template <int WORDS>
__device__ __forceinline__ void run_trace(const RunArgs &a, uint32_t t, uint32_t k, const u32x4 &event, const uint32_t *w) {
    u32x4 *slot = a.trace + 4u * ((size_t)t * a.n_all + a.first + k);
    slot[0] = event;
#pragma unroll
    for (int j = 0; j < (WORDS + 3) / 4; j++) {
        u32x4 r;
        r.x = w[4 * j]; r.y = w[4 * j + 1];
        r.z = 4 * j + 2 < WORDS ? w[4 * j + 2] : 0u; r.w = 4 * j + 3 < WORDS ? w[4 * j + 3] : 0u;
        slot[1 + j] = r;
    }
}

template <int NB, int GENERIC>
__device__ __forceinline__ void run_ww(const SegDev &sg, const DevTable *__restrict__ tables, const RunArgs &a, void *lw, uint32_t k_in) {
    using L = WWLayout<NB>;
    // lanes past the list stay in the wavefront (the action queue is a wave-wide collective): they shadow entry 0 and store nothing
    bool live = k_in < a.n;
    const uint32_t k = live ? k_in : 0u;
    const uint64_t room = a.rooms[k];
    uint32_t w[L::WORDS];
    load_words<L::WORDS>(sg.base, sg.rooms_padded, room, w);
    const uint32_t rk = room_key_from(a.seed_key, a.keys[k]);
    const uint32_t turn0 = a.turns[k];
    const uint32_t human = lane_seat_mask(sg, a.seats, room);   // the room's own seats: per lane
    WwCtx ctx = lane_ww_ctx<GENERIC>(sg, tables, lw, rk, live, human);
    const DevRow *rows = ctx.rows;
    const uint32_t term_mask = ctx.term_mask;
    const uint32_t ALL = (1u << sg.n_players) - 1u;
    WWR<NB> s;
    uint32_t cache;                                           // the record's prepared deal: not of this key, never used
    ww_load_regs<NB>(w, s, cache);
    for (uint32_t t = 0;;) {
        const uint32_t turn = turn0 + t;
        const uint32_t restarted = lane_recycle(sg, s, a.restart, term_mask);   // every turn
        ctx.valid = live;                                     // a stopped lane is a shadow from here on
        const LaneTurn ev = lane_ww_turn<NB, GENERIC>(s, ctx, turn, true);
        const uint32_t p = ev.p;
        t++;
        if (live) {
            ww_store_regs<NB>(s, 0u, w);                      // without a prepared deal
            run_trace<L::WORDS>(a, t - 1u, k, lane_event(turn, ev, s.phase, restarted), w);
            uint32_t why = 0;
            if (a.until & GE_RUN_UNTIL_PERSON) {
                const DevRow nrow = lds_row<false>(rows, s.phase);
                const uint32_t T = ww_targets<NB, true, GENERIC>(s, nrow, ctx, s.template get<F_ALIVE>(), ALL);
                why |= (T & ~s.acted & human) ? GE_RUN_UNTIL_PERSON : 0u;
            }
            why |= ((term_mask >> s.phase) & 1u) ? (a.until & GE_RUN_UNTIL_END) : 0u;
            why |= s.phase != p ? (a.until & GE_RUN_UNTIL_PHASE) : 0u;
            if (why != 0u || t == a.max_turns) {
                store_words<L::WORDS>(sg.base, sg.rooms_padded, room, w);
                u32x2 o; o.x = t; o.y = why;
                a.out[k] = o;
                live = false;
            }
        }
        if (t == a.max_turns || __ballot(live) == 0ull) break;
    }
}

template <int NB, int GENERIC>
__device__ __forceinline__ void run_tt(const SegDev &sg, const DevTable *__restrict__ tables, const RunArgs &a, void *lw, uint32_t k_in) {
    using L = TTLayout<NB>;
    bool live = k_in < a.n;
    const uint32_t k = live ? k_in : 0u;
    const uint64_t room = a.rooms[k];
    uint32_t w[L::WORDS];
    load_words<L::WORDS>(sg.base, sg.rooms_padded, room, w);
    const uint32_t rk = room_key_from(a.seed_key, a.keys[k]);
    const uint32_t turn0 = a.turns[k];
    const CondCtx cc = lane_cond_ctx<GENERIC>(sg, tables);
    const uint32_t term_mask = __builtin_amdgcn_readfirstlane(sg.term_mask);
    // the seats probed are the wavefront's: with a seat plane the union of its rooms' masks, each lane counting only its own bits
    const uint32_t human = lane_seat_mask(sg, a.seats, room) & ((1u << sg.n_players) - 1u);
    const uint32_t probe = a.seats ? wave_seat_union(human, NB) : (uint32_t)__builtin_amdgcn_readfirstlane(human);
    TT<NB> s;
    L::unpack(w, s);
    uint32_t done = tt_done_mask<NB>(s.rounds, sg.rounds);
    for (uint32_t t = 0;;) {
        const uint32_t turn = turn0 + t;
        const uint32_t restarted = lane_recycle(sg, s, a.restart, term_mask);   // every turn
        if (restarted) done = __builtin_amdgcn_readfirstlane(sg.done0);
        const LaneTurn ev = lane_tt_turn<NB, GENERIC>(s, done, sg, tables, cc, lw, live, rk, turn, true, human, term_mask);
        const uint32_t p = ev.p;
        t++;
        if (live) {
            L::pack(s, w);
            run_trace<L::WORDS>(a, t - 1u, k, lane_event(turn, ev, s.phase, restarted), w);
            uint32_t why = 0;
            if ((a.until & GE_RUN_UNTIL_PERSON) && probe != 0u) {   // (wave-uniform)
                const DevRow &nrow = tables[sg.table_idx].rows[s.phase];
                const DevCond &cond = tables[sg.table_idx].conds[s.phase];   // read in place, as inject_group_tt
                for (uint32_t m = probe; m; m &= m - 1u) {
                    TT<NB> c = s;                             // a pending target exactly when an injected action would be accepted
                    const bool ok = inject_tt<NB>(c, nrow, cond, sg.n_players, ctz(m) + 1u, 1u) == GE_OK;
                    why |= (ok && (human & m & (0u - m)) != 0u) ? GE_RUN_UNTIL_PERSON : 0u;
                }
            }
            why |= ((term_mask >> s.phase) & 1u) ? (a.until & GE_RUN_UNTIL_END) : 0u;
            why |= s.phase != p ? (a.until & GE_RUN_UNTIL_PHASE) : 0u;
            if (why != 0u || t == a.max_turns) {
                store_words<L::WORDS>(sg.base, sg.rooms_padded, room, w);
                u32x2 o; o.x = t; o.y = why;
                a.out[k] = o;
                live = false;
            }
        }
        if (t == a.max_turns || __ballot(live) == 0ull) break;
    }
}

// one wavefront per block; its action queue (WaveLdsLow) is the block's dynamic LDS (none for Two-Truths x 4: no queue)
template <int KIND, int GENERIC>
__global__ void __launch_bounds__(64) ge_run_kernel(const SegDev *__restrict__ segs, const DevTable *__restrict__ tables, const RunArgs a) {
    const SegDev &sg = segs[a.seg];
    const uint32_t k = blockIdx.x * 64u + threadIdx.x;
    void *lw = ge_lds;
    if constexpr (KindOf<KIND>::WW) run_ww<KindOf<KIND>::NB, GENERIC>(sg, tables, a, lw, k);
    else run_tt<KindOf<KIND>::NB, GENERIC>(sg, tables, a, lw, k);
}

template <int GEN> hipError_t run_launch(uint32_t kind, dim3 grid, hipStream_t st, const ge_batch *b, const RunArgs &a) {
    return by_kind(kind, [&](auto K) { hipLaunchKernelGGL((ge_run_kernel<K(), GEN>), grid, dim3(64), lane_lds(kind), st, b->segs_dev, b->tables, a); });
}

constexpr uint32_t RUN_MAX_TURNS = 4096u, RUN_MAX_SLOTS = 1u << 20;
constexpr size_t RUN_ONE_COPY = 256u << 10;   // a trace plane up to this size comes back whole with the turn counts: one round trip

}  // namespace

// the checks of ge_batch_run_rooms (n > 0), all before anything runs: ge_batch_step_rooms's first; shared with
// ge_batch_run_rooms_playout (ge_run_playout.inl)
static int run_check(const ge_batch *b, uint64_t n, const uint64_t *rooms, const uint64_t *keys, const uint32_t *turns, uint32_t max_turns,
                     uint32_t until, const uint32_t *played, const ge_room_view *views, size_t views_cap_bytes) {
    const int st = pool_check_entries(b, n, rooms, keys, turns);
    if (st != GE_OK) return st;
    if (!played || max_turns == 0u || max_turns > RUN_MAX_TURNS || n * (uint64_t)max_turns > RUN_MAX_SLOTS) return GE_ERR_ARG;
    if (until & ~(uint32_t)(GE_RUN_UNTIL_PERSON | GE_RUN_UNTIL_END | GE_RUN_UNTIL_PHASE)) return GE_ERR_ARG;
    if (views && views_cap_bytes / sizeof(ge_room_view) < n * (uint64_t)max_turns) return GE_ERR_ARG;
    for (uint64_t k = 0; k < n; k++)
        if ((uint64_t)turns[k] + max_turns > 0xFFFFFFFFull) return GE_ERR_RANGE;
    return GE_OK;
}

// the turn counts and stop bits of the sorted entries (h_out: [played, stopped] x n) into input order; prefix[i] = played turns in
// front of sorted entry i; returns the most turns anybody played
static uint32_t run_counts(const PoolEntries &en, const uint32_t *h_out, uint32_t *played, uint32_t *stopped, std::vector<uint64_t> &prefix) {
    const size_t n = en.size();
    prefix.assign(n + 1u, 0u);
    uint32_t rows_played = 0;
    for (size_t i = 0; i < n; i++) {
        const uint32_t p = h_out[2 * i];
        prefix[i + 1u] = prefix[i] + p;
        rows_played = std::max(rows_played, p);
        played[en.order[i]] = p;
        if (stopped) stopped[en.order[i]] = h_out[2 * i + 1u];
    }
    return rows_played;
}

// the played turns of a trace plane (h_trace: 64 B per room-turn, turn-major) as events and views in input order, split over the
// host threads of ge_batch_read_rooms.  h_dec (ge_run_playout.inl; may be null): 16 B per room-turn, turn-major - the turn's decided
// mask and choice nibbles, ORed into the event as ge_batch_step_rooms_playout does
static void run_decode(const ge_batch *b, const PoolEntries &en, uint32_t max_turns, const std::vector<uint64_t> &prefix, const uint32_t *h_trace,
                       const uint32_t *h_dec, ge_turn_event *events, ge_room_view *views, uint32_t *decided) {
    const size_t n = en.size();
    for_room_ranges(prefix[n], [&](uint64_t lo, uint64_t hi) {
        size_t i = (size_t)(std::upper_bound(prefix.begin(), prefix.end(), lo) - prefix.begin()) - 1u;
        for (uint64_t x = lo; x < hi; x++) {
            while (x >= prefix[i + 1u]) i++;
            const uint32_t t = (uint32_t)(x - prefix[i]);
            const Segment &sg = b->segs[en.seg_at(i)];
            const uint32_t *slot = h_trace + 16u * ((size_t)t * n + i);
            const size_t at = (size_t)en.order[i] * max_turns + t;
            const uint32_t *d = h_dec ? h_dec + 4u * ((size_t)t * n + i) : nullptr;
            if (decided && d) decided[at] = d[0];
            if (events) {
                pool_decode_event(slot, sg.table, events[at]);
                if (d) {
                    const uint64_t dnib = (uint64_t)d[1] | ((uint64_t)d[2] << 32);
                    events[at].acted_now |= (uint16_t)d[0];
                    for (int c = 0; c < 16; c++) events[at].choice[c] |= (uint8_t)((dnib >> (4 * c)) & 15u);
                }
            }
            if (views) {
                uint32_t w[12] = {0};
                for (uint32_t j = 0; j < sg.dev.words; j++) w[j] = slot[4u + j];
                words_to_view(sg.dev.kind, w, sg.table, (int)sg.dev.n_players, views[at]);
            }
        }
    });
}

// segment g's entries of a run staged at dev (rooms at 0, keys, turns): the trace plane from off_trace, (played, stop bits) at off_out
static RunArgs run_args(const ge_batch *b, const PoolEntries &en, uint32_t g, char *dev, size_t off_keys, size_t off_turns, size_t off_trace,
                        size_t off_out, uint32_t max_turns, uint32_t until) {
    const uint32_t lo = en.begin[g];
    RunArgs a;
    a.rooms = reinterpret_cast<const uint64_t *>(dev) + lo;
    a.keys = reinterpret_cast<const uint64_t *>(dev + off_keys) + lo;
    a.turns = reinterpret_cast<const uint32_t *>(dev + off_turns) + lo;
    a.trace = reinterpret_cast<u32x4 *>(dev + off_trace);
    a.out = reinterpret_cast<u32x2 *>(dev + off_out) + lo;
    a.seats = b->seats;
    a.n = en.begin[g + 1u] - lo; a.seg = g; a.seed_key = seed_key((uint32_t)b->seed, (uint32_t)(b->seed >> 32));
    a.restart = (b->flags & GE_FLAG_RESTART) ? 1u : 0u;
    a.max_turns = max_turns; a.until = until; a.n_all = (uint32_t)en.size(); a.first = lo;
    return a;
}

static int run_rooms_impl(ge_batch *b, uint64_t n, const uint64_t *rooms, const uint64_t *keys, const uint32_t *turns, uint32_t max_turns,
                          uint32_t until, uint32_t *played, uint32_t *stopped, ge_turn_event *events, ge_room_view *views, size_t views_cap_bytes) {
    if (n == 0) return GE_OK;
    int st = run_check(b, n, rooms, keys, turns, max_turns, until, played, views, views_cap_bytes);
    if (st != GE_OK) return st;
    GE_ON_DEVICE(b);
    if ((st = sync_impl(b)) != GE_OK) return st;
    const PoolEntries en(b, n, rooms);
    // one upload: [rooms u64 x n][keys u64 x n][turns u32 x n (padded to 16 B)]; then [played, stopped] x n (padded) and the trace plane
    const size_t off_keys = 8 * (size_t)n, off_turns = 16 * (size_t)n, off_out = up16(off_turns + 4 * (size_t)n);
    const size_t off_trace = up16(off_out + 8 * (size_t)n), row_bytes = 64 * (size_t)n;
    const size_t total = off_trace + row_bytes * max_turns;
    uint32_t *host32 = nullptr;
    if ((st = io_stage(b, total, &host32)) != GE_OK) return st;
    unsigned char *host = reinterpret_cast<unsigned char *>(host32);
    en.stage(b, rooms, keys, turns, host, off_keys, off_turns);
    char *dev = nullptr;
    if ((st = pool_scratch(b, total, &dev)) != GE_OK) return st;
    hipStream_t s = b->last_stream;
    if ((st = order_after_previous(b, s)) != GE_OK) return st;
    HIP_TRY(hipMemcpyAsync(dev, host, off_out, hipMemcpyHostToDevice, s));
    hipEvent_t e1 = nullptr;                                      // ge_batch_kernel_time counts the launches of this call as one interval
    if ((st = timing_begin(b, s, &e1)) != GE_OK) return st;
    for (uint32_t g = 0; g < (uint32_t)b->segs.size(); g++) {
        if (en.begin[g + 1u] == en.begin[g]) continue;
        const RunArgs a = run_args(b, en, g, dev, off_keys, off_turns, off_trace, off_out, max_turns, until);
        const dim3 grid((a.n + 63u) / 64u);
        HIP_TRY(b->plan.generic ? run_launch<1>(b->segs[g].dev.kind, grid, s, b, a) : run_launch<0>(b->segs[g].dev.kind, grid, s, b, a));
    }
    if (e1) HIP_TRY(hipEventRecord(e1, s));
    // the turn counts first: only the rows of turns somebody played are copied - unless the whole plane is small
    const uint32_t *h_out = reinterpret_cast<const uint32_t *>(host + off_out);
    const bool whole = row_bytes * max_turns <= RUN_ONE_COPY;
    HIP_TRY(hipMemcpyAsync(host + off_out, dev + off_out, whole ? total - off_out : off_trace - off_out, hipMemcpyDeviceToHost, s));
    if ((st = sync_impl(b)) != GE_OK) return st;
    std::vector<uint64_t> prefix;                                // played turns in front of sorted entry i
    const uint32_t rows_played = run_counts(en, h_out, played, stopped, prefix);
    if (!events && !views) return GE_OK;
    if (!whole) {
        HIP_TRY(hipMemcpyAsync(host + off_trace, dev + off_trace, row_bytes * rows_played, hipMemcpyDeviceToHost, s));
        if ((st = sync_impl(b)) != GE_OK) return st;
    }
    run_decode(b, en, max_turns, prefix, reinterpret_cast<const uint32_t *>(host + off_trace), nullptr, events, views, nullptr);
    return GE_OK;
}

extern "C" {

int ge_batch_run_rooms(ge_batch *b, uint64_t n, const uint64_t *rooms, const uint64_t *keys, const uint32_t *turns, uint32_t max_turns,
                       uint32_t until, uint32_t *played, uint32_t *stopped, ge_turn_event *events, ge_room_view *views, size_t views_cap_bytes) {
    if (!b) return GE_ERR_ARG;
    return guarded([&] {
        return run_rooms_impl(b, n, rooms, keys, turns, max_turns, until, played, stopped, events, views, views_cap_bytes);
    });
}

}  // extern "C"

// ge_run_seats.inl — every room of a range played on until a listed seat must act, in device memory (ge_batch_run_seats, POLICY.md
// §3p): the run-on of ge_run.inl in the form of ge_env.inl's calls - a range of rooms, the caller's stream, results in device memory
// the caller owns, no host copy, no host wait (included at the end of ge_step.hip, behind ge_teach.inl: the existing kernels keep
// their code-object offsets).  Between ge_batch_act_seats and ge_batch_observe_seats it is what ge_batch_step is, except that a
// room stops where the learner has to look at it: a listed seat is a pending target, the game has ended, or the turn limit.
//
// By composition: with T the batch's turn counter, room r of the range takes ge_batch_run_rooms's entry (r, global index of r, T)
// under max_turns and until & 7, and one more stop test, GE_RUN_UNTIL_SEAT: the PERSON test with the listed seats in place of the
// room's seat mask.  The turn is ge_batch_step_rooms's - the room's own mask decides whom the policy plays, the seat list plays no
// part in it.  The turn counter advances by max_turns whatever the rooms played: the RNG is keyed by (room, turn), so a room that
// stopped early simply took no turn at the later indices.
//
// ge_seat_run_kernel<KIND, GENERIC>: one body for both games over ge_pool.inl's Lane (seat_run_lane) - seat_lane's ranged turn loop
// (ge_seats.inl) with ge_run_kernel's stop tests and shadow rule.  Lane = room of the segment's part, one wavefront per block, one
// launch per segment of the range (env_launches).  The action queue is a wave-wide collective, so a lane whose room has stopped
// stores its record, its turn count and its stop bits at that moment - 4-byte stores, consecutive over the wavefront - and stays on
// as a shadow that never acts; the wavefront leaves when no lane is live.  No trace plane, no staging; the GE_FLAG_TRACE buffer is
// not written.  Lanes past the part shadow its first room and store nothing.

namespace {

struct SeatRunArgs {
    uint32_t *played;          // this part's entries: turns played
    uint32_t *stopped;         // ... and the stop bits, or null
    const uint16_t *plane;     // the batch's seat plane, or null (ge_pool.inl lane_seat_mask)
    uint64_t r0, nr;           // the part: segment-local rooms r0 .. r0 + nr - 1
    uint64_t seats;            // nibble j = seats[j] (1-based)
    uint32_t seg, n_seats, seed_key, restart;
    uint32_t turn0, max_turns, until;
};

template <int NB, bool WWP, int GENERIC>
__device__ __forceinline__ void seat_run_lane(const SegDev &sg, const DevTable *__restrict__ tables, const SeatRunArgs &a, void *lw, uint64_t k) {
    using Ln = Lane<NB, WWP, GENERIC>;
    using L = typename Ln::L;
    // lanes past the part stay in the wavefront (the action queue is a wave-wide collective): they shadow its first room and store nothing
    bool live = k < a.nr;
    const uint64_t room = a.r0 + (live ? k : 0u);
    uint32_t w[L::WORDS];
    load_words<L::WORDS>(sg.base, sg.rooms_padded, room, w);
    const uint32_t rk = room_key_from(a.seed_key, sg.first_global + room);
    const uint32_t human = lane_seat_mask(sg, a.plane, room);     // the room's own seats: per lane
    uint32_t listed = 0;                                          // the listed seats: wave-uniform
    for (uint32_t j = 0; j < a.n_seats; j++) listed |= 1u << (((uint32_t)(a.seats >> (4u * j)) & 15u) - 1u);
    listed &= (1u << sg.n_players) - 1u;
    // PERSON is pending(own mask), SEAT is pending(listed mask): one evaluation over the seats either test asks for, read twice
    const uint32_t own = (a.until & GE_RUN_UNTIL_PERSON) ? human : 0u, lst = (a.until & GE_RUN_UNTIL_SEAT) ? listed : 0u;
    const uint32_t probe = Ln::probe(sg, a.plane, own) | Ln::probe(sg, nullptr, lst);
    Ln lane;                                                      // the record's prepared deal is never used (as an indexed step)
    lane.open(sg, tables, lw, w, rk, live, human);
    for (uint32_t t = 0;;) {
        const uint32_t turn = a.turn0 + t;
        lane.recycle(sg, a.restart);                              // every turn
        lane.shadow(!live);                                       // a stopped lane is a shadow from here on
        const LaneTurn ev = lane.turn(turn, false);
        t++;
        if (live) {
            const uint32_t pend = lane.pending(own | lst, probe);
            uint32_t why = (pend & own) ? GE_RUN_UNTIL_PERSON : 0u;
            why |= (pend & lst) ? GE_RUN_UNTIL_SEAT : 0u;
            why |=((lane.term_mask() >> lane.phase()) & 1u) ? (a.until & GE_RUN_UNTIL_END) : 0u;
            why |= lane.phase() != ev.p ? (a.until & GE_RUN_UNTIL_PHASE) : 0u;
            if (why != 0u || t == a.max_turns) {
                lane.pack(w);                                     // stored without a prepared deal
                store_words<L::WORDS>(sg.base, sg.rooms_padded, room, w);
                a.played[k] = t;
                if (a.stopped) a.stopped[k] = why;
                live = false;
            }
        }
        if (t == a.max_turns || __ballot(live) == 0ull) break;
    }
}

// one wavefront per block; its action queue (WaveLdsLow) is the block's dynamic LDS (none for Two-Truths x 4: no queue)
template <int KIND, int GENERIC>
__global__ void __launch_bounds__(64) ge_seat_run_kernel(const SegDev *__restrict__ segs, const DevTable *__restrict__ tables, const SeatRunArgs a) {
    const SegDev &sg = segs[a.seg];
    const uint64_t k = (uint64_t)blockIdx.x * 64u + threadIdx.x;
    void *lw = ge_lds;
    seat_run_lane<KindOf<KIND>::NB, KindOf<KIND>::WW, GENERIC>(sg, tables, a, lw, k);
}

template <int GEN> hipError_t seat_run_launch(uint32_t kind, dim3 grid, hipStream_t st, const ge_batch *b, const SeatRunArgs &a) {
    return by_kind(kind, [&](auto K) { hipLaunchKernelGGL((ge_seat_run_kernel<K(), GEN>), grid, dim3(64), lane_lds(kind), st, b->segs_dev, b->tables, a); });
}

}  // namespace

// the checks of ge_batch_run_seats behind b's, all before anything is launched, in their order (ABI behaviour).  GE_OK with
// *go = false: nothing to do
static int run_seats_check(const ge_batch *b, uint64_t first, uint64_t count, uint32_t n_seats, const uint32_t *seats, uint32_t max_turns, uint32_t until,
                           const uint32_t *played_dev, const uint32_t *stopped_dev, uint64_t *packed, bool *go) {
    *go = false;
    *packed = 0;
    if (max_turns == 0u || max_turns > RUN_MAX_TURNS) return GE_ERR_ARG;
    const uint32_t known = GE_RUN_UNTIL_PERSON | GE_RUN_UNTIL_END | GE_RUN_UNTIL_PHASE | GE_RUN_UNTIL_SEAT;
    if ((until & ~known) || ((until & GE_RUN_UNTIL_SEAT) && n_seats == 0u)) return GE_ERR_ARG;
    if (!played_dev && count > 0u) return GE_ERR_ARG;
    if ((!seats && n_seats > 0u) || n_seats > GE_MAX_PLAYERS) return GE_ERR_ARG;
    for (uint32_t j = 0; j < n_seats; j++)
        for (uint32_t i = 0; i < j; i++)
            if (seats[i] == seats[j]) return GE_ERR_ARG;
    if (first + count > b->n_rooms || first + count < first) return GE_ERR_RANGE;
    for (uint32_t j = 0; j < n_seats; j++) {
        if (seats[j] == 0u) return GE_ERR_ARG;
        for (const Segment &s : b->segs)
            if (std::max(first, s.local_first) < std::min(first + count, s.local_first + s.dev.rooms) && seats[j] > s.dev.n_players) return GE_ERR_ARG;
        if (seats[j] <= GE_MAX_PLAYERS) *packed |= (uint64_t)seats[j] << (4u * j);
    }
    const size_t bytes = (size_t)count * sizeof(uint32_t);        // (count <= n_rooms)
    if (count > 0u && (!env_reachable(b, played_dev, bytes) || (stopped_dev && !env_reachable(b, stopped_dev, bytes)))) return GE_ERR_ARG;
    if (b->turn + max_turns > 0xFFFFFFFFull) return GE_ERR_RANGE;
    *go = count > 0u;
    return GE_OK;
}

extern "C" {

int ge_batch_run_seats(ge_batch *b, uint64_t first, uint64_t count, uint32_t n_seats, const uint32_t *seats, uint32_t max_turns, uint32_t until,
                       uint32_t *played_dev, uint32_t *stopped_dev, void *hip_stream) {
    if (!b) return GE_ERR_ARG;
    return guarded([&] {
        uint64_t packed = 0;
        bool go = false;
        int rc = run_seats_check(b, first, count, n_seats, seats, max_turns, until, played_dev, stopped_dev, &packed, &go);
        if (rc != GE_OK || !go) return rc;
        hipStream_t st = static_cast<hipStream_t>(hip_stream);
        const uint32_t seed_k = seed_key((uint32_t)b->seed, (uint32_t)(b->seed >> 32));
        rc = env_launches(b, first, count, n_seats, packed, st, [&](uint32_t kind, dim3 grid, EnvArgs &e, size_t) {
            const uint64_t at = b->segs[e.seg].local_first + e.r0 - first;   // the part's first entry
            SeatRunArgs a;
            memset(&a, 0, sizeof a);
            a.played = played_dev + at;
            a.stopped = stopped_dev ? stopped_dev + at : nullptr;
            a.plane = b->seats;
            a.r0 = e.r0; a.nr = e.nr; a.seats = packed; a.seg = e.seg; a.n_seats = n_seats; a.seed_key = seed_k;
            a.restart = (b->flags & GE_FLAG_RESTART) ? 1u : 0u;
            a.turn0 = (uint32_t)b->turn; a.max_turns = max_turns; a.until = until;
            return b->plan.generic ? seat_run_launch<1>(kind, grid, st, b, a) : seat_run_launch<0>(kind, grid, st, b, a);
        });
        if (rc != GE_OK) return rc;
        b->turn += max_turns;                                     // whatever the rooms played
        return (int)GE_OK;
    });
}

}  // extern "C"

// ge_teach.inl — a seat of every room advised into device memory the caller owns (ge_batch_teach_seats, POLICY.md §3o): the
// teacher beside ge_env.inl's observations and actions (included at the end of ge_step.hip, behind ge_env.inl: the existing kernels
// keep their code-object offsets).  The result is ge_batch_advise_seats's, byte for byte, for the pairs (room, seat) of a range of
// rooms and a seat list; the stream contract is ge_batch_observe_seats's - launched on the caller's stream behind the batch's
// earlier work, no host copy, no host wait - so nothing here uses the indexed calls' pinned staging, and no counter comes back.
//
// Without a counter to read, the entry layout is fixed by shape alone.  A pair owns cap = playout_max_cands + 1 consecutive entry
// slots of ge_batch_rollout_seats - slot c - 1 for choice c, the last slot for the entry without an action - and cap - 1
// consecutive actions, one per option slot, so slot i's CSR slice starts at the pair's first action + min(i, cap - 1) and the last
// slot's is empty.  A slot that is not played (an illegal choice, or any slot of a pair with legal == 0) is dead: the playouts are
// ge_rollout_kernel<.., ACT = 4>, unchanged, whose wavefronts leave a slot with a replica range x > y before they load, write a
// status or reduce anything; a live slot's range is [0, n_rollouts), which plays what ACT = 2 plays.
//
// Slots are played in passes of at most 65 536 (advise_units' CHUNK); a part is the rooms of one segment inside one pass.  Per
// pass: ge_teach_plan per part, one memset over the pass's accumulator rows, one playout launch per part on the grid of all its
// slots, ge_teach_reduce per part; the passes of a call are enqueued back to back (as ge_run_playout.inl enqueues its turns).
//
//   ge_teach_plan    lane = pair.  The record loaded as ge_observe_kernel loads it, `legal` by the same loop over G::inject on
//                    copies, the seat list a nibble per seat in the arguments.  It writes the live slots' rooms, keys, turns, seats
//                    and actions, every slot's CSR word and replica range, and the pair's 16-byte plan word (legal, phase id).
//   ge_teach_reduce  lane = pair.  Words 0, 51 + s - 1 and 63 + s - 1 of the pair's live rows (row = slot: nothing is compacted),
//                    `best` by ge_advise_reduce's rule, the ge_advice as 14 16-byte vectors, every index static.  The stores: the
//                    wavefront's 64 records go through LDS, 240 bytes apart there, and come out as 14 stores of 1 KiB of
//                    consecutive bytes each, as ge_observe_kernel's do.  Each lane storing its own record, a store instruction's
//                    lanes 224 bytes apart, was measured beside it on an MI355X and dropped (profiles/teach_probe.txt; Werewolf x 8,
//                    kernel-trace medians per launch): 7.6 against 6.6 us at 4 096 pairs, 8.4 against 7.5 us at 7 281 pairs (a pass of
//                    65 536 rooms x 1 seat), 7.5 against 6.7 us at 7 280 pairs of 4 seats.  The reduce is 0.4 .. 1.1 % of a call.

namespace {

constexpr uint32_t TEACH_CHUNK = 65536u;        // entry slots of a pass: advise_units' CHUNK
constexpr uint32_t TEACH_LDS_VEC = 15u;         // a record's stride in the reduce's LDS stage, in 16-byte units (odd: the 8 lanes of a
                                                // 16-byte LDS store group fall on distinct banks)

struct TeachPlanArgs {
    const int32_t *phase_ids;               // the segment's phase id per dense row
    const uint64_t *keys;                   // the part's rooms' keys, or null: key_base + (k << 20)
    u32x4 *plan;                            // per pair of the part: legal, phase id, 0, 0
    uint64_t *e_rooms, *e_keys;             // the pass's entry slots (RollArgs<4>'s arrays)
    uint32_t *e_turns, *e_seats, *e_first, *e_players, *e_choices;
    int32_t *e_status;
    u32x2 *e_range;
    uint64_t r0, key_base;                  // the part: segment-local rooms r0 .., and the key of its first room
    uint64_t seats;                         // nibble j = seats[j] (1-based)
    uint32_t pairs, seg, n_seats, cap;      // pairs = rooms * n_seats; cap: slots per pair
    uint32_t e_base, a_base;                // the part's first slot and first action in the pass
    uint32_t turn, n_rollouts, full_view;
};

struct TeachReduceArgs {
    const u32x4 *plan;
    const unsigned long long *acc;          // the part's first accumulator row, ROLL_STRIDE words per slot
    u32x4 *out;                             // the part's first ge_advice
    uint64_t seats;
    uint32_t pairs, n_seats, cap, by_score; // by_score: the value of `best` is the score (Two-Truths), else the wins
};

template <int KIND>
__global__ void __launch_bounds__(64) ge_teach_plan(const SegDev *__restrict__ segs, const DevTable *__restrict__ tables, const TeachPlanArgs a) {
    constexpr int NB = KindOf<KIND>::NB;
    constexpr bool WWP = KindOf<KIND>::WW;
    using G = PlayoutGame<NB, WWP>;
    using L = typename G::L;
    const uint32_t p = blockIdx.x * 64u + threadIdx.x;
    if (p >= a.pairs) return;
    const SegDev &sg = segs[a.seg];
    const uint32_t k = p / a.n_seats, j = p - k * a.n_seats;
    const uint32_t seat = (uint32_t)(a.seats >> (4u * j)) & 15u;
    const uint64_t room = a.r0 + k;
    uint32_t w[L::WORDS];
    load_words<L::WORDS>(sg.base, sg.rooms_padded, room, w);
    typename G::S s;
    L::unpack(w, s);
    const DevRow &row = tables[sg.table_idx].rows[s.phase];
    const DevCond &cond = tables[sg.table_idx].conds[s.phase];   // read in place, as inject_group_ww / inject_group_tt
    const uint32_t n = sg.n_players, C = WWP ? n : 3u;
    uint32_t legal = 0;
    for (uint32_t c = 1; c <= C; c++) {                       // ge_advise_plan's loop: legal exactly when the injected action would be accepted
        typename G::S t = s;
        legal |= (G::inject(t, row, cond, n, seat, c) == GE_OK ? 1u : 0u) << (c - 1u);
    }
    u32x4 pl;
    pl.x = legal; pl.y = (uint32_t)a.phase_ids[s.phase & (GE_MAX_PHASES - 1u)]; pl.z = 0u; pl.w = 0u;
    a.plan[p] = pl;
    const uint64_t key = a.keys ? a.keys[k] : a.key_base + ((uint64_t)k << 20);
    const uint32_t view = a.full_view ? 0u : seat, last = a.cap - 1u;
    const uint32_t e0 = a.e_base + p * a.cap, a0 = a.a_base + p * last;
    for (uint32_t i = 0; i < a.cap; i++) {                    // the option slots, then the entry without an action
        const uint32_t e = e0 + i;
        const bool live = i < last ? ((legal >> i) & 1u) != 0u : legal != 0u;
        u32x2 rg;
        rg.x = live ? 0u : 1u; rg.y = live ? a.n_rollouts : 0u;   // x > y: the playout kernel leaves the slot untouched
        a.e_range[e] = rg;
        a.e_first[e] = a0 + i;                                // (the last slot's slice is empty: it starts where the next pair's does)
        if (!live) continue;
        a.e_rooms[e] = room; a.e_keys[e] = key; a.e_turns[e] = a.turn; a.e_seats[e] = view;
        a.e_status[e] = GE_OK;
        if (i < last) { a.e_players[a0 + i] = seat; a.e_choices[a0 + i] = i + 1u; }
    }
    a.e_first[e0 + a.cap] = a0 + last;                        // the end of the last slice: what the next pair's first slot holds too
}

// one lane per pair of a part, whatever its game: only the plan and the accumulators are read
__global__ void __launch_bounds__(64) ge_teach_reduce(const TeachReduceArgs a) {
    __shared__ u32x4 stage[64u * TEACH_LDS_VEC];
    const uint32_t pb = blockIdx.x * 64u, p = pb + threadIdx.x;
    const bool valid = p < a.pairs;
    u32x4 z; z.x = 0u; z.y = 0u; z.z = 0u; z.w = 0u;
    u32x4 pl = z;
    if (valid) pl = a.plan[p];
    const uint32_t legal = pl.x, q = valid ? p : 0u;
    const uint32_t s0 = ((uint32_t)(a.seats >> (4u * (q % a.n_seats))) & 15u) - 1u;
    const unsigned long long *row = a.acc + (size_t)q * a.cap * ROLL_STRIDE;
    auto put = [&](int i, u32x4 v) { stage[threadIdx.x * TEACH_LDS_VEC + (uint32_t)i] = v; };
    uint32_t best = 0;
    unsigned long long top = 0;
#pragma unroll
    for (int c = 0; c < (int)ADVISE_OPTIONS; c++) {           // choice c + 1's row is the pair's slot c
        u32x4 o = z;
        if ((legal >> c) & 1u) {
            const unsigned long long *r = row + (size_t)c * ROLL_STRIDE;
            const unsigned long long wins = r[51u + s0], score = r[63u + s0];
            const unsigned long long v = a.by_score ? score : wins;
            if (best == 0u || v > top) { best = (uint32_t)c + 1u; top = v; }
            o.x = (uint32_t)r[0]; o.y = (uint32_t)wins; o.z = (uint32_t)score; o.w = (uint32_t)(score >> 32);
        }
        put(2 + c, o);
    }
    u32x4 o = z, h = z;
    if (legal) {                                              // the entry without an action: the pair's last slot
        const unsigned long long *r = row + (size_t)(a.cap - 1u) * ROLL_STRIDE;
        const unsigned long long score = r[63u + s0];
        o.x = (uint32_t)r[0]; o.y = (uint32_t)r[51u + s0]; o.z = (uint32_t)score; o.w = (uint32_t)(score >> 32);
        h.x = (uint32_t)GE_OK; h.y = legal; h.z = best; h.w = pl.y;
    } else {
        h.x = (uint32_t)GE_ERR_ARG;                           // refused: GE_ERR_ARG and nothing else
    }
    put(1, o);
    put(0, h);
    __syncthreads();
    const uint32_t left = a.pairs - pb;                       // (the block holds a pair: pb < pairs)
    const uint32_t vecs = (left < 64u ? left : 64u) * ADVISE_VEC;
    auto *out = (__attribute__((address_space(1))) u32x4 *)(uintptr_t)a.out + (size_t)pb * ADVISE_VEC;
#pragma unroll
    for (uint32_t i = 0; i < ADVISE_VEC; i++) {               // vector x of the wavefront's records: record x / 14, its part x % 14
        const uint32_t x = i * 64u + threadIdx.x, rec = x / ADVISE_VEC, part = x - rec * ADVISE_VEC;
        if (x < vecs) out[x] = stage[rec * TEACH_LDS_VEC + part];
    }
}

hipError_t teach_launch(uint32_t kind, dim3 grid, hipStream_t st, const ge_batch *b, const TeachPlanArgs &a) {
    return by_kind(kind, [&](auto K) { hipLaunchKernelGGL((ge_teach_plan<K()>), grid, dim3(64), 0, st, b->segs_dev, b->tables, a); });
}
hipError_t teach_launch(dim3 grid, hipStream_t st, const TeachReduceArgs &a) {
    hipLaunchKernelGGL(ge_teach_reduce, grid, dim3(64), 0, st, a);
    return hipGetLastError();
}

// the rooms of one segment inside one pass
struct TeachPart {
    uint32_t seg, pass;
    uint64_t lo;                // its first room (batch-local)
    uint32_t rooms, cap;        // cap: slots per pair
    uint32_t p_base, e_base, a_base;   // its first pair, slot and action in the pass
};

}  // namespace

// the parts and passes of a range: consecutive rooms fill a pass up to TEACH_CHUNK slots, whole rooms only (a room's pairs are
// at most 12 x 13 slots).  max_pairs / max_slots: the most a pass holds
static void teach_parts(const ge_batch *b, uint64_t first, uint64_t count, uint32_t n_seats, std::vector<TeachPart> &parts, uint32_t &n_pass,
                        uint32_t &max_pairs, uint32_t &max_slots) {
    uint32_t pass_pairs = 0, pass_slots = 0, pass_acts = 0;
    n_pass = 0; max_pairs = 0; max_slots = 0;
    for (uint32_t g = 0; g < (uint32_t)b->segs.size(); g++) {
        const Segment &s = b->segs[g];
        uint64_t lo = std::max(first, s.local_first);
        const uint64_t hi = std::min(first + count, s.local_first + s.dev.rooms);
        const uint32_t cap = playout_max_cands(s.dev) + 1u, per_room = cap * n_seats;
        while (lo < hi) {
            if (n_pass == 0 || pass_slots + per_room > TEACH_CHUNK) { n_pass++; pass_pairs = pass_slots = pass_acts = 0; }
            const uint32_t rooms = (uint32_t)std::min<uint64_t>(hi - lo, (TEACH_CHUNK - pass_slots) / per_room);
            parts.push_back(TeachPart{g, n_pass - 1u, lo, rooms, cap, pass_pairs, pass_slots, pass_acts});
            pass_pairs += rooms * n_seats; pass_slots += rooms * per_room; pass_acts += rooms * n_seats * (cap - 1u);
            max_pairs = std::max(max_pairs, pass_pairs); max_slots = std::max(max_slots, pass_slots);
            lo += rooms;
        }
    }
}

static int teach_seats_impl(ge_batch *b, uint64_t first, uint64_t count, uint32_t n_seats, uint64_t packed, const uint64_t *keys_dev, uint64_t key0,
                            uint32_t turn, uint32_t n_rollouts, uint32_t max_turns, uint64_t seed, uint32_t flags, ge_advice *out_dev, hipStream_t st) {
    GE_ON_DEVICE(b);
    std::vector<TeachPart> parts;
    uint32_t n_pass = 0, max_pairs = 0, max_slots = 0;
    teach_parts(b, first, count, n_seats, parts, n_pass, max_pairs, max_slots);
    // the scratch, device only: [plan 16 B x the most pairs of a pass], then a pass's entry slots with their replica ranges
    const PassEntries pe(16 * (size_t)max_pairs, max_slots, true);
    char *dev = nullptr;
    int rc = pool_scratch(b, pe.o.total, &dev);               // grows only for a larger shape than the batch has served (may wait)
    if (rc != GE_OK) return rc;
    if ((rc = order_after_previous(b, st)) != GE_OK) return rc;
    hipEvent_t e1 = nullptr;                                  // ge_batch_kernel_time counts the launches of this call as one interval
    if ((rc = timing_begin(b, st, &e1)) != GE_OK) return rc;
    u32x4 *plan = reinterpret_cast<u32x4 *>(dev);
    u32x2 *range = reinterpret_cast<u32x2 *>(dev + pe.range);
    for (uint32_t p = 0; p < n_pass; p++) {
        uint32_t slots = 0;
        for (const TeachPart &t : parts) {                    // 1. plan
            if (t.pass != p) continue;
            const Segment &s = b->segs[t.seg];
            TeachPlanArgs a;
            memset(&a, 0, sizeof a);
            a.phase_ids = b->phase_ids + (size_t)t.seg * GE_MAX_PHASES;
            a.keys = keys_dev ? keys_dev + (t.lo - first) : nullptr;
            a.plan = plan + t.p_base;
            bind_entries(a, dev, pe);
            a.e_range = range;
            a.r0 = t.lo - s.local_first; a.key_base = key0 + (t.lo << 20); a.seats = packed;
            a.pairs = t.rooms * n_seats; a.seg = t.seg; a.n_seats = n_seats; a.cap = t.cap;
            a.e_base = t.e_base; a.a_base = t.a_base;
            a.turn = turn; a.n_rollouts = n_rollouts; a.full_view = (flags & GE_ADVISE_FULL_VIEW) ? 1u : 0u;
            HIP_TRY(teach_launch(s.dev.kind, dim3((a.pairs + 63u) / 64u), st, b, a));
            b->launches++;
            slots = t.e_base + a.pairs * t.cap;
        }
        HIP_TRY(hipMemsetAsync(dev + pe.o.acc, 0, 8 * (size_t)ROLL_STRIDE * slots, st));
        for (const TeachPart &t : parts) {                    // 2. the playouts, on the grid of every slot: a dead slot's wavefronts leave at once
            if (t.pass != p) continue;
            const uint32_t n = t.rooms * n_seats * t.cap;
            const PlayoutUnit u{t.seg, 0u, 0u, t.e_base, n, p};
            RollArgs<4> ra = rollout_form_args<4>(unit_rollout_args(b, dev, pe, u, n, seed, n_rollouts, max_turns), dev, pe.o, t.e_base);
            ra.range = range + t.e_base;
            HIP_TRY(rollout_launch_counted(b, st, ra));
            b->launches++;
        }
        for (const TeachPart &t : parts) {                    // 3. the advice records, where the caller wants them
            if (t.pass != p) continue;
            const uint32_t kind = b->segs[t.seg].dev.kind;
            TeachReduceArgs a;
            a.plan = plan + t.p_base;
            a.acc = reinterpret_cast<const unsigned long long *>(dev + pe.o.acc) + (size_t)ROLL_STRIDE * t.e_base;
            a.out = reinterpret_cast<u32x4 *>(out_dev + (size_t)(t.lo - first) * n_seats);
            a.seats = packed;
            a.pairs = t.rooms * n_seats; a.n_seats = n_seats; a.cap = t.cap; a.by_score = (kind == K_WW8 || kind == K_WW12) ? 0u : 1u;
            HIP_TRY(teach_launch(dim3((a.pairs + 63u) / 64u), st, a));
            b->launches++;
        }
    }
    if (e1) HIP_TRY(hipEventRecord(e1, st));
    return GE_OK;
}

extern "C" {

int ge_batch_teach_seats(ge_batch *b, uint64_t first, uint64_t count, uint32_t n_seats, const uint32_t *seats, const uint64_t *keys_dev, uint64_t key0,
                         uint32_t turn, uint32_t n_rollouts, uint32_t max_turns, uint64_t seed, uint32_t flags, ge_advice *out_dev, size_t cap_bytes,
                         void *hip_stream) {
    if (!b) return GE_ERR_ARG;
    // all before anything is launched, in this order (ABI behaviour): the flags and ge_batch_advise_seats's caps, env_check's checks
    // in its order with keys_dev vetted as out_dev is, the turn range, the cost cap; then nothing to do
    if (flags & ~(uint32_t)GE_ADVISE_FULL_VIEW) return GE_ERR_ARG;
    if (n_rollouts == 0 || n_rollouts > (1u << 20) || max_turns > 4096u) return GE_ERR_ARG;
    return guarded([&] {
        uint64_t packed = 0;
        bool go = false;
        const int rc = env_check(b, first, count, n_seats, seats, out_dev, sizeof(ge_advice), nullptr, 0, cap_bytes, &packed, &go);
        if (rc != GE_OK) return rc;
        if (go && keys_dev && !env_reachable(b, keys_dev, (size_t)count * sizeof(uint64_t))) return (int)GE_ERR_ARG;
        if ((uint64_t)turn + max_turns > 0xFFFFFFFFull) return (int)GE_ERR_RANGE;
        uint64_t cost = 0;                                    // ge_batch_advise_seats's cap and reservation, per pair
        for (const Segment &s : b->segs) {
            const uint64_t lo = std::max(first, s.local_first), hi = std::min(first + count, s.local_first + s.dev.rooms);
            if (lo >= hi || n_seats == 0u) continue;
            const uint64_t per_room = (uint64_t)n_seats * (playout_max_cands(s.dev) + 1u) * n_rollouts;   // < 2^28
            if (hi - lo > (1ull << 26) / per_room) return (int)GE_ERR_ARG;
            cost += (hi - lo) * per_room;
            if (cost > (1ull << 26)) return (int)GE_ERR_ARG;
        }
        if (!go) return (int)GE_OK;
        return teach_seats_impl(b, first, count, n_seats, packed, keys_dev, key0, turn, n_rollouts, max_turns, seed, flags, out_dev,
                                static_cast<hipStream_t>(hip_stream));
    });
}

}  // extern "C"

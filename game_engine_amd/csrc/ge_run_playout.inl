// ge_run_playout.inl — listed rooms with playout seats played on until a person is needed (ge_batch_run_rooms_playout, POLICY.md
// §3g): ge_batch_step_rooms_playout turn after turn without the host in between (included at the end of ge_step.hip, behind
// ge_run.inl: the existing kernels keep their code-object offsets).  Everything a turn does is other files' code: the checks, the
// grouping and the staging are ge_pool.inl's and ge_run.inl's (pool_check_entries, PoolEntries, run_check), the units and passes,
// the plan of a room, the decision and the host side of a pass - its entry block, the kernels' arguments, the rounds of §3h - are
// ge_playout.inl's (playout_units, playout_plan_room, ge_playout_decide, PassEntries .. play_unit), the playout is ge_rollout.inl's
// (roll_ww / roll_tt, ACT = 2), the turn with its trace store and its stop tests is ge_run.inl's (run_ww / run_tt with one turn to
// play, run_args), and so is the decoding of the trace plane (run_counts, run_decode).  What this file adds is the form in
// which they follow each other on the stream: three thin kernels that take what the host used to know from device memory.
//
// Per listed room, in device memory between the launches: its next turn (`cur`, the uploaded turns, counted up), a live flag, and
// (played, stop bits) once it has stopped.  Per turn t the host enqueues, for the units of each pass in turn:
//   1. ge_runp_plan: ge_playout_plan's room, for a live room at turn cur[k]; a stopped room plans no entries.  The unit takes its
//      entries from counter (unit, t) - zeroed at upload, so no counter is ever reset - and each planning lane zeroes the
//      accumulators of the entries it has just taken (40 16-byte stores per entry), instead of a memset over the unit's capacity.
//   2. ge_runp_rollout: the playouts of the unit's entries, their number read from counter (unit, t) on the device.  A block
//      strides over the (entry, 64 replicas) pairs up to count x waves; a block beyond that leaves before it touches anything.  The
//      same kernel serves both grid shapes the probe compares: a fixed grid (RUNP_GRID_BLOCKS) and one block per pair of the unit's
//      capacity.
//   3. ge_playout_decide, unchanged: a room without entries (every stopped room) is skipped; the decided mask and the choice
//      nibbles go to the turn's row of a plane of their own (16 B per room-turn, turn-major, zeroed), ORed into the events on the host.
// and then, per segment present,
//   4. ge_runp_turn: ge_run_kernel's lane with max_turns = 1 - recycle, turn, trace slot (row t of the plane), stop tests, record
//      stored without a prepared deal - for the live rooms; a stopped room's lane is a shadow exactly as a lane past the list is.
//      Behind it the lane updates its room: cur + 1, and either (t + 1, stop bits) with the live flag cleared, or one more in the
//      live count of turn t.
// The host enqueues turns in groups of RUNP_GROUP and reads one live count (4 bytes) between groups: ceil(max played / G) waits plus
// the first sync and the copy back (the counts, then the rows of the turns somebody played; one round trip when they are few),
// whatever n is.  Turns enqueued behind the last live room's stop cost their launches only: every
// block leaves at its first test.

namespace {

constexpr uint32_t RUNP_GROUP = 8;             // turns enqueued between two reads of the live count (profiles/run_playout_probe.txt)
constexpr uint32_t RUNP_GRID_BLOCKS = 8192;    // the fixed playout grid: 8 wavefronts per SIMD of 256 CUs

// what a room carries from turn to turn (sorted positions of one launch's rooms)
struct RunpRooms {
    uint32_t *live;            // 1 while the room plays on
    uint32_t *cur;             // its next turn
    u32x2 *fin;                // (played, stop bits), written when it stops
    uint32_t *live_cnt;        // [max_turns]: rooms still live after turn t (zeroed at upload)
    uint32_t t, max_turns;
};

// HALVE (GE_PLAYOUT_HALVING, POLICY.md §3h): each entry taken also gets round 0's replica range
template <int KIND, bool HALVE>
__device__ __forceinline__ void runp_plan_lane(const SegDev *__restrict__ segs, const DevTable *__restrict__ tables, const PlanArgs &a,
                                               const uint32_t *__restrict__ live, u32x4 *acc, u32x2 *e_range, uint32_t n_rollouts) {
    const uint32_t k = blockIdx.x * 64u + threadIdx.x;
    if (k >= a.n) return;
    if (live[k] == 0u) { a.room_cnt[k] = 0u; return; }
    const SegDev &sg = segs[a.seg];
    playout_plan_room<KindOf<KIND>::NB, KindOf<KIND>::WW, HALVE>(sg, tables, a, k, e_range, n_rollouts);
    const uint32_t cnt = a.room_cnt[k];                       // the entries this lane has just taken start from zero
    u32x4 *z = acc + (size_t)a.room_first[k] * (ROLL_STRIDE / 2u);
    u32x4 zero; zero.x = 0u; zero.y = 0u; zero.z = 0u; zero.w = 0u;
    for (uint32_t j = 0; j < cnt * (ROLL_STRIDE / 2u); j++) z[j] = zero;
}

template <int KIND>
__global__ void __launch_bounds__(64) ge_runp_plan(const SegDev *__restrict__ segs, const DevTable *__restrict__ tables, const PlanArgs a,
                                                   const uint32_t *__restrict__ live, u32x4 *acc) {
    runp_plan_lane<KIND, false>(segs, tables, a, live, acc, nullptr, 0u);
}
template <int KIND>
__global__ void __launch_bounds__(64) ge_runp_plan_ranged(const SegDev *__restrict__ segs, const DevTable *__restrict__ tables, const PlanArgs a,
                                                          const uint32_t *__restrict__ live, u32x4 *acc, u32x2 *e_range, uint32_t n_rollouts) {
    runp_plan_lane<KIND, true>(segs, tables, a, live, acc, e_range, n_rollouts);
}

// ge_rollout_kernel<.., ACT = 2> with the number of entries taken from device memory
template <int KIND, int GENERIC>
__global__ void __launch_bounds__(64) ge_runp_rollout(const SegDev *__restrict__ segs, const DevTable *__restrict__ tables, const RollArgs<2> a,
                                                      const uint32_t *__restrict__ count) {
    __shared__ unsigned long long part[ROLL_FIELDS];
    __shared__ uint32_t h_end[16], h_score[16];
    const SegDev &sg = segs[a.seg];
    const uint32_t pairs = (uint32_t)__builtin_amdgcn_readfirstlane(*count) * a.waves;   // <= 65536 entries x 2^14 wavefronts
    void *lw = ge_lds;
    for (uint32_t x = blockIdx.x; x < pairs; x += gridDim.x) {
        const uint32_t e = x / a.waves, r = (x - e * a.waves) * 64u + threadIdx.x;
        if (threadIdx.x < ROLL_FIELDS) part[threadIdx.x] = 0;
        if (threadIdx.x < 16) { h_end[threadIdx.x] = 0; h_score[threadIdx.x] = 0; }
        __syncthreads();
        if constexpr (KindOf<KIND>::WW) roll_ww<KindOf<KIND>::NB, GENERIC, 2>(sg, tables, a, lw, e, r, part, h_end, h_score);
        else roll_tt<KindOf<KIND>::NB, GENERIC, 2>(sg, tables, a, lw, e, r, part, h_end, h_score);
        __syncthreads();                                      // the reduction has read `part` before the next pair clears it
    }
}

// ge_rollout_kernel<.., ACT = 4> in the same shape: one round of §3h over the entries' replica ranges, `waves` that round's.  A
// copy of the loop above and not a shared body: with the loop in a function of both (by reference or by value) the compiler
// emits other instructions for the unflagged kernel, which has to stay as it was
template <int KIND, int GENERIC>
__global__ void __launch_bounds__(64) ge_runp_rollout_ranged(const SegDev *__restrict__ segs, const DevTable *__restrict__ tables, const RollArgs<4> a,
                                                             const uint32_t *__restrict__ count) {
    __shared__ unsigned long long part[ROLL_FIELDS];
    __shared__ uint32_t h_end[16], h_score[16];
    const SegDev &sg = segs[a.seg];
    const uint32_t pairs = (uint32_t)__builtin_amdgcn_readfirstlane(*count) * a.waves;
    void *lw = ge_lds;
    for (uint32_t x = blockIdx.x; x < pairs; x += gridDim.x) {
        const uint32_t e = x / a.waves, r = (x - e * a.waves) * 64u + threadIdx.x;
        if (threadIdx.x < ROLL_FIELDS) part[threadIdx.x] = 0;
        if (threadIdx.x < 16) { h_end[threadIdx.x] = 0; h_score[threadIdx.x] = 0; }
        __syncthreads();
        if constexpr (KindOf<KIND>::WW) roll_ww<KindOf<KIND>::NB, GENERIC, 4>(sg, tables, a, lw, e, r, part, h_end, h_score);
        else roll_tt<KindOf<KIND>::NB, GENERIC, 4>(sg, tables, a, lw, e, r, part, h_end, h_score);
        __syncthreads();
    }
}

// one turn of the live rooms of a segment: ge_run_kernel's lane with one turn to play, then the room's state
template <int KIND, int GENERIC>
__global__ void __launch_bounds__(64) ge_runp_turn(const SegDev *__restrict__ segs, const DevTable *__restrict__ tables, const RunArgs a, const RunpRooms x) {
    const SegDev &sg = segs[a.seg];
    const uint32_t k = blockIdx.x * 64u + threadIdx.x;
    const bool mine = k < a.n && x.live[k] != 0u;
    if (__ballot(mine) == 0ull) return;                       // no live room in this wavefront
    void *lw = ge_lds;
    const uint32_t k_in = mine ? k : 0xFFFFFFFFu;             // a stopped room's lane is a lane past the list: a shadow
    if constexpr (KindOf<KIND>::WW) run_ww<KindOf<KIND>::NB, GENERIC>(sg, tables, a, lw, k_in);
    else run_tt<KindOf<KIND>::NB, GENERIC>(sg, tables, a, lw, k_in);
    bool on = false;
    if (mine) {
        const u32x2 o = a.out[k];                             // (1, stop bits): what the lane has just written
        on = o.y == 0u && x.t + 1u != x.max_turns;
        x.cur[k] = x.cur[k] + 1u;
        if (!on) {
            u32x2 f; f.x = x.t + 1u; f.y = o.y;
            x.fin[k] = f;
            x.live[k] = 0u;
        }
    }
    const uint64_t still = __ballot(on);
    if (threadIdx.x == 0u && still != 0ull) atomicAdd(x.live_cnt + x.t, (uint32_t)__popcll(still));
}

hipError_t runp_launch(uint32_t kind, dim3 grid, hipStream_t st, const ge_batch *b, const PlanArgs &a, const uint32_t *live, u32x4 *acc) {
    return by_kind(kind, [&](auto K) { hipLaunchKernelGGL((ge_runp_plan<K()>), grid, dim3(64), 0, st, b->segs_dev, b->tables, a, live, acc); });
}
template <int GEN> hipError_t runp_launch(uint32_t kind, dim3 grid, hipStream_t st, const ge_batch *b, const RollArgs<2> &a, const uint32_t *count) {
    return by_kind(kind, [&](auto K) { hipLaunchKernelGGL((ge_runp_rollout<K(), GEN>), grid, dim3(64), lane_lds(kind), st, b->segs_dev, b->tables, a, count); });
}
hipError_t runp_launch(uint32_t kind, dim3 grid, hipStream_t st, const ge_batch *b, const PlanArgs &a, const uint32_t *live, u32x4 *acc, u32x2 *e_range,
                       uint32_t n_rollouts) {
    return by_kind(kind, [&](auto K) {
        hipLaunchKernelGGL((ge_runp_plan_ranged<K()>), grid, dim3(64), 0, st, b->segs_dev, b->tables, a, live, acc, e_range, n_rollouts);
    });
}
template <int GEN> hipError_t runp_launch(uint32_t kind, dim3 grid, hipStream_t st, const ge_batch *b, const RollArgs<4> &a, const uint32_t *count) {
    return by_kind(kind, [&](auto K) { hipLaunchKernelGGL((ge_runp_rollout_ranged<K(), GEN>), grid, dim3(64), lane_lds(kind), st, b->segs_dev, b->tables, a, count); });
}
template <int GEN> hipError_t runp_launch(uint32_t kind, dim3 grid, hipStream_t st, const ge_batch *b, const RunArgs &a, const RunpRooms &x) {
    return by_kind(kind, [&](auto K) { hipLaunchKernelGGL((ge_runp_turn<K(), GEN>), grid, dim3(64), lane_lds(kind), st, b->segs_dev, b->tables, a, x); });
}

// Probe-only switches, read once per process, for the A/B runs of tools/run_playout_probe.py (DESIGN.md §4 names them; neither
// changes a result): GE_RUNP_GROUP = turns per group, 1 .. 64 (anything else: RUNP_GROUP); GE_RUNP_GRID = 1 the capacity grid
// instead of the fixed striding grid
uint32_t runp_group() {
    static const uint32_t g = [] { const char *e = getenv("GE_RUNP_GROUP"); const int v = e ? atoi(e) : 0; return v >= 1 && v <= 64 ? (uint32_t)v : RUNP_GROUP; }();
    return g;
}
bool runp_capacity_grid() {
    static const bool c = [] { const char *e = getenv("GE_RUNP_GRID"); return e && atoi(e) == 1; }();
    return c;
}

}  // namespace

static int run_playout_impl(ge_batch *b, uint64_t n, const uint64_t *rooms, const uint64_t *keys, const uint32_t *turns, const uint32_t *masks,
                            const uint64_t *pkeys, uint32_t n_rollouts, uint32_t pmax, uint64_t seed, uint32_t flags, uint32_t max_turns,
                            uint32_t until, uint32_t *played, uint32_t *stopped, uint32_t *decided, ge_turn_event *events, ge_room_view *views) {
    GE_ON_DEVICE(b);
    int st = sync_impl(b);
    if (st != GE_OK) return st;
    const PoolEntries en(b, n, rooms);
    const std::vector<uint32_t> &order = en.order;
    std::vector<PlayoutUnit> units;
    uint32_t n_pass = 0, max_cap = 0;
    playout_units(b, en, masks, units, n_pass, max_cap);
    const uint32_t n_units = (uint32_t)units.size();
    // one layout, each array from a 16 B boundary.  Upload: [rooms u64][keys u64][pkeys u64][cur u32][masks u32][live u32 = 1]
    // [fin 8 B = 0][entry counters u32 x units x max_turns = 0][live counts u32 x max_turns = 0].  Behind it what comes back - the
    // trace plane (64 B per room-turn) and the decision plane (16 B per room-turn) - and then what stays on the device: [one-turn
    // out 8 B][room_first u32][room_cnt u32] and a pass's entries
    const size_t N = (size_t)n, T = max_turns;
    const size_t o_keys = 8 * N, o_pkeys = 16 * N, o_cur = 24 * N, o_masks = up16(o_cur + 4 * N), o_live = up16(o_masks + 4 * N);
    const size_t o_fin = up16(o_live + 4 * N), o_ctr = up16(o_fin + 8 * N), o_lcnt = up16(o_ctr + 4 * (size_t)n_units * T);
    const size_t o_up_end = up16(o_lcnt + 4 * T);
    const size_t o_trace = o_up_end, o_dec = o_trace + 64 * N * T, host_total = o_dec + 16 * N * T;
    const size_t o_one = host_total, o_rfirst = up16(o_one + 8 * N), o_rcnt = up16(o_rfirst + 4 * N);
    const bool halving = (flags & GE_PLAYOUT_HALVING) != 0u;
    const PassEntries pe(up16(o_rcnt + 4 * N), max_cap, halving);
    uint32_t *host32 = nullptr;
    if ((st = io_stage(b, host_total, &host32)) != GE_OK) return st;
    unsigned char *host = reinterpret_cast<unsigned char *>(host32);
    en.stage(b, rooms, keys, turns, host, o_keys, o_cur);
    uint64_t *h_pkeys = reinterpret_cast<uint64_t *>(host + o_pkeys);
    uint32_t *h_masks = reinterpret_cast<uint32_t *>(host + o_masks), *h_live = reinterpret_cast<uint32_t *>(host + o_live);
    for (size_t i = 0; i < N; i++) { h_pkeys[i] = pkeys[order[i]]; h_masks[i] = masks[order[i]]; h_live[i] = 1u; }
    memset(host + o_fin, 0, o_up_end - o_fin);
    char *dev = nullptr;
    if ((st = pool_scratch(b, pe.o.total, &dev)) != GE_OK) return st;
    hipStream_t s = b->last_stream;
    if ((st = order_after_previous(b, s)) != GE_OK) return st;
    HIP_TRY(hipMemcpyAsync(dev, host, o_up_end, hipMemcpyHostToDevice, s));
    hipEvent_t e1 = nullptr;                                      // ge_batch_kernel_time counts the launches of this call as one interval
    if ((st = timing_begin(b, s, &e1)) != GE_OK) return st;
    const PassRooms pr = pass_rooms(b, dev, o_keys, o_pkeys, o_cur, o_masks, o_rfirst, o_rcnt, flags);   // a room's turn: its `cur`
    uint32_t *d_live = reinterpret_cast<uint32_t *>(dev + o_live), *d_cur = reinterpret_cast<uint32_t *>(dev + o_cur);
    const uint32_t G = runp_group();
    uint32_t t_end = 0;                                           // turns enqueued
    while (t_end < max_turns) {
        const uint32_t g_end = std::min<uint64_t>(max_turns, (uint64_t)t_end + G);
        HIP_TRY(hipMemsetAsync(dev + o_dec + 16 * N * t_end, 0, 16 * N * (g_end - t_end), s));
        for (uint32_t t = t_end; t < g_end; t++) {
            for (uint32_t p = 0; p < n_pass; p++) {
                for (const PlayoutUnit &u : units) {              // 1. plan
                    if (u.pass != p) continue;
                    const PlanArgs a = plan_args(pr, u, reinterpret_cast<uint32_t *>(dev + o_ctr) + (size_t)(&u - units.data()) * T + t, dev, pe);
                    const dim3 grid((u.cnt + 63u) / 64u);
                    u32x4 *acc = reinterpret_cast<u32x4 *>(dev + pe.o.acc);
                    HIP_TRY(halving ? runp_launch(b->segs[u.seg].dev.kind, grid, s, b, a, d_live + u.lo, acc, reinterpret_cast<u32x2 *>(dev + pe.range), n_rollouts)
                                    : runp_launch(b->segs[u.seg].dev.kind, grid, s, b, a, d_live + u.lo, acc));
                }
                for (const PlayoutUnit &u : units) {              // 2. the playouts, their number read on the device
                    if (u.pass != p) continue;
                    const uint32_t *cnt = reinterpret_cast<const uint32_t *>(dev + o_ctr) + (size_t)(&u - units.data()) * T + t;
                    const uint32_t kind = b->segs[u.seg].dev.kind;
                    const auto launch = [&](const auto &ra) {     // the unit's capacity in pairs is <= 2^26: the cost cap
                        const uint64_t cap_pairs = (uint64_t)ra.n * ra.waves;
                        const dim3 grid((uint32_t)(runp_capacity_grid() ? cap_pairs : std::min<uint64_t>(cap_pairs, RUNP_GRID_BLOCKS)));
                        return b->plan.generic ? runp_launch<1>(kind, grid, s, b, ra, cnt) : runp_launch<0>(kind, grid, s, b, ra, cnt);
                    };
                    HIP_TRY(play_unit(b, s, dev, pe, pr, u, unit_rollout_args(b, dev, pe, u, u.e_cap, seed, n_rollouts, pmax), halving, launch));
                }
                for (const PlayoutUnit &u : units) {              // 3. decide and log
                    if (u.pass != p) continue;
                    const DecideArgs a = decide_args(pr, u, reinterpret_cast<u32x4 *>(dev + o_dec) + N * t + u.lo, dev, pe);
                    HIP_TRY(playout_launch(b->segs[u.seg].dev.kind, dim3((u.cnt + 63u) / 64u), s, b, a));
                }
            }
            for (uint32_t g = 0; g < (uint32_t)b->segs.size(); g++) {   // 4. the turn, its trace row and the rooms' state
                if (en.begin[g + 1u] == en.begin[g]) continue;
                const RunArgs a = run_args(b, en, g, dev, o_keys, o_cur, o_trace + 64 * N * t, o_one, 1u, until);
                const uint32_t lo = a.first;
                RunpRooms x;
                x.live = d_live + lo; x.cur = d_cur + lo;
                x.fin = reinterpret_cast<u32x2 *>(dev + o_fin) + lo;
                x.live_cnt = reinterpret_cast<uint32_t *>(dev + o_lcnt);
                x.t = t; x.max_turns = max_turns;
                const dim3 grid((a.n + 63u) / 64u);
                const uint32_t kind = b->segs[g].dev.kind;
                HIP_TRY(b->plan.generic ? runp_launch<1>(kind, grid, s, b, a, x) : runp_launch<0>(kind, grid, s, b, a, x));
            }
        }
        t_end = g_end;
        if (t_end == max_turns) break;                            // every room has stopped by now
        uint32_t *h_left = reinterpret_cast<uint32_t *>(host + o_lcnt);
        HIP_TRY(hipMemcpyAsync(h_left, dev + o_lcnt + 4 * (size_t)(t_end - 1u), 4, hipMemcpyDeviceToHost, s));
        if ((st = sync_impl(b)) != GE_OK) {
            if (e1) (void)hipEventRecord(e1, s);                 // the timing pair is taken: ge_batch_kernel_time must find it recorded
            return st;
        }
        if ((st = order_after_previous(b, s)) != GE_OK) return st;
        if (*h_left == 0u) break;
    }
    if (e1) HIP_TRY(hipEventRecord(e1, s));
    // the turn counts first: only the rows of turns somebody played are copied - unless the rows enqueued are few bytes, which then
    // come back with the counts in one round trip (as run_rooms_impl does it)
    const bool rows = events || views || decided;
    const bool whole = 80 * N * t_end <= RUN_ONE_COPY;
    HIP_TRY(hipMemcpyAsync(host + o_fin, dev + o_fin, 8 * N, hipMemcpyDeviceToHost, s));
    if (rows && whole) {
        HIP_TRY(hipMemcpyAsync(host + o_trace, dev + o_trace, 64 * N * t_end, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(host + o_dec, dev + o_dec, 16 * N * t_end, hipMemcpyDeviceToHost, s));
    }
    if ((st = sync_impl(b)) != GE_OK) return st;
    std::vector<uint64_t> prefix;
    const uint32_t rows_played = run_counts(en, reinterpret_cast<const uint32_t *>(host + o_fin), played, stopped, prefix);
    if (rows && !whole) {
        if ((st = order_after_previous(b, s)) != GE_OK) return st;
        HIP_TRY(hipMemcpyAsync(host + o_trace, dev + o_trace, 64 * N * rows_played, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(host + o_dec, dev + o_dec, 16 * N * rows_played, hipMemcpyDeviceToHost, s));
        if ((st = sync_impl(b)) != GE_OK) return st;
    }
    if (rows)
        run_decode(b, en, max_turns, prefix, reinterpret_cast<const uint32_t *>(host + o_trace), reinterpret_cast<const uint32_t *>(host + o_dec), events,
                   views, decided);
    return GE_OK;
}

extern "C" {

int ge_batch_run_rooms_playout(ge_batch *b, uint64_t n, const uint64_t *rooms, const uint64_t *keys, const uint32_t *turns,
                               const uint32_t *playout_masks, const uint64_t *playout_keys, uint32_t n_rollouts, uint32_t playout_max_turns,
                               uint64_t seed, uint32_t flags, uint32_t max_turns, uint32_t until, uint32_t *played, uint32_t *stopped,
                               uint32_t *decided, ge_turn_event *events, ge_room_view *views, size_t views_cap_bytes) {
    if (!b) return GE_ERR_ARG;
    if (n != 0) {                                                 // ge_batch_run_rooms's checks, in its order
        const int st = run_check(b, n, rooms, keys, turns, max_turns, until, played, views, views_cap_bytes);
        if (st != GE_OK) return st;
    }
    // then ge_batch_step_rooms_playout's; the last turn's playouts must fit the turn range
    const int pst = playout_check(b, n, rooms, turns, playout_masks, playout_keys, n_rollouts, playout_max_turns, flags, n ? max_turns - 1u : 0u);
    if (pst != GE_OK) return pst;
    if (n == 0) return GE_OK;
    return guarded([&] {
        return run_playout_impl(b, n, rooms, keys, turns, playout_masks, playout_keys, n_rollouts, playout_max_turns, seed, flags, max_turns, until,
                                played, stopped, decided, events, views);
    });
}

}  // extern "C"

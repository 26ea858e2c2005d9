// ge_timeline.inl — a run-on with a forecast of every turn (ge_batch_run_rooms_forecast, POLICY.md §3i): ge_batch_run_rooms, and
// for point p = 0 .. played[k] of entry k the ge_batch_rollout_seats entry of the room as it stood at that point (included at the
// end of ge_step.hip, behind ge_run_playout.inl: the existing kernels keep their code-object offsets).  Everything a point does is
// other files' code: the checks, the grouping and the staging are ge_pool.inl's and ge_run.inl's (PoolEntries, run_check), the run
// is ge_run.inl's kernel, unchanged, with its decoding of the trace plane (run_counts, run_decode), the playouts are
// ge_rollout.inl's (ACT = 2 for point 0, ACT = 5 for the traced turns).  What this file adds is the order on the stream and the
// accumulator plane.
//
// The run leaves only its last record in the room, but every turn's record lies in its trace plane on the device.  So, on one
// stream and without a host wait in between:
//   1. point 0: the seat-view playouts (ACT = 2, empty action lists) of the listed rooms as they stand, into row 0 of the plane;
//   2. the run: ge_run_kernel into the call's trace plane and its (played, stop bits);
//   3. points 1 .. max_turns: the playouts from a traced turn (ACT = 5), one block per (turn, entry, 64 replicas); a block of a
//      turn its entry did not play reads the run's turn count and leaves.
// One launch per segment present in each of the three.
//
// Accumulator plane: ROLL_STRIDE words per point, turn-major like the trace plane - row p * n + i for point p of sorted entry i -
// zeroed by a fill on the stream; the rows of the points anybody reached are one contiguous block from its start, so the host
// copies max(played) + 1 rows of it and max(played) rows of the trace plane, after the turn counts (one round trip when both
// planes are small, as run_rooms_impl has it).

namespace {

constexpr uint32_t TIMELINE_MAX_POINTS = 1u << 16;   // 640 B of accumulators per point

}  // namespace

// ge_batch_run_rooms_forecast's own checks, behind run_check (made for n == 0 too, as ge_batch_run_rooms_playout's are)
static int timeline_check(const ge_batch *b, uint64_t n, const uint64_t *rooms, const uint32_t *turns, uint32_t max_turns, const uint64_t *forecast_keys,
                          const uint32_t *seats, uint32_t n_rollouts, uint32_t pmax, const ge_rollout_stats *stats, size_t stats_cap_bytes) {
    const uint64_t points = n * ((uint64_t)max_turns + 1u);
    if (!forecast_keys || !stats || stats_cap_bytes / sizeof(ge_rollout_stats) < points) return GE_ERR_ARG;
    if (n_rollouts == 0u || n_rollouts > (1u << 20) || pmax > 4096u) return GE_ERR_ARG;
    if (points > TIMELINE_MAX_POINTS || points * n_rollouts > (1ull << 26)) return GE_ERR_ARG;
    if (seats)
        for (uint64_t k = 0; k < n; k++)                          // (rooms[k] is in range: its segment is known)
            if (seats[k] > b->segs[pool_segment_of(b, rooms[k])].dev.n_players) return GE_ERR_ARG;
    for (uint64_t k = 0; k < n; k++)
        if ((uint64_t)turns[k] + max_turns + pmax > 0xFFFFFFFFull) return GE_ERR_RANGE;
    return GE_OK;
}

static int run_forecast_impl(ge_batch *b, uint64_t n, const uint64_t *rooms, const uint64_t *keys, const uint32_t *turns, uint32_t max_turns,
                             uint32_t until, const uint64_t *fkeys, const uint32_t *seats, uint32_t n_rollouts, uint32_t pmax, uint64_t seed,
                             uint32_t *played, uint32_t *stopped, ge_turn_event *events, ge_room_view *views, ge_rollout_stats *stats) {
    GE_ON_DEVICE(b);
    int st = sync_impl(b);
    if (st != GE_OK) return st;
    const PoolEntries en(b, n, rooms);
    const std::vector<uint32_t> &order = en.order;
    // one upload, each array from a 16 B boundary: [rooms u64][keys u64][turns u32][forecast keys u64][seats u32][first_action u32 x
    // (n + 1) = 0][status i32 = 0]; then what comes back: [played, stopped] x n, the trace plane, the accumulator plane
    const size_t N = (size_t)n, T = max_turns;
    const size_t o_keys = 8 * N, o_turns = 16 * N, o_fkeys = up16(o_turns + 4 * N), o_seats = o_fkeys + 8 * N, o_first = up16(o_seats + 4 * N);
    const size_t o_status = up16(o_first + 4 * (N + 1u)), o_up_end = up16(o_status + 4 * N);
    const size_t o_out = o_up_end, o_trace = up16(o_out + 8 * N), trace_row = 64 * N, acc_row = 8 * (size_t)ROLL_STRIDE * N;
    const size_t o_acc = o_trace + trace_row * T, total = o_acc + acc_row * (T + 1u);
    uint32_t *host32 = nullptr;
    if ((st = io_stage(b, total, &host32)) != GE_OK) return st;
    unsigned char *host = reinterpret_cast<unsigned char *>(host32);
    en.stage(b, rooms, keys, turns, host, o_keys, o_turns);
    uint64_t *h_fkeys = reinterpret_cast<uint64_t *>(host + o_fkeys);
    uint32_t *h_seats = reinterpret_cast<uint32_t *>(host + o_seats);
    for (size_t i = 0; i < N; i++) { h_fkeys[i] = fkeys[order[i]]; h_seats[i] = seats ? seats[order[i]] : 0u; }
    memset(host + o_first, 0, o_up_end - o_first);
    char *dev = nullptr;
    if ((st = pool_scratch(b, total, &dev)) != GE_OK) return st;
    hipStream_t s = b->last_stream;
    if ((st = order_after_previous(b, s)) != GE_OK) return st;
    HIP_TRY(hipMemcpyAsync(dev, host, o_up_end, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(dev + o_acc, 0, acc_row * (T + 1u), s));
    hipEvent_t e1 = nullptr;                                      // ge_batch_kernel_time counts the launches of this call as one interval
    if ((st = timing_begin(b, s, &e1)) != GE_OK) return st;
    const uint32_t n_seg = (uint32_t)b->segs.size();
    const uint32_t seed_f = seed_key((uint32_t)seed, (uint32_t)(seed >> 32));
    const uint32_t waves = (n_rollouts + 63u) / 64u;
    // the playout arguments of segment g's entries [lo, lo + cnt): forecast keys, first turns, seats; no actions
    auto roll_args = [&](uint32_t g, uint32_t lo, uint32_t cnt, auto &a) {
        a.rooms = reinterpret_cast<const uint64_t *>(dev) + lo;
        a.keys = reinterpret_cast<const uint64_t *>(dev + o_fkeys) + lo;
        a.turns = reinterpret_cast<const uint32_t *>(dev + o_turns) + lo;
        a.n = cnt; a.seg = g; a.seed_key = seed_f; a.n_rollouts = n_rollouts; a.max_turns = pmax; a.waves = waves;
        a.settle_mask = rollout_settle_mask(b->segs[g]);
        a.first_action = reinterpret_cast<const uint32_t *>(dev + o_first) + lo;
        a.players = a.choices = reinterpret_cast<const uint32_t *>(dev + o_first);   // (every list is empty: never read)
        a.status = reinterpret_cast<int32_t *>(dev + o_status) + lo;
        a.seats = reinterpret_cast<const uint32_t *>(dev + o_seats) + lo;
    };
    for (uint32_t g = 0; g < n_seg; g++) {                        // 1. point 0, from the batch records
        const uint32_t lo = en.begin[g], cnt = en.begin[g + 1u] - lo;
        if (!cnt) continue;
        RollArgs<2> a;
        roll_args(g, lo, cnt, a);
        a.acc = reinterpret_cast<unsigned long long *>(dev + o_acc) + (size_t)ROLL_STRIDE * lo;
        const dim3 grid(cnt * waves);
        const uint32_t kind = b->segs[g].dev.kind;
        HIP_TRY((b->plan.generic ? rollout_launch<1, 2>(kind, grid, s, b, a) : rollout_launch<0, 2>(kind, grid, s, b, a)));
    }
    for (uint32_t g = 0; g < n_seg; g++) {                        // 2. the run
        if (en.begin[g + 1u] == en.begin[g]) continue;
        const RunArgs a = run_args(b, en, g, dev, o_keys, o_turns, o_trace, o_out, max_turns, until);
        const dim3 grid((a.n + 63u) / 64u);
        HIP_TRY(b->plan.generic ? run_launch<1>(b->segs[g].dev.kind, grid, s, b, a) : run_launch<0>(b->segs[g].dev.kind, grid, s, b, a));
    }
    for (uint32_t g = 0; g < n_seg; g++) {                        // 3. points 1 .. max_turns, from the trace plane
        const uint32_t lo = en.begin[g], cnt = en.begin[g + 1u] - lo;
        if (!cnt) continue;
        RollArgs<5> a;
        roll_args(g, lo, cnt, a);
        a.rooms = nullptr;
        a.acc = reinterpret_cast<unsigned long long *>(dev + o_acc) + (size_t)ROLL_STRIDE * (N + lo);   // row 1 of the plane
        a.trace = reinterpret_cast<const u32x4 *>(dev + o_trace);
        a.run_out = reinterpret_cast<const u32x2 *>(dev + o_out) + lo;
        a.n_all = (uint32_t)n; a.first = lo;
        const dim3 grid(cnt * max_turns * waves);                // <= 2^26 / 64 + 2^16 blocks (the caps on the points)
        const uint32_t kind = b->segs[g].dev.kind;
        HIP_TRY((b->plan.generic ? rollout_launch<1, 5>(kind, grid, s, b, a) : rollout_launch<0, 5>(kind, grid, s, b, a)));
    }
    if (e1) HIP_TRY(hipEventRecord(e1, s));
    // the turn counts first: only the rows of the turns somebody played are copied - unless both planes are small
    const bool whole = total - o_trace <= RUN_ONE_COPY;
    HIP_TRY(hipMemcpyAsync(host + o_out, dev + o_out, whole ? total - o_out : o_trace - o_out, hipMemcpyDeviceToHost, s));
    if ((st = sync_impl(b)) != GE_OK) return st;
    std::vector<uint64_t> prefix;                                // played turns in front of sorted entry i
    const uint32_t rows_played = run_counts(en, reinterpret_cast<const uint32_t *>(host + o_out), played, stopped, prefix);
    if (!whole) {
        if ((st = order_after_previous(b, s)) != GE_OK) return st;
        if (events || views) HIP_TRY(hipMemcpyAsync(host + o_trace, dev + o_trace, trace_row * rows_played, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(host + o_acc, dev + o_acc, acc_row * (rows_played + 1u), hipMemcpyDeviceToHost, s));
        if ((st = sync_impl(b)) != GE_OK) return st;
    }
    if (events || views)
        run_decode(b, en, max_turns, prefix, reinterpret_cast<const uint32_t *>(host + o_trace), nullptr, events, views, nullptr);
    const unsigned long long *h_acc = reinterpret_cast<const unsigned long long *>(host + o_acc);
    for (size_t i = 0; i < N; i++) {                              // scattered back into input order
        const size_t k = order[i];
        for (uint32_t p = 0; p <= played[k]; p++)
            rollout_stats_from(h_acc + (size_t)ROLL_STRIDE * (p * N + i), n_rollouts, (uint64_t)turns[k] + p + pmax, stats[k * (T + 1u) + p]);
    }
    return GE_OK;
}

extern "C" {

int ge_batch_run_rooms_forecast(ge_batch *b, uint64_t n, const uint64_t *rooms, const uint64_t *keys, const uint32_t *turns, uint32_t max_turns,
                                uint32_t until, const uint64_t *forecast_keys, const uint32_t *seats, uint32_t n_rollouts, uint32_t playout_max_turns,
                                uint64_t seed, uint32_t *played, uint32_t *stopped, ge_turn_event *events, ge_room_view *views, size_t views_cap_bytes,
                                ge_rollout_stats *stats, size_t stats_cap_bytes) {
    if (!b) return GE_ERR_ARG;
    if (n != 0) {                                                 // ge_batch_run_rooms's checks, in its order
        const int st = run_check(b, n, rooms, keys, turns, max_turns, until, played, views, views_cap_bytes);
        if (st != GE_OK) return st;
    }
    const int fst = timeline_check(b, n, rooms, turns, max_turns, forecast_keys, seats, n_rollouts, playout_max_turns, stats, stats_cap_bytes);
    if (fst != GE_OK) return fst;
    if (n == 0) return GE_OK;
    return guarded([&] {
        return run_forecast_impl(b, n, rooms, keys, turns, max_turns, until, forecast_keys, seats, n_rollouts, playout_max_turns, seed, played,
                                 stopped, events, views, stats);
    });
}

}  // extern "C"

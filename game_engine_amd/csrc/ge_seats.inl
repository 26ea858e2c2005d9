// ge_seats.inl — each room's own host-driven seats (ge_batch_set_seats / get_seats / clear_seats, POLICY.md §3l) and the
// whole-batch step of a batch that has them (included at the end of ge_step.hip, behind ge_find.inl: the existing kernels keep
// their code-object offsets; it needs ge_batch's internals).
//
// The reference runs one thread per room and who sits where is that room's own business (src/app/api/copilotkit/route.ts:24-37);
// a segment's human_mask fixes it for all rooms of the segment at ge_batch_create.  The seat plane lifts that: uint16_t[n_rooms]
// in batch-local room order beside the records (ge_batch::seats) with a host mirror (ge_batch::seats_host), allocated by the
// first ge_batch_set_seats and filled with the segments' masks.  It is configuration, not game state: no kernel but
// ge_seats_fill / ge_seats_scatter writes it, and reset, set_turn, record writes and restarts leave it alone.
//
// Who reads it: the indexed lane (ge_pool.inl lane_seat_mask - the plane pointer, possibly null, is an argument of ge_pool_kernel,
// ge_run_kernel / ge_runp_turn and ge_find_kernel) and ge_seat_step_kernel below.  The flagship step kernels (ge_kernels.inl) never
// see it: a batch with a plane does not launch them.
//
// ge_seat_step_kernel<KIND, GENERIC>: ge_batch_step on a batch with a plane, one body for both games over ge_pool.inl's Lane
// (seat_lane).  ge_run_kernel's turn loop in ranged form - lane =
// room of the segment, key = the room's global index, turns turn0 .. turn0 + k - 1, no stop tests, no trace plane; the event of each
// turn goes into the segment's GE_FLAG_TRACE buffer (store_event) when the batch traces.  So room r takes exactly
// ge_batch_step_rooms's entry (r, its global index, turn) turn after turn under its own mask: the record's prepared deal is
// ignored, assignments deal on the spot, the record is stored without a deal, the Werewolf x 12 side plane is neither read nor
// written (ge_pool.inl, "Prepared role deals").  One launch per segment and per max_fuse turns, plain launches only.

namespace {

// plane[first .. first + n) = mask: a segment's rooms take its human_mask
__global__ void __launch_bounds__(256) ge_seats_fill(uint16_t *__restrict__ plane, uint64_t first, uint64_t n, uint32_t mask) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) plane[first + i] = (uint16_t)mask;
}

// plane[rooms[k]] = masks[k]: one 2-byte store per listed room (the host checked every room; distinct rooms, distinct addresses)
__global__ void __launch_bounds__(64) ge_seats_scatter(uint16_t *__restrict__ plane, uint64_t n_rooms, const uint64_t *__restrict__ rooms,
                                                       const uint32_t *__restrict__ masks, uint64_t n) {
    const uint64_t k = (uint64_t)blockIdx.x * 64u + threadIdx.x;
    if (k >= n) return;
    const uint64_t room = rooms[k];
    if (room >= n_rooms) return;
    plane[room] = (uint16_t)masks[k];
}

struct SeatStepArgs {
    const uint16_t *seats;     // the batch's seat plane
    uint32_t seg, seed_key, restart, trace;
    uint32_t turn0, n_turns;
};

template <int NB, bool WWP, int GENERIC>
__device__ __forceinline__ void seat_lane(const SegDev &sg, const DevTable *__restrict__ tables, const SeatStepArgs &a, void *lw, uint64_t room_in) {
    using Ln = Lane<NB, WWP, GENERIC>;
    using L = typename Ln::L;
    // lanes past the segment stay in the wavefront (the action queue is a wave-wide collective): they shadow room 0 and store nothing
    const bool valid = room_in < sg.rooms;
    const uint64_t room = valid ? room_in : 0u;
    uint32_t w[L::WORDS];
    load_words<L::WORDS>(sg.base, sg.rooms_padded, room, w);
    const uint32_t rk = room_key_from(a.seed_key, sg.first_global + room);
    Ln lane;                                                  // the record's prepared deal is never used (as an indexed step)
    lane.open(sg, tables, lw, w, rk, valid, lane_seat_mask(sg, a.seats, room));
    const bool trace = a.trace != 0u;
    for (uint32_t t = 0; t < a.n_turns; t++) {
        const uint32_t turn = a.turn0 + t;
        const uint32_t restarted = lane.recycle(sg, a.restart);   // every turn
        const LaneTurn ev = lane.turn(turn, trace);
        if (trace && valid) store_event(sg.trace, sg.rooms_padded, t, room, turn, ev.p, lane.phase(), restarted, ev.newly, ev.choice);
    }
    if (!valid) return;
    lane.pack(w);                                             // stored without a prepared deal
    store_words<L::WORDS>(sg.base, sg.rooms_padded, room, w);
}

// one wavefront per block; its action queue (WaveLdsLow) is the block's dynamic LDS (none for Two-Truths x 4: no queue)
template <int KIND, int GENERIC>
__global__ void __launch_bounds__(64) ge_seat_step_kernel(const SegDev *__restrict__ segs, const DevTable *__restrict__ tables, const SeatStepArgs a) {
    const SegDev &sg = segs[a.seg];
    const uint64_t room = (uint64_t)blockIdx.x * 64u + threadIdx.x;
    void *lw = ge_lds;
    seat_lane<KindOf<KIND>::NB, KindOf<KIND>::WW, GENERIC>(sg, tables, a, lw, room);
}

template <int GEN> hipError_t seat_step_launch(uint32_t kind, dim3 grid, hipStream_t st, const ge_batch *b, const SeatStepArgs &a) {
    return by_kind(kind, [&](auto K) { hipLaunchKernelGGL((ge_seat_step_kernel<K(), GEN>), grid, dim3(64), lane_lds(kind), st, b->segs_dev, b->tables, a); });
}

}  // namespace

// ge_batch_step of a batch with a seat plane (step_impl made the range checks and set the device)
static int seat_step_impl(ge_batch *b, uint32_t n_turns, hipStream_t st) {
    b->last_step_turns = n_turns;
    int ord = order_after_previous(b, st);
    if (ord != GE_OK) return ord;
    const uint32_t seed_k = seed_key((uint32_t)b->seed, (uint32_t)(b->seed >> 32));
    uint32_t left = n_turns;
    while (left) {
        const uint32_t k = left < b->max_fuse ? left : b->max_fuse;
        hipEvent_t e1 = nullptr;
        int tb = timing_begin(b, st, &e1);
        if (tb != GE_OK) return tb;
        for (uint32_t g = 0; g < (uint32_t)b->segs.size(); g++) {
            const SegDev &d = b->segs[g].dev;
            SeatStepArgs a;
            a.seats = b->seats;
            a.seg = g; a.seed_key = seed_k;
            a.restart = (b->flags & GE_FLAG_RESTART) ? 1u : 0u;
            a.trace = (b->flags & GE_FLAG_TRACE) ? 1u : 0u;
            a.turn0 = (uint32_t)b->turn; a.n_turns = k;
            const dim3 grid((uint32_t)((d.rooms + 63u) / 64u));
            HIP_TRY(b->plan.generic ? seat_step_launch<1>(d.kind, grid, st, b, a) : seat_step_launch<0>(d.kind, grid, st, b, a));
            b->launches++;
        }
        if (e1) HIP_TRY(hipEventRecord(e1, st));
        b->turn += k;
        left -= k;
    }
    return GE_OK;
}

static int set_seats_impl(ge_batch *b, uint64_t n, const uint64_t *rooms, const uint32_t *masks) {
    if (n == 0) return GE_OK;
    if (!rooms || !masks) return GE_ERR_ARG;
    int st = pool_check_rooms(b, n, rooms);                       // all-or-nothing: GE_ERR_RANGE for a room outside, then GE_ERR_ARG for a repeated one
    if (st != GE_OK) return st;
    for (uint64_t k = 0; k < n; k++)
        if ((masks[k] >> b->segs[pool_segment_of(b, rooms[k])].dev.n_players) != 0u) return GE_ERR_ARG;
    GE_ON_DEVICE(b);
    if ((st = sync_impl(b)) != GE_OK) return st;
    // one upload: [rooms u64 x n][masks u32 x n]
    const size_t off_masks = 8 * (size_t)n, total = off_masks + 4 * (size_t)n;
    uint32_t *host32 = nullptr;
    if ((st = io_stage(b, total, &host32)) != GE_OK) return st;
    unsigned char *host = reinterpret_cast<unsigned char *>(host32);
    memcpy(host, rooms, 8 * (size_t)n);
    memcpy(host + off_masks, masks, 4 * (size_t)n);
    char *dev = nullptr;
    if ((st = pool_scratch(b, total, &dev)) != GE_OK) return st;
    hipStream_t s = b->last_stream;
    uint16_t *plane = b->seats;
    std::vector<uint16_t> mirror;
    if (!plane) {                                                 // the first set: the plane and its mirror, every room its segment's mask
        mirror.resize((size_t)b->n_rooms);                        // (bad_alloc: GE_ERR_NOMEM through guarded, nothing allocated yet)
        for (const Segment &sg : b->segs)
            std::fill(mirror.begin() + (size_t)sg.local_first, mirror.begin() + (size_t)(sg.local_first + sg.dev.rooms), (uint16_t)sg.dev.human_mask);
        if (hipMalloc(reinterpret_cast<void **>(&plane), 2 * (size_t)b->n_rooms) != hipSuccess) {
            (void)hipGetLastError();
            return GE_ERR_NOMEM;                                  // the batch stays without a plane, usable as before
        }
    }
    // what is left can only fail in the runtime; a plane allocated by this call is released then, so the batch keeps the state it had
    auto run = [&]() -> int {
        if (!b->seats)
            for (const Segment &sg : b->segs) {
                const uint64_t blocks = (sg.dev.rooms + 255u) / 256u;
                hipLaunchKernelGGL(ge_seats_fill, dim3((uint32_t)(blocks < 2048u ? blocks : 2048u)), dim3(256), 0, s, plane, sg.local_first, sg.dev.rooms,
                                   sg.dev.human_mask);
                HIP_TRY(hipGetLastError());
            }
        HIP_TRY(hipMemcpyAsync(dev, host, total, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(ge_seats_scatter, dim3((uint32_t)((n + 63u) / 64u)), dim3(64), 0, s, plane, b->n_rooms, reinterpret_cast<const uint64_t *>(dev),
                           reinterpret_cast<const uint32_t *>(dev + off_masks), n);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(s));
        return GE_OK;
    };
    if ((st = run()) != GE_OK) {
        if (!b->seats) (void)hipFree(plane);
        return st;
    }
    if (!b->seats) { b->seats = plane; b->seats_host.swap(mirror); }
    for (uint64_t k = 0; k < n; k++) b->seats_host[(size_t)rooms[k]] = (uint16_t)masks[k];
    return GE_OK;
}

static int clear_seats_impl(ge_batch *b) {
    if (!b->seats) return GE_OK;
    GE_ON_DEVICE(b);
    int st = sync_impl(b);                                        // a step that reads the plane may be in flight
    if (st != GE_OK) return st;
    HIP_TRY(hipFree(b->seats));
    b->seats = nullptr;
    std::vector<uint16_t>().swap(b->seats_host);
    return GE_OK;
}

extern "C" {

int ge_batch_set_seats(ge_batch *b, uint64_t n, const uint64_t *rooms, const uint32_t *masks) {
    if (!b) return GE_ERR_ARG;
    return guarded([&] { return set_seats_impl(b, n, rooms, masks); });
}

int ge_batch_get_seats(ge_batch *b, uint64_t first, uint64_t count, uint32_t *dst) {
    if (!b || (!dst && count)) return GE_ERR_ARG;
    if (first + count > b->n_rooms || first + count < first) return GE_ERR_RANGE;
    if (!b->seats_host.empty()) {
        for (uint64_t i = 0; i < count; i++) dst[i] = b->seats_host[(size_t)(first + i)];
        return GE_OK;
    }
    for (const Segment &sg : b->segs) {
        const uint64_t lo = std::max(first, sg.local_first), hi = std::min(first + count, sg.local_first + sg.dev.rooms);
        for (uint64_t r = lo; r < hi; r++) dst[r - first] = sg.dev.human_mask;
    }
    return GE_OK;
}

int ge_batch_clear_seats(ge_batch *b) {
    if (!b) return GE_ERR_ARG;
    return guarded([&] { return clear_seats_impl(b); });
}

}  // extern "C"

// ge_decide.inl — decision lists (ge_batch_gather_seats, ge_batch_act_listed; POLICY.md §3q): the (room, seat) entries of a range
// that must act or have ended, compacted in entry order into device memory the caller owns with their observations, and the way
// to play from such a list (included at the end of ge_step.hip, behind ge_run_seats.inl: the existing kernels keep their
// code-object offsets).  Both calls are compositions of ge_env.inl's calls and keep their stream contract: launched on the
// caller's stream behind the batch's earlier work, no host copy, no host wait.  Their scratch is pool_scratch, which grows only
// for a larger shape than the batch has served.
//
// ge_batch_gather_seats: ge_find.inl's three kinds of launch, none of which waits for another block, for (room, seat) pairs -
//   ge_gather_test   lane = room, the record loaded as ge_find_kernel loads it.  SEAT is Lane::pending under the mask of the listed
//                    seats (§3p: legal != 0, word for word), END is the terminal phase, under which every listed seat is due.  One
//                    word per room - bit j: entry (room, seats[j]) is due - and one due-entry count per wavefront (a __ballot and
//                    a popcount per listed seat).  One launch per segment of the range, its words padded to whole wavefronts.
//   ge_gather_scan   find_scan_block (ge_find.inl) over the wavefront counts; it also stores n_dev = {min(M, cap), M}.
//   ge_gather_emit   lane = room, one wavefront per block, one launch per segment.  A wavefront without a due entry, or whose
//                    offset lies at or beyond cap, leaves before it loads a record; a listed seat that none of its rooms has due is
//                    skipped (__ballot).  A due (room, seat) gets its record from ObsRoom (ge_env.inl) - the code of
//                    ge_observe_kernel, shared - at: the wavefront's offset + the due entries of the wavefront's earlier rooms +
//                    the rank of the seat among the room's due seats.  What lies at or beyond cap is dropped.  So the order of
//                    the list is entry order, whatever order the blocks ran in.
//                    The stores: each lane stores its own record, vector by vector as obs_columns completes them.  The other form
//                    was measured beside it on an MI355X and dropped (profiles/decisions_probe_stores.txt; numbers in
//                    include/ge_step.h): the wavefront's records of one seat staged through LDS as ge_observe_kernel's are, the
//                    destination index beside each, twelve consecutive lanes storing a record's 192 bytes - slower here, unlike
//                    there, because a list's destinations are scattered.
//
// ge_batch_act_listed: a dense choice plane (zeroed) and a dense status plane in scratch, ge_list_scatter (lane = list position,
// n = min(*n_dev, cap) read on the device), ge_act_kernel unchanged over the planes, ge_list_status (lane = list position).  A
// record is written by ge_act_kernel's lane of its room and by nothing else, whatever the list holds.

namespace {

constexpr uint32_t LIST_BLOCK = 256u;           // threads of a list kernel's block
constexpr uint32_t LIST_MAX_BLOCKS = 1u << 20;  // ... and the most blocks of one (a lane strides over the list beyond that)

struct GatherArgs {
    uint32_t *res;             // this part's due words (padded to whole wavefronts)
    uint32_t *counts;          // test: this part's wavefront counts
    const uint64_t *offsets;   // emit: this part's wavefront offsets
    u32x4 *obs;                // emit: the list's records
    uint32_t *entries;         // emit: ... and their entry indices
    const int32_t *phase_ids;  // the segment's phase id per dense row
    uint64_t r0, nr;           // the part: segment-local rooms r0 .. r0 + nr - 1
    uint64_t seats;            // nibble j = seats[j] (1-based)
    uint64_t cap;              // emit: entries the list holds
    uint32_t entry0;           // emit: the entry of the part's first room and seats[0]
    uint32_t seg, n_seats, want;
};

template <int NB, bool WWP, int GENERIC>
__device__ __forceinline__ uint32_t gather_lane(const SegDev &sg, const DevTable *__restrict__ tables, const GatherArgs &a, uint64_t room) {
    using Ln = Lane<NB, WWP, GENERIC>;
    using L = typename Ln::L;
    uint32_t w[L::WORDS];
    load_words<L::WORDS>(sg.base, sg.rooms_padded, room, w);
    uint32_t listed = 0;                                      // the listed seats: wave-uniform
    for (uint32_t j = 0; j < a.n_seats; j++) listed |= 1u << (((uint32_t)(a.seats >> (4u * j)) & 15u) - 1u);
    listed &= (1u << sg.n_players) - 1u;
    const uint32_t lst = (a.want & GE_GATHER_SEAT) ? listed : 0u;
    const uint32_t probe = Ln::probe(sg, nullptr, lst);
    Ln lane;                                                  // no turn is played: no queue, no key, nobody host-driven
    lane.open(sg, tables, nullptr, w, 0u, true, 0u);
    uint32_t due = probe != 0u ? lane.pending(lst, probe) : 0u;   // (wave-uniform)
    due |= (a.want & GE_GATHER_END) && ((lane.term_mask() >> lane.phase()) & 1u) ? listed : 0u;
    uint32_t word = 0;                                        // seat bits -> seat-list positions
    for (uint32_t j = 0; j < a.n_seats; j++) word |= ((due >> (((uint32_t)(a.seats >> (4u * j)) & 15u) - 1u)) & 1u) << j;
    return word;
}

template <int KIND, int GENERIC>
__global__ void __launch_bounds__(FIND_BLOCK) ge_gather_test(const SegDev *__restrict__ segs, const DevTable *__restrict__ tables, const GatherArgs a) {
    const SegDev &sg = segs[a.seg];
    const uint64_t k = (uint64_t)blockIdx.x * FIND_BLOCK + threadIdx.x;
    const bool valid = k < a.nr;
    const uint64_t room = a.r0 + (valid ? k : 0u);            // lanes past the part test its first room and report nothing
    uint32_t word = gather_lane<KindOf<KIND>::NB, KindOf<KIND>::WW, GENERIC>(sg, tables, a, room);
    word = valid ? word : 0u;
    uint32_t n = 0;
    for (uint32_t j = 0; j < a.n_seats; j++) n += (uint32_t)__popcll(__ballot((word >> j) & 1u));
    const uint64_t padded = (a.nr + 63u) & ~(uint64_t)63u;
    if (k < padded) {                                         // (wave-uniform: padded is a multiple of 64)
        a.res[k] = word;
        if ((threadIdx.x & 63u) == 0u) a.counts[k >> 6] = n;
    }
}

// find_scan_block, and n_dev = {entries the list gets, entries that are due}
__global__ void __launch_bounds__(FIND_SCAN_WAVES) ge_gather_scan(const uint32_t *__restrict__ counts, uint64_t n_waves, uint64_t *__restrict__ offsets,
                                                                  uint64_t cap, uint32_t *__restrict__ n_dev) {
    const uint64_t all = find_scan_block(counts, n_waves, offsets);
    if (threadIdx.x == 0u) {                                  // (all < 2^32: the host refuses a range of more entries)
        n_dev[0] = (uint32_t)(all < cap ? all : cap);
        n_dev[1] = (uint32_t)all;
    }
}

template <int KIND>
__global__ void __launch_bounds__(64) ge_gather_emit(const SegDev *__restrict__ segs, const DevTable *__restrict__ tables, const GatherArgs a) {
    const SegDev &sg = segs[a.seg];
    const uint64_t k = (uint64_t)blockIdx.x * 64u + threadIdx.x;   // (below the part's padded rooms: the grid is their wavefronts)
    const uint32_t word = a.res[k];                           // 0 past the part
    if (__ballot(word != 0u) == 0ull) return;
    const uint64_t base = a.offsets[blockIdx.x];
    if (base >= a.cap) return;                                // (wave-uniform)
    uint32_t before = 0;                                      // due entries of the wavefront's earlier rooms
    for (uint32_t j = 0; j < a.n_seats; j++) {
        const uint64_t m = __ballot((word >> j) & 1u);
        before += __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    }
    const uint64_t at0 = base + before;
    const uint64_t room = a.r0 + (k < a.nr ? k : 0u);         // lanes past the part read its first room and store nothing
    ObsRoom<KindOf<KIND>::NB, KindOf<KIND>::WW> o;
    o.open(sg, tables, a.phase_ids, room);
    auto *out = (__attribute__((address_space(1))) u32x4 *)(uintptr_t)a.obs;
    for (uint32_t j = 0; j < a.n_seats; j++) {
        const bool due = ((word >> j) & 1u) != 0u;
        if (__ballot(due) == 0ull) continue;                  // no room of the wavefront has this seat due
        const uint32_t seat = (uint32_t)(a.seats >> (4u * j)) & 15u;
        const uint64_t at = at0 + (uint32_t)__popc(word & ((1u << j) - 1u));
        const bool keep = due && at < a.cap;
        if (keep) a.entries[at] = a.entry0 + (uint32_t)k * a.n_seats + j;
        if (keep) o.record(seat, [&](int i, u32x4 v) { out[at * OBS_VEC + (uint32_t)i] = v; });
    }
}

// D[entries[i]] = choices[i] for i < min(*n, cap), entries below `total` only
__global__ void __launch_bounds__(LIST_BLOCK) ge_list_scatter(const uint32_t *__restrict__ n_dev, uint64_t cap, const uint32_t *__restrict__ entries,
                                                              const int32_t *__restrict__ choices, int32_t *__restrict__ dense, uint32_t total) {
    const uint64_t n = *n_dev < cap ? *n_dev : cap;
    for (uint64_t i = (uint64_t)blockIdx.x * LIST_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * LIST_BLOCK) {
        const uint32_t e = entries[i];
        if (e < total) dense[e] = choices[i];
    }
}

// status[i] = S[entries[i]] for i < min(*n, cap); GE_ERR_ARG for an entry at or above `total`
__global__ void __launch_bounds__(LIST_BLOCK) ge_list_status(const uint32_t *__restrict__ n_dev, uint64_t cap, const uint32_t *__restrict__ entries,
                                                             const int32_t *__restrict__ dense, int32_t *__restrict__ status, uint32_t total) {
    const uint64_t n = *n_dev < cap ? *n_dev : cap;
    for (uint64_t i = (uint64_t)blockIdx.x * LIST_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * LIST_BLOCK) {
        const uint32_t e = entries[i];
        status[i] = e < total ? dense[e] : (int32_t)GE_ERR_ARG;
    }
}

template <int GEN> hipError_t gather_test_launch(uint32_t kind, dim3 grid, hipStream_t st, const ge_batch *b, const GatherArgs &a) {
    return by_kind(kind, [&](auto K) { hipLaunchKernelGGL((ge_gather_test<K(), GEN>), grid, dim3(FIND_BLOCK), 0, st, b->segs_dev, b->tables, a); });
}
hipError_t gather_emit_launch(uint32_t kind, dim3 grid, hipStream_t st, const ge_batch *b, const GatherArgs &a) {
    return by_kind(kind, [&](auto K) { hipLaunchKernelGGL((ge_gather_emit<K()>), grid, dim3(64), 0, st, b->segs_dev, b->tables, a); });
}

dim3 list_grid(uint64_t cap) {
    const uint64_t blocks = (cap + LIST_BLOCK - 1u) / LIST_BLOCK;
    return dim3((uint32_t)std::min<uint64_t>(std::max<uint64_t>(blocks, 1u), LIST_MAX_BLOCKS));
}

}  // namespace

static_assert(GE_GATHER_SEAT == 1u && GE_GATHER_END == 2u, "want's bits");

static int gather_seats_impl(ge_batch *b, uint64_t first, uint64_t count, uint32_t n_seats, uint64_t packed, uint32_t want, ge_seat_obs *obs_dev,
                             uint32_t *entries_dev, uint64_t cap, uint32_t *n_dev, hipStream_t st) {
    GE_ON_DEVICE(b);
    // the parts of the range, a segment each; their due words padded to whole wavefronts
    struct Part { uint32_t seg; uint64_t r0, nr, lo, res_off; };
    std::vector<Part> part;
    uint64_t n_words = 0;
    for (uint32_t g = 0; g < (uint32_t)b->segs.size(); g++) {
        const Segment &s = b->segs[g];
        const uint64_t lo = std::max(first, s.local_first), hi = std::min(first + count, s.local_first + s.dev.rooms);
        if (lo >= hi) continue;
        part.push_back({g, lo - s.local_first, hi - lo, lo, n_words});
        n_words += (hi - lo + 63u) & ~(uint64_t)63u;
    }
    const uint64_t n_waves = n_words / 64u;
    // scratch: [due words][wavefront counts][wavefront offsets u64]
    const size_t off_cnt = 4 * (size_t)n_words, off_pre = up16(off_cnt + 4 * (size_t)n_waves), total = off_pre + 8 * (size_t)n_waves;
    char *dev = nullptr;
    int rc = pool_scratch(b, total, &dev);                    // grows only for a larger shape than the batch has served (may wait)
    if (rc != GE_OK) return rc;
    if ((rc = order_after_previous(b, st)) != GE_OK) return rc;
    hipEvent_t e1 = nullptr;                                  // ge_batch_kernel_time counts the launches of this call as one interval
    if ((rc = timing_begin(b, st, &e1)) != GE_OK) return rc;
    uint32_t *d_res = reinterpret_cast<uint32_t *>(dev), *d_cnt = reinterpret_cast<uint32_t *>(dev + off_cnt);
    uint64_t *d_pre = reinterpret_cast<uint64_t *>(dev + off_pre);
    auto args = [&](const Part &p) {
        GatherArgs a;
        memset(&a, 0, sizeof a);
        a.res = d_res + p.res_off; a.counts = d_cnt + p.res_off / 64u; a.offsets = d_pre + p.res_off / 64u;
        a.obs = reinterpret_cast<u32x4 *>(obs_dev); a.entries = entries_dev;
        a.phase_ids = b->phase_ids + (size_t)p.seg * GE_MAX_PHASES;
        a.r0 = p.r0; a.nr = p.nr; a.seats = packed; a.cap = cap;
        a.entry0 = (uint32_t)((p.lo - first) * n_seats);
        a.seg = p.seg; a.n_seats = n_seats; a.want = want;
        return a;
    };
    for (const Part &p : part) {
        const dim3 grid((uint32_t)((p.nr + FIND_BLOCK - 1u) / FIND_BLOCK));
        const uint32_t kind = b->segs[p.seg].dev.kind;
        HIP_TRY(b->plan.generic ? gather_test_launch<1>(kind, grid, st, b, args(p)) : gather_test_launch<0>(kind, grid, st, b, args(p)));
        b->launches++;
    }
    hipLaunchKernelGGL(ge_gather_scan, dim3(1), dim3(FIND_SCAN_WAVES), 0, st, d_cnt, n_waves, d_pre, cap, n_dev);
    HIP_TRY(hipGetLastError());
    b->launches++;
    for (const Part &p : part) {
        if (cap == 0u) break;
        HIP_TRY(gather_emit_launch(b->segs[p.seg].dev.kind, dim3((uint32_t)((p.nr + 63u) / 64u)), st, b, args(p)));
        b->launches++;
    }
    if (e1) HIP_TRY(hipEventRecord(e1, st));
    return GE_OK;
}

static int act_listed_impl(ge_batch *b, uint64_t first, uint64_t count, uint32_t n_seats, uint64_t packed, const uint32_t *n_dev, uint64_t cap,
                           const uint32_t *entries_dev, const int32_t *choices_dev, int32_t *status_dev, hipStream_t st) {
    const uint32_t total = (uint32_t)(count * n_seats);       // (below 2^32: checked)
    const size_t off_st = up16(4 * (size_t)total), bytes = off_st + (status_dev ? 4 * (size_t)total : 0u);
    char *dev = nullptr;
    {
        GE_ON_DEVICE(b);
        const int rc = pool_scratch(b, bytes, &dev);          // grows only for a larger shape than the batch has served (may wait)
        if (rc != GE_OK) return rc;
    }
    int32_t *dense = reinterpret_cast<int32_t *>(dev), *dense_st = status_dev ? reinterpret_cast<int32_t *>(dev + off_st) : nullptr;
    // one interval, ordered by env_launches: the memset and the scatter in front of its first launch, the status gather behind its last
    bool opened = false;
    uint32_t left = 0;
    for (const Segment &s : b->segs)
        left += std::max(first, s.local_first) < std::min(first + count, s.local_first + s.dev.rooms) ? 1u : 0u;
    hipError_t tail = hipSuccess;
    const int rc = env_launches(b, first, count, n_seats, packed, st, [&](uint32_t kind, dim3 grid, EnvArgs &a, size_t entry) {
        if (!opened) {
            opened = true;
            hipError_t e = hipMemsetAsync(dense, 0, 4 * (size_t)total, st);
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL(ge_list_scatter, list_grid(cap), dim3(LIST_BLOCK), 0, st, n_dev, cap, entries_dev, choices_dev, dense, total);
            if ((e = hipGetLastError()) != hipSuccess) return e;
            b->launches++;
        }
        a.choices = dense + entry;
        a.status = dense_st ? dense_st + entry : nullptr;
        hipError_t e = act_launch(kind, grid, st, b, a);
        if (e == hipSuccess && --left == 0u && status_dev) {
            hipLaunchKernelGGL(ge_list_status, list_grid(cap), dim3(LIST_BLOCK), 0, st, n_dev, cap, entries_dev, dense_st, status_dev, total);
            tail = hipGetLastError();
            b->launches++;
        }
        return e;
    });
    if (rc != GE_OK) return rc;
    HIP_TRY(tail);
    return GE_OK;
}

extern "C" {

int ge_batch_gather_seats(ge_batch *b, uint64_t first, uint64_t count, uint32_t n_seats, const uint32_t *seats, uint32_t want, ge_seat_obs *obs_dev,
                          uint32_t *entries_dev, uint64_t cap, uint32_t *n_dev, void *hip_stream) {
    if (!b) return GE_ERR_ARG;
    // all before anything is launched, in this order (ABI behaviour)
    if (want == 0u || (want & ~(uint32_t)(GE_GATHER_SEAT | GE_GATHER_END))) return GE_ERR_ARG;
    if (!n_dev) return GE_ERR_ARG;
    const bool some = count > 0u && n_seats > 0u;
    if (some && cap > 0u && (!obs_dev || !entries_dev)) return GE_ERR_ARG;
    return guarded([&] {
        if (some && !seats) return (int)GE_ERR_ARG;           // ge_batch_observe_seats's checks from here on
        uint64_t packed = 0;
        const int rc = env_check_list(b, first, count, n_seats, seats, &packed);
        if (rc != GE_OK) return rc;
        if (some && cap > 0u) {
            if (cap > ~(size_t)0 / sizeof(ge_seat_obs)) return (int)GE_ERR_ARG;
            if (!env_reachable(b, obs_dev, (size_t)cap * sizeof(ge_seat_obs)) || !env_reachable(b, entries_dev, (size_t)cap * sizeof(uint32_t)))
                return (int)GE_ERR_ARG;
        }
        if (!env_reachable(b, n_dev, 2 * sizeof(uint32_t))) return (int)GE_ERR_ARG;
        if (count * (uint64_t)n_seats >= (1ull << 32)) return (int)GE_ERR_ARG;   // (count <= n_rooms, n_seats <= 12: no wrap)
        hipStream_t st = static_cast<hipStream_t>(hip_stream);
        if (!some) {                                          // nothing is due in an empty range: n_dev = {0, 0}, stored on the stream
            GE_ON_DEVICE(b);
            const int ro = order_after_previous(b, st);
            if (ro != GE_OK) return ro;
            HIP_TRY(hipMemsetAsync(n_dev, 0, 2 * sizeof(uint32_t), st));
            return (int)GE_OK;
        }
        return gather_seats_impl(b, first, count, n_seats, packed, want, obs_dev, entries_dev, std::min<uint64_t>(cap, count * (uint64_t)n_seats), n_dev, st);
    });
}

int ge_batch_act_listed(ge_batch *b, uint64_t first, uint64_t count, uint32_t n_seats, const uint32_t *seats, const uint32_t *n_dev, uint64_t cap,
                        const uint32_t *entries_dev, const int32_t *choices_dev, int32_t *status_dev, void *hip_stream) {
    if (!b) return GE_ERR_ARG;
    return guarded([&] {
        // ge_batch_act_seats's checks in their order (ABI behaviour), n_dev and the list beside seats
        const bool some = count > 0u && n_seats > 0u;
        if (some && (!seats || !n_dev || (cap > 0u && (!entries_dev || !choices_dev)))) return (int)GE_ERR_ARG;
        uint64_t packed = 0;
        const int rc = env_check_list(b, first, count, n_seats, seats, &packed);
        if (rc != GE_OK) return rc;
        if (count * (uint64_t)n_seats >= (1ull << 32)) return (int)GE_ERR_ARG;
        if (!some) return (int)GE_OK;
        if (cap > ~(size_t)0 / sizeof(uint32_t)) return (int)GE_ERR_ARG;
        const size_t bytes = (size_t)cap * sizeof(uint32_t);
        if (!env_reachable(b, n_dev, sizeof(uint32_t))) return (int)GE_ERR_ARG;
        if (cap > 0u && (!env_reachable(b, entries_dev, bytes) || !env_reachable(b, choices_dev, bytes) || (status_dev && !env_reachable(b, status_dev, bytes))))
            return (int)GE_ERR_ARG;
        if (cap == 0u) return (int)GE_OK;                     // an empty list: no choice, no status
        return act_listed_impl(b, first, count, n_seats, packed, n_dev, cap, entries_dev, choices_dev, status_dev, static_cast<hipStream_t>(hip_stream));
    });
}

}  // extern "C"

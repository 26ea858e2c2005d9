// ge_env.inl — a seat of every room observed into, and played from, device memory the caller owns (ge_batch_observe_seats,
// ge_batch_act_seats; POLICY.md §3n): the pair of calls that turns a resident batch into an environment for a decision maker that
// lives on the GPU (included at the end of ge_step.hip, behind ge_advise.inl: the existing kernels keep their code-object
// offsets).  Between them ge_batch_step is unchanged.  Both calls keep ge_batch_step's stream contract - launched on the
// caller's stream behind the batch's earlier work, no host copy, no host wait - so nothing here uses the indexed calls' staging.
//
//   ObsRoom            a room as its seats are shown it - the record unpacked, what its seats' records share, and one seat's record
//                      vector by vector; ge_observe_kernel and ge_gather_emit (ge_decide.inl) both build their records with it.
//   ge_observe_kernel  lane = room, one wavefront per block, the record loaded as ge_find_kernel loads it; one launch per
//                      segment of the range, the seat list by value in the arguments (a nibble per seat: no array to index).
//                      Per listed seat: the knowledge sets of §3c from the statements ge_rollout.inl's re-deal itself runs
//                      (GE_VIEW_SETS_WW, GE_VIEW_SHOWN_TT) - what the re-deal may change is what is hidden -, `legal` by
//                      ge_advise_plan's loop over inject_ww / inject_tt on copies of the record, the bitboards
//                      unpacked into the view's byte columns in registers (every index static: no scratch), then 12 x 16 bytes.
//                      The stores: the wavefront's 64 records go through LDS - 208 bytes apart there, which keeps the 16-byte LDS
//                      stores of a lane group on distinct banks - and come out as 12 stores of 1 KiB of consecutive bytes each.
//                      Two other layouts were measured beside it on an MI355X and dropped (profiles/env_probe.txt; Werewolf x 8,
//                      launch interval, medians of 15): each lane storing its own record, a store instruction's 64 lanes 192 x
//                      n_seats bytes apart - 83.9 us against 60.3 us at 1 048 576 rooms x 1 seat (2.80 against 3.90 TB/s of records
//                      read and observations written), 340.4 against 266.8 us x 4 seats, 13.7 against 11.9 us at 65 536 rooms x 1
//                      seat - and the same with streaming stores, 452.6 us at 1 048 576 x 1.
//   ge_act_kernel      lane = room: ge_inject_kernel's body with the room's actions read from choices_dev - seat seats[j]'s choice
//                      at (room - first) * n_seats + j, 0 = none - in ascending j; a room without a choice is not stored.

namespace {

constexpr uint32_t OBS_VEC = 12u;               // sizeof(ge_seat_obs) / 16
constexpr uint32_t OBS_LDS_VEC = 13u;           // a record's stride in LDS, in 16-byte units

struct EnvArgs {
    u32x4 *obs;                // observe: record (k * n_seats + j) * OBS_VEC of this part
    const int32_t *choices;    // act: entry k * n_seats + j of this part
    int32_t *status;           // act: the same entries, or null
    const int32_t *phase_ids;  // the segment's phase id per dense row
    uint64_t r0, nr;           // the part: segment-local rooms r0 .. r0 + nr - 1
    uint64_t seats;            // nibble j = seats[j] (1-based)
    uint32_t seg, n_seats;
};

// vectors 2 .. 10 of a record are players[12][12], four players (twelve words) to three vectors; put(i, v) takes vector i as soon
// as it is complete, so that no more than four players' columns are live at a time
template <class PUT> __device__ __forceinline__ void obs_put_four(int g, const uint32_t *q, PUT &&put) {
#pragma unroll
    for (int i = 0; i < 3; i++) {
        u32x4 v;
        v.x = q[4 * i]; v.y = q[4 * i + 1]; v.z = q[4 * i + 2]; v.w = q[4 * i + 3];
        put(2 + 3 * g + i, v);
    }
}

// the byte columns of a Werewolf record as seat `seat` is shown them (§3n): put(2 .. 10) = players[12][12], put(11) = det[12]
template <int NB, class PUT>
__device__ __forceinline__ void obs_columns(WW<NB> s, uint32_t seat, uint32_t n, uint32_t act, bool done, uint32_t &unknown, uint32_t &won, PUT &&put) {
    using nib_t = typename WW<NB>::nib_t;
    GE_VIEW_SETS_WW(s, seat, n)
    (void)nB;
    won = done && (((s.alive & team_w) == 0u ? s.team_v : team_w) & me) != 0u ? 1u : 0u;   // the true team: seat_wins's rule
    const uint32_t H = U, HT = U & ~(Uw | Uv);
    const bool priv = act == ACT_WOLF_TARGET || act == ACT_DOCTOR_PROTECT || act == ACT_DETECTIVE;
    nib_t hn = 0;                                             // H as a nibble mask
#pragma unroll
    for (int c = 0; c < NB; c++) hn |= ((H >> c) & 1u) ? nib_t(15) << (4 * c) : nib_t(0);
    s.rb0 &= ~H; s.rb1 &= ~H; s.rb2 &= ~H; s.secret &= ~H; s.elig &= ~H; s.sub &= ~H;
    s.sel &= ~hn;
    s.team_v &= ~HT; s.team_w &= ~HT;
    if (priv) { s.acted &= ~H; s.choice &= ~hn; }
    if (!s_det) { s.det_v = 0u; s.det_w = 0u; }
    unknown = H;
    u32x4 dv;
    dv.x = 0u; dv.y = 0u; dv.z = 0u; dv.w = 0u;
#pragma unroll
    for (int g = 0; g < 3; g++) {
        uint32_t q[12], d4 = 0u;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int c = 4 * g + i;
            uint32_t w0 = 0u, w1 = 0u, w2 = 0u;
            if (c < NB) {
                const uint32_t live = (uint32_t)c < n ? 0xFFFFFFFFu : 0u;
                const uint32_t role = ((s.rb0 >> c) & 1u) | ((s.rb1 >> c) & 1u) << 1 | ((s.rb2 >> c) & 1u) << 2;
                const uint32_t team = ((s.team_v >> c) & 1u) ? 1u : ((s.team_w >> c) & 1u) ? 2u : 0u;
                w0 = (role | team << 8 | ((s.alive >> c) & 1u) << 16 | ((s.revealed >> c) & 1u) << 24) & live;
                w1 = (((s.can_vote >> c) & 1u) | ((s.secret >> c) & 1u) << 8 | ((s.elig >> c) & 1u) << 16 | ((s.sub >> c) & 1u) << 24) & live;
                w2 = (((uint32_t)(s.sel >> (4 * c)) & 15u) | ((s.acted >> c) & 1u) << 8 | ((uint32_t)(s.choice >> (4 * c)) & 15u) << 16) & live;
                const uint32_t d = ((s.det_v >> c) & 1u) ? 1u : ((s.det_w >> c) & 1u) ? 2u : 0u;
                d4 |= (d & live) << (8 * i);
            }
            q[3 * i] = w0; q[3 * i + 1] = w1; q[3 * i + 2] = w2;
        }
        if (g == 0) dv.x = d4; else if (g == 1) dv.y = d4; else dv.z = d4;
        obs_put_four(g, q, put);
    }
    put(11, dv);
}

// ... and of a Two-Truths record: the lie of a speaker that has not revealed it is hidden from every other seat
template <int NB, class PUT>
__device__ __forceinline__ void obs_columns(TT<NB> s, uint32_t seat, uint32_t n, uint32_t, bool done, uint32_t &unknown, uint32_t &won, PUT &&put) {
    uint32_t top = 0u, mine = 0u;
#pragma unroll
    for (int c = 0; c < NB; c++) {                            // static indices: the record stays in registers
        const uint32_t sc = (uint32_t)c < n ? (s.score[c / 4] >> (8 * (c % 4))) & 255u : 0u;
        top = sc > top ? sc : top;
        mine = (uint32_t)c == seat - 1u ? sc : mine;
    }
    won = done && mine == top ? 1u : 0u;                      // the highest total_score, ties count: seat_wins's rule
    const uint32_t spk = s.speaker & ((1u << n) - 1u), sp = spk ? ctz(spk) : 0u;   // the lowest speaker
    const bool hid = spk != 0u && !GE_VIEW_SHOWN_TT(sp, s.revealed, seat);
    if (hid) s.lie &= ~(3u << (2u * sp));
    unknown = hid ? 1u << sp : 0u;
#pragma unroll
    for (int g = 0; g < 3; g++) {
        uint32_t q[12];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int c = 4 * g + i;
            uint32_t w0 = 0u, w1 = 0u, w2 = 0u;
            if (c < NB) {
                const uint32_t live = (uint32_t)c < n ? 0xFFFFFFFFu : 0u;
                w0 = (((s.speaker >> c) & 1u) | ((s.submitted >> c) & 1u) << 8 | ((s.lie >> (2 * c)) & 3u) << 16 | ((s.revealed >> c) & 1u) << 24) & live;
                w1 = (((s.can_vote >> c) & 1u) | ((s.vote >> (2 * c)) & 3u) << 8 | ((s.has_voted >> c) & 1u) << 16 |
                      ((s.score[c / 4] >> (8 * (c % 4))) & 255u) << 24) & live;
                w2 = (((uint32_t)(s.rounds >> (4 * c)) & 15u) | ((s.acted >> c) & 1u) << 8 | ((s.choice >> (2 * c)) & 3u) << 16) & live;
            }
            q[3 * i] = w0; q[3 * i + 1] = w1; q[3 * i + 2] = w2;
        }
        obs_put_four(g, q, put);
    }
    u32x4 dv;
    dv.x = 0u; dv.y = 0u; dv.z = 0u; dv.w = 0u;
    put(11, dv);
}

// a room as its seats are shown it: the record loaded and unpacked, what every seat's record shares, and record(seat, put) - the
// `legal` loop, the columns and the two header vectors of one seat.  ge_observe_kernel and ge_gather_emit (ge_decide.inl) both
// build their records here
template <int NB, bool WWP> struct ObsRoom {
    using G = PlayoutGame<NB, WWP>;
    using L = typename G::L;
    typename G::S s;
    const DevRow *row;
    const DevCond *cond;
    uint32_t n, act, phase_id;
    bool done;
    u32x4 h1;
    __device__ __forceinline__ void open(const SegDev &sg, const DevTable *__restrict__ tables, const int32_t *__restrict__ phase_ids, uint64_t room) {
        uint32_t w[L::WORDS];
        load_words<L::WORDS>(sg.base, sg.rooms_padded, room, w);
        L::unpack(w, s);
        row = &tables[sg.table_idx].rows[s.phase];
        cond = &tables[sg.table_idx].conds[s.phase];          // read in place, as inject_group_ww / inject_group_tt
        n = sg.n_players; act = (row->r0 >> 2) & 7u;
        done = ((sg.term_mask >> s.phase) & 1u) != 0u;
        h1.x = (uint32_t)phase_ids[s.prev & (GE_MAX_PHASES - 1u)]; h1.y = s.end_turn == END_NONE ? 0xFFFFFFFFu : s.end_turn; h1.z = s.games; h1.w = 0u;
        phase_id = (uint32_t)phase_ids[s.phase & (GE_MAX_PHASES - 1u)];   // (a row index is below 32: the mask keeps any record inside the table)
    }
    template <class PUT> __device__ __forceinline__ void record(uint32_t seat, PUT &&put) const {
        const uint32_t C = WWP ? n : 3u;
        uint32_t legal = 0;
        for (uint32_t c = 1; c <= C; c++) {                   // ge_advise_plan's loop: legal exactly when the injected action would be accepted
            typename G::S t = s;
            legal |= (G::inject(t, *row, *cond, n, seat, c) == GE_OK ? 1u : 0u) << (c - 1u);
        }
        uint32_t unknown, won;
        obs_columns(s, seat, n, act, done, unknown, won, put);
        u32x4 h0;
        h0.x = seat | n << 8 | (WWP ? (uint32_t)GE_PACK_WEREWOLF : (uint32_t)GE_PACK_TWO_TRUTHS) << 16 | act << 24;
        h0.y = s.phase | (done ? 1u : 0u) << 8 | won << 16;
        h0.z = legal | unknown << 16;
        h0.w = phase_id;
        put(0, h0);
        put(1, h1);
    }
};

template <int KIND>
__global__ void __launch_bounds__(64) ge_observe_kernel(const SegDev *__restrict__ segs, const DevTable *__restrict__ tables, const EnvArgs a) {
    __shared__ u32x4 stage[64u * OBS_LDS_VEC];
    const SegDev &sg = segs[a.seg];
    const uint64_t kb = (uint64_t)blockIdx.x * 64u, k = kb + threadIdx.x;
    const bool valid = k < a.nr;
    const uint64_t room = a.r0 + (valid ? k : 0u);            // lanes past the part read its first room and store nothing
    ObsRoom<KindOf<KIND>::NB, KindOf<KIND>::WW> o;
    o.open(sg, tables, a.phase_ids, room);
    auto *out = (__attribute__((address_space(1))) u32x4 *)(uintptr_t)a.obs;
    for (uint32_t j = 0; j < a.n_seats; j++) {
        const uint32_t seat = (uint32_t)(a.seats >> (4u * j)) & 15u;
        o.record(seat, [&](int i, u32x4 v) { stage[threadIdx.x * OBS_LDS_VEC + (uint32_t)i] = v; });
        __syncthreads();
        const uint64_t left = a.nr - kb;                      // (the block holds a room: kb < nr)
        const uint32_t live = left < 64u ? (uint32_t)left : 64u;
#pragma unroll
        for (uint32_t i = 0; i < OBS_VEC; i++) {              // vector x of the wavefront's live * 12: record x / 12, its part x % 12
            const uint32_t x = i * 64u + threadIdx.x, rec = x / OBS_VEC, part = x - rec * OBS_VEC;
            if (rec < live) out[((kb + rec) * a.n_seats + j) * OBS_VEC + part] = stage[rec * OBS_LDS_VEC + part];
        }
        __syncthreads();                                      // the next seat's records overwrite the stage
    }
}

template <int KIND>
__global__ void __launch_bounds__(64) ge_act_kernel(const SegDev *__restrict__ segs, const DevTable *__restrict__ tables, const EnvArgs a) {
    using G = PlayoutGame<KindOf<KIND>::NB, KindOf<KIND>::WW>;
    using L = typename G::L;
    const SegDev &sg = segs[a.seg];
    const uint64_t k = (uint64_t)blockIdx.x * 64u + threadIdx.x;
    if (k >= a.nr) return;
    const uint64_t room = a.r0 + k;
    uint32_t w[L::WORDS];
    load_words<L::WORDS>(sg.base, sg.rooms_padded, room, w);
    typename G::S s;
    L::unpack(w, s);
    const DevRow &row = tables[sg.table_idx].rows[s.phase];
    const DevCond &cond = tables[sg.table_idx].conds[s.phase];   // read in place, as inject_group_ww / inject_group_tt
    bool any = false;
    for (uint32_t j = 0; j < a.n_seats; j++) {
        const int32_t c = a.choices[k * a.n_seats + j];
        int st = GE_OK;
        if (c != 0) {
            any = true;
            st = c < 0 || c > 15 ? (int)GE_ERR_ARG : G::inject(s, row, cond, sg.n_players, (uint32_t)(a.seats >> (4u * j)) & 15u, (uint32_t)c);
        }
        if (a.status) a.status[k * a.n_seats + j] = st;
    }
    if (!any) return;                                         // no entry of ge_batch_inject_actions names this room
    L::pack(s, w);
    store_words<L::WORDS>(sg.base, sg.rooms_padded, room, w);
}

hipError_t observe_launch(uint32_t kind, dim3 grid, hipStream_t st, const ge_batch *b, const EnvArgs &a) {
    return by_kind(kind, [&](auto K) { hipLaunchKernelGGL((ge_observe_kernel<K()>), grid, dim3(64), 0, st, b->segs_dev, b->tables, a); });
}
hipError_t act_launch(uint32_t kind, dim3 grid, hipStream_t st, const ge_batch *b, const EnvArgs &a) {
    return by_kind(kind, [&](auto K) { hipLaunchKernelGGL((ge_act_kernel<K()>), grid, dim3(64), 0, st, b->segs_dev, b->tables, a); });
}

// the first and the last byte of [p, p + bytes) are memory the batch's device reaches: its own, managed, or pinned host memory
bool env_reachable(const ge_batch *b, const void *p, size_t bytes) {
    const char *ends[2] = {static_cast<const char *>(p), static_cast<const char *>(p) + (bytes ? bytes - 1u : 0u)};
    for (const char *q : ends) {
        hipPointerAttribute_t at;
        memset(&at, 0, sizeof at);
        if (hipPointerGetAttributes(&at, q) != hipSuccess) { (void)hipGetLastError(); return false; }
        const bool ok = (at.type == hipMemoryTypeDevice && at.device == b->device) || at.type == hipMemoryTypeManaged || at.type == hipMemoryTypeHost;
        if (!ok) return false;
    }
    return true;
}

}  // namespace

static_assert(sizeof(ge_seat_obs) == 16 * OBS_VEC, "an observation is 12 16-byte stores");
static_assert(offsetof(ge_seat_obs, legal) == 8 && offsetof(ge_seat_obs, phase_id) == 12 && offsetof(ge_seat_obs, prev_phase_id) == 16 &&
              offsetof(ge_seat_obs, players) == 32 && offsetof(ge_seat_obs, det) == 176, "header, header, nine vectors of columns, det");

// the seat list and the range of a ranged seat call, in their order (ABI behaviour): at most twelve seats, pairwise distinct; the
// range inside the batch; every seat one of each segment the range touches.  *packed: nibble j = seats[j]
static int env_check_list(const ge_batch *b, uint64_t first, uint64_t count, uint32_t n_seats, const uint32_t *seats, uint64_t *packed) {
    if (n_seats > GE_MAX_PLAYERS) return GE_ERR_ARG;
    *packed = 0;
    for (uint32_t j = 0; seats && j < n_seats; j++)
        for (uint32_t i = 0; i < j; i++)
            if (seats[i] == seats[j]) return GE_ERR_ARG;
    if (first + count > b->n_rooms || first + count < first) return GE_ERR_RANGE;
    for (uint32_t j = 0; seats && j < n_seats; j++) {
        if (seats[j] == 0u) return GE_ERR_ARG;
        for (const Segment &s : b->segs)
            if (std::max(first, s.local_first) < std::min(first + count, s.local_first + s.dev.rooms) && seats[j] > s.dev.n_players) return GE_ERR_ARG;
        if (seats[j] <= GE_MAX_PLAYERS) *packed |= (uint64_t)seats[j] << (4u * j);
    }
    return GE_OK;
}

// the checks both calls share, in their order (ABI behaviour); dev / dev2: the call's device pointers (dev2 may be null) and their
// bytes per entry.  GE_OK with *go = false: nothing to do
static int env_check(const ge_batch *b, uint64_t first, uint64_t count, uint32_t n_seats, const uint32_t *seats, const void *dev, size_t per_entry,
                     const void *dev2, size_t per_entry2, size_t cap_bytes, uint64_t *packed, bool *go) {
    *go = false;
    const bool some = count > 0u && n_seats > 0u;
    if (some && (!seats || !dev)) return GE_ERR_ARG;
    const int rc = env_check_list(b, first, count, n_seats, seats, packed);
    if (rc != GE_OK) return rc;
    const uint64_t entries = count * (uint64_t)n_seats;       // (count <= n_rooms, n_seats <= 12)
    if (cap_bytes / per_entry < entries) return GE_ERR_ARG;
    if (some && (!env_reachable(b, dev, (size_t)entries * per_entry) || (dev2 && !env_reachable(b, dev2, (size_t)entries * per_entry2)))) return GE_ERR_ARG;
    *go = some;
    return GE_OK;
}

// one launch per segment of the range: launch(segment, args) with the part's rooms and its first entry
template <class F> static int env_launches(ge_batch *b, uint64_t first, uint64_t count, uint32_t n_seats, uint64_t packed, hipStream_t st, F &&launch) {
    GE_ON_DEVICE(b);
    int rc = order_after_previous(b, st);
    if (rc != GE_OK) return rc;
    hipEvent_t e1 = nullptr;                                  // ge_batch_kernel_time counts the launches of this call as one interval
    if ((rc = timing_begin(b, st, &e1)) != GE_OK) return rc;
    for (uint32_t g = 0; g < (uint32_t)b->segs.size(); g++) {
        const Segment &s = b->segs[g];
        const uint64_t lo = std::max(first, s.local_first), hi = std::min(first + count, s.local_first + s.dev.rooms);
        if (lo >= hi) continue;
        EnvArgs a;
        memset(&a, 0, sizeof a);
        a.phase_ids = b->phase_ids + (size_t)g * GE_MAX_PHASES;
        a.r0 = lo - s.local_first; a.nr = hi - lo; a.seats = packed; a.seg = g; a.n_seats = n_seats;
        HIP_TRY(launch(s.dev.kind, dim3((uint32_t)((a.nr + 63u) / 64u)), a, (size_t)(lo - first) * n_seats));
        b->launches++;
    }
    if (e1) HIP_TRY(hipEventRecord(e1, st));
    return GE_OK;
}

extern "C" {

int ge_batch_observe_seats(ge_batch *b, uint64_t first, uint64_t count, uint32_t n_seats, const uint32_t *seats, ge_seat_obs *obs_dev, size_t cap_bytes,
                           void *hip_stream) {
    if (!b) return GE_ERR_ARG;
    return guarded([&] {
        uint64_t packed = 0;
        bool go = false;
        const int rc = env_check(b, first, count, n_seats, seats, obs_dev, sizeof(ge_seat_obs), nullptr, 0, cap_bytes, &packed, &go);
        if (rc != GE_OK || !go) return rc;
        hipStream_t st = static_cast<hipStream_t>(hip_stream);
        return env_launches(b, first, count, n_seats, packed, st, [&](uint32_t kind, dim3 grid, EnvArgs &a, size_t entry) {
            a.obs = reinterpret_cast<u32x4 *>(obs_dev + entry);
            return observe_launch(kind, grid, st, b, a);
        });
    });
}

int ge_batch_act_seats(ge_batch *b, uint64_t first, uint64_t count, uint32_t n_seats, const uint32_t *seats, const int32_t *choices_dev,
                       int32_t *status_dev, void *hip_stream) {
    if (!b) return GE_ERR_ARG;
    return guarded([&] {
        uint64_t packed = 0;
        bool go = false;
        const int rc = env_check(b, first, count, n_seats, seats, choices_dev, sizeof(int32_t), status_dev, sizeof(int32_t), ~(size_t)0, &packed, &go);
        if (rc != GE_OK || !go) return rc;
        hipStream_t st = static_cast<hipStream_t>(hip_stream);
        return env_launches(b, first, count, n_seats, packed, st, [&](uint32_t kind, dim3 grid, EnvArgs &a, size_t entry) {
            a.choices = choices_dev + entry;
            a.status = status_dev ? status_dev + entry : nullptr;
            return act_launch(kind, grid, st, b, a);
        });
    });
}

}  // extern "C"

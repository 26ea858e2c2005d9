// ge_pool.inl — the indexed single-turn step (ge_batch_step_rooms), the indexed read (ge_batch_read_rooms_at) and the indexed
// write (ge_batch_write_rooms_at): many game threads hosted in one resident batch, each slot stepped under its own RNG key and
// turn number (included at the end of ge_step.hip, behind every other kernel: the existing kernels keep their code-object
// offsets; it needs ge_batch's internals).
//
// The reference runs one LangGraph thread per room and a thread plays a turn only when its own message arrives
// (src/app/api/copilotkit/route.ts:24-37).  ge_batch_step moves every room under one batch-wide turn counter; here a list of
// entries k moves room rooms[k] by one turn keyed as global room keys[k] at turn turns[k] - what a lone batch with first_room =
// keys[k] and turn counter turns[k] does to that room in one ge_batch_step(b, 1).
//
// One lane per entry.  What a step launch keeps uniform per wavefront - the turn, the deal period, the room key - is per lane
// here; the turn itself is ge_device.h's single-turn form (ww_turn / tt_turn, SINGLE), in the lone-wavefront build: these
// launches are a few wavefronts at tick sizes, a chain of latencies, and that build reads its tables where they lie in global
// memory (GE_SINGLE_GLOBAL's reasoning) instead of filling LDS behind a barrier.
//
// Prepared role deals.  A prepared deal is a pure function of (seed, global room, game index) tagged only by the game index
// (Werewolf x 8: the record's upper half-word 7; Werewolf x 12: the side plane of ge_kernels.inl run_ww), so a deal prepared
// for a slot under the batch's own key would mislead a turn under another key.  So an indexed step never reads or writes the
// side plane, ignores a record's prepared deal, deals on the spot (ww_apply_effect), and stores every record without one - as
// ge_batch_write_rooms does.  Ordinary ge_batch_step calls before or after on the same batch stay exact: the side plane still
// holds only deals of the slots' own keys, and a record without a deal gets its next one prepared or dealt on the spot.
//
// Mixed batches: entries are grouped by segment on the host (a stable counting sort) and each segment present gets one launch of
// its layout's kernel - a wavefront never mixes layouts (the action queue is a wave-wide collective).
//
// The indexed write (ge_batch_write_rooms_at) is the scatter twin of the indexed read: a thread adopted mid-game into a slot of a
// resident batch.  The host packs each view with view_to_words - the record ge_batch_write_rooms stores for it, without a prepared
// deal (Werewolf x 8: word 7's upper half is 0) - and ge_pool_scatter stores it plane by plane.  The Werewolf x 12 side plane is not
// touched, as ge_batch_write_rooms does not touch it: a deal there is a function of the slot's own key and the game index alone, so
// it stays right for whatever record is written over the slot.
//
// Shared with the other indexed files (ge_rollout.inl, ge_playout.inl, ge_run.inl), each written here once: KindOf (a compile-time
// KIND as players' bound and game), by_kind + lane_lds (the launch of a segment's kind and its LDS size), up16, the entry checks
// (pool_check_rooms / pool_check_entries: their order and their errors are ABI behaviour), PoolEntries (the listed rooms grouped by
// segment and their staging as [rooms][keys][turns]), launch_pool_turn and pool_decode_event.  On the device: the indexed lane's
// context (lane_cond_ctx, lane_ww_ctx), recycle rule (lane_recycle), turn call (lane_ww_turn, lane_tt_turn) and event words
// (lane_event), and Lane<NB, WWP, GENERIC>, which wraps them per game - record, constants, recycle, turn, pack, PERSON test - so
// that a kernel body is written once for both games: pool_lane here, seat_lane (ge_seats.inl), find_lane (ge_find.inl),
// seat_run_lane (ge_run_seats.inl: a turn loop with stop tests over the type, within the baseline it was given).  The turn
// loop of ge_run.inl and the playouts of ge_rollout.inl keep a body per game (run_ww / run_tt, roll_ww / roll_tt) on the functions
// the type wraps: over the type their builds spill more scalar registers than tools/asm_baseline.json allows
// (profiles/indexed_lane_asm.txt).

namespace {

// a compile-time KIND as (players' bound NB, is Werewolf)
template <int KIND> struct KindOf {
    static constexpr int NB = KIND == K_TT4 ? 4 : KIND == K_WW8 || KIND == K_TT8 ? 8 : 12;
    static constexpr bool WW = KIND == K_WW8 || KIND == K_WW12;
};

// ---- the indexed lane, shared by ge_pool_kernel, ge_run_kernel (ge_run.inl) and ge_rollout_kernel (ge_rollout.inl): one lane plays
// single turns of one room in the lone-wavefront single-turn build, tables read in place, its key and turn its own

__device__ __forceinline__ CondShape pool_cond_shape(const DevTable &tb) {
    return CondShape{(uint32_t)__builtin_amdgcn_readfirstlane(tb.cond_shape), (uint32_t)__builtin_amdgcn_readfirstlane(tb.cond_g[0]), (uint32_t)__builtin_amdgcn_readfirstlane(tb.cond_g[1]),
                     (uint32_t)__builtin_amdgcn_readfirstlane(tb.cond_fields[0]), (uint32_t)__builtin_amdgcn_readfirstlane(tb.cond_fields[1])};
}

// the segment's generic target conditions, read in place
template <int GENERIC> __device__ __forceinline__ CondCtx lane_cond_ctx(const SegDev &sg, const DevTable *__restrict__ tables) {
    return CondCtx{reinterpret_cast<const unsigned char *>(tables[sg.table_idx].cond_img),
                   GENERIC ? pool_cond_shape(tables[sg.table_idx]) : CondShape{0u, 0u, 0u, 0u, 0u}};
}

// the lane's mask of host-driven seats: the room's own once the batch has a seat plane (ge_seats.inl; `seats` is a kernel argument,
// so the test is wave-uniform), else its segment's.  room: segment-local
__device__ __forceinline__ uint32_t lane_seat_mask(const SegDev &sg, const uint16_t *__restrict__ seats, uint64_t room) {
    return seats ? (uint32_t)seats[sg.local_first + room] : sg.human_mask;
}

// the seats that are host-driven in some lane of the wavefront (bits below nb)
__device__ __forceinline__ uint32_t wave_seat_union(uint32_t mask, int nb) {
    uint32_t any = 0;
    for (int i = 0; i < nb; i++) any |= __ballot((mask >> i) & 1u) != 0ull ? 1u << i : 0u;
    return any;
}

// Werewolf: what the lane's turns keep constant.  human: the seats left to people - the lane's own mask (lane_seat_mask), or 0 where
// the policy plays every seat (the playouts); valid: the lane holds a real entry (else it shadows one and never acts)
template <int GENERIC> __device__ __forceinline__ WwCtx lane_ww_ctx(const SegDev &sg, const DevTable *__restrict__ tables, void *lw, uint32_t rk, bool valid, uint32_t human) {
    const unsigned char *img = reinterpret_cast<const unsigned char *>(tables + sg.table_idx);
    const CondCtx cc = lane_cond_ctx<GENERIC>(sg, tables);
    const uint32_t term_mask = __builtin_amdgcn_readfirstlane(sg.term_mask);
    return WwCtx{reinterpret_cast<const DevRow *>(img), cc, lw, img + IMG_NTH8, reinterpret_cast<const uint32_t *>(img + IMG_ORD8), valid, sg.n_players, sg.nw,
                 sg.phase0_idx, rk, human, term_mask};
}

// a finished room of a restarting batch becomes the init template with one more game, saturating (Two-Truths: the caller reloads
// `done` from sg.done0)
template <class S> __device__ __forceinline__ uint32_t lane_recycle(const SegDev &sg, S &s, uint32_t restart, uint32_t term_mask) {
    if (!(restart && ((term_mask >> s.phase) & 1u))) return 0u;
    uint32_t ir[20];
    load_init_regs<S::NREGS>(sg, ir);
    const uint32_t g = s.games;
    S s0;
    s0.from_regs(ir);
    s = s0;
    s.games = g < 0xFFFFu ? g + 1u : g;
    return 1u;
}

// what a turn logged: the phase it started in, who acted, what they chose
struct LaneTurn { uint32_t p, newly; uint64_t choice; };

template <int NB, int GENERIC> __device__ __forceinline__ LaneTurn lane_ww_turn(WWR<NB> &s, const WwCtx &ctx, uint32_t turn, bool log) {
    DevRow row = lds_row<false>(ctx.rows, s.phase);
    LaneTurn t = {s.phase, 0u, 0ull};
    Deal deal = {0u, 0u, 0u, 0u, 0u};                         // no prepared deal (gv = 0): an assignment deals on the spot
    uint32_t tk = turn_key(ctx.rkey, turn);
    ww_turn<NB, true, GENERIC, true>(s, row, ctx, turn, tk, log, deal, false, t.newly, t.choice, nullptr);
    return t;
}

template <int NB, int GENERIC>
__device__ __forceinline__ LaneTurn lane_tt_turn(TT<NB> &s, uint32_t &done, const SegDev &sg, const DevTable *__restrict__ tables, const CondCtx &cc, void *lw,
                                                 bool valid, uint32_t rk, uint32_t turn, bool log, uint32_t human, uint32_t term_mask) {
    const unsigned char *img = reinterpret_cast<const unsigned char *>(tables + sg.table_idx);
    const DevRow *rows = reinterpret_cast<const DevRow *>(img);
    DevRow row = lds_row<false>(rows, s.phase);
    LaneTurn t = {s.phase, 0u, 0ull};
    tt_turn<NB, tt_uses_queue(NB, true), false, GENERIC, true>(s, done, row, rows, cc, lw, img + IMG_NTH8, valid, sg.n_players, sg.rounds, sg.phase0_idx, rk,
                                                             turn, log, human, term_mask, t.newly, t.choice);
    return t;
}

// the four event words of a turn: turn | from, to, restarted, acted (as the GE_FLAG_TRACE record) | choice nibbles
__device__ __forceinline__ u32x4 lane_event(uint32_t turn, const LaneTurn &t, uint32_t q, uint32_t restarted) {
    u32x4 v;
    v.x = turn; v.y = t.p | (q << 8) | (restarted << 16) | (t.newly << 20);
    v.z = (uint32_t)t.choice; v.w = (uint32_t)(t.choice >> 32);
    return v;
}

// ---- Lane<NB, WWP, GENERIC>: what the two games' indexed lanes differ in - the record and its state, what the lane's turns keep
// constant, the call that plays a turn and how the PERSON test finds a pending seat
template <int NB, bool WWP, int GENERIC> struct Lane;

template <int NB, int GENERIC> struct Lane<NB, true, GENERIC> {
    using L = WWLayout<NB>;
    WwCtx ctx;
    WWR<NB> s;
    // the lane's constants and the record w into its state (human, valid: lane_ww_ctx)
    __device__ __forceinline__ void open(const SegDev &sg, const DevTable *__restrict__ tables, void *lw, const uint32_t *w, uint32_t rk, bool valid, uint32_t human) {
        ctx = lane_ww_ctx<GENERIC>(sg, tables, lw, rk, valid, human);
        uint32_t cache;                                       // the record's prepared deal: not of this key, never used
        ww_load_regs<NB>(w, s, cache);
    }
    __device__ __forceinline__ uint32_t recycle(const SegDev &sg, uint32_t restart) { return lane_recycle(sg, s, restart, ctx.term_mask); }
    // on: from here on the lane shadows its room and never acts (a room of a turn loop that has stopped)
    __device__ __forceinline__ void shadow(bool on) { ctx.valid = !on; }
    __device__ __forceinline__ LaneTurn turn(uint32_t turn, bool log) { return lane_ww_turn<NB, GENERIC>(s, ctx, turn, log); }
    // the canonical record: stored without a prepared deal
    __device__ __forceinline__ void pack(uint32_t *w) const { ww_store_regs<NB>(s, 0u, w); }
    __device__ __forceinline__ uint32_t phase() const { return s.phase; }
    __device__ __forceinline__ uint32_t term_mask() const { return ctx.term_mask; }
    // wave-uniform, 0: no lane of the wavefront has a host-driven seat, so the PERSON test finds nothing.  The scan skips the test
    // then; the run-on's loop does not branch on it (the branch costs its Werewolf builds scalar registers: profiles/indexed_lane_asm.txt)
    static __device__ __forceinline__ uint32_t probe(const SegDev &, const uint16_t *__restrict__ seats, uint32_t human) {
        return (seats ? __ballot(human != 0u) != 0ull : __builtin_amdgcn_readfirstlane(human) != 0u) ? 1u : 0u;
    }
    // the PERSON test: the seats of `human` that are pending targets of the record as it stands - the turn's own ww_targets on the
    // row of its phase, less who has acted
    __device__ __forceinline__ uint32_t pending(uint32_t human, uint32_t) const {
        const DevRow row = lds_row<false>(ctx.rows, s.phase);
        const uint32_t T = ww_targets<NB, true, GENERIC>(s, row, ctx, s.template get<F_ALIVE>(), (1u << ctx.n) - 1u);
        return T & ~s.acted & human;
    }
};

template <int NB, int GENERIC> struct Lane<NB, false, GENERIC> {
    using L = TTLayout<NB>;
    TT<NB> s;
    uint32_t done;                                            // tt_done_mask of s.rounds, maintained by the turn
    const SegDev *sg;
    const DevTable *tables;
    CondCtx cc;
    void *lw;
    bool valid;
    uint32_t rk, human, tmask;
    __device__ __forceinline__ void open(const SegDev &sg_, const DevTable *__restrict__ tables_, void *lw_, const uint32_t *w, uint32_t rk_, bool valid_, uint32_t human_) {
        sg = &sg_; tables = tables_; lw = lw_; rk = rk_; valid = valid_; human = human_;
        cc = lane_cond_ctx<GENERIC>(sg_, tables_);
        tmask = __builtin_amdgcn_readfirstlane(sg_.term_mask);
        L::unpack(w, s);
        done = tt_done_mask<NB>(s.rounds, sg_.rounds);
    }
    __device__ __forceinline__ uint32_t recycle(const SegDev &sg_, uint32_t restart) {
        const uint32_t restarted = lane_recycle(sg_, s, restart, tmask);
        if (restarted) done = __builtin_amdgcn_readfirstlane(sg_.done0);
        return restarted;
    }
    __device__ __forceinline__ void shadow(bool on) { valid = !on; }
    __device__ __forceinline__ LaneTurn turn(uint32_t turn, bool log) {
        return lane_tt_turn<NB, GENERIC>(s, done, *sg, tables, cc, lw, valid, rk, turn, log, human, tmask);
    }
    __device__ __forceinline__ void pack(uint32_t *w) const { L::pack(s, w); }
    __device__ __forceinline__ uint32_t phase() const { return s.phase; }
    __device__ __forceinline__ uint32_t term_mask() const { return tmask; }
    // wave-uniform: the seats the PERSON test tries are the wavefront's - with a seat plane the union of its rooms' masks, each
    // lane counting only its own bits; 0: the test finds nothing
    static __device__ __forceinline__ uint32_t probe(const SegDev &sg_, const uint16_t *__restrict__ seats, uint32_t mask) {
        const uint32_t h = mask & ((1u << sg_.n_players) - 1u);
        return seats ? wave_seat_union(h, NB) : (uint32_t)__builtin_amdgcn_readfirstlane(h);
    }
    // the PERSON test (the turn has its target set inline): the seats of `mask` for which inject_tt on a copy of the record, choice
    // 1, is accepted - the test ge_batch_inject_actions itself makes, as ge_playout_plan uses it
    __device__ __forceinline__ uint32_t pending(uint32_t mask, uint32_t probe) const {
        uint32_t pend = 0;
        if (probe != 0u) {                                    // (wave-uniform)
            const DevRow &row = tables[sg->table_idx].rows[s.phase];
            const DevCond &cond = tables[sg->table_idx].conds[s.phase];   // read in place, as inject_group_tt
            for (uint32_t m = probe; m; m &= m - 1u) {
                TT<NB> c = s;                                 // a pending target exactly when an injected action would be accepted
                pend |= inject_tt<NB>(c, row, cond, sg->n_players, ctz(m) + 1u, 1u) == GE_OK ? m & (0u - m) & mask : 0u;
            }
        }
        return pend;
    }
};

// ---- ge_pool_kernel: one turn of each listed room

struct PoolArgs {
    const uint64_t *rooms;     // segment-local room of each entry of this launch
    const uint64_t *keys;      // global room index its RNG stream is keyed by
    const uint32_t *turns;     // its turn number
    uint32_t *events;          // [n] x 4 words: lane_event
    const uint16_t *seats;     // the batch's seat plane, or null (lane_seat_mask)
    uint32_t n, seg, seed_key, restart;
};

template <int NB, bool WWP, int GENERIC>
__device__ __forceinline__ void pool_lane(const SegDev &sg, const DevTable *__restrict__ tables, const PoolArgs &a, void *lw, uint32_t k_in) {
    using Ln = Lane<NB, WWP, GENERIC>;
    using L = typename Ln::L;
    // lanes past the list stay in the wavefront (the action queue is a wave-wide collective): they shadow entry 0 and store nothing
    const bool valid = k_in < a.n;
    const uint32_t k = valid ? k_in : 0u;
    const uint64_t room = a.rooms[k];
    uint32_t w[L::WORDS];
    load_words<L::WORDS>(sg.base, sg.rooms_padded, room, w);
    const uint32_t rk = room_key_from(a.seed_key, a.keys[k]);
    const uint32_t turn = a.turns[k];
    Ln lane;
    lane.open(sg, tables, lw, w, rk, valid, lane_seat_mask(sg, a.seats, room));
    const uint32_t restarted = lane.recycle(sg, a.restart);
    const LaneTurn t = lane.turn(turn, true);
    if (!valid) return;
    reinterpret_cast<u32x4 *>(a.events)[k] = lane_event(turn, t, lane.phase(), restarted);
    lane.pack(w);
    store_words<L::WORDS>(sg.base, sg.rooms_padded, room, w);
}

// one wavefront per block; its action queue (WaveLdsLow) is the block's dynamic LDS (none for Two-Truths x 4: no queue)
template <int KIND, int GENERIC>
__global__ void __launch_bounds__(64) ge_pool_kernel(const SegDev *__restrict__ segs, const DevTable *__restrict__ tables, const PoolArgs a) {
    const SegDev &sg = segs[a.seg];
    const uint32_t k = blockIdx.x * 64u + threadIdx.x;
    void *lw = ge_lds;
    pool_lane<KindOf<KIND>::NB, KindOf<KIND>::WW, GENERIC>(sg, tables, a, lw, k);
}

// ge_batch_read_rooms_at: the packed record of batch room rooms[k] -> out[k * 12 ..] (its segment's words; the rest untouched)
__global__ void __launch_bounds__(64) ge_pool_gather(const SegDev *__restrict__ segs, uint32_t n_seg, const uint64_t *__restrict__ rooms, uint64_t n,
                                                      uint32_t *__restrict__ out) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint64_t room = rooms[k];
    uint32_t si = 0;
    for (uint32_t j = 1; j < n_seg; j++)
        if (room >= segs[j].local_first) si = j;
    const SegDev &sg = segs[si];
    const uint64_t r = room - sg.local_first;
    if (r >= sg.rooms) return;                                // (the host checked every room)
    const int W = (int)sg.words;
    for (int j = 0; j < planes_of(W); j++) {
        const int pw = plane_words(W, j);
        const uint32_t *plane = reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(sg.base) + plane_offset(sg.rooms_padded, j));
        for (int x = 0; x < pw; x++) out[k * 12u + 4u * (uint32_t)j + (uint32_t)x] = plane[r * (uint64_t)pw + (uint64_t)x];
    }
}

// ge_batch_write_rooms_at: the packed record src[k * 12 ..] (12 words, 16-byte aligned; its segment's words used) -> batch room
// rooms[k], plane by plane: a 4-word plane is one 16-byte store, the 2-word last plane of a 6- or 10-word layout one 8-byte store
__global__ void __launch_bounds__(64) ge_pool_scatter(const SegDev *__restrict__ segs, uint32_t n_seg, const uint64_t *__restrict__ rooms, uint64_t n,
                                                       const uint32_t *__restrict__ src) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint64_t room = rooms[k];
    uint32_t si = 0;
    for (uint32_t j = 1; j < n_seg; j++)
        if (room >= segs[j].local_first) si = j;
    const SegDev &sg = segs[si];
    const uint64_t r = room - sg.local_first;
    if (r >= sg.rooms) return;                                // (the host checked every room)
    const u32x4 *in = reinterpret_cast<const u32x4 *>(src) + 3u * k;
    const int W = (int)sg.words;
    for (int j = 0; j < planes_of(W); j++) {
        const int pw = plane_words(W, j);
        char *plane = reinterpret_cast<char *>(sg.base) + plane_offset(sg.rooms_padded, j);
        const u32x4 v = in[j];
        if (pw == 4) {
            reinterpret_cast<u32x4 *>(plane)[r] = v;
        } else if (pw == 2) {
            u32x2 h; h.x = v.x; h.y = v.y;
            reinterpret_cast<u32x2 *>(plane)[r] = h;
        } else {
            for (int x = 0; x < pw; x++) reinterpret_cast<uint32_t *>(plane)[r * (uint64_t)pw + (uint64_t)x] = v[x];
        }
    }
}

// the device scratch of the indexed calls (shared with ge_batch_inject_actions: every user synchronises before it returns)
int pool_scratch(ge_batch *b, size_t bytes, char **out) {
    if (b->inj_cap < bytes) {
        if (b->inj_buf) (void)hipFree(b->inj_buf);
        b->inj_buf = nullptr; b->inj_cap = 0;
        const size_t cap = bytes < 4096 ? 4096 : bytes * 2;
        if (hipMalloc(&b->inj_buf, cap) != hipSuccess) return GE_ERR_NOMEM;
        b->inj_cap = cap;
    }
    *out = static_cast<char *>(b->inj_buf);
    return GE_OK;
}

// index of the segment holding batch room `room` (< n_rooms)
uint32_t pool_segment_of(const ge_batch *b, uint64_t room) {
    uint32_t si = 0;
    for (uint32_t j = 1; j < (uint32_t)b->segs.size(); j++)
        if (room >= b->segs[j].local_first) si = j;
    return si;
}

// the action queue of a lone wavefront as dynamic LDS: Two-Truths x 4 has no queue
uint32_t lane_lds(uint32_t kind) { return kind == K_TT4 ? 0u : (uint32_t)sizeof(WaveLdsLow); }

// a segment's kind as a compile-time KIND: f(std::integral_constant<int, KIND>) launches that kernel
template <class F> hipError_t by_kind(uint32_t kind, F &&f) {
    switch (kind) {
    case K_WW8: f(std::integral_constant<int, K_WW8>{}); break;
    case K_WW12: f(std::integral_constant<int, K_WW12>{}); break;
    case K_TT4: f(std::integral_constant<int, K_TT4>{}); break;
    case K_TT8: f(std::integral_constant<int, K_TT8>{}); break;
    default: f(std::integral_constant<int, K_TT12>{}); break;
    }
    return hipGetLastError();
}

template <int GEN> hipError_t pool_launch(uint32_t kind, dim3 grid, hipStream_t st, const ge_batch *b, const PoolArgs &a) {
    return by_kind(kind, [&](auto K) { hipLaunchKernelGGL((ge_pool_kernel<K(), GEN>), grid, dim3(64), lane_lds(kind), st, b->segs_dev, b->tables, a); });
}

size_t up16(size_t x) { return (x + 15u) & ~(size_t)15u; }

}  // namespace

// the rooms of an indexed call (n > 0), all before anything runs: every room in the batch (GE_ERR_RANGE), none listed twice (GE_ERR_ARG)
static int pool_check_rooms(const ge_batch *b, uint64_t n, const uint64_t *rooms) {
    for (uint64_t k = 0; k < n; k++)                              // all-or-nothing: every entry is checked before anything runs
        if (rooms[k] >= b->n_rooms) return GE_ERR_RANGE;
    std::vector<uint64_t> sorted(rooms, rooms + n);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return GE_ERR_ARG;
    return GE_OK;
}

// the entry checks of ge_batch_step_rooms (n > 0): shared with ge_batch_step_rooms_playout (ge_playout.inl) and ge_batch_run_rooms
// (ge_run.inl).  A turn out of range answers as a room out of range does, so which of the two loops finds it first does not show
static int pool_check_entries(const ge_batch *b, uint64_t n, const uint64_t *rooms, const uint64_t *keys, const uint32_t *turns) {
    if (!rooms || !keys || !turns || n > 0x7FFFFFFFull) return GE_ERR_ARG;
    for (uint64_t k = 0; k < n; k++)
        if (turns[k] == 0xFFFFFFFFu) return GE_ERR_RANGE;
    return pool_check_rooms(b, n, rooms);
}

// n listed rooms grouped by segment (a stable counting sort): the entry at sorted position i is order[i], of segment seg_of[order[i]];
// segment g holds the sorted positions [begin[g], begin[g + 1]).  Every indexed call stages and launches in this order: one launch
// per segment with entries
struct PoolEntries {
    std::vector<uint32_t> seg_of, begin, order;
    PoolEntries(const ge_batch *b, uint64_t n, const uint64_t *rooms)
        : seg_of((size_t)n), begin(b->segs.size() + 1u, 0u), order((size_t)n) {
        const uint32_t n_seg = (uint32_t)b->segs.size();
        for (uint64_t k = 0; k < n; k++) { seg_of[k] = pool_segment_of(b, rooms[k]); begin[seg_of[k] + 1u]++; }
        for (uint32_t s = 0; s < n_seg; s++) begin[s + 1u] += begin[s];
        std::vector<uint32_t> at(begin.begin(), begin.end() - 1);
        for (uint64_t k = 0; k < n; k++) order[at[seg_of[k]]++] = (uint32_t)k;
    }
    size_t size() const { return order.size(); }
    uint32_t seg_at(size_t i) const { return seg_of[order[i]]; }
    // [rooms u64 x n] at host, [keys u64 x n] at host + off_keys, [turns u32 x n] at host + off_turns, sorted, rooms segment-local
    void stage(const ge_batch *b, const uint64_t *rooms, const uint64_t *keys, const uint32_t *turns, unsigned char *host, size_t off_keys,
               size_t off_turns) const {
        uint64_t *h_rooms = reinterpret_cast<uint64_t *>(host), *h_keys = reinterpret_cast<uint64_t *>(host + off_keys);
        uint32_t *h_turns = reinterpret_cast<uint32_t *>(host + off_turns);
        for (size_t i = 0; i < size(); i++) {
            const uint32_t k = order[i];
            h_rooms[i] = rooms[k] - b->segs[seg_of[k]].local_first;
            h_keys[i] = keys[k];
            h_turns[i] = turns[k];
        }
    }
};

// the four event words of a turn (lane_event) as read_events_impl decodes the trace record
static void pool_decode_event(const uint32_t *w, const ge_game_table &tb, ge_turn_event &e) {
    memset(&e, 0, sizeof e);
    e.turn = w[0];
    e.from_phase_id = tb.rows[w[1] & 255u].phase_id;
    e.to_phase_id = tb.rows[(w[1] >> 8) & 255u].phase_id;
    e.restarted = (w[1] >> 16) & 1u;
    e.acted_now = (uint16_t)(w[1] >> 20);
    const uint64_t ch = (uint64_t)w[2] | ((uint64_t)w[3] << 32);
    for (int c = 0; c < 16; c++) e.choice[c] = (uint8_t)((ch >> (4 * c)) & 15u);
}

// one turn of the entries staged at dev (rooms at 0, keys, turns), a launch per segment present; events: 16 B per sorted entry
static int launch_pool_turn(ge_batch *b, hipStream_t s, const PoolEntries &en, char *dev, size_t off_keys, size_t off_turns, size_t off_ev) {
    const uint32_t seed_k = seed_key((uint32_t)b->seed, (uint32_t)(b->seed >> 32));
    for (uint32_t g = 0; g < (uint32_t)b->segs.size(); g++) {
        const uint32_t lo = en.begin[g], cnt = en.begin[g + 1u] - lo;
        if (!cnt) continue;
        PoolArgs a;
        a.rooms = reinterpret_cast<const uint64_t *>(dev) + lo;
        a.keys = reinterpret_cast<const uint64_t *>(dev + off_keys) + lo;
        a.turns = reinterpret_cast<const uint32_t *>(dev + off_turns) + lo;
        a.events = reinterpret_cast<uint32_t *>(dev + off_ev) + 4u * (size_t)lo;
        a.seats = b->seats;
        a.n = cnt; a.seg = g; a.seed_key = seed_k;
        a.restart = (b->flags & GE_FLAG_RESTART) ? 1u : 0u;
        const dim3 grid((cnt + 63u) / 64u);
        HIP_TRY(b->plan.generic ? pool_launch<1>(b->segs[g].dev.kind, grid, s, b, a) : pool_launch<0>(b->segs[g].dev.kind, grid, s, b, a));
    }
    return GE_OK;
}

static int step_rooms_impl(ge_batch *b, uint64_t n, const uint64_t *rooms, const uint64_t *keys, const uint32_t *turns, ge_turn_event *events) {
    if (n == 0) return GE_OK;
    int st = pool_check_entries(b, n, rooms, keys, turns);
    if (st != GE_OK) return st;
    GE_ON_DEVICE(b);
    if ((st = sync_impl(b)) != GE_OK) return st;
    const PoolEntries en(b, n, rooms);
    // one upload: [rooms u64 x n][keys u64 x n][turns u32 x n (padded to 16 B)], then events 16 B x n
    const size_t off_keys = 8 * (size_t)n, off_turns = 16 * (size_t)n, off_ev = up16(off_turns + 4 * (size_t)n);
    const size_t total = off_ev + 16 * (size_t)n;
    uint32_t *host32 = nullptr;
    if ((st = io_stage(b, total, &host32)) != GE_OK) return st;
    unsigned char *host = reinterpret_cast<unsigned char *>(host32);
    en.stage(b, rooms, keys, turns, host, off_keys, off_turns);
    char *dev = nullptr;
    if ((st = pool_scratch(b, total, &dev)) != GE_OK) return st;
    hipStream_t s = b->last_stream;
    if ((st = order_after_previous(b, s)) != GE_OK) return st;
    HIP_TRY(hipMemcpyAsync(dev, host, off_ev, hipMemcpyHostToDevice, s));
    if ((st = launch_pool_turn(b, s, en, dev, off_keys, off_turns, off_ev)) != GE_OK) return st;
    uint32_t *h_ev = reinterpret_cast<uint32_t *>(host + off_ev);
    HIP_TRY(hipMemcpyAsync(h_ev, dev + off_ev, 16 * (size_t)n, hipMemcpyDeviceToHost, s));
    if ((st = sync_impl(b)) != GE_OK) return st;
    if (events)
        for (size_t i = 0; i < n; i++) pool_decode_event(h_ev + 4 * i, b->segs[en.seg_at(i)].table, events[en.order[i]]);
    return GE_OK;
}

static int read_rooms_at_impl(ge_batch *b, uint64_t n, const uint64_t *rooms, ge_room_view *dst) {
    for (uint64_t k = 0; k < n; k++)
        if (rooms[k] >= b->n_rooms) return GE_ERR_RANGE;
    if (n == 0) return GE_OK;
    GE_ON_DEVICE(b);
    int st = sync_impl(b);
    if (st != GE_OK) return st;
    // [rooms u64 x n][records 12 words x n]
    const size_t off_rec = 8 * (size_t)n, total = off_rec + 48 * (size_t)n;
    uint32_t *host32 = nullptr;
    if ((st = io_stage(b, total, &host32)) != GE_OK) return st;
    unsigned char *host = reinterpret_cast<unsigned char *>(host32);
    memcpy(host, rooms, 8 * (size_t)n);
    char *dev = nullptr;
    if ((st = pool_scratch(b, total, &dev)) != GE_OK) return st;
    hipStream_t s = b->last_stream;
    if ((st = order_after_previous(b, s)) != GE_OK) return st;
    HIP_TRY(hipMemcpyAsync(dev, host, off_rec, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(ge_pool_gather, dim3((uint32_t)((n + 63u) / 64u)), dim3(64), 0, s, b->segs_dev, (uint32_t)b->segs.size(),
                       reinterpret_cast<const uint64_t *>(dev), n, reinterpret_cast<uint32_t *>(dev + off_rec));
    HIP_TRY(hipGetLastError());
    const uint32_t *h_rec = reinterpret_cast<const uint32_t *>(host + off_rec);
    HIP_TRY(hipMemcpyAsync(host + off_rec, dev + off_rec, 48 * (size_t)n, hipMemcpyDeviceToHost, s));
    if ((st = sync_impl(b)) != GE_OK) return st;
    for (uint64_t k = 0; k < n; k++) {
        const Segment &sg = b->segs[pool_segment_of(b, rooms[k])];
        uint32_t w[12] = {0};
        for (uint32_t x = 0; x < sg.dev.words; x++) w[x] = h_rec[12 * k + x];
        words_to_view(sg.dev.kind, w, sg.table, (int)sg.dev.n_players, dst[k]);
    }
    return GE_OK;
}

static int write_rooms_at_impl(ge_batch *b, uint64_t n, const uint64_t *rooms, const ge_room_view *src) {
    if (n == 0) return GE_OK;
    int st = pool_check_rooms(b, n, rooms);                       // all-or-nothing: every entry is checked before anything is written
    if (st != GE_OK) return st;
    std::vector<uint32_t> seg_of((size_t)n);
    for (uint64_t k = 0; k < n; k++) {
        seg_of[k] = pool_segment_of(b, rooms[k]);
        const Segment &sg = b->segs[seg_of[k]];
        if (!view_fits(src[k], sg.table, sg.dev.n_players)) { g_last_rejected_room = rooms[k]; return GE_ERR_ARG; }
    }
    GE_ON_DEVICE(b);
    if ((st = sync_impl(b)) != GE_OK) return st;
    // one upload: [rooms u64 x n (padded to 16 B)][records 12 words x n]
    const size_t off_rec = up16(8 * (size_t)n), total = off_rec + 48 * (size_t)n;
    uint32_t *host32 = nullptr;
    if ((st = io_stage(b, total, &host32)) != GE_OK) return st;
    unsigned char *host = reinterpret_cast<unsigned char *>(host32);
    memcpy(host, rooms, 8 * (size_t)n);
    uint32_t *h_rec = reinterpret_cast<uint32_t *>(host + off_rec);
    for_room_ranges(n, [&](uint64_t lo, uint64_t hi) {
        for (uint64_t k = lo; k < hi; k++) {
            const Segment &sg = b->segs[seg_of[k]];
            uint32_t *w = h_rec + 12 * k;
            memset(w, 0, 48);
            view_to_words(sg.dev.kind, src[k], sg.table, w);
        }
    });
    char *dev = nullptr;
    if ((st = pool_scratch(b, total, &dev)) != GE_OK) return st;
    hipStream_t s = b->last_stream;
    if ((st = order_after_previous(b, s)) != GE_OK) return st;
    HIP_TRY(hipMemcpyAsync(dev, host, total, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(ge_pool_scatter, dim3((uint32_t)((n + 63u) / 64u)), dim3(64), 0, s, b->segs_dev, (uint32_t)b->segs.size(),
                       reinterpret_cast<const uint64_t *>(dev), n, reinterpret_cast<const uint32_t *>(dev + off_rec));
    HIP_TRY(hipGetLastError());
    return sync_impl(b);
}

extern "C" {

int ge_batch_step_rooms(ge_batch *b, uint64_t n, const uint64_t *rooms, const uint64_t *keys, const uint32_t *turns,
                        ge_turn_event *events) {
    if (!b) return GE_ERR_ARG;
    return guarded([&] { return step_rooms_impl(b, n, rooms, keys, turns, events); });
}

int ge_batch_read_rooms_at(ge_batch *b, uint64_t n, const uint64_t *rooms, ge_room_view *dst, size_t cap_bytes) {
    if (!b || (n && (!rooms || !dst))) return GE_ERR_ARG;
    if (cap_bytes / sizeof(ge_room_view) < n) return GE_ERR_ARG;
    return guarded([&] { return read_rooms_at_impl(b, n, rooms, dst); });
}

int ge_batch_write_rooms_at(ge_batch *b, uint64_t n, const uint64_t *rooms, const ge_room_view *src) {
    if (!b || (n && (!rooms || !src))) return GE_ERR_ARG;
    return guarded([&] { return write_rooms_at_impl(b, n, rooms, src); });
}

}  // extern "C"

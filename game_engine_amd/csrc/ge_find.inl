// ge_find.inl — the rooms of a resident batch that need attention (ge_batch_find_rooms, POLICY.md §3k): the stop tests of
// ge_batch_run_rooms over a whole range of rooms as they stand, and an ordered compaction of the hits (included at the end of
// ge_step.hip, behind ge_timeline.inl: the existing kernels keep their code-object offsets).  Nothing is written but the call's
// own scratch (pool_scratch): records, prepared deals, the turn counter and the trace buffer stay as they are.
//
// Three kinds of launch, none of which waits for another block:
//   ge_find_kernel   lane = room, the record loaded as the step kernels load it (load_words: 16-byte plane loads, a wavefront
//                    reads 64 consecutive elements of each plane).  One result word per room - why | pending << 8 | row << 24,
//                    or 0 - and one match count per wavefront (__ballot + popcount).  One launch per segment of the range: a
//                    segment's part of the range owns a stretch of result words padded to whole wavefronts.
//   ge_find_scan     one block: the exclusive scan of the wavefront counts, FIND_SCAN_WAVES of them per pass, and the total
//                    (find_scan_block: ge_decide.inl's ge_gather_scan is the same block with another way to report the total).
//   ge_find_emit     re-reads the result words (not the records) and stores each hit at its wavefront's offset + its rank among
//                    the wavefront's hits (mbcnt), dropping what lies at or beyond cap.  So the order of the output is the order
//                    of the rooms, whatever the order the blocks ran in.
//
// The PERSON test is ge_batch_run_rooms's, as ge_pool.inl's lane type has it (Lane::pending; ge_run.inl's turn loop keeps its own
// inline copy per game, see ge_pool.inl's header): Werewolf - the row of the room's phase, ww_targets less who has acted, within
// the human mask; Two-Truths - inject_tt on a copy of the record per seat of the human mask, choice 1.  `pending` is that mask
// seat by seat.  The mask is the room's own where the batch has a seat plane (ge_pool.inl lane_seat_mask), so the test is per
// lane; a wavefront whose rooms have no host-driven seat still skips it wave-uniformly (Lane::probe).

namespace {

constexpr uint32_t FIND_BLOCK = 256u;           // threads of a test / emit block: four wavefronts
constexpr uint32_t FIND_SCAN_WAVES = 1024u;     // wavefront counts one pass of the scan block covers (65 536 rooms)

struct FindArgs {
    uint32_t *res;             // this part's result words (padded to whole wavefronts)
    uint32_t *counts;          // this part's wavefront counts
    const uint16_t *seats;     // the batch's seat plane, or null (ge_pool.inl lane_seat_mask)
    uint64_t r0, nr;           // the part: segment-local rooms r0 .. r0 + nr - 1
    uint32_t seg, want, row_mask, pad;
};

// a part of the range: result words [res_off, next part's res_off) are batch rooms lo, lo + 1, ...
struct FindParts {
    uint64_t res_off[GE_MAX_SEGMENTS], lo[GE_MAX_SEGMENTS];
    uint32_t seg[GE_MAX_SEGMENTS];
    uint32_t n;
};

__device__ __forceinline__ uint32_t find_word(uint32_t want, uint32_t pending, uint32_t phase, uint32_t term_mask, uint32_t row_mask) {
    uint32_t why = pending ? (want & GE_FIND_PERSON) : 0u;
    why |= ((term_mask >> phase) & 1u) ? (want & GE_FIND_END) : 0u;
    why |= ((row_mask >> phase) & 1u) ? (want & GE_FIND_PHASE) : 0u;
    return why ? why | (pending << 8) | (phase << 24) : 0u;
}

template <int NB, bool WWP, int GENERIC>
__device__ __forceinline__ uint32_t find_lane(const SegDev &sg, const DevTable *__restrict__ tables, const FindArgs &a, uint64_t room) {
    using Ln = Lane<NB, WWP, GENERIC>;
    using L = typename Ln::L;
    uint32_t w[L::WORDS];
    load_words<L::WORDS>(sg.base, sg.rooms_padded, room, w);
    const uint32_t human = lane_seat_mask(sg, a.seats, room);
    const uint32_t probe = Ln::probe(sg, a.seats, human);
    Ln lane;                                                  // no turn is played: no queue, no key
    lane.open(sg, tables, nullptr, w, 0u, true, human);
    const uint32_t pending = (a.want & GE_FIND_PERSON) && probe != 0u ? lane.pending(human, probe) : 0u;   // (wave-uniform)
    return find_word(a.want, pending, lane.phase(), lane.term_mask(), a.row_mask);
}

template <int KIND, int GENERIC>
__global__ void __launch_bounds__(FIND_BLOCK) ge_find_kernel(const SegDev *__restrict__ segs, const DevTable *__restrict__ tables, const FindArgs a) {
    const SegDev &sg = segs[a.seg];
    const uint64_t k = (uint64_t)blockIdx.x * FIND_BLOCK + threadIdx.x;
    const bool valid = k < a.nr;
    const uint64_t room = a.r0 + (valid ? k : 0u);            // lanes past the part test its first room and report nothing
    uint32_t r = find_lane<KindOf<KIND>::NB, KindOf<KIND>::WW, GENERIC>(sg, tables, a, room);
    r = valid ? r : 0u;
    const uint64_t hits = __ballot(r != 0u);
    const uint64_t padded = (a.nr + 63u) & ~(uint64_t)63u;
    if (k < padded) {                                         // (wave-uniform: padded is a multiple of 64)
        a.res[k] = r;
        if ((threadIdx.x & 63u) == 0u) a.counts[k >> 6] = (uint32_t)__popcll(hits);
    }
}

// counts[0 .. n_waves) -> offsets[w] = hits in front of wavefront w; returns all of them (in every thread).  One block of
// FIND_SCAN_WAVES threads: the body of ge_find_scan and of ge_gather_scan (ge_decide.inl)
__device__ __forceinline__ uint64_t find_scan_block(const uint32_t *__restrict__ counts, uint64_t n_waves, uint64_t *__restrict__ offsets) {
    __shared__ uint32_t wave_sum[FIND_SCAN_WAVES / 64u];
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
    uint64_t carry = 0;
    uint32_t next = t < n_waves ? counts[t] : 0u;
    for (uint64_t base = 0; base < n_waves; base += FIND_SCAN_WAVES) {
        const uint32_t v = next;
        const uint64_t nx = base + FIND_SCAN_WAVES + t;
        next = nx < n_waves ? counts[nx] : 0u;                // the next pass's load, in flight during this one
        uint32_t inc = v;                                     // inclusive scan inside the wavefront
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t o = __shfl_up(inc, d);
            inc += lane >= d ? o : 0u;
        }
        if (lane == 63u) wave_sum[wv] = inc;
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (uint32_t j = 0; j < FIND_SCAN_WAVES / 64u; j++) {
            const uint32_t x = wave_sum[j];
            before += j < wv ? x : 0u;
            all += x;
        }
        if (base + t < n_waves) offsets[base + t] = carry + before + (inc - v);
        carry += all;
        __syncthreads();
    }
    return carry;
}

// ... and *total = all of them
__global__ void __launch_bounds__(FIND_SCAN_WAVES) ge_find_scan(const uint32_t *__restrict__ counts, uint64_t n_waves, uint64_t *__restrict__ offsets,
                                                                uint64_t *__restrict__ total) {
    const uint64_t all = find_scan_block(counts, n_waves, offsets);
    if (threadIdx.x == 0u) *total = all;
}

// result word j -> hits[offset of its wavefront + rank], if below cap
__global__ void __launch_bounds__(FIND_BLOCK) ge_find_emit(const uint32_t *__restrict__ res, uint64_t n_words, const uint64_t *__restrict__ offsets,
                                                           const FindParts parts, u32x4 *__restrict__ hits, uint64_t cap) {
    const uint64_t j = (uint64_t)blockIdx.x * FIND_BLOCK + threadIdx.x;
    if (j >= n_words) return;                                 // (wave-uniform: n_words is a multiple of 64)
    const uint32_t r = res[j];
    const uint64_t m = __ballot(r != 0u);
    if (r == 0u) return;
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    const uint64_t at = offsets[j >> 6] + rank;
    if (at >= cap) return;
    uint32_t p = 0;
    for (uint32_t x = 1; x < parts.n; x++)
        if (j >= parts.res_off[x]) p = x;
    const uint64_t room = parts.lo[p] + (j - parts.res_off[p]);
    u32x4 h;                                                  // ge_room_hit: room, why, pending | row << 16 | segment << 24 (the host puts the phase id for the row)
    h.x = (uint32_t)room; h.y = (uint32_t)(room >> 32);
    h.z = r & 255u;
    h.w = ((r >> 8) & 0xFFFFu) | ((r >> 24) << 16) | (parts.seg[p] << 24);
    hits[at] = h;
}

template <int GEN> hipError_t find_launch(uint32_t kind, dim3 grid, hipStream_t st, const ge_batch *b, const FindArgs &a) {
    return by_kind(kind, [&](auto K) { hipLaunchKernelGGL((ge_find_kernel<K(), GEN>), grid, dim3(FIND_BLOCK), 0, st, b->segs_dev, b->tables, a); });
}

}  // namespace

static_assert(sizeof(ge_room_hit) == 16, "a hit is one 16-byte store");
static_assert(GE_FIND_PERSON == GE_RUN_UNTIL_PERSON && GE_FIND_END == GE_RUN_UNTIL_END, "the tests of ge_batch_run_rooms");

static int find_rooms_impl(ge_batch *b, uint64_t first, uint64_t count, uint32_t want, const uint32_t *phase_masks, ge_room_hit *hits, uint64_t cap,
                           uint64_t *n_hits, uint64_t *n_match) {
    // all before anything runs, in this order (ABI behaviour)
    if (want == 0u || (want & ~(uint32_t)(GE_FIND_PERSON | GE_FIND_END | GE_FIND_PHASE))) return GE_ERR_ARG;
    if (!n_hits || !n_match) return GE_ERR_ARG;
    if (!hits && cap > 0u) return GE_ERR_ARG;
    uint32_t row_mask[GE_MAX_SEGMENTS] = {0};                   // the phase ids asked for, as rows of each segment's table
    if (want & GE_FIND_PHASE) {
        if (!phase_masks) return GE_ERR_ARG;
        for (size_t g = 0; g < b->segs.size(); g++) {
            const ge_game_table &tb = b->segs[g].table;
            if (tb.n_phases < 32 && (phase_masks[g] >> tb.n_phases) != 0u) return GE_ERR_ARG;
            for (int r = 0; r < tb.n_phases; r++)
                if (tb.rows[r].phase_id >= 0 && tb.rows[r].phase_id < 32 && ((phase_masks[g] >> tb.rows[r].phase_id) & 1u)) row_mask[g] |= 1u << r;
        }
    }
    if (first + count > b->n_rooms || first + count < first) return GE_ERR_RANGE;
    if (count == 0u) { *n_hits = 0; *n_match = 0; return GE_OK; }
    GE_ON_DEVICE(b);
    int st = sync_impl(b);
    if (st != GE_OK) return st;
    // the parts of the range, a segment each; their result words padded to whole wavefronts
    struct Part { uint32_t seg; uint64_t r0, nr, res_off; };
    std::vector<Part> part;
    FindParts fp;
    memset(&fp, 0, sizeof fp);
    uint64_t n_words = 0;
    for (uint32_t g = 0; g < (uint32_t)b->segs.size(); g++) {
        const Segment &s = b->segs[g];
        const uint64_t lo = std::max(first, s.local_first), hi = std::min(first + count, s.local_first + s.dev.rooms);
        if (lo >= hi) continue;
        fp.res_off[fp.n] = n_words; fp.lo[fp.n] = lo; fp.seg[fp.n] = g; fp.n++;
        part.push_back({g, lo - s.local_first, hi - lo, n_words});
        n_words += (hi - lo + 63u) & ~(uint64_t)63u;
    }
    const uint64_t n_waves = n_words / 64u, hit_cap = std::min(cap, count);
    // scratch: [result words][wavefront counts][wavefront offsets u64][total u64, padded][hits 16 B x min(cap, count)]
    const size_t off_cnt = 4 * (size_t)n_words, off_pre = up16(off_cnt + 4 * (size_t)n_waves), off_tot = off_pre + 8 * (size_t)n_waves;
    const size_t off_hits = up16(off_tot + 8), total = off_hits + 16 * (size_t)hit_cap;
    char *dev = nullptr;
    if ((st = pool_scratch(b, total, &dev)) != GE_OK) return st;
    hipStream_t s = b->last_stream;
    if ((st = order_after_previous(b, s)) != GE_OK) return st;
    hipEvent_t e1 = nullptr;                                      // ge_batch_kernel_time counts the launches of this call as one interval
    if ((st = timing_begin(b, s, &e1)) != GE_OK) return st;
    for (const Part &p : part) {
        FindArgs a;
        a.res = reinterpret_cast<uint32_t *>(dev) + p.res_off;
        a.counts = reinterpret_cast<uint32_t *>(dev + off_cnt) + p.res_off / 64u;
        a.seats = b->seats;
        a.r0 = p.r0; a.nr = p.nr; a.seg = p.seg; a.want = want; a.row_mask = row_mask[p.seg]; a.pad = 0;
        const dim3 grid((uint32_t)((p.nr + FIND_BLOCK - 1u) / FIND_BLOCK));
        HIP_TRY(b->plan.generic ? find_launch<1>(b->segs[p.seg].dev.kind, grid, s, b, a) : find_launch<0>(b->segs[p.seg].dev.kind, grid, s, b, a));
    }
    uint64_t *d_pre = reinterpret_cast<uint64_t *>(dev + off_pre), *d_tot = reinterpret_cast<uint64_t *>(dev + off_tot);
    hipLaunchKernelGGL(ge_find_scan, dim3(1), dim3(FIND_SCAN_WAVES), 0, s, reinterpret_cast<const uint32_t *>(dev + off_cnt), n_waves, d_pre, d_tot);
    HIP_TRY(hipGetLastError());
    if (hit_cap) {
        hipLaunchKernelGGL(ge_find_emit, dim3((uint32_t)((n_words + FIND_BLOCK - 1u) / FIND_BLOCK)), dim3(FIND_BLOCK), 0, s,
                           reinterpret_cast<const uint32_t *>(dev), n_words, d_pre, fp, reinterpret_cast<u32x4 *>(dev + off_hits), hit_cap);
        HIP_TRY(hipGetLastError());
    }
    if (e1) HIP_TRY(hipEventRecord(e1, s));
    // the total first; then the hits there are, and no more
    uint32_t *host32 = nullptr;
    if ((st = io_stage(b, 16, &host32)) != GE_OK) return st;
    HIP_TRY(hipMemcpyAsync(host32, d_tot, 8, hipMemcpyDeviceToHost, s));
    if ((st = sync_impl(b)) != GE_OK) return st;
    uint64_t matched;
    memcpy(&matched, host32, 8);
    const uint64_t got = std::min(matched, hit_cap);
    if (got) {
        if ((st = io_stage(b, 16 * (size_t)got, &host32)) != GE_OK) return st;
        HIP_TRY(hipMemcpyAsync(host32, dev + off_hits, 16 * (size_t)got, hipMemcpyDeviceToHost, s));
        if ((st = sync_impl(b)) != GE_OK) return st;
        for (uint64_t i = 0; i < got; i++) {
            const uint32_t *h = host32 + 4 * i;
            ge_room_hit &o = hits[i];
            o.room = (uint64_t)h[0] | ((uint64_t)h[1] << 32);
            o.why = h[2];
            o.pending = (uint16_t)(h[3] & 0xFFFFu);
            o.segment = (uint8_t)(h[3] >> 24);
            o.phase_id = (uint8_t)b->segs[o.segment].table.rows[(h[3] >> 16) & 255u].phase_id;
        }
    }
    *n_hits = got; *n_match = matched;
    return GE_OK;
}

extern "C" {

int ge_batch_find_rooms(ge_batch *b, uint64_t first, uint64_t count, uint32_t want, const uint32_t *phase_masks, ge_room_hit *hits, uint64_t cap,
                        uint64_t *n_hits, uint64_t *n_match) {
    if (!b) return GE_ERR_ARG;
    return guarded([&] { return find_rooms_impl(b, first, count, want, phase_masks, hits, cap, n_hits, n_match); });
}

}  // extern "C"

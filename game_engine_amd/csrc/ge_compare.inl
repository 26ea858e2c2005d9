// ge_compare.inl — paired comparison of playout entries (ge_batch_rollout_compare, POLICY.md §3e): entry k against its baseline
// entry, playout by playout (included at the end of ge_step.hip, behind ge_playout.inl: the existing kernels keep their
// code-object offsets).  The call is rollout_call of ge_rollout.inl with act = 3: its checks, its chunk staging over ge_pool.inl's
// PoolEntries and its launch by kind; what this file adds is the comparison kernel behind the playouts and the entry point
// (and ge_batch_rollout_beliefs's, which is either call under POLICY.md §3j).
//
// The playouts are ge_batch_rollout_seats's, launched as form ACT = 3 of ge_rollout_kernel (ge_rollout.inl): the same turns and
// the same reduction, and one byte more per lane - the outcome X of its replica for the entry's subject seat - stored into the
// entry's row of an outcome plane in the call's device scratch (waves * 64 bytes per row, a lane past R stores 0).  The plane
// never leaves the device.
//
// ge_compare_kernel is a launch of its own behind the playouts of every segment of the chunk, on the same stream: an entry and
// its baseline are played by different workgroups, usually on different compute units, and a compute unit's vector L1 is not
// refreshed by the stores of others; the kernel boundary is what makes every outcome byte (and every refusal in `status`)
// visible.  The comparison therefore cannot be folded into the playout kernel.
//
// Reduction.  One wavefront per entry walks its row and its baseline's row, 16 bytes per lane and 1 KiB per step, keeps the five
// sums per lane in 32-bit registers (a lane sees at most 2^20 / 64 bytes of at most 255 each: diff_sq <= 2^14 x 255^2 < 2^31),
// folds them with wave_sum (ge_kernels.inl) and lane 0 stores the entry's six words once.  Chosen over one wavefront per
// (entry, 64 replicas) with u64 atomics, as roll_reduce does: there a wavefront has tens to hundreds of turns of work behind
// each atomic, here it would have one 64-byte load, so the atomics (and a memset of the accumulators before them) would be
// the whole cost; a row is read at full width instead, nothing needs zeroing, and the n * R bytes of both rows are small beside
// the playouts that wrote them.  Lanes past R hold 0 in both rows and so add nothing; no masking is needed.  Every sum is an
// integer sum formed in a fixed order, so the result does not depend on the order the wavefronts arrive in.

namespace {

struct CompareArgs {
    const int32_t *status;      // the chunk's verdicts (sorted positions): GE_OK unless the device refused the entry
    const uint32_t *baseline;   // entry e's baseline, as a sorted position of the same chunk
    uint32_t n, n_rollouts, row;   // row: bytes per row (waves * 64)
};

// out: 6 words per entry, in ge_compare_stats's order
__global__ void __launch_bounds__(64) ge_compare_kernel(const unsigned char *__restrict__ plane, unsigned long long *__restrict__ out,
                                                        const CompareArgs a) {
    const uint32_t e = blockIdx.x, lane = threadIdx.x;
    const uint32_t be = (uint32_t)__builtin_amdgcn_readfirstlane(a.baseline[e]);
    const bool ok = __builtin_amdgcn_readfirstlane(a.status[e]) == GE_OK && __builtin_amdgcn_readfirstlane(a.status[be]) == GE_OK;
    uint32_t better = 0, worse = 0, gain = 0, loss = 0, sq = 0;
    if (ok && be != e) {                                      // (wave-uniform; a refused entry's row was never written)
        const unsigned char *pk = plane + (size_t)e * a.row, *pb = plane + (size_t)be * a.row;
        for (uint32_t off = lane * 16u; off < a.row; off += 1024u) {   // row is a multiple of 64: off + 16 <= row
            const u32x4 vk = *reinterpret_cast<const u32x4 *>(pk + off), vb = *reinterpret_cast<const u32x4 *>(pb + off);
#pragma unroll
            for (int j = 0; j < 4; j++)
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const uint32_t x = (vk[j] >> (8 * q)) & 255u, y = (vb[j] >> (8 * q)) & 255u;
                    const uint32_t up = x > y ? x - y : 0u, down = y > x ? y - x : 0u;
                    better += x > y ? 1u : 0u;
                    worse += y > x ? 1u : 0u;
                    gain += up;
                    loss += down;
                    sq += (up + down) * (up + down);
                }
        }
    }
    const uint64_t s0 = wave_sum(better), s1 = wave_sum(worse), s2 = wave_sum(gain), s3 = wave_sum(loss), s4 = wave_sum(sq);
    if (lane == 0) {
        unsigned long long *o = out + 6u * (size_t)e;
        o[0] = ok ? a.n_rollouts : 0u; o[1] = s0; o[2] = s1; o[3] = s2; o[4] = s3; o[5] = s4;
    }
}

}  // namespace

static hipError_t compare_launch(hipStream_t s, char *dev, const RollStage &o, uint32_t cn, uint32_t n_rollouts, uint32_t waves) {
    static_assert(sizeof(ge_compare_stats) == 48, "ge_compare_kernel stores six words per entry");
    CompareArgs a;
    a.status = reinterpret_cast<const int32_t *>(dev + o.status);
    a.baseline = reinterpret_cast<const uint32_t *>(dev + o.baseline);
    a.n = cn; a.n_rollouts = n_rollouts; a.row = waves * 64u;
    hipLaunchKernelGGL(ge_compare_kernel, dim3(cn), dim3(64), 0, s, reinterpret_cast<const unsigned char *>(dev + o.plane),
                       reinterpret_cast<unsigned long long *>(dev + o.cmp), a);
    return hipGetLastError();
}

extern "C" {

int ge_batch_rollout_compare(ge_batch *b, uint64_t n, const uint64_t *rooms, const uint64_t *keys, const uint32_t *turns, const uint32_t *seats,
                             const uint32_t *first_action, const uint32_t *player_ids, const uint32_t *choices, int32_t *entry_status,
                             uint32_t n_rollouts, uint32_t max_turns, uint64_t seed, ge_rollout_stats *out, const uint32_t *baseline,
                             const uint32_t *subjects, ge_compare_stats *cmp) {
    RollRequest r = {n, rooms, keys, turns, seats, first_action, player_ids, choices, entry_status, n_rollouts, max_turns, seed, out, 3};
    r.baseline = baseline; r.subjects = subjects; r.cmp = cmp;
    return rollout_call(b, r);
}

// ge_batch_rollout_seats (no comparison arrays) or ge_batch_rollout_compare under the entries' beliefs (POLICY.md §3j): forms
// ACT = 6 / 7 of ge_rollout_kernel.  Some but not all of the comparison arrays: act 3, whose first check refuses the call
int ge_batch_rollout_beliefs(ge_batch *b, uint64_t n, const uint64_t *rooms, const uint64_t *keys, const uint32_t *turns, const uint32_t *seats,
                             const uint32_t *first_action, const uint32_t *player_ids, const uint32_t *choices, int32_t *entry_status,
                             const uint8_t *beliefs, uint32_t n_rollouts, uint32_t max_turns, uint64_t seed, ge_rollout_stats *out,
                             const uint32_t *baseline, const uint32_t *subjects, ge_compare_stats *cmp) {
    const bool comparing = baseline || subjects || cmp;
    RollRequest r = {n, rooms, keys, turns, seats, first_action, player_ids, choices, entry_status, n_rollouts, max_turns, seed, out, comparing ? 3 : 2};
    r.baseline = baseline; r.subjects = subjects; r.cmp = cmp;
    r.weighted = true; r.beliefs = beliefs;
    return rollout_call(b, r);
}

}  // extern "C"

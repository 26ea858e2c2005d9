// ge_plan.h - what ge_batch_step launches, decided from plain values: the tuning knobs (read from the environment once per
// process), the batch-time plan (block size, grid, record loads, Two-Truths shape builds), the plan of one launch (which
// kernel build, which grid) and the sequence of launches of one step.  Plain C++17 beside ge_host.h, no HIP: ge_step.hip maps a
// plan to a template instantiation and launches it, tests/native/launch_plan.cpp prints plans under g++ with ASan + UBSan
// (tests/test_launch_plan.py).  Every figure quoted here was measured on MI355X; the file names are under profiles/.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <algorithm>

#include "../../include/ge_step.h"
#include "ge_layout.h"

namespace ge {

// ---- the knobs: tuning / A-B runs and the forced builds of tests/test_gpu_knobs.py.  get(name) = getenv or a test's own table
struct LaunchKnobs {
    uint32_t block_threads = 0;                          // GE_BLOCK_THREADS = 64 / 128 / 256: rooms per block (0: by size)
    int nt_loads = -1;                                   // GE_NT_LOADS = 0 / 1: plain / streaming record loads (-1: by layout and size)
    bool no_generic_shapes = false;                      // GE_NO_GENERIC_SHAPES: the rolled condition walk for every table
    uint64_t low_rooms = 1024u * 64u + 1u;               // GE_LOWOCC_ROOMS: below this many rooms the lone-wavefront build
    uint32_t single_block = 0;                           // GE_SINGLE_BLOCK = 256 / 512 / 1024: rooms per block of large single-turn launches (0: by size)
    int half_waves = -1;                                 // GE_HALF_WAVES = 0 / 1: half-filled lone wavefronts off / on (-1: by size)
    bool no_graph = false;                               // GE_NO_GRAPH: plain launches where a step would replay a graph
};

template <class Get> inline LaunchKnobs parse_knobs(Get &&get) {
    LaunchKnobs k;
    auto one_of = [&get](const char *name, unsigned long a, unsigned long b, unsigned long c) {   // any other value: as if unset
        const char *e = get(name);
        const unsigned long v = e ? strtoul(e, nullptr, 10) : 0ul;
        return (v == a || v == b || v == c) ? (uint32_t)v : 0u;
    };
    k.block_threads = one_of("GE_BLOCK_THREADS", 64, 128, 256);
    k.single_block = one_of("GE_SINGLE_BLOCK", 256, 512, 1024);
    if (const char *e = get("GE_NT_LOADS")) k.nt_loads = atoi(e);
    if (const char *e = get("GE_HALF_WAVES")) k.half_waves = atoi(e);
    if (const char *e = get("GE_LOWOCC_ROOMS")) k.low_rooms = strtoull(e, nullptr, 10);
    k.no_generic_shapes = get("GE_NO_GENERIC_SHAPES") != nullptr;
    k.no_graph = get("GE_NO_GRAPH") != nullptr;
    return k;
}

inline const LaunchKnobs &launch_knobs() {               // the process's knobs: the environment as the first batch found it
    static const LaunchKnobs k = parse_knobs([](const char *name) { return (const char *)getenv(name); });
    return k;
}

// ---- the batch-time plan: everything a launch's plan needs of the batch
struct PlanSeg { uint32_t kind, words; uint64_t rooms; };
struct BatchPlan {
    const LaunchKnobs *knobs = nullptr;                  // the process's (launch_knobs), or a test's own
    uint32_t n_seg = 0, kind0 = 0;
    uint64_t rooms0 = 0;
    uint32_t tt_queue_min = 5;                           // ge_kernels.inl GE_TT_LOW_QUEUE_MIN, passed in by ge_step.hip (which asserts that plan_uses_queue is tt_uses_queue)
    uint32_t block_threads = 256, n_blocks = 0;          // the fused launches' rooms per block and grid ...
    uint32_t block_begin[GE_MAX_SEGMENTS] = {0};         // ... in which segment k starts at this block (segments are padded to the block size)
    bool low = false;                                    // the lone-wavefront builds (ge_device.h LOWOCC)
    bool stream_loads = false;                           // a single-game batch's large single-turn launches load the record with streaming loads
    bool generic = false;                                // some phase has a generic target condition: the GENERIC kernel builds are launched
    uint32_t gshape = 0;                                 // ... a single Two-Truths table whose conditions all fit 1 x 1 / 1 x 2 literal slots: 2 / 3 = the shape-specialised fused builds
    uint32_t cond_bytes = 0;                             // ... and their blocks keep this much of literal image in LDS (the largest table's)
    uint32_t stamp_records = 0;                          // wavefronts of the batch's largest launch (the GE_STAMPS = 2 timeline: a record each)
};

// ---- one launch of the step kernel.  What is launched is chosen from four facts, each a template argument of the kernels so that
// every build gets its own register allocation (ge_kernels.inl): the record layout (or "mixed": several segments), LOWOCC (up to
// one wavefront per SIMD), GENERIC (some table has a generic target condition) and SINGLE (the launch is exactly one turn).
enum LoadForm : uint32_t { LOAD_DEFAULT = 0, LOAD_ALT = 1, LOAD_NO_RECYCLE = 2 };
struct LaunchPlan {
    bool low, single, mixed;
    uint32_t gen;                                        // the kernels' GENERIC: 0, 1 (rolled walk), 2 / 3 (BatchPlan::gshape)
    LoadForm load;
    uint32_t bt, blocks, rpb;                            // threads per block, blocks, rooms per block
    bool queue, pull;                                    // the block's LDS holds action queues / pull queues (ge_kernels.inl step_lds_bytes)
};

constexpr bool plan_uses_queue(uint32_t kind, bool low, uint32_t tt_queue_min) {   // Two-Truths lone wavefronts of few players run without a queue
    return kind == K_WW8 || kind == K_WW12 || !low || (kind == K_TT4 ? 4u : kind == K_TT8 ? 8u : 12u) >= tt_queue_min;
}
constexpr bool plan_pull_queue(uint32_t kind, bool low, uint32_t gen, bool single) { return kind == K_WW8 && low && gen == 0u && !single; }

inline LaunchPlan launch_plan(const BatchPlan &b, uint32_t n_turns, bool restart) {
    const LaunchKnobs &kn = *b.knobs;
    LaunchPlan p;
    p.single = n_turns == 1u; p.mixed = b.n_seg > 1; p.low = b.low;
    const bool low = p.low, single = p.single, one_game = !p.mixed;
    p.gen = !b.generic ? 0u : (one_game && b.gshape && !single) ? b.gshape : 1u;
    // (the large-batch single-turn kernels of the shipped games exist with plain and with streaming record loads: ALT = the form that is not the
    // layout's default - Werewolf x 8 plain, the others streaming - launched when the batch's stream_loads (batch_plan: record_loads) differs
    // from that default.  The fused lone-wavefront Werewolf x 8 kernel compiles in whether its turns recycle finished rooms - ge_kernels.inl
    // run_ww: the default form is the restart-on kernel, NO_RECYCLE the restart-off one)
    p.load = (one_game && single && !low && p.gen == 0u && b.stream_loads != (b.kind0 != K_WW8)) ? LOAD_ALT
           : (one_game && b.kind0 == K_WW8 && low && !single && p.gen == 0u && !restart) ? LOAD_NO_RECYCLE : LOAD_DEFAULT;
    p.queue = p.mixed || plan_uses_queue(b.kind0, low, b.tt_queue_min);
    p.pull = one_game && p.load != LOAD_ALT && plan_pull_queue(b.kind0, low, p.gen, single);
    uint32_t &bt = p.bt, &blocks = p.blocks, &rpb = p.rpb;
    bt = b.block_threads; blocks = b.n_blocks;
    rpb = bt;                                                   // rooms per block
    // One turn per launch (max_fuse = 1, or the tail of a step): a block's first act is to fill its 7 KB of LDS tables behind a
    // barrier - the fewer blocks, the less of that per launch - so a large single-game Werewolf x 8 batch runs these launches in
    // blocks of 512 rooms (GE_SINGLE_BLOCK = 256 / 512 / 1024 overrides, for A/B runs); a single game's rooms start at block 0,
    // so the grid is just the rooms over the block size
    // (profiles/r04_ab_single_block.txt, sustained us per launch at 256 / 512 / 1 024 rooms per block: Werewolf x 8 14.23 / 14.01 /
    // 14.22 at 1 M rooms and 386 / 373 / 377 at 33 M; Werewolf x 12 34.4 / 34.6 / 37.9 at 2 M; Two-Truths x 4 10.2 / 10.2 / 10.4)
    if (single && one_game && !b.generic && !low && bt == 256u) {
        // (not below 393 216 rooms: 300 000 rooms are 586 blocks of 512 - 2.3 per CU - and take 6.69 us against 6.10 in 256-room blocks)
        bt = kn.single_block ? kn.single_block : (b.kind0 == K_WW8 && b.rooms0 >= 393216u ? 512u : 256u);
        blocks = (uint32_t)((b.rooms0 + bt - 1u) / bt);
        rpb = bt;
    }
    // A single-game batch of up to 262 144 rooms is cut into 64-room blocks (batch_plan: more, shorter blocks balance a fused launch
    // better).  Its single-turn launches on the large-batch kernels run 256-room blocks all the same - a quarter of the table fills:
    // sustained us per launch, 64- against 256-room blocks (profiles/r05_k1_midsize.txt): Werewolf x 8 at 131 072 / 262 144 rooms
    // 4.96 / 6.35 -> 4.21 / 5.40, Two-Truths x 4 at 262 144 5.14 -> 4.58, Werewolf x 12 at 131 072 / 262 144 5.80 / 7.53 -> 5.10 / 6.90
    // (-8 .. -15 %; -29 % at 524 000 rooms, which batch_plan now cuts into 256-room blocks anyway; the lone-wavefront kernels, which fill
    // nothing, are level at 131 072 rooms and slower beyond).  A mixed batch's segments are padded to its block size, so it keeps it.
    if (single && one_game && !low && bt < 256u && kn.single_block == 0u) {
        bt = 256u;
        blocks = (uint32_t)((b.rooms0 + bt - 1u) / bt);
        rpb = bt;
    }
    // Half-filled lone wavefronts: a fused launch over a single-game batch of at most 32 768 rooms runs 32 rooms per wavefront (still
    // at most one wavefront per SIMD).  A lone wavefront's time is its instruction stream, whatever its lanes hold, and a wavefront of
    // 32 rooms almost never needs the second round of its action queue that 43 % (Werewolf x 8) to 86 % (x 12) of the 64-room
    // wave-turns take: at 32 768 rooms Werewolf x 8 1.09 -> 0.97 us per turn (-11 %), x 12 -16 %, Two-Truths x 4 / 8 / 12 -9 / -16 /
    // -19 % (profiles/r05_ab_half_waves.txt).  Not beyond 32 768: two such wavefronts on a SIMD take 1.39 us against 1.06 for one
    // full one - at this occupancy a SIMD issues about one instruction per 4 cycles in all.  Not for single-turn launches (twice the
    // blocks to fill tables for: up to +9 %).  GE_HALF_WAVES=0 / 1 forces it off / on (A/B, and a knob run of the test suite)
    const bool half_fits = one_game && low && bt == 64u && (!single || kn.half_waves == 1);
    if (half_fits && (kn.half_waves == 1 || (kn.half_waves != 0 && b.rooms0 <= 32768u))) {
        rpb = 32u;
        blocks = (uint32_t)((b.rooms0 + 31u) / 32u);
    } else if (half_fits && kn.half_waves != 0 && b.rooms0 < 65536u) {
        // between 32 768 and 65 536 rooms: as few rooms per wavefront as still give every SIMD at most one (49 152 rooms = 1 024 wavefronts of 48):
        // us per turn against 64 rooms per wavefront (profiles/r05_rooms_per_wavefront.txt) Werewolf x 8 at 40 000 / 49 152 / 57 000 rooms
        // 1.08 / 1.06 / 1.05 -> 0.98 / 0.96 / 1.02, x 12 1.51 / 1.49 / 1.49 -> 1.29 / 1.35 / 1.43, Two-Truths x 7 1.15 -> 1.01 / 1.01 / 1.09, x 4 -4 %
        rpb = (uint32_t)((b.rooms0 + 1023u) / 1024u);
        blocks = (uint32_t)((b.rooms0 + rpb - 1u) / rpb);
    }
    return p;
}

// seg[0 .. n_seg): the segments in batch order.  generic: some table has a generic row; cond_shape: the first table's
// DevTable::cond_shape where it has a literal image (else 0); cond_bytes: the largest table's literal image.  kn must outlive the plan.
inline BatchPlan batch_plan(const LaunchKnobs &kn, const PlanSeg *seg, uint32_t n_seg, uint32_t max_fuse, bool generic, uint32_t cond_shape, uint32_t cond_bytes,
                            uint32_t tt_queue_min = 5) {
    BatchPlan b;
    b.knobs = &kn; b.n_seg = n_seg; b.kind0 = seg[0].kind; b.rooms0 = seg[0].rooms; b.tt_queue_min = tt_queue_min;
    b.generic = generic; b.cond_bytes = cond_bytes;
    uint64_t n_rooms = 0;
    for (uint32_t k = 0; k < n_seg; k++) n_rooms += seg[k].rooms;
    // Rooms per block.  Up to four wavefronts per SIMD (262 144 rooms) 64-room blocks are as fast as any and balance best; beyond, a block's
    // LDS (the 7 KB table image + its wavefronts' queues) caps a CU at 5 wavefronts per SIMD when every wavefront brings its own image, and
    // the launch takes a second round: fused us per turn at 393 216 / 524 000 rooms, 64- against 256-room blocks: Werewolf x 8 3.50 / 4.66 ->
    // 2.54 / 3.52, Two-Truths x 4 at 524 000 3.31 -> 2.35, Werewolf x 12 6.46 -> 4.87 (-24 .. -28 %; level at 262 144 and below;
    // profiles/r05_fused_midsize.txt).  (Until round 5 the switch was at 524 288 rooms.)
    b.block_threads = n_rooms > (1u << 18) ? 256u : 64u;
    // a batch that only ever runs single-turn launches (max_fuse = 1) on the large-batch kernels: 256-room blocks at once (launch_plan does
    // the same per launch for a single-game batch; a mixed batch's block size is fixed here, its segments are padded to it)
    if (max_fuse == 1u && n_rooms > 65536u) b.block_threads = 256u;
    if (kn.block_threads) b.block_threads = kn.block_threads;   // tuning / A-B runs: 64, 128 or 256
    for (uint32_t k = 0; k < n_seg; k++) {
        b.block_begin[k] = b.n_blocks;
        b.n_blocks += (uint32_t)((seg[k].rooms + b.block_threads - 1) / b.block_threads);
    }
    // up to one wavefront per SIMD (1 024 SIMDs x 64 rooms) -> the branch-lean lone-wavefront build (ge_device.h LOWOCC):
    // 65 536 rooms 1.283 vs 1.372 us/turn; from the first SIMD with two wavefronts on the large-batch build is as fast or
    // faster (69 632 rooms 1.680 vs 1.668, 131 072: 1.791 vs 1.738; tools/threshold_probe.sh, profiles/r02_threshold.txt).
    // GE_LOWOCC_ROOMS overrides the threshold (tuning / A-B runs).  Mixed batches with generic tables: the large-batch build serves every size
    b.low = n_rooms < kn.low_rooms && !(generic && n_seg > 1);
    // record_loads - the record loads of a single-game batch's large single-turn launches, plain or streaming (non-temporal), by layout and by where the state
    // lives (ge_kernels.inl load_words; profiles/r05_ab_ww8_nt_loads.txt, r05_ab_nt_others.txt): beyond the 256 MiB Infinity Cache of MI355X
    // every layout streams; while the cache holds the state plain loads are served from it (+4 ... +18 % at 100 - 250 MiB), except that the
    // smallest states measured - Two-Truths at 24 MiB, Werewolf x 12 at 80 MiB - are level or 2 % better streaming.  GE_NT_LOADS=0 / 1 forces
    // plain / streaming (A/B, knob runs)
    {
        const size_t mib = (size_t)1 << 20, small = b.kind0 == K_WW8 ? 0 : b.kind0 == K_WW12 ? 96 * mib : 48 * mib;
        size_t touched = 0;                                     // what a launch reads: the records' own words (a layout's last plane is allocated 16 bytes wide)
        for (uint32_t k = 0; k < n_seg; k++) touched += (size_t)seg[k].words * 4u * ((seg[k].rooms + 255u) & ~uint64_t(255));
        b.stream_loads = kn.nt_loads >= 0 ? kn.nt_loads != 0 : (touched > 288 * mib || touched <= small);
    }
    // Two-Truths fused launches on a table whose generic conditions all have one of the common shapes: the shape-specialised builds
    // (GE_NO_GENERIC_SHAPES, A/B runs: the rolled walk for every table)
    if (n_seg == 1 && b.kind0 != K_WW8 && b.kind0 != K_WW12 && cond_shape && !kn.no_generic_shapes) {
        const uint32_t ncl = cond_shape & 7u, len = (cond_shape >> 4) & 7u;
        b.gshape = (ncl == 1u && len == 1u) ? 2u : (ncl == 1u && len == 2u) ? 3u : 0u;
    }
    // GE_STAMPS = 2 (diagnostic build): a timeline record per wavefront of a launch, so as many as the largest launch has - a
    // fused launch of half-filled lone wavefronts has up to twice the rooms over 64
    for (uint32_t n_turns : {max_fuse, 1u}) {
        const LaunchPlan p = launch_plan(b, n_turns, false);
        b.stamp_records = std::max(b.stamp_records, p.blocks * (p.bt / 64u));
    }
    return b;
}

// ---- the launches of one ge_batch_step(n_turns): max_fuse turns each, the last one the rest
constexpr uint32_t GRAPH_MIN_LAUNCHES = 4;
struct LaunchSeq {
    uint32_t n_launch, max_fuse, tail;                   // tail: turns of the last launch
    uint32_t turns(uint32_t i) const { return i + 1u < n_launch ? max_fuse : tail; }
    // some launch is a single turn (its Werewolf x 12 segments take deals from the side plane)
    bool has_single() const { return n_launch && (max_fuse == 1u || tail == 1u); }
    // A step that needs many launches (small max_fuse: interactive or traced stepping) is launch-bound for small batches: worth a graph replay
    // (GE_NO_GRAPH, A/B runs: never)
    bool worth_graph(const LaunchKnobs &kn) const { return n_launch >= GRAPH_MIN_LAUNCHES && !kn.no_graph; }
};
inline LaunchSeq launch_sequence(uint32_t n_turns, uint32_t max_fuse) {
    const uint32_t n = n_turns / max_fuse + (n_turns % max_fuse ? 1u : 0u);
    return {n, max_fuse, n_turns % max_fuse ? n_turns % max_fuse : (n ? max_fuse : 0u)};
}

}  // namespace ge

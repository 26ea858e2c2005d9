// The launch decisions of ge_batch_step (csrc/ge_plan.h: knobs, batch-time plan, per-launch plan, launch sequence) on the CPU,
// built with g++ under AddressSanitizer + UBSan and driven by tests/test_launch_plan.py.  Never loaded into Python.
//   launch_plan [GE_KNOB=value ...] plans    shapes on stdin, "max_fuse generic cond_shape kind:rooms[,kind:rooms ...]" each (kinds ww8 ww12 tt4
//                                            tt8 tt12; cond_shape in hex, ncl | len << 4, 0 = no literal image): per shape the lines B (batch-time
//                                            plan), F0 / F1 (the fused launch, n_turns = max_fuse, restart off / on), S (the single-turn launch)
//                                            and T (the GE_STAMPS = 2 record count)
//   launch_plan [GE_KNOB=value ...] table    the same lines for every shape of the sweep
//   launch_plan [GE_KNOB=value ...] check    the sweep's invariants: "checked N cases, V violations", each violation on a line of its own
//   launch_plan [GE_KNOB=value ...] seq      "n_turns max_fuse" pairs on stdin: the step's launches, whether one is a single turn, whether the step replays a graph
// The knobs are given as the environment would give them (parse_knobs), so an invalid value is ignored here as it is there.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../game_engine_amd/csrc/ge_host.h"
#include "../../game_engine_amd/csrc/ge_plan.h"

using namespace ge;

static const char *const KIND_NAMES[K_COUNT] = {"ww8", "ww12", "tt4", "tt8", "tt12"};

struct Shape {
    uint32_t max_fuse = 64, cond_shape = 0, n_seg = 0;
    bool generic = false;
    PlanSeg seg[GE_MAX_SEGMENTS];
    std::string key() const {
        char buf[64];
        std::string s;
        for (uint32_t k = 0; k < n_seg; k++) {
            snprintf(buf, sizeof buf, "%s%s:%llu", k ? "," : "", KIND_NAMES[seg[k].kind], (unsigned long long)seg[k].rooms);
            s += buf;
        }
        snprintf(buf, sizeof buf, " fuse=%u gen=%d shape=0x%02x", max_fuse, generic ? 1 : 0, cond_shape);
        return s + buf;
    }
};

static void add_seg(Shape &sh, uint32_t kind, uint64_t rooms) { sh.seg[sh.n_seg++] = {kind, (uint32_t)words_of(kind), rooms}; }

struct Plans { BatchPlan b; LaunchPlan f0, f1, s; };
static Plans plans_of(const LaunchKnobs &kn, const Shape &sh) {
    Plans p;
    p.b = batch_plan(kn, sh.seg, sh.n_seg, sh.max_fuse, sh.generic, sh.cond_shape, sh.generic ? 64u : 0u);
    p.f0 = launch_plan(p.b, sh.max_fuse, false); p.f1 = launch_plan(p.b, sh.max_fuse, true); p.s = launch_plan(p.b, 1, false);
    return p;
}

static void print_launch(const char *tag, const std::string &key, const LaunchPlan &p) {
    static const char *const LOADS[] = {"default", "alt", "no_recycle"};
    printf("%s %s : low=%d single=%d mixed=%d gen=%u load=%s bt=%u blocks=%u rpb=%u queue=%d pull=%d\n", tag, key.c_str(), p.low, p.single, p.mixed,
           p.gen, LOADS[p.load], p.bt, p.blocks, p.rpb, p.queue, p.pull);
}
static void print_plans(const Shape &sh, const Plans &p) {
    const std::string key = sh.key();
    printf("B %s : bt=%u nblocks=%u begin=", key.c_str(), p.b.block_threads, p.b.n_blocks);
    for (uint32_t k = 0; k < sh.n_seg; k++) printf("%s%u", k ? "," : "", p.b.block_begin[k]);
    printf(" low=%d stream=%d gshape=%u\n", p.b.low, p.b.stream_loads, p.b.gshape);
    print_launch("F0", key, p.f0); print_launch("F1", key, p.f1); print_launch("S", key, p.s);
    printf("T %s : %u\n", key.c_str(), p.b.stamp_records);
}

// ---- the sweep: every room count 1 .. 2 048, every multiple of 1 021 up to 600 000, each threshold +- 1; all five kinds and a two- and a
// four-segment mix of equal parts (the count is the batch's total, which is what the thresholds are about); max_fuse 1 and 64; non-generic
// tables, generic ones of no common shape and of the two shapes with builds of their own
template <class F> static void sweep(F &&f) {
    std::vector<uint64_t> rooms;
    for (uint64_t r = 1; r <= 2048; r++) rooms.push_back(r);
    for (uint64_t r = 1021; r <= 600000; r += 1021) rooms.push_back(r);
    // 32 768 half-filled wavefronts, 65 536 / 65 537 lone wavefronts, 262 144 block size, 393 216 single-turn block size, and the record-load
    // bounds in rooms of each layout (48 MiB: Two-Truths x 4 / 8 / 12 at 24 / 32 / 48 bytes; 96 MiB: Werewolf x 12 at 40; 288 MiB: all five)
    for (uint64_t t : {32768ull, 65536ull, 65537ull, 131072ull, 262144ull, 393216ull, 524288ull, 2097152ull, 1572864ull, 1048576ull, 2516480ull, 9437184ull,
                       7549696ull, 12582912ull, 6291456ull})
        for (uint64_t r = t - 1; r <= t + 1; r++) rooms.push_back(r);
    const uint32_t cond_shapes[] = {0u, 0x22u, 0x11u, 0x21u};
    for (uint64_t r : rooms)
        for (uint32_t form = 0; form < K_COUNT + 2; form++)
            for (uint32_t fuse : {1u, 64u})
                for (uint32_t g = 0; g < 4; g++) {
                    Shape sh;
                    sh.max_fuse = fuse; sh.generic = g != 0; sh.cond_shape = cond_shapes[g];
                    if (form < K_COUNT) add_seg(sh, form, r);
                    else {
                        const uint32_t n = form == K_COUNT ? 2u : 4u;
                        static const uint32_t mix[4] = {K_WW8, K_TT4, K_WW12, K_TT12};
                        if (r < n) continue;
                        for (uint32_t k = 0; k < n; k++) add_seg(sh, mix[k], r / n + (k < r % n ? 1u : 0u));
                    }
                    f(sh);
                }
}

static uint64_t n_violations = 0;
static void violation(const Shape &sh, const char *plan, const char *what) { n_violations++; printf("VIOLATION %s %s: %s\n", plan, sh.key().c_str(), what); }

static void check_launch(const Shape &sh, const Plans &P, const LaunchPlan &p, const char *tag, bool restart, bool default_knobs) {
    const uint64_t rooms = sh.seg[0].rooms;
    if (!p.mixed) {                                                   // the grid covers the rooms, and no block is idle
        if (!((uint64_t)(p.blocks - 1u) * p.rpb < rooms && rooms <= (uint64_t)p.blocks * p.rpb)) violation(sh, tag, "grid does not cover the rooms exactly");
    } else {
        uint32_t acc = 0;
        for (uint32_t k = 0; k < sh.n_seg; k++) {
            if (P.b.block_begin[k] != acc) violation(sh, tag, "block_begin is not the running sum of the segments' blocks");
            acc += (uint32_t)((sh.seg[k].rooms + p.bt - 1u) / p.bt);
        }
        if (p.blocks != acc || p.bt != P.b.block_threads) violation(sh, tag, "a mixed launch left its batch's block size or grid");
    }
    if (p.rpb > p.bt || (p.rpb < p.bt && !(p.low && p.bt == 64u))) violation(sh, tag, "rooms per block");
    if (p.bt != 64u && p.bt != 128u && p.bt != 256u && p.bt != 512u && p.bt != 1024u) violation(sh, tag, "block size");
    if (default_knobs && p.low && p.blocks * (p.bt / 64u) > 1024u) violation(sh, tag, "more than 1 024 lone wavefronts");
    if (p.load == LOAD_ALT && !(p.single && !p.low && p.gen == 0u && !p.mixed)) violation(sh, tag, "ALT load form");
    if (p.load == LOAD_NO_RECYCLE && !(p.low && !p.single && p.gen == 0u && !p.mixed && sh.seg[0].kind == K_WW8 && !restart)) violation(sh, tag, "NO_RECYCLE load form");
    if (P.b.stamp_records < p.blocks * (p.bt / 64u)) violation(sh, tag, "fewer stamp records than wavefronts");
}

int main(int argc, char **argv) {
    std::vector<std::string> env;
    const char *mode = nullptr;
    for (int i = 1; i < argc; i++) { if (strchr(argv[i], '=')) env.push_back(argv[i]); else mode = argv[i]; }
    if (!mode) { fprintf(stderr, "usage: launch_plan [GE_KNOB=value ...] plans | table | check | seq\n"); return 2; }
    const LaunchKnobs kn = parse_knobs([&env](const char *name) -> const char * {
        const size_t n = strlen(name);
        for (const std::string &e : env) if (e.compare(0, n, name) == 0 && e[n] == '=') return e.c_str() + n + 1;
        return nullptr;
    });
    char line[512];
    if (!strcmp(mode, "plans")) {
        while (fgets(line, sizeof line, stdin)) {
            Shape sh;
            unsigned gen = 0;
            char segs[400];
            if (sscanf(line, "%u %u %x %399s", &sh.max_fuse, &gen, &sh.cond_shape, segs) != 4 || sh.max_fuse == 0) { fprintf(stderr, "bad shape: %s", line); return 2; }
            sh.generic = gen != 0;
            for (char *tok = strtok(segs, ","); tok; tok = strtok(nullptr, ",")) {
                char *colon = strchr(tok, ':');
                uint32_t kind = K_COUNT;
                for (uint32_t k = 0; colon && k < K_COUNT; k++) if (strlen(KIND_NAMES[k]) == (size_t)(colon - tok) && !strncmp(tok, KIND_NAMES[k], colon - tok)) kind = k;
                if (kind == K_COUNT || sh.n_seg == GE_MAX_SEGMENTS || strtoull(colon + 1, nullptr, 10) == 0) { fprintf(stderr, "bad segment: %s\n", tok); return 2; }
                add_seg(sh, kind, strtoull(colon + 1, nullptr, 10));
            }
            if (!sh.n_seg) { fprintf(stderr, "no segment: %s", line); return 2; }
            print_plans(sh, plans_of(kn, sh));
        }
    } else if (!strcmp(mode, "table")) {
        sweep([&](const Shape &sh) { print_plans(sh, plans_of(kn, sh)); });
    } else if (!strcmp(mode, "check")) {
        uint64_t cases = 0;
        const bool default_knobs = env.empty();
        sweep([&](const Shape &sh) {
            const Plans P = plans_of(kn, sh);
            check_launch(sh, P, P.f0, "F0", false, default_knobs); check_launch(sh, P, P.f1, "F1", true, default_knobs); check_launch(sh, P, P.s, "S", false, default_knobs);
            cases++;
        });
        printf("checked %llu cases, %llu violations\n", (unsigned long long)cases, (unsigned long long)n_violations);
        return n_violations ? 1 : 0;
    } else if (!strcmp(mode, "seq")) {
        uint32_t n_turns, max_fuse;
        while (fgets(line, sizeof line, stdin)) {
            if (sscanf(line, "%u %u", &n_turns, &max_fuse) != 2 || max_fuse == 0) { fprintf(stderr, "bad pair: %s", line); return 2; }
            const LaunchSeq q = launch_sequence(n_turns, max_fuse);
            printf("Q %u %u : launches=", n_turns, max_fuse);
            for (uint32_t i = 0; i < q.n_launch; i++) printf("%s%u", i ? "," : "", q.turns(i));
            printf(" single=%d graph=%d\n", q.has_single(), q.worth_graph(kn));
        }
    } else { fprintf(stderr, "unknown mode %s\n", mode); return 2; }
    return 0;
}

#!/usr/bin/env python3
"""What the lone-wavefront turn loops run inside their LDS waits, read from the assembly that is shipped
(game_engine_amd/csrc/ge_step.s, `make -C game_engine_amd/csrc asm`).

A lone wavefront has no neighbour on its SIMD to hide an LDS round trip: the only thing that covers one is the wavefront's own
instructions between the read and the `s_waitcnt lgkmcnt` that first waits for it.  The source places such work on purpose
(ge_device.h: ww_queue_actions' shadow1 / shadow2, the pins of ww_turn), but where it ends up is the scheduler's decision -
this tool reports it, and --check pins it.

For every turn loop (outermost loop that holds the queue's LDS atomic) of the named kernels, and every LDS read in it: the
`s_waitcnt` that first waits for that read, and the vector / scalar instructions issued between the two.  The path is the one a
turn takes: exec-masked blocks are entered (their skip is not taken), unconditional branches are followed, and a forward
wave-uniform branch (scc / vcc) in the turn loop's own blocks is taken - that is the skip of the deal block, which runs on
every GE_DEAL_PERIOD-th turn only; inside the loop over queue rounds such a branch falls through (another round).  A block
of the loop that the compiler laid out behind the loop's back edge (a rare path: entered by a wave-uniform branch, it jumps back) is not entered.  LDS and
scalar-memory operations complete in issue order for this purpose: `lgkmcnt(n)` covers a read once at most n such
operations were issued behind it.
Reads are named by their place in the turn: `ord` (before the slot writes), `slot` (the first round's), `slot+` (a later
round's, inside the queue loop), `head` / `head+` (the pull queue's head word, read in front of the context that `slot` / `slot+` then is), `result` (behind the atomics), `row` (everything after: the entered row, a recycled room).
The fused lone Werewolf x 8 turn (ge_device.h ww_queue_actions) lays the second round out of line - a block of its own outside the loop over rounds, behind the turn loop's back edge in the tail-recycling loops: its
reads are `head2` (the head word, where the round reads one of its own) and `slot2` (the context, the read whose next LDS operation is
the round's atomic).  With the head words of both rounds read at once the first read is a two-address one and still `head`.

For the first round's slot read the walk goes on to the round's LDS atomic: `to atomic` = the vector instructions between that
read and the atomic, i.e. the first round with whatever the scheduler interleaved with it - the placement that is adopted
(shadow2 beside the first round) shows there and not in front of a wait.
The floors are per kernel and read, the least over the kernel's turn loops (no loop ordinal in a key).

    python tools/asm_shadow.py [file.s]        the table (no file: ge_step.s, rebuilt first if it is older than its sources)
    python tools/asm_shadow.py --json          the same as JSON
    python tools/asm_shadow.py --check         exit 1 if a count is below its floor in tools/asm_shadow_baseline.json
    python tools/asm_shadow.py --paths         per turn loop, as JSON: the common turn from the loop header to its back edge - instructions on it,
                                               branches taken on it, role-deal blocks it runs through (tools/asm_shadow_paths.json pins the last
                                               two for the Werewolf x 8 kernel: tests/test_asm_cold_deal.py); `two_round`: the same walk through
                                               the out-of-line second round (instructions, taken branches), where the loop has one
    python tools/asm_shadow.py --write         record today's counts as the floors (those in front of a wait capped at 32)
It reads instruction mnemonics only: LDS reads, LDS atomics and writes (to name the reads), waits, branches, and whether an
instruction is a vector or a scalar one.

Counts, vector + scalar instructions in front of the wait (Werewolf x 8 fused lone kernel, untraced tail-restart loop; the other
loops and Werewolf x 12 alike):
                                              ord        slot       result    slot read to atomic (x 8 / x 12)
    before (shadow2 behind the result read)   15 + 0     9 + 2      0 + 4      67 / 119   the scheduler had sunk all of shadow2 below the wait
    with a scheduling fence behind shadow2    15 + 0     9 + 2     20 + 7      67 / 119   measured level with `before` (profiles/ab_lone_shadow.txt)
    first round peeled, shadow2 in its block  15 + 0     6 + 4      4 + 0      80 / 130   +2.0 %: what is adopted
What the measurements say (profiles/ab_lone_shadow.txt): instructions in front of a wait are not the whole story.  Holding
shadow2 in front of the result wait was level, and the counters of the adopted form show unchanged wait cycles - its gain is the
loop control the peel removes.  The floors pin today's placement; a change that lowers one is to be measured, not assumed.
"""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASM = os.path.join(ROOT, "game_engine_amd", "csrc", "ge_step.s")
BASELINE = os.path.join(ROOT, "tools", "asm_shadow_baseline.json")
# the fused lone-wavefront kernels whose turn goes through an LDS action queue
KERNELS = {
    "ge_step_kernelILi0ELb1ELi0ELb0ELi0E": "Werewolf x 8, lone-wavefront, fused",
    "ge_step_kernelILi1ELb1ELi0ELb0ELi0E": "Werewolf x 12, lone-wavefront, fused",
    "ge_step_kernelILi3ELb1ELi0ELb0ELi0E": "Two-Truths x 8, lone-wavefront, fused",
    "ge_step_kernelILi4ELb1ELi0ELb0ELi0E": "Two-Truths x 12, lone-wavefront, fused",
    "ge_step_kernel_mixedILb1ELi0ELb0E": "mixed batch, lone-wavefront, fused",
}
# floors are capped: 32 instructions of a lone wavefront are ~150 cycles, more than any LDS round trip of the turn - a wait with that
# much in front of it is covered, and removing work from a long stretch must not fail the check
CAP = 32
LIMIT = 4000                                           # instructions walked from a read before giving up

INSN = re.compile(r"^\t([a-z_0-9]+)\b(.*)")
LABEL = re.compile(r"^(\.LBB\d+_\d+):")


def kernel_bodies(lines):
    """mangled-name fragment -> (first, last) line index of the kernel's code"""
    out = {}
    for i, ln in enumerate(lines):
        m = re.match(r"^(_ZN\S*):", ln)
        if not m:
            continue
        for frag in KERNELS:
            if re.search(r"\d" + frag + "E+v", m.group(1)):
                end = next(j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end"))
                out[frag] = (i, end)
    return out


def lgkm_wait(args):
    """n of `lgkmcnt(n)` in a wait's operands; a bare immediate waits for everything; None: no LDS / scalar-memory wait"""
    m = re.search(r"lgkmcnt\((\d+)\)", args)
    if m:
        return int(m.group(1))
    return 0 if re.match(r"\s*(0x[0-9a-f]+|\d+)\s*$", args) else None


def is_lgkm(op):
    return op.startswith("ds_") or op.startswith("s_load") or op.startswith("s_buffer_load") or op in ("s_memtime", "s_memrealtime", "s_sendmsg")


def loops_of(lines, lo, hi):
    """turn loops of a kernel: [(header label, first line, last line)] of the Depth=1 loops"""
    heads = [LABEL.match(lines[i]).group(1) for i in range(lo, hi) if "Loop Header: Depth=1" in lines[i] and LABEL.match(lines[i])]
    out = []
    for h in heads:
        tag = re.compile(r"(Header=|Parent Loop )" + re.escape(h[2:]) + r"\b")
        blocks = [i for i in range(lo, hi) if LABEL.match(lines[i]) and (lines[i].startswith(h + ":") or tag.search(lines[i]))]
        blocks += [i + 1 for i in blocks if i + 1 < hi and tag.search(lines[i + 1])]     # (an inner header's second comment line)
        first, last = min(blocks), max(blocks)
        end = next((j for j in range(last + 1, hi) if LABEL.match(lines[j])), hi)
        out.append((h, first, end))
    return out


ATOMIC = re.compile(r"ds_(or|add|and|max|min|xor)")
PATHS = os.path.join(ROOT, "tools", "asm_shadow_paths.json")
# the draw constants (17 .. 20) * GOLDEN of deal_roles' four picks (ge_device.h): only a role-deal block holds them
DEAL_MARKS = tuple(hex((0x9E3779B9 * (17 + j)) & 0xFFFFFFFF) for j in range(4))


def cold_from(lines, head, first, end):
    """the line behind the turn loop's back edge (its first branch to the header): blocks of the loop that stand behind it are
    rare paths the compiler laid out of line - they are entered by a wave-uniform branch and jump back.  No such branch: `end`"""
    back = re.compile(r"^\ts_c?branch\w*\s+" + re.escape(head) + r"\s*$")
    return next((i + 1 for i in range(first, end) if back.match(lines[i].split(";")[0].rstrip())), end)


def second_round_blocks(lines, labels, first, end):
    """The second queue round as a block of its own, entered by a forward wave-uniform branch and left by an
    unconditional one - wherever the compiler laid it (behind the back edge in the tail-recycling loops, in front of it in the
    others).  What tells it from a deal block and from the first round's: a context read (ds_read_b128) and then an LDS atomic stand in it before any
    wave-uniform branch.  [(first line, last line)]"""
    out = []
    for i in range(first, end):
        m = INSN.match(lines[i])
        if not m or not m.group(1).startswith(("s_cbranch_scc", "s_cbranch_vcc")):
            continue
        t = labels.get(m.group(2).strip())
        if t is None or t <= i or any(a <= t <= b for a, b in out):
            continue
        read = False
        for j in range(t, end):
            mj = INSN.match(lines[j])
            if mj and (mj.group(1) == "s_branch" or mj.group(1).startswith(("s_cbranch_scc", "s_cbranch_vcc"))) or "Loop Header" in lines[j]:
                break
            read |= bool(mj) and mj.group(1) == "ds_read_b128"
            if mj and ATOMIC.match(mj.group(1)) and read:
                stop = next((k for k in range(j, end) if INSN.match(lines[k]) and INSN.match(lines[k]).group(1) == "s_branch"), end - 1)
                out.append((t, stop))
                break
    return out


def turn_path(lines, labels, head, first, end, two=False):
    """the common turn from the loop header to its back edge, by walk()'s rules (exec-masked blocks entered, the skip of an in-line
    wave-uniform block taken, no branch into an out-of-line block, the loop over further queue rounds left at once): instructions on
    it, branches taken on it (the back edge among them), and how many role-deal blocks it runs through.
    two: the turn that needs a second queue round where that round is a block behind the back edge - the branch into
    that block is taken and its branch back followed; None if the loop has no such block"""
    def in_queue_loop(i):
        j = next(j for j in range(i, first - 1, -1) if LABEL.match(lines[j]))
        return "Depth=2" in lines[j] or "Inner Loop Header" in lines[j + 1]
    cold = cold_from(lines, head, first, end)
    second = second_round_blocks(lines, labels, first, end)
    entered = False
    i, n, taken, marks = labels[head], 0, 0, 0
    for _ in range(40 * LIMIT):
        m = INSN.match(lines[i])
        if not m:
            i += 1
            continue
        op, args = m.group(1), m.group(2)
        if op == "s_endpgm":
            return None
        n += 1
        marks += any(c in lines[i] for c in DEAL_MARKS)
        if op == "s_branch" or op.startswith("s_cbranch_scc") or op.startswith("s_cbranch_vcc"):
            t = labels.get(args.strip())
            if t is not None and op != "s_branch" and any(a == t for a, _ in second) and not any(a <= i <= b for a, b in second):
                if two:
                    entered, taken, i = True, taken + 1, t
                else:
                    i += 1                                  # the one-round turn falls through
                continue
            if t is not None and t <= i and op != "s_branch" and any(a <= i <= b for a, b in second):
                taken, i = taken + 1, t                     # back from the second round to where the turn goes on (no third round)
                continue
            if t is not None and t <= i and (op == "s_branch" or not in_queue_loop(i)):
                if two and not entered:
                    return None
                return {"insns": n, "taken": taken + 1, "deal_blocks": (marks + 3) // 4}
            if t is not None and t > i and (op == "s_branch" or (t < cold and not in_queue_loop(i))):
                taken += 1
                i = t
                continue
        i += 1
    return None


def walk(lines, labels, start, first, end, to_atomic=False, cold=None, second=()):
    """from the LDS read at `start`: (wait line or None, vector, scalar, LDS) instructions issued up to its wait; to_atomic: the
    walk goes on to the first LDS atomic, and a fifth value counts the vector instructions from the read to there"""
    def in_queue_loop(i):                                   # the block of line i belongs to the loop over queue rounds
        j = next(j for j in range(i, first - 1, -1) if LABEL.match(lines[j]))
        return "Depth=2" in lines[j] or "Inner Loop Header" in lines[j + 1]
    cold = end if cold is None else cold                    # blocks from there on are out of line (cold_from): not the common turn
    behind = v = s = d = 0
    found = None                                            # (wait line, v, s, d) once the read's wait is passed
    i, steps = start + 1, 0
    while steps < LIMIT:
        m = INSN.match(lines[i])
        if not m:
            i += 1
            continue
        op, args = m.group(1), m.group(2)
        steps += 1
        if op == "s_endpgm":
            break
        if found and ATOMIC.match(op):
            return found + (v,)
        if op == "s_waitcnt":
            n = lgkm_wait(args)
            if not found and n is not None and n <= behind:
                found = (i, v, s, d)
                if not to_atomic:
                    return found
            i += 1
            continue
        if op == "s_branch":
            s += 1
            i = labels[args.strip()]
            continue
        if op.startswith("s_cbranch_scc") or op.startswith("s_cbranch_vcc"):
            s += 1
            t = labels[args.strip()]
            into_second = any(a == t for a, _ in second) and not any(a <= i <= b for a, b in second)
            i = t if (i < t < cold and not in_queue_loop(i) and not into_second) else i + 1
            continue
        if is_lgkm(op):
            behind += 1
            d += op.startswith("ds_")
        elif op.startswith("v_"):
            v += 1
        elif op.startswith("s_"):
            s += 1
        i += 1
    return found + (None,) if found and to_atomic else found or (None, v, s, d)


def fresh_asm():
    """game_engine_amd/csrc/ge_step.s, rebuilt (`make asm`) if it is missing or older than a file it is made from"""
    csrc = os.path.dirname(ASM)
    srcs = [os.path.join(csrc, n) for n in os.listdir(csrc) if n.endswith((".hip", ".inl", ".h", ".sed")) or n == "Makefile"]
    srcs.append(os.path.join(ROOT, "include", "ge_step.h"))
    if not os.path.exists(ASM) or os.path.getmtime(ASM) < max(os.path.getmtime(p) for p in srcs):
        p = subprocess.run(["make", "-C", csrc, "asm"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if p.returncode != 0:
            sys.stderr.write(p.stdout)
            raise SystemExit("make asm failed")
    return ASM


def collect(path):
    with open(path) as f:
        lines = f.read().split("\n")
    rows = []
    for frag, (lo, hi) in sorted(kernel_bodies(lines).items(), key=lambda kv: kv[1]):
        labels = {LABEL.match(lines[i]).group(1): i for i in range(lo, hi) if LABEL.match(lines[i])}
        n_loop = 0
        for head, first, end in loops_of(lines, lo, hi):
            cold = cold_from(lines, head, first, end)
            second = second_round_blocks(lines, labels, first, end)
            ops = [(i, INSN.match(lines[i]).group(1)) for i in range(first, end) if INSN.match(lines[i])]
            atomics = [i for i, op in ops if ATOMIC.match(op)]
            writes = [i for i, op in ops if op.startswith("ds_write")]
            if not atomics or not writes:                       # not a turn loop with an action queue
                continue
            def in_queue_loop(i):
                j = next(j for j in range(i, first - 1, -1) if LABEL.match(lines[j]))
                return "Depth=2" in lines[j] or "Inner Loop Header" in lines[j + 1]
            def in_second(i):
                return any(a <= i <= b for a, b in second)
            seen = {}
            reads = [(i, op) for i, op in ops if op.startswith("ds_read")]
            for n, (i, op) in enumerate(reads):
                # the pull queue (ge_device.h WaveLdsPull): a slot reads its head word, then the owner's 16-byte context
                heads_ctx = op in ("ds_read_b32", "ds_read2st64_b32") and n + 1 < len(reads) and reads[n + 1][1] == "ds_read_b128" and i >= writes[0] and \
                    (in_queue_loop(i) and in_queue_loop(reads[n + 1][0]) or reads[n + 1][0] < atomics[0] or in_second(i) and not in_queue_loop(reads[n + 1][0]))
                next_lds = next((o for j, o in ops if j > i and o.startswith("ds_")), "")
                if i < writes[0]:
                    role = "ord"
                elif in_second(i) and not in_queue_loop(i) and (heads_ctx or op == "ds_read_b128" and ATOMIC.match(next_lds)):
                    role = "head2" if heads_ctx else "slot2"     # the second round out of line
                elif in_queue_loop(i):
                    role = "head+" if heads_ctx else "slot+"
                elif i < atomics[0]:
                    role = "head" if heads_ctx else "slot"
                elif "result" not in seen:
                    role = "result"
                else:
                    role = "row"
                seen[role] = seen.get(role, 0) + 1
                wait, v, s, d, *rest = walk(lines, labels, i, first, end, to_atomic=(role == "slot"), cold=cold, second=second)
                rows.append({"kernel": KERNELS[frag], "loop": n_loop, "read": f"{role}{seen[role] if seen[role] > 1 else ''}", "op": op,
                             "wait": (INSN.match(lines[wait]).group(0).strip() if wait is not None else None),
                             "vector": v, "scalar": s, "lds": d, "to_atomic": rest[0] if rest else None})
            n_loop += 1
    return rows


def paths(path):
    """per turn loop (numbered as in collect): turn_path's figures and the loop's static size"""
    with open(path) as f:
        lines = f.read().split("\n")
    out = {}
    for frag, (lo, hi) in sorted(kernel_bodies(lines).items(), key=lambda kv: kv[1]):
        labels = {LABEL.match(lines[i]).group(1): i for i in range(lo, hi) if LABEL.match(lines[i])}
        n_loop = 0
        for head, first, end in loops_of(lines, lo, hi):
            ops = [INSN.match(lines[i]).group(1) for i in range(first, end) if INSN.match(lines[i])]
            if not any(ATOMIC.match(op) for op in ops) or not any(op.startswith("ds_write") for op in ops):
                continue
            p = turn_path(lines, labels, head, first, end)
            if p:
                out[f"{KERNELS[frag]} / loop {n_loop}"] = dict(p, static=len(ops), out_of_line=cold_from(lines, head, first, end) < end)
                p2 = turn_path(lines, labels, head, first, end, two=True)
                if p2:
                    out[f"{KERNELS[frag]} / loop {n_loop}"]["two_round"] = {"insns": p2["insns"], "taken": p2["taken"]}
            n_loop += 1
    return out


def key(r):
    return f"{r['kernel']} / loop {r['loop']} / {r['read']}"


def least(rows):
    """kernel / read -> the least counts over the kernel's turn loops (loops come and go with the source: the floors name none)"""
    out = {}
    for r in rows:
        k = f"{r['kernel']} / {r['read']}"
        o = out.setdefault(k, {"vector": r["vector"], "scalar": r["scalar"], "both": r["vector"] + r["scalar"]})
        o["vector"], o["scalar"], o["both"] = min(o["vector"], r["vector"]), min(o["scalar"], r["scalar"]), min(o["both"], r["vector"] + r["scalar"])
        if r["to_atomic"] is not None:
            o["to_atomic"] = min(o.get("to_atomic", r["to_atomic"]), r["to_atomic"])
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    src = args[0] if args else fresh_asm()
    rows = collect(src)
    pth = paths(src)
    if "--paths" in sys.argv:
        print(json.dumps(pth, indent=1, sort_keys=True))
    elif "--json" in sys.argv:
        print(json.dumps(rows, indent=1))
    else:
        print(f"{'kernel / turn loop / read':64s} {'read':14s} {'vector':>6s} {'scalar':>6s} {'LDS':>4s} {'to atomic':>9s}  first wait")
        for r in rows:
            print(f"{key(r):64s} {r['op']:14s} {r['vector']:6d} {r['scalar']:6d} {r['lds']:4d} {r['to_atomic'] if r['to_atomic'] is not None else '':>9}  {r['wait']}")
        print(f"\n{'kernel / turn loop: the common turn, header to back edge':64s} {'instructions':>12s} {'taken branches':>14s} {'deal blocks':>11s} {'loop size':>9s}")
        for k, p in pth.items():
            print(f"{k:64s} {p['insns']:12d} {p['taken']:14d} {p['deal_blocks']:11d} {p['static']:9d}")
    got = least(rows)
    if "--write" in sys.argv:
        for o in got.values():
            o["vector"], o["scalar"], o["both"] = min(o["vector"], CAP), min(o["scalar"], CAP), min(o["both"], CAP)
        with open(BASELINE, "w") as f:
            json.dump(got, f, indent=1, sort_keys=True)
            f.write("\n")
        with open(PATHS, "w") as f:
            json.dump({k: {"deal_blocks": p["deal_blocks"], "taken": p["taken"]} for k, p in pth.items() if "Werewolf x 8" in k}, f, indent=1, sort_keys=True)
            f.write("\n")
    if "--check" in sys.argv:
        with open(BASELINE) as f:
            floor = json.load(f)
        bad = [f"{k}: missing from the assembly" for k in floor if k not in got]
        for k, fl in floor.items():
            g = got.get(k)
            if g and (g["vector"] < fl["vector"] or g["both"] < fl["both"]):
                bad.append(f"{k}: {g['vector']} vector, {g['both']} vector + scalar in front of the wait; floors {fl['vector']}, {fl['both']}")
            if g and "to_atomic" in fl and g.get("to_atomic", 0) < fl["to_atomic"]:
                bad.append(f"{k}: {g.get('to_atomic')} vector instructions from the slot read to the round's atomic, floor {fl['to_atomic']}")
        if bad:
            raise SystemExit("LDS shadow check failed:\n  " + "\n  ".join(bad))


if __name__ == "__main__":
    main()

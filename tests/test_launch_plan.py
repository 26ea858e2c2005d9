"""The launch decisions of ge_batch_step on the CPU (csrc/ge_plan.h: knobs, batch-time plan, per-launch plan, launch sequence),
through tests/native/launch_plan.cpp built with g++ -fsanitize=address,undefined (a stand-alone program, never loaded here).

The pinned rows sit on both sides of every size threshold; their expected values were printed by the code these functions
replaced (the differential of profiles/launch_plan_equiv.txt), the stamp record counts are blocks * (bt / 64) by hand.
Compact forms - batch: "bt nblocks block_begin low stream_loads gshape"; launch: "low gen load bt blocks rpb queue pull".

The sweep's mixes are equal parts of the total (the C5 shape).  A ragged mix of 65 473 .. 65 536 rooms in all can pad to
n_seg - 1 more than 1 024 lone wavefronts (ceil per segment); the lone-wavefront invariant below is about the sizes swept."""
import os
import subprocess

import pytest

from conftest import ROOT

# (shape "max_fuse generic cond_shape segments", batch plan, fused launch with restart off, single-turn launch, stamp records)
PINNED = [
    # 65 536 / 65 537 rooms: the lone-wavefront builds or not; 32 768 / 32 769 .. 65 535: 32 rooms per wavefront, then ceil(rooms / 1024)
    ("64 0 0 ww8:65536", "64 1024 0 1 0 0", "1 0 no_recycle 64 1024 64 1 1", "1 0 default 64 1024 64 1 0", 1024),
    ("64 0 0 ww8:65537", "64 1025 0 0 0 0", "0 0 default 64 1025 64 1 0", "0 0 default 256 257 256 1 0", 1028),
    ("64 0 0 ww8:32768", "64 512 0 1 0 0", "1 0 no_recycle 64 1024 32 1 1", "1 0 default 64 512 64 1 0", 1024),
    ("64 0 0 ww8:32769", "64 513 0 1 0 0", "1 0 no_recycle 64 993 33 1 1", "1 0 default 64 513 64 1 0", 993),
    ("64 0 0 ww8:65535", "64 1024 0 1 0 0", "1 0 no_recycle 64 1024 64 1 1", "1 0 default 64 1024 64 1 0", 1024),
    ("64 0 0 ww8:40000", "64 625 0 1 0 0", "1 0 no_recycle 64 1000 40 1 1", "1 0 default 64 625 64 1 0", 1000),
    ("64 0 0 ww8:49152", "64 768 0 1 0 0", "1 0 no_recycle 64 1024 48 1 1", "1 0 default 64 768 64 1 0", 1024),
    ("64 0 0 ww12:40000", "64 625 0 1 1 0", "1 0 default 64 1000 40 1 0", "1 0 default 64 625 64 1 0", 1000),
    # 262 144 / 262 145 rooms in all: 64- or 256-room blocks; max_fuse = 1 at 65 536 / 65 537
    ("64 0 0 ww8:262144", "64 4096 0 0 0 0", "0 0 default 64 4096 64 1 0", "0 0 default 256 1024 256 1 0", 4096),
    ("64 0 0 ww8:262145", "256 1025 0 0 0 0", "0 0 default 256 1025 256 1 0", "0 0 default 256 1025 256 1 0", 4100),
    ("1 0 0 ww8:65536", "64 1024 0 1 0 0", "1 0 default 64 1024 64 1 0", "1 0 default 64 1024 64 1 0", 1024),
    ("1 0 0 ww8:65537", "256 257 0 0 0 0", "0 0 default 256 257 256 1 0", "0 0 default 256 257 256 1 0", 1028),
    # single-turn Werewolf x 8 at 393 215 / 393 216: 256- or 512-room blocks; a not-low batch of 64-room blocks: 256-room single-turn blocks
    ("64 0 0 ww8:393215", "256 1536 0 0 0 0", "0 0 default 256 1536 256 1 0", "0 0 default 256 1536 256 1 0", 6144),
    ("64 0 0 ww8:393216", "256 1536 0 0 0 0", "0 0 default 256 1536 256 1 0", "0 0 default 512 768 512 1 0", 6144),
    ("64 0 0 ww8:131072", "64 2048 0 0 0 0", "0 0 default 64 2048 64 1 0", "0 0 default 256 512 256 1 0", 2048),
    # record loads: each kind's `small` bound (48 MiB Two-Truths, 96 MiB Werewolf x 12) ...
    ("64 0 0 tt4:2097152", "256 8192 0 0 1 0", "0 0 default 256 8192 256 1 0", "0 0 default 256 8192 256 1 0", 32768),
    ("64 0 0 tt4:2097153", "256 8193 0 0 0 0", "0 0 default 256 8193 256 1 0", "0 0 alt 256 8193 256 1 0", 32772),
    ("64 0 0 tt8:1572864", "256 6144 0 0 1 0", "0 0 default 256 6144 256 1 0", "0 0 default 256 6144 256 1 0", 24576),
    ("64 0 0 tt8:1572865", "256 6145 0 0 0 0", "0 0 default 256 6145 256 1 0", "0 0 alt 256 6145 256 1 0", 24580),
    ("64 0 0 tt12:1048576", "256 4096 0 0 1 0", "0 0 default 256 4096 256 1 0", "0 0 default 256 4096 256 1 0", 16384),
    ("64 0 0 tt12:1048577", "256 4097 0 0 0 0", "0 0 default 256 4097 256 1 0", "0 0 alt 256 4097 256 1 0", 16388),
    ("64 0 0 ww12:2516480", "256 9830 0 0 1 0", "0 0 default 256 9830 256 1 0", "0 0 default 256 9830 256 1 0", 39320),
    ("64 0 0 ww12:2516481", "256 9831 0 0 0 0", "0 0 default 256 9831 256 1 0", "0 0 alt 256 9831 256 1 0", 39324),
    # ... and 288 MiB touched, per layout
    ("64 0 0 ww8:9437184", "256 36864 0 0 0 0", "0 0 default 256 36864 256 1 0", "0 0 default 512 18432 512 1 0", 147456),
    ("64 0 0 ww8:9437185", "256 36865 0 0 1 0", "0 0 default 256 36865 256 1 0", "0 0 alt 512 18433 512 1 0", 147464),
    ("64 0 0 tt8:9437184", "256 36864 0 0 0 0", "0 0 default 256 36864 256 1 0", "0 0 alt 256 36864 256 1 0", 147456),
    ("64 0 0 tt8:9437185", "256 36865 0 0 1 0", "0 0 default 256 36865 256 1 0", "0 0 default 256 36865 256 1 0", 147460),
    ("64 0 0 ww12:7549696", "256 29491 0 0 0 0", "0 0 default 256 29491 256 1 0", "0 0 alt 256 29491 256 1 0", 117964),
    ("64 0 0 ww12:7549697", "256 29492 0 0 1 0", "0 0 default 256 29492 256 1 0", "0 0 default 256 29492 256 1 0", 117968),
    ("64 0 0 tt4:12582912", "256 49152 0 0 0 0", "0 0 default 256 49152 256 1 0", "0 0 alt 256 49152 256 1 0", 196608),
    ("64 0 0 tt4:12582913", "256 49153 0 0 1 0", "0 0 default 256 49153 256 1 0", "0 0 default 256 49153 256 1 0", 196612),
    ("64 0 0 tt12:6291456", "256 24576 0 0 0 0", "0 0 default 256 24576 256 1 0", "0 0 alt 256 24576 256 1 0", 98304),
    ("64 0 0 tt12:6291457", "256 24577 0 0 1 0", "0 0 default 256 24577 256 1 0", "0 0 default 256 24577 256 1 0", 98308),
    # gshape 0 / 2 / 3 (fused launches only; Two-Truths only)
    ("64 1 22 tt4:3000", "64 47 0 1 1 0", "1 1 default 64 94 32 0 0", "1 1 default 64 47 64 0 0", 94),
    ("64 1 11 tt4:3000", "64 47 0 1 1 2", "1 2 default 64 94 32 0 0", "1 1 default 64 47 64 0 0", 94),
    ("64 1 21 tt8:140001", "64 2188 0 0 1 3", "0 3 default 64 2188 64 1 0", "0 1 default 256 547 256 1 0", 2188),
    ("64 1 11 ww8:3000", "64 47 0 1 0 0", "1 1 default 64 94 32 1 0", "1 1 default 64 47 64 1 0", 94),
    # a mixed batch keeps its block size, blocks = the sum over segments; a generic mixed batch is never low
    ("64 0 0 ww8:1250,tt4:1250", "64 40 0,20 1 0 0", "1 0 default 64 40 64 1 0", "1 0 default 64 40 64 1 0", 40),
    ("64 0 0 ww8:150000,tt4:150000", "256 1172 0,586 0 0 0", "0 0 default 256 1172 256 1 0", "0 0 default 256 1172 256 1 0", 4688),
    ("64 0 0 ww8:100,ww12:70,tt4:65,tt12:1", "64 7 0,2,4,6 1 0 0", "1 0 default 64 7 64 1 0", "1 0 default 64 7 64 1 0", 7),
    ("64 1 22 ww8:1250,tt4:1250", "64 40 0,20 0 0 0", "0 1 default 64 40 64 1 0", "0 1 default 64 40 64 1 0", 40),
]

# per knob: the override taking effect, and (where a value can be invalid) an invalid value changing nothing
KNOB_ROWS = [
    ("GE_BLOCK_THREADS=128", ("64 0 0 ww8:3000", "128 24 0 1 0 0", "1 0 no_recycle 128 24 128 1 1", "1 0 default 128 24 128 1 0", 48)),
    ("GE_BLOCK_THREADS=100", ("64 0 0 ww8:3000", "64 47 0 1 0 0", "1 0 no_recycle 64 94 32 1 1", "1 0 default 64 47 64 1 0", 94)),
    ("GE_SINGLE_BLOCK=1024", ("64 0 0 ww8:1048576", "256 4096 0 0 0 0", "0 0 default 256 4096 256 1 0", "0 0 default 1024 1024 1024 1 0", 16384)),
    ("GE_SINGLE_BLOCK=300", ("64 0 0 ww8:1048576", "256 4096 0 0 0 0", "0 0 default 256 4096 256 1 0", "0 0 default 512 2048 512 1 0", 16384)),
    ("GE_NT_LOADS=1", ("64 0 0 ww8:140001", "64 2188 0 0 1 0", "0 0 default 64 2188 64 1 0", "0 0 alt 256 547 256 1 0", 2188)),
    ("GE_NT_LOADS=-1", ("64 0 0 ww8:140001", "64 2188 0 0 0 0", "0 0 default 64 2188 64 1 0", "0 0 default 256 547 256 1 0", 2188)),
    ("GE_LOWOCC_ROOMS=0", ("64 0 0 ww8:3000", "64 47 0 0 0 0", "0 0 default 64 47 64 1 0", "0 0 default 256 12 256 1 0", 48)),
    ("GE_LOWOCC_ROOMS=99999999", ("64 0 0 ww8:140001", "64 2188 0 1 0 0", "1 0 no_recycle 64 2188 64 1 1", "1 0 default 64 2188 64 1 0", 2188)),
    ("GE_HALF_WAVES=0", ("64 0 0 ww8:3000", "64 47 0 1 0 0", "1 0 no_recycle 64 47 64 1 1", "1 0 default 64 47 64 1 0", 47)),
    ("GE_HALF_WAVES=1", ("64 0 0 ww8:49152", "64 768 0 1 0 0", "1 0 no_recycle 64 1536 32 1 1", "1 0 default 64 1536 32 1 0", 1536)),
    ("GE_HALF_WAVES=-1", ("64 0 0 ww8:49152", "64 768 0 1 0 0", "1 0 no_recycle 64 1024 48 1 1", "1 0 default 64 768 64 1 0", 1024)),
    ("GE_NO_GENERIC_SHAPES=1", ("64 1 11 tt4:3000", "64 47 0 1 1 0", "1 1 default 64 94 32 0 0", "1 1 default 64 47 64 0 0", 94)),
]

# default knobs, and every setting of tests/test_gpu_knobs.py, tools/half_waves_ab.sh and tools/k1_block_ab.sh
SWEEP_KNOBS = [
    "", "GE_LOWOCC_ROOMS=0", "GE_LOWOCC_ROOMS=99999999", "GE_LOWOCC_ROOMS=0 GE_BLOCK_THREADS=256", "GE_LOWOCC_ROOMS=99999999 GE_BLOCK_THREADS=128",
    "GE_NT_LOADS=1 GE_LOWOCC_ROOMS=0", "GE_NT_LOADS=1", "GE_NT_LOADS=0 GE_LOWOCC_ROOMS=0", "GE_NT_LOADS=0", "GE_HALF_WAVES=0", "GE_HALF_WAVES=1",
    "GE_SINGLE_BLOCK=256", "GE_SINGLE_BLOCK=512", "GE_SINGLE_BLOCK=1024",
]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("launch_plan") / "launch_plan"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-o", str(out),
                           os.path.join(ROOT, "tests", "native", "launch_plan.cpp")])
    return str(out)


def run(exe, knobs, mode, stdin=""):
    p = subprocess.run([exe, *knobs.split(), mode], input=stdin, capture_output=True, text=True, timeout=600)
    return p.returncode, p.stdout, p.stderr


def plans(exe, knobs, shapes):
    """{shape: {tag: fields}} of the program's B / F0 / F1 / S / T lines, in the compact forms of PINNED."""
    rc, out, err = run(exe, knobs, "plans", "".join(s + "\n" for s in shapes))
    assert rc == 0, err[-2000:]
    got = [{} for _ in shapes]
    for i, line in enumerate(out.splitlines()):
        tag, rest = line.split(" ", 1)
        val = rest.rsplit(" : ", 1)[1]
        if tag == "T":
            got[i // 5][tag] = int(val)
            continue
        d = dict(f.split("=") for f in val.split())
        if tag == "B":
            got[i // 5][tag] = " ".join(d[k] for k in ("bt", "nblocks", "begin", "low", "stream", "gshape"))
        else:
            n_seg = shapes[i // 5].split()[3].count(",") + 1
            single = tag == "S" or shapes[i // 5].split()[0] == "1"
            assert d["single"] == str(int(single)) and d["mixed"] == str(int(n_seg > 1)), line
            got[i // 5][tag] = " ".join(d[k] for k in ("low", "gen", "load", "bt", "blocks", "rpb", "queue", "pull"))
    return got


def check_rows(exe, knobs, rows):
    got = plans(exe, knobs, [r[0] for r in rows])
    for (shape, batch, fused, single, stamps), g in zip(rows, got):
        assert (g["B"], g["F0"], g["S"], g["T"]) == (batch, fused, single, stamps), (knobs, shape, g)
        assert g["F1"] == fused.replace("no_recycle", "default"), (knobs, shape, g)   # restart on: only the recycle form differs


def test_pinned_plans_on_both_sides_of_every_threshold(exe):
    check_rows(exe, "", PINNED)


@pytest.mark.parametrize("knob,row", KNOB_ROWS, ids=[k for k, _ in KNOB_ROWS])
def test_knob_overrides_and_invalid_values(exe, knob, row):
    check_rows(exe, knob, [row])


@pytest.mark.parametrize("knobs", SWEEP_KNOBS, ids=[k.replace("GE_", "").replace(" ", "+").lower() or "default" for k in SWEEP_KNOBS])
def test_invariants_over_the_sweep(exe, knobs):
    """Grid coverage, block shape, at most 1 024 lone wavefronts (default knobs), where the ALT and NO_RECYCLE forms may appear,
    and a stamp record for every wavefront of the fused and the single-turn launch (launch_plan.cpp check_launch)."""
    rc, out, err = run(exe, knobs, "check")
    # 2 680 room counts x 7 forms x 2 max_fuse x 4 tables, less the 32 mixes of fewer rooms than segments
    assert rc == 0 and out.splitlines()[-1] == "checked 150048 cases, 0 violations", (out[-3000:], err[-2000:])


@pytest.mark.parametrize("knobs", ["", "GE_NO_GRAPH=1"], ids=["default", "no_graph=1"])
def test_launch_sequence(exe, knobs):
    """The turns of every launch of a step, "a single-turn launch is due", and whether the step replays a graph: at least
    GRAPH_MIN_LAUNCHES = 4 launches, never under GE_NO_GRAPH (pinned: 255 turns in 32 launches of 8 and in 4 launches of up to 64 replay, 129 turns in 3 launches do not)."""
    pairs = [(n, f) for n in (1, 2, 63, 64, 65, 128, 129, 255) for f in (1, 8, 64)]
    rc, out, err = run(exe, knobs, "seq", "".join(f"{n} {f}\n" for n, f in pairs))
    graph = {tuple(int(x) for x in l.split(" : ")[0].split()[1:]): l.rsplit("graph=", 1)[1] for l in out.splitlines()}
    assert (graph[255, 8], graph[129, 64], graph[255, 64]) == (("0", "0", "0") if knobs else ("1", "0", "1")), out
    assert rc == 0, err[-2000:]
    for (n, f), line in zip(pairs, out.splitlines()):
        head, rest = line.split(" : ")
        assert head == f"Q {n} {f}"
        d = dict(x.split("=") for x in rest.split())
        turns = [int(t) for t in d["launches"].split(",")]
        assert sum(turns) == n and all(t == f for t in turns[:-1]) and 1 <= turns[-1] <= f, line
        assert d["single"] == str(int(1 in turns)), line
        assert d["single"] == str(int(n % f == 1 or f == 1)), line              # the expression the sequence replaced
        assert d["graph"] == str(int(len(turns) >= 4 and not knobs)), line

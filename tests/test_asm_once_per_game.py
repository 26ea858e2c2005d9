"""The once-per-game work of the lone-wavefront Werewolf x 8 turn is out of its tail-recycling turn loops, from the assembly that is
shipped (CPU: hipcc -S needs no GPU).  `tools/asm_shadow.py --paths` counts the instructions of the common turn of every turn loop,
from the loop header to its back edge; tools/asm_once_per_game.json holds those counts for the two tail-recycling loops (untraced,
traced) on the parent commit and with the deal kept as words and the restart known at compile time (ge_device.h DEAL_WORDS,
TAIL_RECYCLE / TAIL_KEEP; the keys of the file's `parts` are the names the two had as switches): the role words of a prepared deal
are no longer rebuilt on every turn, and a recycling turn no longer records an `end_turn` that recycling overwrites.  Instruction
counts only; what they are worth in time is profiles/ab_lone_once_per_game.txt."""
import json
import os
import subprocess
import sys

from conftest import ROOT

TOOL = os.path.join(ROOT, "tools", "asm_shadow.py")
KERNEL = "Werewolf x 8, lone-wavefront, fused"


def test_tail_loops_are_shorter_than_the_parents():
    p = subprocess.run([sys.executable, TOOL, "--paths"], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-1500:])
    got = {k: v for k, v in json.loads(p.stdout).items() if k.startswith(KERNEL + " / loop ")}
    with open(os.path.join(ROOT, "tools", "asm_once_per_game.json")) as f:
        pinned = json.load(f)
    assert pinned["margin"] == 10 and pinned["parent"] == {"traced": 384, "untraced": 357}
    # head and tail form, each traced and untraced: the peeled last turn of a launch is straight-line code, not a fifth loop
    assert len(got) == 4, f"the kernel has {len(got)} turn loops: {sorted(got)}"
    # the tail-recycling loops are the two whose deal blocks stand behind the back edge (tests/test_asm_cold_deal.py); the
    # traced one stores an event per turn and is the longer
    tail = sorted(v["insns"] for v in got.values() if v["deal_blocks"] == 0)
    assert len(tail) == 2, "not two tail-recycling loops"
    for name, insns in zip(("untraced", "traced"), tail):
        assert insns <= pinned["change"][name], f"{name} tail loop: {insns} instructions on the common turn, pinned {pinned['change'][name]}"
        assert insns <= pinned["parent"][name] - pinned["margin"], f"{name} tail loop: {insns} instructions, the parent's had {pinned['parent'][name]}"

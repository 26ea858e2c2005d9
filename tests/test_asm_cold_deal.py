"""The rare role-deal paths of the lone-wavefront Werewolf x 8 turn stand behind its turn loops, from the assembly that is shipped
(CPU: hipcc -S needs no GPU).  `tools/asm_shadow.py --paths` walks the common turn of every turn loop from the loop header to its
back edge; tools/asm_shadow_paths.json pins, per loop of the Werewolf x 8 fused lone kernel, how many role-deal blocks that
path runs through and how many branches are taken on it (the figures of the adopted build, profiles/ab_lone_cold_deal.txt).  In
the tail-recycling loops (ge_device.h ww_apply_effect, TAILR) the path holds neither the on-the-spot deal of
ww_apply_effect nor the `deal_now` block of ww_prepare_deal; the head-restart loops keep the parent's form and figures."""
import json
import os
import subprocess
import sys

from conftest import ROOT

TOOL = os.path.join(ROOT, "tools", "asm_shadow.py")
KERNEL = "Werewolf x 8, lone-wavefront, fused"


def test_deal_blocks_stand_behind_the_turn_loops():
    p = subprocess.run([sys.executable, TOOL, "--paths"], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-1500:])
    got = json.loads(p.stdout)
    with open(os.path.join(ROOT, "tools", "asm_shadow_paths.json")) as f:
        pinned = json.load(f)
    assert len(pinned) == 4 and all(k.startswith(KERNEL + " / loop ") for k in pinned)      # a loop per trace setting and restart form
    assert sorted(k for k in got if k.startswith(KERNEL)) == sorted(pinned), "the kernel's turn loops are not the pinned ones"
    for k, want in pinned.items():
        assert got[k]["deal_blocks"] <= want["deal_blocks"], f"{k}: the common turn runs through {got[k]['deal_blocks']} role-deal blocks, pinned {want['deal_blocks']}"
        assert got[k]["taken"] <= want["taken"], f"{k}: {got[k]['taken']} branches taken on the common turn, pinned {want['taken']}"
    cold = [k for k, want in pinned.items() if want["deal_blocks"] == 0]
    assert len(cold) == 2, "the two tail-recycling loops (untraced, traced) are the ones with both deal blocks out of line"
    for k in cold:
        assert got[k]["out_of_line"] and got[k]["insns"] < got[k]["static"] - 200, f"{k}: no block of the loop stands behind its back edge"

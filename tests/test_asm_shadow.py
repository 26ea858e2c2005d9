"""What the lone-wavefront turn loops run inside their LDS waits, from the assembly that is shipped (CPU: hipcc -S needs no GPU):
`tools/asm_shadow.py --check` fails when fewer instructions than tools/asm_shadow_baseline.json records stand between an LDS read
and the wait for it - a compiler or source change that moves the shadow work shows up here and gets measured, instead of
costing a few per cent on the GPU that nobody looks for.  The counting rule itself is pinned on a hand-written listing."""
import json
import os
import subprocess
import sys

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
TOOL = os.path.join(ROOT, "tools", "asm_shadow.py")


def test_shadow_work_stands_in_front_of_its_waits():
    """The guard of the adopted placement is the `to_atomic` floor of the first slot read (Werewolf x 8: 80 vector instructions
    from that read to the first round's atomic, 67 with the second shadow's work elsewhere; x 12: 130 against 119).  The
    `result` rows only have to be non-zero, and what stands there today is the read's own address arithmetic (1 - 4
    instructions), not shadow work: that assertion keeps the rows and their waits found, it guards nothing."""
    p = subprocess.run([sys.executable, TOOL, "--json", "--check"], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-1500:])
    rows = json.loads(p.stdout)
    results = [r for r in rows if r["read"] == "result" and r["kernel"].startswith("Werewolf")]
    assert {r["kernel"] for r in results} == {"Werewolf x 8, lone-wavefront, fused", "Werewolf x 12, lone-wavefront, fused"}
    assert len(results) >= 6                                     # x 8: a loop per trace setting and restart form; x 12: per trace setting
    for r in results:
        assert r["vector"] > 0 and r["wait"], f"nothing covers the result read: {r}"
    with open(os.path.join(ROOT, "tools", "asm_shadow_baseline.json")) as f:
        floor = json.load(f)
    assert all(floor[f"{r['kernel']} / result"]["vector"] > 0 for r in results)
    # what the adopted placement is: the second shadow's work stands between the first slot read and the first round's atomic
    # (Werewolf x 8: 80 vector instructions there, 67 with that work behind the result read)
    slots = [r for r in rows if r["read"] == "slot" and r["kernel"].startswith("Werewolf")]
    assert slots and all(r["to_atomic"] >= floor[f"{r['kernel']} / slot"]["to_atomic"] > 0 for r in slots)


LISTING = """\
_ZN12_GLOBAL__N_114ge_step_kernelILi0ELb1ELi0ELb0ELi0EEEvPKNS_6SegDevE: ; @kernel
\ts_load_dword s0, s[0:1], 0x0
.LBB0_1:                                ; =>This Loop Header: Depth=1
\tds_read_b32 v1, v0 offset:1024
\tv_add_u32_e32 v2, v2, v3
\tds_write_b64 v4, v[5:6]
\ts_waitcnt lgkmcnt(1)
\tds_write_b128 v4, v[8:11]
\tds_read_b128 v[8:11], v4
\tv_add_u32_e32 v2, v2, v3
\ts_mov_b32 s4, 0
.LBB0_2:                                ;   Parent Loop BB0_1 Depth=1
                                        ; =>  This Inner Loop Header: Depth=2
\ts_waitcnt lgkmcnt(0)
\tds_or_b32 v1, v2
\ts_cbranch_vccnz .LBB0_4
; %bb.3:                                ;   in Loop: Header=BB0_2 Depth=2
\tds_read_b128 v[8:11], v4
\ts_branch .LBB0_2
.LBB0_4:                                ;   in Loop: Header=BB0_1 Depth=1
\tds_read_b32 v1, v0
\ts_cmp_eq_u32 s5, 0
\ts_cbranch_scc1 .LBB0_6
; %bb.5:                                ;   in Loop: Header=BB0_1 Depth=1
\tv_mul_lo_u32 v7, v7, v7
\tv_mul_lo_u32 v7, v7, v7
\tv_mul_lo_u32 v7, v7, v7
.LBB0_6:                                ;   in Loop: Header=BB0_1 Depth=1
\tv_xor_b32_e32 v2, v2, v3
\tv_xor_b32_e32 v2, v2, v3
\ts_waitcnt vmcnt(0)
\ts_waitcnt lgkmcnt(0)
\tv_lshrrev_b32_e32 v4, 1, v1
\ts_cbranch_scc0 .LBB0_1
; %bb.7:
\ts_endpgm
.Lfunc_end0:
"""


def test_counting_rule_on_a_listing(tmp_path):
    """ord: covered by lgkmcnt(1) with one LDS operation behind it, 1 vector; slot: 1 vector + 1 scalar up to the queue loop's
    wait; slot+: the branch back, nothing else; result: the wave-uniform skip of the deal block is taken (its three multiplies
    are not counted), a wait for another counter is not the read's."""
    import asm_shadow
    f = tmp_path / "listing.s"
    f.write_text(LISTING)
    rows = asm_shadow.collect(str(f))
    assert [r["to_atomic"] for r in rows if r["read"] == "slot"] == [1]      # the vector add behind the slot read, up to ds_or
    got = {r["read"]: (r["vector"], r["scalar"], r["lds"], r["wait"]) for r in rows}
    assert got == {"ord": (1, 0, 1, "s_waitcnt lgkmcnt(1)"), "slot": (1, 1, 0, "s_waitcnt lgkmcnt(0)"),
                   "slot+": (0, 1, 0, "s_waitcnt lgkmcnt(0)"), "result": (2, 2, 0, "s_waitcnt lgkmcnt(0)")}

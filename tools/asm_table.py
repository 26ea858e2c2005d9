#!/usr/bin/env python3
"""Registers, spills, scratch, LDS and occupancy of every kernel of libge_step.so, from the compiler's own remarks
(`make -C game_engine_amd/csrc asm` = hipcc -S -Rpass-analysis=kernel-resource-usage): the source of DESIGN.md's register
table, so that the document cannot drift from the build.

    python tools/asm_table.py            run `make asm` and print the table (markdown)
    python tools/asm_table.py --json     the same as JSON (tools/design_tables.py reads this)
    python tools/asm_table.py --check    exit 1 if ANY kernel uses scratch or spills a vector register, or spills more scalar
                                         registers (to VGPR lanes: v_writelane / v_readlane, no memory) than the committed
                                         baseline tools/asm_baseline.json allows for it (--write-baseline records today's)
tests/test_asm_table.py runs --check on the CPU (hipcc -S needs no GPU), so the table of DESIGN.md and this claim stay pinned.
"""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "game_engine_amd", "csrc")
KINDS = ["Werewolf x 8", "Werewolf x 12", "Two-Truths x 4", "Two-Truths x 8", "Two-Truths x 12"]
KEYS = {"Function Name": "name", "TotalSGPRs": "sgprs", "VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch",
        "Occupancy [waves/SIMD]": "occupancy", "SGPRs Spill": "sgpr_spill", "VGPRs Spill": "vgpr_spill", "LDS Size [bytes/block]": "lds_static"}


def describe(mangled: str) -> dict:
    """ge_step_kernel<KIND, LOWOCC, GENERIC, SINGLE, LD> / ge_step_kernel_mixed<LOWOCC, GENERIC, SINGLE> / the helper kernels"""
    m = re.search(r"ge_step_kernel_mixedILb([01])ELi(\d)ELb([01])E", mangled)
    if m:
        low, gen = m.group(1) == "1", int(m.group(2))
        return {"kernel": "ge_step_kernel_mixed", "layout": "mixed batch", "lowocc": low, "generic": gen, "single": m.group(3) == "1"}
    m = re.search(r"ge_step_kernelILi(\d)ELb([01])ELi(\d)ELb([01])ELi(\d)E", mangled)
    if m:
        return {"kernel": "ge_step_kernel", "layout": KINDS[int(m.group(1))], "lowocc": m.group(2) == "1", "generic": int(m.group(3)),
                "single": m.group(4) == "1", "ld": int(m.group(5))}
    m = re.search(r"ge_pool_kernelILi(\d)ELi(\d)E", mangled)
    if m:
        return {"kernel": "ge_pool_kernel", "layout": KINDS[int(m.group(1))], "lowocc": True, "generic": int(m.group(2)), "single": True}
    m = re.search(r"ge_run_kernelILi(\d)ELi(\d)E", mangled)
    if m:
        return {"kernel": "ge_run_kernel", "layout": KINDS[int(m.group(1))], "lowocc": True, "generic": int(m.group(2)), "single": True}
    m = re.search(r"ge_find_kernelILi(\d)ELi(\d)E", mangled)
    if m:
        return {"kernel": "ge_find_kernel", "layout": KINDS[int(m.group(1))], "lowocc": False, "generic": int(m.group(2)), "single": True}
    m = re.search(r"ge_seat_step_kernelILi(\d)ELi(\d)E", mangled)
    if m:
        return {"kernel": "ge_seat_step_kernel", "layout": KINDS[int(m.group(1))], "lowocc": True, "generic": int(m.group(2)), "single": False}
    m = re.search(r"ge_seat_run_kernelILi(\d)ELi(\d)E", mangled)
    if m:
        return {"kernel": "ge_seat_run_kernel", "layout": KINDS[int(m.group(1))], "lowocc": True, "generic": int(m.group(2)), "single": True}
    m = re.search(r"ge_gather_testILi(\d)ELi(\d)E", mangled)
    if m:
        return {"kernel": "ge_gather_test", "layout": KINDS[int(m.group(1))], "lowocc": False, "generic": int(m.group(2)), "single": True}
    m = re.search(r"ge_gather_emitILi(\d)E", mangled)
    if m:
        return {"kernel": "ge_gather_emit", "layout": KINDS[int(m.group(1))], "lowocc": False, "generic": False, "single": True}
    m = re.search(r"ge_rollout_kernelILi(\d)ELi(\d)E(?:Li(\d)E)?", mangled)
    if m:
        return {"kernel": "ge_rollout_kernel", "layout": KINDS[int(m.group(1))], "lowocc": True, "generic": int(m.group(2)), "single": True,
                "act": int(m.group(3) or 0)}
    m = re.search(r"ge_advise_planILi(\d)E", mangled)
    if m:
        return {"kernel": "ge_advise_plan", "layout": KINDS[int(m.group(1))], "lowocc": False, "generic": False, "single": True}
    m = re.search(r"ge_observe_kernelILi(\d)E", mangled)
    if m:
        return {"kernel": "ge_observe_kernel", "layout": KINDS[int(m.group(1))], "lowocc": False, "generic": False, "single": True}
    m = re.search(r"ge_act_kernelILi(\d)E", mangled)
    if m:
        return {"kernel": "ge_act_kernel", "layout": KINDS[int(m.group(1))], "lowocc": False, "generic": False, "single": True}
    m = re.search(r"ge_teach_planILi(\d)E", mangled)
    if m:
        return {"kernel": "ge_teach_plan", "layout": KINDS[int(m.group(1))], "lowocc": False, "generic": False, "single": True}
    m = re.search(r"ge_playout_plan_rangedILi(\d)E", mangled)
    if m:
        return {"kernel": "ge_playout_plan_ranged", "layout": KINDS[int(m.group(1))], "lowocc": False, "generic": False, "single": True}
    m = re.search(r"ge_runp_plan_rangedILi(\d)E", mangled)
    if m:
        return {"kernel": "ge_runp_plan_ranged", "layout": KINDS[int(m.group(1))], "lowocc": False, "generic": False, "single": True}
    m = re.search(r"ge_runp_rollout_rangedILi(\d)ELi(\d)E", mangled)
    if m:
        return {"kernel": "ge_runp_rollout_ranged", "layout": KINDS[int(m.group(1))], "lowocc": True, "generic": int(m.group(2)), "single": True}
    m = re.search(r"ge_playout_(plan|decide)ILi(\d)E", mangled)
    if m:
        return {"kernel": "ge_playout_" + m.group(1), "layout": KINDS[int(m.group(2))], "lowocc": False, "generic": False, "single": True}
    m = re.search(r"ge_runp_(rollout|turn)ILi(\d)ELi(\d)E", mangled)
    if m:
        return {"kernel": "ge_runp_" + m.group(1), "layout": KINDS[int(m.group(2))], "lowocc": True, "generic": int(m.group(3)), "single": True}
    m = re.search(r"ge_runp_planILi(\d)E", mangled)
    if m:
        return {"kernel": "ge_runp_plan", "layout": KINDS[int(m.group(1))], "lowocc": False, "generic": False, "single": True}
    m = re.search(r"N_1\d+(ge_[a-z_0-9]+?)E", mangled)
    return {"kernel": m.group(1) if m else mangled, "layout": "-", "lowocc": False, "generic": False, "single": False}


def collect(rebuild=True):
    cmd = ["make", "-C", CSRC, "asm"] + (["-B"] if rebuild else [])
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout)
        raise SystemExit("make asm failed")
    rows, cur = [], None
    for line in p.stdout.splitlines():
        m = re.search(r"remark: ([^:]+): (.*?) \[-Rpass-analysis", line)
        if not m or m.group(1).strip() not in KEYS:
            continue
        key, val = KEYS[m.group(1).strip()], m.group(2).strip()
        if key == "name":
            cur = {"name": val}
            cur.update(describe(val))
            rows.append(cur)
        elif cur is not None:
            cur[key] = int(val)
    return rows


def label(r):
    if r["kernel"] == "ge_pool_kernel":                          # ge_batch_step_rooms: one launch per segment present
        return f"{r['layout']}, indexed single-turn (ge_batch_step_rooms)" + (", GENERIC" if r["generic"] else "")
    if r["kernel"] == "ge_run_kernel":                           # ge_batch_run_rooms: one launch per segment present
        return f"{r['layout']}, indexed turn loop (ge_batch_run_rooms)" + (", GENERIC" if r["generic"] else "")
    if r["kernel"] == "ge_find_kernel":                          # ge_batch_find_rooms: one launch per segment of the range
        return f"{r['layout']}, test of a range of rooms (ge_batch_find_rooms)" + (", GENERIC" if r["generic"] else "")
    if r["kernel"] in ("ge_find_scan", "ge_find_emit"):          # ge_batch_find_rooms: behind the test launches
        what = {"ge_find_scan": "the scan of the wavefront counts", "ge_find_emit": "the ordered store of the hits"}[r["kernel"]]
        return f"{r['kernel']} (ge_batch_find_rooms: {what})"
    if r["kernel"] == "ge_seat_step_kernel":                     # ge_batch_step of a batch with a seat plane: one launch per segment and per max_fuse turns
        return f"{r['layout']}, whole-batch step under per-room seats (ge_batch_step after ge_batch_set_seats)" + (", GENERIC" if r["generic"] else "")
    if r["kernel"] == "ge_seat_run_kernel":                      # ge_batch_run_seats: one launch per segment of the range
        return f"{r['layout']}, seat run-on (ge_batch_run_seats)" + (", GENERIC" if r["generic"] else "")
    if r["kernel"] == "ge_gather_test":                          # ge_batch_gather_seats: one launch per segment of the range
        return f"{r['layout']}, due seats of a range of rooms (ge_batch_gather_seats)" + (", GENERIC" if r["generic"] else "")
    if r["kernel"] == "ge_gather_emit":                          # ge_batch_gather_seats: one launch per segment of the range, behind the scan
        return f"{r['layout']}, the ordered store of the due seats' observations (ge_batch_gather_seats)"
    if r["kernel"] == "ge_gather_scan":                          # ge_batch_gather_seats: between the test and the emit launches
        return "ge_gather_scan (ge_batch_gather_seats: the scan of the wavefront counts, and the list's two counts)"
    if r["kernel"] in ("ge_list_scatter", "ge_list_status"):     # ge_batch_act_listed: around ge_act_kernel
        what = {"ge_list_scatter": "the listed choices into the dense plane", "ge_list_status": "the listed entries' statuses from the dense plane"}[r["kernel"]]
        return f"{r['kernel']} (ge_batch_act_listed: {what})"
    if r["kernel"] in ("ge_seats_fill", "ge_seats_scatter"):     # ge_batch_set_seats
        what = {"ge_seats_fill": "a segment's mask for its rooms", "ge_seats_scatter": "the listed rooms' masks"}[r["kernel"]]
        return f"{r['kernel']} (ge_batch_set_seats: {what})"
    if r["kernel"] == "ge_advise_plan":                          # ge_batch_advise_seats: one launch per unit of listed entries
        return f"{r['layout']}, advised seats, plan (ge_batch_advise_seats)"
    if r["kernel"] == "ge_advise_reduce":                        # ge_batch_advise_seats: behind the playouts of a unit
        return "ge_advise_reduce (ge_batch_advise_seats: the advice records from the accumulators)"
    if r["kernel"] == "ge_observe_kernel":                       # ge_batch_observe_seats: one launch per segment of the range
        return f"{r['layout']}, seat observations (ge_batch_observe_seats)"
    if r["kernel"] == "ge_act_kernel":                           # ge_batch_act_seats: one launch per segment of the range
        return f"{r['layout']}, seat actions from device memory (ge_batch_act_seats)"
    if r["kernel"] == "ge_teach_plan":                           # ge_batch_teach_seats: one launch per part of a pass
        return f"{r['layout']}, taught seats, plan (ge_batch_teach_seats)"
    if r["kernel"] == "ge_teach_reduce":                         # ge_batch_teach_seats: behind the playouts of a pass
        return "ge_teach_reduce (ge_batch_teach_seats: the advice records from the accumulators)"
    if r["kernel"] == "ge_rollout_kernel" and r.get("act") == 4:  # GE_PLAYOUT_HALVING: one launch per unit and round
        return f"{r['layout']}, playouts over a replica range (GE_PLAYOUT_HALVING)" + (", GENERIC" if r["generic"] else "")
    if r["kernel"] == "ge_playout_plan_ranged":
        return f"{r['layout']}, playout seats, plan with replica ranges (GE_PLAYOUT_HALVING)"
    if r["kernel"] == "ge_runp_plan_ranged":
        return f"{r['layout']}, run-on with playout seats, plan with replica ranges (GE_PLAYOUT_HALVING)"
    if r["kernel"] == "ge_runp_rollout_ranged":
        return f"{r['layout']}, run-on with playout seats, playouts over a replica range (GE_PLAYOUT_HALVING)" + (", GENERIC" if r["generic"] else "")
    if r["kernel"] == "ge_playout_halve":
        return "ge_playout_halve (GE_PLAYOUT_HALVING: the cut between two rounds)"
    if r["kernel"] == "ge_rollout_kernel" and r.get("act") == 5:  # ge_batch_run_rooms_forecast: one launch per segment present, behind the run
        return f"{r['layout']}, playouts from a traced turn (ge_batch_run_rooms_forecast)" + (", GENERIC" if r["generic"] else "")
    if r["kernel"] == "ge_rollout_kernel" and r.get("act") in (6, 7):   # ge_batch_rollout_beliefs: one launch per segment present
        what = "weighted by beliefs" if r["act"] == 6 else "weighted by beliefs, outcome kept"
        return f"{r['layout']}, playouts from a seat's view {what} (ge_batch_rollout_beliefs)" + (", GENERIC" if r["generic"] else "")
    if r["kernel"] == "ge_rollout_kernel" and r.get("act") == 3:  # ge_batch_rollout_compare: one launch per segment present
        return f"{r['layout']}, playouts that keep their outcome (ge_batch_rollout_compare)" + (", GENERIC" if r["generic"] else "")
    if r["kernel"] == "ge_rollout_kernel" and r.get("act") == 2:  # ge_batch_rollout_seats: one launch per segment present
        return f"{r['layout']}, playouts from a seat's view (ge_batch_rollout_seats)" + (", GENERIC" if r["generic"] else "")
    if r["kernel"] == "ge_rollout_kernel" and r.get("act"):      # ge_batch_rollout_actions: one launch per segment present
        return f"{r['layout']}, playouts after actions (ge_batch_rollout_actions)" + (", GENERIC" if r["generic"] else "")
    if r["kernel"] == "ge_rollout_kernel":                       # ge_batch_rollout_rooms: one launch per segment present
        return f"{r['layout']}, playouts (ge_batch_rollout_rooms)" + (", GENERIC" if r["generic"] else "")
    if r["kernel"] in ("ge_playout_plan", "ge_playout_decide"):  # ge_batch_step_rooms_playout: one launch per unit of rooms
        return f"{r['layout']}, playout seats, {r['kernel'][11:]} (ge_batch_step_rooms_playout)"
    if r["kernel"] in ("ge_runp_plan", "ge_runp_rollout", "ge_runp_turn"):   # ge_batch_run_rooms_playout: enqueued per turn
        what = {"ge_runp_plan": "plan of the live rooms", "ge_runp_rollout": "playouts counted on the device", "ge_runp_turn": "turn of the live rooms"}[r["kernel"]]
        return f"{r['layout']}, run-on with playout seats, {what} (ge_batch_run_rooms_playout)" + (", GENERIC" if r["generic"] else "")
    if r["kernel"] == "ge_compare_kernel":                       # ge_batch_rollout_compare: one launch per chunk, behind the playouts
        return "ge_compare_kernel (ge_batch_rollout_compare: an entry against its baseline)"
    if r["kernel"] not in ("ge_step_kernel", "ge_step_kernel_mixed"):
        return r["kernel"]
    form = "single-turn" if r["single"] else "fused"
    occ = "lone-wavefront" if r["lowocc"] else "large-batch"
    shape = {0: "", 1: ", GENERIC", 2: ", GENERIC 1 x 1", 3: ", GENERIC 1 x 2"}[int(r["generic"])]
    return f"{r['layout']}, {occ}, {form}{shape}" + {0: "", 1: ", plain record loads", 2: ", streaming record loads", 3: ", restart off"}[r.get("ld", 0)]


def markdown(rows):
    out = ["| build | VGPRs | SGPRs | SGPR spills | VGPR spills | scratch B/lane | wavefronts / SIMD |", "|---|---|---|---|---|---|---|"]
    order = sorted(rows, key=lambda r: (r["kernel"] not in ("ge_step_kernel", "ge_step_kernel_mixed"), r["generic"], r["single"], r["layout"], not r["lowocc"]))
    for r in order:
        out.append(f"| {label(r)} | {r.get('vgprs', 0)} | {r.get('sgprs', 0)} | {r.get('sgpr_spill', 0)} | {r.get('vgpr_spill', 0)} | "
                   f"{r.get('scratch', 0)} | {r.get('occupancy', 0)} |")
    return "\n".join(out)


def main():
    rows = collect(rebuild=True)
    if "--json" in sys.argv:
        print(json.dumps(rows, indent=1))
        return
    print(markdown(rows))
    base_path = os.path.join(ROOT, "tools", "asm_baseline.json")
    if "--write-baseline" in sys.argv:
        with open(base_path, "w") as f:
            json.dump({label(r): r.get("sgpr_spill", 0) for r in rows if r.get("sgpr_spill", 0)}, f, indent=1, sort_keys=True)
            f.write("\n")
    if "--check" in sys.argv:
        with open(base_path) as f:
            allowed = json.load(f)
        bad = [f"{label(r)}: scratch {r.get('scratch', 0)} B/lane, {r.get('vgpr_spill', 0)} VGPR spills" for r in rows
               if r.get("scratch", 0) or r.get("vgpr_spill", 0)]
        bad += [f"{label(r)}: {r.get('sgpr_spill', 0)} SGPR spills, baseline {allowed.get(label(r), 0)}" for r in rows
                if r.get("sgpr_spill", 0) > allowed.get(label(r), 0)]
        if bad:
            raise SystemExit("register check failed: " + "; ".join(bad))


if __name__ == "__main__":
    main()

"""gpurun_out/prof_<tag>/ (written by scripts/profile_bench.sh on the GPU box) -> profiles/<tag>_*.
Usage: python scripts/summarise_profiles.py r01"""
import csv
import glob
import json
import os
import shutil
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
tag = sys.argv[1] if len(sys.argv) > 1 else "r01"
src = os.path.join(ROOT, "gpurun_out", f"prof_{tag}")
dst = os.path.join(ROOT, "profiles")


def find(sub, suffix):
    g = glob.glob(os.path.join(src, sub, "**", f"*{suffix}"), recursive=True)
    return g[0] if g else None


for suffix in ("kernel_stats.csv", "domain_stats.csv"):
    f = find("stats", suffix)
    if f:
        shutil.copy(f, os.path.join(dst, f"{tag}_bench_{suffix}"))
b = os.path.join(src, "bench_under_rocprof.json")
if os.path.exists(b):
    shutil.copy(b, os.path.join(dst, f"{tag}_bench_under_rocprof.json"))


def pmc(sub, counter):
    f = find(sub, "counter_collection.csv")
    per = {}
    if not f:
        return per
    for row in csv.DictReader(open(f)):
        if row["Counter_Name"] != counter:
            continue
        name = row["Kernel_Name"].split("(")[0]
        per.setdefault(name, []).append(float(row["Counter_Value"]))
    return {k: {"launches": len(v), "mean_kb_per_launch": sum(v) / len(v)} for k, v in per.items() if k.startswith("void kge::")}


fetch, write = pmc("fetch", "FETCH_SIZE"), pmc("write", "WRITE_SIZE")
out = {"command": "scripts/profile_bench.sh " + tag + " : rocprofv3 --pmc FETCH_SIZE, then --pmc WRITE_SIZE (separate passes), "
                  "each over `python bench.py --full --steps 10 --warmup 2 --no-cpu-baseline --no-eval --also none`",
       "correction": "MI355X_MICROARCH.md (HBM section): on gfx950 FETCH_SIZE reports half the bytes of 16 B/lane coalesced "
                     "reads -> doubled here; WRITE_SIZE used as reported (KB). Both count L2<->fabric traffic, Infinity-Cache "
                     "hits included, so for these cache-resident tables they bound HBM traffic from above.",
       "kernels": {}}
for k in sorted(set(fetch) | set(write)):
    e = {"FETCH_SIZE": fetch.get(k), "WRITE_SIZE": write.get(k)}
    fb = 2.0 * 1024 * fetch[k]["mean_kb_per_launch"] if k in fetch else None
    wb = 1024.0 * write[k]["mean_kb_per_launch"] if k in write else None
    e["fetch_bytes_per_launch_corrected"] = fb
    e["write_bytes_per_launch"] = wb
    e["bytes_per_launch"] = (fb or 0.0) + (wb or 0.0)
    out["kernels"][k] = e
step = [k for k in out["kernels"] if "train_fwdbwd_kernel" in k or "tile_backward_kernel" in k]
out["train_step_kernels"] = step
out["train_step_hbm_bytes_per_launch"] = sum(out["kernels"][k]["bytes_per_launch"] for k in step)
rnd = tag[:3] + "_" if tag[:1] == "r" and tag[1:3].isdigit() and tag[:3] != "r01" else ""   # round-1 files keep their names
json.dump(out, open(os.path.join(dst, rnd + "pmc_traffic.json"), "w"), indent=1)

# MFMA utilisation of the rank kernel: MfmaUtil = SQ_VALU_MFMA_BUSY_CYCLES / (GRBM_GUI_ACTIVE per XCD * #SIMD)
f = find("mfma", "counter_collection.csv")
if f:
    disp = {}   # per dispatch: the screened evaluate() launches this kernel too, and it returns at once (guard) -- keep the real runs
    for row in csv.DictReader(open(f)):
        if "rank_count_mfma" in row["Kernel_Name"]:
            disp.setdefault(row.get("Dispatch_Id", row.get("Dispatch_ID")), {})[row["Counter_Name"]] = float(row["Counter_Value"])
    per = {}
    for d in disp.values():
        if d.get("SQ_VALU_MFMA_BUSY_CYCLES", 0.0) > 1e6:
            for k, v in d.items():
                per.setdefault(k, []).append(v)
    if per:
        m = {k: sum(v) / len(v) for k, v in per.items()}
        gui = m.get("GRBM_GUI_ACTIVE", 0.0) / 8.0          # summed over the 8 XCDs
        mf = {"kernel": "rank_count_mfma_pipe_kernel", "launches": len(next(iter(per.values()))), "mean_per_launch": m,
              "gui_active_cycles_per_xcd": gui,
              "mfma_flop_per_launch": m.get("SQ_INSTS_VALU_MFMA_MOPS_F32", 0.0) * 512.0,
              "mfma_util": m.get("SQ_VALU_MFMA_BUSY_CYCLES", 0.0) / (gui * 1024.0) if gui else None,
              "note": "SQ_VALU_MFMA_BUSY_CYCLES = 64 cycles per v_mfma_f32_32x32x2_f32; 1024 SIMDs; GRBM_GUI_ACTIVE is reported "
                      "summed over 8 XCDs.  scripts/mfma_peak.hip (pure MFMA loop, same instruction) sustains 124-144 TFLOP/s on "
                      "this box, i.e. the practical ceiling is ~0.9 of the 157.3 TFLOP/s spec."}
        json.dump(mf, open(os.path.join(dst, rnd + "pmc_mfma.json"), "w"), indent=1)
        print("mfma util:", mf["mfma_util"])
    # the int8 screening kernel of evaluate() (round 3): 32 busy cycles per v_mfma_i32_32x32x32_i8
    per = {}
    for row in csv.DictReader(open(f)):
        if "rank_screen_kernel" in row["Kernel_Name"]:
            per.setdefault(row["Counter_Name"], []).append(float(row["Counter_Value"]))
    if per:
        m = {k: sum(v) / len(v) for k, v in per.items()}
        gui = m.get("GRBM_GUI_ACTIVE", 0.0) / 8.0
        sc = {"kernel": "rank_screen_kernel", "launches": len(next(iter(per.values()))), "mean_per_launch": m,
              "gui_active_cycles_per_xcd": gui,
              "mfma_instructions_per_launch": m.get("SQ_VALU_MFMA_BUSY_CYCLES", 0.0) / 32.0,
              "mfma_util": m.get("SQ_VALU_MFMA_BUSY_CYCLES", 0.0) / (gui * 1024.0) if gui else None,
              "note": "v_mfma_i32_32x32x32_i8: 32 busy cycles each, 6 per 32x32 output block and 32-unit slab (three int8 limbs per "
                      "side, the six most significant limb products); two waves per SIMD (256 registers each).  Round 5's kernel "
                      "stages BOTH operands through LDS two stages ahead (round 4's took the query fragments from L2 one stage "
                      "ahead: MfmaUtil 0.38, profiles/r04_pmc_screen.json)"}
        json.dump(sc, open(os.path.join(dst, rnd + "pmc_screen.json"), "w"), indent=1)
        print("screen kernel mfma util:", sc["mfma_util"])
print(json.dumps({k: out["kernels"][k]["bytes_per_launch"] for k in out["kernels"]}, indent=1))
print("train step:", out["train_step_hbm_bytes_per_launch"])

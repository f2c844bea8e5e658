#!/usr/bin/env python3
"""Shared-negative training for the distance models (SharedDistanceNegatives, kge_train_shared_dist.hip) against the per-corruption
step on the SAME negatives, by the method of bench_shared_negatives.py: synthetic FB15k-237 sizes (N = 14 505, R = 237), B = 10 000,
G = M, for TransE k = 200 with multiclass_nll and RotatE k = 200 with self_adversarial, M = 64, 256, 1024.

  (a) shared   : amdkge_sample_shared -> amdkge_train_shared_dist_fwdbwd (three distance tiles) -> amdkge_opt_step
  (b) override : the equivalent [(B * M), 3] rows as neg_override of the existing step at eta = M: amdkge_train_step_tiled where its
                 plan takes the shape, otherwise amdkge_train_fwdbwd + amdkge_opt_step.  Building the rows is NOT timed.  (b) needs
                 nothing this script's feature adds: `--only b --root DIR` runs it on a build of the parent commit.

Method: HIP events around each step, `--warmup` untimed steps per configuration, then `--reps` timed steps; the median is reported
with the minimum and the maximum.  triples/s counts the B * (1 + M) scored triples of a step.  The split between the three tile modes
needs KERNEL time: run the script once more under `rocprofv3 --kernel-trace --stats` with `--only a --models MODEL --M M` and hand
the kernel-stats csv to `--tile-stats MODEL:M=stats.csv`.  Per mode that adds the time per step and the VALU lane-slots a pair-unit
took: time x the vector peak (256 CUs x 4 SIMDs x 32 lanes per clock x 2.4 GHz = 78.6 T lane-operations/s) / (B M k) -- the number of
lane-operations the mode could have issued per pair-unit at peak, to be read against the instructions a pair-unit needs.

usage: bench_shared_distance.py [--models TransE RotatE] [--M 64 256 1024] [--only a|b] [--root DIR] [--reps 20] [--warmup 3]
                                [--out profiles/shared_distance.json]
                                [--tile-stats MODEL:M=stats.csv ... [--from-json earlier.json] [--stats-steps N]]"""
import argparse
import csv
import json
import os
import re
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

VALU_PEAK = 256 * 4 * 32 * 2.4e9
CONFIGS = {"TransE": "multiclass_nll", "RotatE": "self_adversarial"}
LOSS_PARAMS = {"multiclass_nll": (0.0, 0.0), "self_adversarial": (3.0, 0.5)}   # (margin, alpha): the defaults of the loss classes
K_UNITS, B = 200, 10000
MODES = {0: "fwd", 1: "dq", 2: "de"}


def override_rows(torch, batch, ids, side, G):
    """device restatement of the step's definition: row j * B + i = positive i with its side[i] entity replaced by ids[i // G][j]"""
    Bn, M = int(batch.shape[0]), int(ids.shape[1])
    i = torch.arange(Bn, device=batch.device).repeat(M)
    j = torch.arange(M, device=batch.device).repeat_interleave(Bn)
    repl = ids.long()[i // min(G, Bn), j].int()
    subj = side[i] != 0
    pos = batch[i]
    return torch.stack([torch.where(subj, repl, pos[:, 0]), pos[:, 1], torch.where(subj, pos[:, 2], repl)], 1).contiguous()


def summary(ms, M):
    med = statistics.median(ms)
    return {"ms_per_step": med, "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms), "triples_per_s": B * (1 + M) / (med * 1e-3)}


def run(models, Ms, only, reps, warmup):
    import torch

    from ampligraph_amd import _ffi
    from ampligraph_amd.datasets import make_synthetic_kg
    from ampligraph_amd.engine import KgeEngine

    d = make_synthetic_kg()
    N, R = d["n_ents"], d["n_rels"]
    X = torch.as_tensor(d["train"]).cuda()
    nb = int(X.shape[0]) // B
    out = {"k": K_UNITS, "B": B, "N": N, "R": R, "valu_peak_lane_ops_per_s": VALU_PEAK, "results": []}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for model in models:
        loss_name = CONFIGS[model]
        eng = KgeEngine(model, K_UNITS, N, R, max_rel_size=R)
        rng = np.random.default_rng(0)
        eng.set_tables(rng.uniform(-.02, .02, (N, eng.K)).astype(np.float32), rng.uniform(-.1, .1, (R, eng.K)).astype(np.float32))
        eng.prepare_training("adam")
        loss = _ffi.Loss(_ffi.LOSSES[loss_name], 0, *LOSS_PARAMS[loss_name])
        has_dist = hasattr(eng, "train_shared_dist_fwdbwd")
        has_draw = hasattr(eng, "sample_shared")
        for M in Ms:
            G = M
            res = {"model": model, "loss": loss_name, "M": M, "G": G, "pair_units_per_step": B * M * K_UNITS}
            for path in ("a", "b"):
                if only and path != only:
                    continue
                if path == "a" and not has_dist:
                    res["a"] = {"skipped": "this build has no distance-tile shared step"}
                    continue
                ms, how = [], None
                try:
                    for s in range(-warmup, reps):
                        xb = X[(s % nb) * B:(s % nb + 1) * B]
                        o = _ffi.Opt(2, 2, 1e-3, .9, .999, 1e-7, 0.0, s + warmup + 1)
                        if path == "a":
                            ev[0].record()
                            ids, side = eng.sample_shared(xb, G, M, 0, s + warmup)
                            eng.train_shared_dist_fwdbwd(xb, G, M, ids, side, loss)
                            eng.opt_step(o)
                            ev[1].record()
                            how = "sample_shared + train_shared_dist_fwdbwd + opt_step"
                        else:
                            if has_draw:
                                ids, side = eng.sample_shared(xb, G, M, 0, s + warmup)
                            else:   # a build without the draw: any ids of the same structure cost the same
                                g = torch.Generator(device="cuda").manual_seed(s + warmup)
                                ids = torch.randint(0, N, (-(-B // G), M), device="cuda", dtype=torch.int32, generator=g)
                                side = torch.randint(0, 2, (B,), device="cuda", dtype=torch.int32, generator=g)
                            negs = override_rows(torch, xb, ids, side, G)
                            torch.cuda.synchronize()
                            tiled = eng.tiled_supported(B, M)
                            ev[0].record()
                            if tiled:
                                eng.train_step_tiled(xb, M, loss, o, 0, s + warmup, neg_override=negs)
                            else:
                                eng.train_fwdbwd(xb, M, loss, 0, s + warmup, neg_override=negs)
                                eng.opt_step(o)
                            ev[1].record()
                            how = "train_step_tiled(neg_override)" if tiled else "train_fwdbwd(neg_override) + opt_step"
                        torch.cuda.synchronize()
                        if s >= 0:
                            ms.append(ev[0].elapsed_time(ev[1]))
                    res[path] = dict(summary(ms, M), path=how)
                except (_ffi.AmdKgeError, ValueError) as e:   # a shape the existing step does not take is a result, not a crash
                    res[path] = {"unsupported": str(e)}
            if "a" in res and "b" in res and "ms_per_step" in res["a"] and "ms_per_step" in res["b"]:
                res["speedup_a_over_b"] = res["b"]["ms_per_step"] / res["a"]["ms_per_step"]
                res["a_beats_b_beyond_b_spread"] = res["b"]["ms_per_step"] - res["a"]["ms_per_step"] > res["b"]["max_ms"] - res["b"]["min_ms"]
            out["results"].append(res)
    return out


def tile_time_per_step(stats_csv, steps):
    """rocprofv3's kernel_stats csv -> {mode: ns per step} of the dist_tile_kernel<MODEL, MODE> instantiations, and every other kernel's"""
    per = {"fwd": 0.0, "dq": 0.0, "de": 0.0, "other": 0.0}
    for row in csv.DictReader(open(stats_csv)):
        name, ns = row.get("Name", ""), float(row["TotalDurationNs"])
        m = re.search(r"dist_tile_kernel<\s*\d+\s*,\s*(\d+)\s*>", name)
        per[MODES[int(m.group(1))] if m else "other"] += ns
    return {k: v / steps for k, v in per.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", nargs="+", default=list(CONFIGS), choices=list(CONFIGS))
    ap.add_argument("--M", type=int, nargs="+", default=[64, 256, 1024])
    ap.add_argument("--only", choices=["a", "b"], default=None)
    ap.add_argument("--root", default=ROOT, help="the tree the package is imported from (default: this one; a build of the parent for its (b))")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--tile-stats", nargs="*", default=[], help="MODEL:M=kernel_stats.csv of an `--only a --models MODEL --M M` run under rocprofv3 (same --reps / --warmup)")
    ap.add_argument("--from-json", default=None, help="take the timings from an earlier --out file (no GPU run) and only add --tile-stats to them")
    ap.add_argument("--stats-steps", type=int, default=None, help="steps of the profiled runs (default: --reps + --warmup)")
    a = ap.parse_args()
    if a.from_json:
        out = json.load(open(a.from_json))
    else:
        sys.path.insert(0, os.path.abspath(a.root))
        import torch

        if not torch.cuda.is_available():
            sys.exit("bench_shared_distance: needs a GPU (no CPU fallback)")
        out = run(a.models, a.M, a.only, a.reps, a.warmup)
    for spec in a.tile_stats:
        key, path = spec.split("=", 1)
        model, m = key.split(":")
        for res in out["results"]:
            if res["model"] == model and res["M"] == int(m):
                per = tile_time_per_step(path, a.stats_steps or a.reps + a.warmup)
                res["kernel_ms_per_step"] = {k: v * 1e-6 for k, v in per.items()}
                res["lane_slots_per_pair_unit"] = {k: per[k] * 1e-9 * VALU_PEAK / res["pair_units_per_step"] for k in ("fwd", "dq", "de")}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

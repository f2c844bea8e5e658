#!/usr/bin/env python3
"""Shared-negative training against the per-corruption step on the SAME negatives, at the C2 shape (synthetic FB15k-237 sizes:
N = 14 505, R = 237, ComplEx k = 200, B = 10 000, multiclass_nll), for M = 64, 256, 1024 corruptions per positive with G = M.

  (a) shared   : amdkge_sample_shared -> amdkge_train_shared_fwdbwd (three matrix products) -> amdkge_opt_step
  (b) override : the equivalent [(B * M), 3] rows as neg_override of the existing step at eta = M: amdkge_train_step_tiled where its
                 plan takes the shape, otherwise amdkge_train_fwdbwd + amdkge_opt_step.  Building the rows is NOT timed.  (b) needs
                 nothing this script's feature adds (`--only b` runs on a build without it: the baseline of the parent commit).

Method: HIP events around each step, `--warmup` untimed steps per configuration, then `--reps` timed steps; the median is reported
with the minimum and the maximum.  triples/s counts the B * (1 + M) scored triples of a step.  The share of the fp32 MFMA peak
(157.3 TFLOP/s) needs KERNEL time: run the script once more under `rocprofv3 --kernel-trace --stats` with `--only a` and hand the
kernel-stats csv to `--gemm-stats`, which adds 6 B M K flops over the three shared_gemm_kernel instantiations' time per step.

usage: bench_shared_negatives.py [--M 64 256 1024] [--only a|b] [--reps 20] [--warmup 3] [--out profiles/shared_negatives.json]
                                 [--gemm-stats M=stats.csv ... [--from-json earlier.json] [--stats-steps N]]"""
import argparse
import csv
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ampligraph_amd import _ffi   # noqa: E402
from ampligraph_amd.datasets import make_synthetic_kg   # noqa: E402
from ampligraph_amd.engine import KgeEngine   # noqa: E402

MFMA_F32_PEAK = 157.3e12
MODEL, K_UNITS, B = "ComplEx", 200, 10000


def override_rows(batch, ids, side, G):
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


def run(Ms, only, reps, warmup):
    d = make_synthetic_kg()
    N, R = d["n_ents"], d["n_rels"]
    eng = KgeEngine(MODEL, K_UNITS, N, R, max_rel_size=R)
    rng = np.random.default_rng(0)
    eng.set_tables(rng.uniform(-.02, .02, (N, eng.K)).astype(np.float32), rng.uniform(-.1, .1, (R, eng.K)).astype(np.float32))
    eng.prepare_training("adam")
    loss = _ffi.Loss(_ffi.LOSSES["multiclass_nll"], 0, 0.0, 0.0)
    X = torch.as_tensor(d["train"]).cuda()
    nb = int(X.shape[0]) // B
    out = {"model": MODEL, "k": K_UNITS, "B": B, "N": N, "R": R, "loss": "multiclass_nll", "row_floats": eng.Ks, "results": []}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    has_shared = hasattr(eng, "train_shared_fwdbwd")
    for M in Ms:
        G = M
        res = {"M": M, "G": G, "gemm_flops_per_step": 6 * B * M * eng.Ks}
        for path in ("a", "b"):
            if only and path != only:
                continue
            if path == "a" and not has_shared:
                res["a"] = {"skipped": "this build has no shared-negative path"}
                continue
            ms, how = [], None
            try:
                for s in range(-warmup, reps):
                    xb = X[(s % nb) * B:(s % nb + 1) * B]
                    o = _ffi.Opt(2, 2, 1e-3, .9, .999, 1e-7, 0.0, s + warmup + 1)
                    if path == "a":
                        ev[0].record()
                        ids, side = eng.sample_shared(xb, G, M, 0, s + warmup)
                        eng.train_shared_fwdbwd(xb, G, M, ids, side, loss)
                        eng.opt_step(o)
                        ev[1].record()
                        how = "sample_shared + train_shared_fwdbwd + opt_step"
                    else:
                        if has_shared:
                            ids, side = eng.sample_shared(xb, G, M, 0, s + warmup)
                        else:   # the parent build: any ids of the same structure cost the same
                            g = torch.Generator(device="cuda").manual_seed(s + warmup)
                            ids = torch.randint(0, N, (-(-B // G), M), device="cuda", dtype=torch.int32, generator=g)
                            side = torch.randint(0, 2, (B,), device="cuda", dtype=torch.int32, generator=g)
                        negs = override_rows(xb, ids, side, G)
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
        out["results"].append(res)
    return out


def gemm_time_per_step(stats_csv, steps):
    """rocprofv3's kernel_stats csv -> ns per step spent in the three shared_gemm_kernel instantiations"""
    tot = 0.0
    for row in csv.DictReader(open(stats_csv)):
        if "shared_gemm_kernel" in row.get("Name", ""):
            tot += float(row["TotalDurationNs"])
    return tot / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, nargs="+", default=[64, 256, 1024])
    ap.add_argument("--only", choices=["a", "b"], default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--gemm-stats", nargs="*", default=[], help="M=kernel_stats.csv of a `--only a --M M` run under rocprofv3 (same --reps / --warmup)")
    ap.add_argument("--from-json", default=None, help="take the timings from an earlier --out file (no GPU run) and only add --gemm-stats to them")
    ap.add_argument("--stats-steps", type=int, default=None, help="steps of the profiled runs (default: --reps + --warmup)")
    a = ap.parse_args()
    if a.from_json:
        out = json.load(open(a.from_json))
    elif not torch.cuda.is_available():
        sys.exit("bench_shared_negatives: needs a GPU (no CPU fallback)")
    else:
        out = run(a.M, a.only, a.reps, a.warmup)
    for spec in a.gemm_stats:
        m, path = spec.split("=", 1)
        for res in out["results"]:
            if res["M"] == int(m):
                ns = gemm_time_per_step(path, a.stats_steps or a.reps + a.warmup)
                res["gemm_kernel_ms_per_step"] = ns * 1e-6
                res["gemm_share_of_mfma_f32_peak"] = res["gemm_flops_per_step"] / (ns * 1e-9) / MFMA_F32_PEAK if ns > 0 else None
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
